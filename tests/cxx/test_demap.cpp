// test_demap.cpp -- hzsdr::stream::Demapper (go-sdr_amd/cxx/hzsdr.hpp) over the C ABI in a HOST context: a text sent as
// 16-QAM symbols (Gray per axis, written out here) through a block interleaver and a flip sequence made here; the
// demapper's values, in the decoder's order and sign, spell the text by their signs alone; a block with counts is
// obeyed; real four-level symbols; sizes and plan; configurations out of bounds are refused.  Prints "demap-cxx ok" and
// exits 0.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "go-sdr_amd/cxx/hzsdr.hpp"

static int failures = 0;
#define CHECK(cond)                                                \
    do {                                                           \
        if (!(cond)) {                                             \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                            \
        }                                                          \
    } while (0)

int main() {
    using namespace hzsdr;
    Context ctx(0);
    const std::string text = "demapper";  // 64 bits: 16 symbols of 4 bits
    const size_t S = 16, m = 4, N = S * m, R = 3, rows_il = 8, cols_il = 8;
    // a level by its two-bit Gray label: 00 -> -3, 01 -> -1, 11 -> +1, 10 -> +3
    const float level[4] = {-3, -1, 3, 1};
    stream::Demapper::Config dc;
    dc.bits_per_symbol = m, dc.symbols = S, dc.gains = {0.5f, 1.0f, 2.0f};
    for (unsigned p = 0; p < 16; p++) dc.points.push_back(level[p >> 2]), dc.points.push_back(level[p & 3]);
    for (size_t k = 0; k < N; k++) dc.perm.push_back((uint32_t)((k % cols_il) * rows_il + k / cols_il));  // written by rows, sent by columns
    std::vector<int> prbs(N);
    for (size_t k = 0; k < N; k++) prbs[k] = (int)((k * 2654435761u >> 7) & 1u);
    dc.flip.assign(N / 8, 0);
    for (size_t k = 0; k < N; k++)
        if (prbs[k]) dc.flip[k / 8] |= (uint8_t)(0x80u >> (k % 8));
    // the transmitter: randomise, interleave, map
    std::vector<int> sent(N);
    for (size_t k = 0; k < N; k++) sent[dc.perm[k]] = ((text[k / 8] >> (7 - k % 8)) & 1) ^ prbs[k];
    std::vector<float> x(R * 2 * (2 * S), 0.0f);  // R rows of cap = 2 frames
    for (size_t r = 0; r < R; r++)
        for (size_t s = 0; s < S; s++) {
            const unsigned p = (unsigned)(sent[4 * s] << 3 | sent[4 * s + 1] << 2 | sent[4 * s + 2] << 1 | sent[4 * s + 3]);
            x[(r * 2) * 2 * S + 2 * s] = dc.points[2 * p] + 0.3f * (float)r, x[(r * 2) * 2 * S + 2 * s + 1] = dc.points[2 * p + 1] - 0.2f * (float)r;
        }
    {
        stream::Demapper d(ctx, HZSDR_DEMAP_C64, dc, R);
        CHECK(d.Rows() == R && d.Symbols() == S && d.FrameFloats() == 2 * S && d.BitsPerSymbol() == m && d.Values() == N);
        CHECK(std::get<0>(d.Plan()) == 8 && std::get<1>(d.Plan()) == 64 && std::get<2>(d.Plan()) == 4 * N &&
              std::get<3>(d.Plan()) == (HZSDR_DEMAP_FORM_GROUPED | HZSDR_DEMAP_FORM_PERM));
        const std::vector<uint32_t> counts = {1, 0, 5};
        const std::vector<float> v = d.Run(x.data(), 2, 0, counts.data());
        CHECK(v.size() == R * 2 * N);
        for (size_t r = 0; r < R; r += 2) {
            std::string back(8, '\0');
            for (size_t k = 0; k < N; k++)
                if (!std::signbit(v[(r * 2) * N + k])) back[k / 8] = (char)(back[k / 8] | (0x80 >> (k % 8)));
            CHECK(back == text);
        }
        for (size_t k = 0; k < 2 * N; k++) CHECK(v[2 * N + k] == 0.0f);          // row 1 handles nothing
        size_t written = 0;
        for (size_t k = 0; k < N; k++) {
            CHECK(v[N + k] == 0.0f);
            written += v[5 * N + k] != 0.0f;
        }
        CHECK(written == N / 2);  // row 0's second slot is not touched; row 2's is: symbols of 0 + 0i, whose inner/outer bits have a value
        // the gain scales a row's values: row 0 without noise, 0.5 * (d0 - d1)
        dc.gains = {1.0f};
        stream::Demapper one(ctx, HZSDR_DEMAP_C64, dc, 1);
        const std::vector<float> u = one.Run(x.data(), 1);
        for (size_t k = 0; k < N; k++) CHECK(u[k] * 0.5f == v[k]);
    }
    {
        // four real levels: the sign of the first bit is the level's side, the second bit says inner (1) or outer (0)
        stream::Demapper::Config pc;
        pc.bits_per_symbol = 2, pc.symbols = 4, pc.points = {-3, -1, 3, 1};
        stream::Demapper d(ctx, HZSDR_DEMAP_REAL_F32, pc);
        const float lv[4] = {-2.9f, -1.2f, 0.8f, 3.3f};
        const std::vector<float> v = d.Run(lv, 1);
        const bool want[8] = {false, false, false, true, true, true, true, false};
        for (size_t k = 0; k < 8; k++) CHECK(!std::signbit(v[k]) == want[k]);
    }
    try {
        stream::Demapper::Config bad = dc;
        bad.perm[5] = (uint32_t)N;
        stream::Demapper d(ctx, HZSDR_DEMAP_C64, bad);
        CHECK(!"a perm entry at S m accepted");
    } catch (const Error &e) {
        CHECK(e.status == HZSDR_ERR_INVALID_ARGUMENT);
    }
    try {
        stream::Demapper d(ctx, 7, dc);
        CHECK(!"an unknown kind accepted");
    } catch (const Error &e) {
        CHECK(e.status == HZSDR_ERR_FORMAT_UNKNOWN);
    }
    try {
        stream::Demapper::Config bad = dc;
        bad.flip.pop_back();
        stream::Demapper d(ctx, HZSDR_DEMAP_C64, bad);
        CHECK(!"a short flip accepted");
    } catch (const std::invalid_argument &) {
    }
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("demap-cxx ok\n");
    return 0;
}

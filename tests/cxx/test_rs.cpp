// test_rs.cpp -- hzsdr::stream::ReedSolomon behind hzsdr::stream::Viterbi (go-sdr_amd/cxx/hzsdr.hpp) over the C ABI in a
// HOST context: a text as two interleaved codewords of a shortened Reed-Solomon code (0x11D, fcr 0, prim 1, 6 parity
// symbols, n = 20), scrambled, then the K = 7 rate 1/2 code; rows with more and more wrong BYTES planted before the
// inner code come through Viterbi::Decode unchanged (the inner code sees a clean frame) and ReedSolomon::Decode takes
// them out: up to three per codeword are corrected and counted, four fail that codeword; a block with counts and
// pitches is obeyed; sizes and plan; configurations out of bounds are refused.  Prints "rs-cxx ok" and exits 0.
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

static unsigned parity(unsigned v) { return (unsigned)__builtin_popcount(v) & 1u; }

static unsigned gf_mul(unsigned a, unsigned b) {
    unsigned r = 0;
    for (; b; b >>= 1) {
        if (b & 1u) r ^= a;
        a <<= 1;
        if (a & 0x100u) a ^= 0x11Du;
    }
    return r;
}

int main() {
    using namespace hzsdr;
    Context ctx(0);
    const unsigned NR = 6, N = 20, KK = N - NR, I = 2, K = 7;
    const size_t F = I * N, IK = I * KK, D = 8 * F, T = D + K - 1, P = 2 * T, R = 5;
    const std::string text = "outer code behind the inner.";
    CHECK(text.size() == IK);
    // the generator prod_j (x - alpha^j), the coefficient of x^NR first
    std::vector<unsigned> g(NR + 1, 0);
    g[0] = 1;
    unsigned root = 1;
    for (unsigned j = 0; j < NR; j++) {
        for (unsigned i = j + 1; i > 0; i--) g[i] ^= gf_mul(g[i - 1], root);
        root = gf_mul(root, 2);
    }
    std::vector<uint8_t> frame(F), scramble = {0xFF, 0x48, 0x0E};
    for (unsigned i = 0; i < I; i++) {
        std::vector<unsigned> rem(N, 0);
        for (unsigned p = 0; p < KK; p++) rem[p] = (uint8_t)text[i + p * I];
        for (unsigned p = 0; p < KK; p++) {
            const unsigned lead = rem[p];
            for (unsigned j = 1; j <= NR; j++) rem[p + j] ^= gf_mul(lead, g[j]);
        }
        for (unsigned p = 0; p < N; p++) frame[i + p * I] = (uint8_t)(p < KK ? (uint8_t)text[i + p * I] : rem[p]);
    }
    for (size_t m = 0; m < F; m++) frame[m] ^= scramble[m % 3];
    // row r: r wrong bytes in codeword 1, then the inner code over the frame's bits
    std::vector<uint8_t> coded(R * ((P + 7) / 8), 0);
    const size_t FB = (P + 7) / 8;
    for (size_t r = 0; r < R; r++) {
        std::vector<uint8_t> f = frame;
        for (size_t e = 0; e < r; e++) f[1 + (2 + 4 * e) * I] ^= (uint8_t)(0x80u >> e);
        unsigned state = 0;
        for (size_t t = 0; t < T; t++) {
            const unsigned u = t < D ? (unsigned)(f[t / 8] >> (7 - t % 8)) & 1u : 0u;
            const unsigned reg = (u << (K - 1)) | state;
            const unsigned c0 = parity(reg & 0171u), c1 = parity(reg & 0133u) ^ 1u;
            if (c0) coded[r * FB + (2 * t) / 8] |= (uint8_t)(0x80u >> ((2 * t) % 8));
            if (c1) coded[r * FB + (2 * t + 1) / 8] |= (uint8_t)(0x80u >> ((2 * t + 1) % 8));
            state = reg >> 1;
        }
    }
    stream::Viterbi::Config vc;
    vc.inv = 2, vc.data_bits = D;
    stream::ReedSolomon::Config rc;
    rc.gfpoly = 0x11D, rc.fcr = 0, rc.prim = 1, rc.nroots = NR, rc.n = N, rc.interleave = I, rc.scramble = scramble;
    {
        stream::Viterbi v(ctx, HZSDR_VITERBI_BITS, vc, R);
        stream::ReedSolomon rs(ctx, rc, R);
        CHECK(rs.Rows() == R && rs.DataSymbols() == KK && rs.Correctable() == 3 && rs.FrameBytes() == F && rs.DataBytes() == IK && v.DataBytes() == F);
        CHECK(std::get<0>(rs.Plan()) == I && std::get<1>(rs.Plan()) < 8192 && std::get<2>(rs.Plan()) == 16 && std::get<3>(rs.Plan()) >= 1);
        const auto decoded = v.Decode(coded.data(), 1);
        const auto clean = rs.Decode(decoded);
        CHECK(clean.size() == R);
        for (size_t r = 0; r < R; r++) {
            CHECK(decoded[r].size() == 1 && decoded[r][0].metric == 0 && clean[r].size() == 1);
            const auto &c = clean[r][0];
            if (r <= 3) {
                CHECK(std::string(c.bytes.begin(), c.bytes.end()) == text && c.errors == r && c.failed == 0 && c.ok);
            } else {
                CHECK(c.errors == 0 && c.failed == 1 && !c.ok);
                for (size_t m = 0; m < IK; m += 2) CHECK(c.bytes[m] == (uint8_t)text[m]);
            }
        }
        // a block with counts and pitches: row 1 decodes nothing, row 2 one of two slots
        const size_t pitch = F + 3, stride = 2 * pitch + 1;
        std::vector<uint8_t> block(R * stride, 0x3C);
        for (size_t r = 0; r < R; r++)
            for (size_t f = 0; f < 2; f++) std::copy(decoded[r][0].bytes.begin(), decoded[r][0].bytes.end(), block.begin() + (long)(r * stride + f * pitch));
        const std::vector<uint32_t> counts = {2, 0, 1, 9, 2};
        const auto some = rs.Decode(block.data(), 2, stride, pitch, counts.data());
        CHECK(some[0].size() == 2 && some[1].empty() && some[2].size() == 1 && some[3].size() == 2 && some[3][1].errors == 3 && some[4][1].failed == 1);
        CHECK(some[2][0].bytes == clean[2][0].bytes && some[0][1].bytes == clean[0][0].bytes);
    }
    try {
        stream::ReedSolomon::Config bad = rc;
        bad.gfpoly = 0x11B;
        stream::ReedSolomon r(ctx, bad);
        CHECK(!"a polynomial that is not primitive accepted");
    } catch (const Error &e) {
        CHECK(e.status == HZSDR_ERR_INVALID_ARGUMENT);
    }
    try {
        stream::ReedSolomon::Config bad = rc;
        bad.prim = 85;
        stream::ReedSolomon r(ctx, bad);
        CHECK(!"prim = 85 accepted");
    } catch (const Error &e) {
        CHECK(e.status == HZSDR_ERR_INVALID_ARGUMENT);
    }
    try {
        stream::ReedSolomon::Config bad = rc;
        bad.in_map.assign(255, 0);
        stream::ReedSolomon r(ctx, bad);
        CHECK(!"a map of 255 bytes accepted");
    } catch (const std::invalid_argument &) {
    }
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("rs-cxx ok\n");
    return 0;
}

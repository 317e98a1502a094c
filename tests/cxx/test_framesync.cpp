// test_framesync.cpp -- hzsdr::stream::FrameSync (go-sdr_amd/cxx/hzsdr.hpp) over the C ABI in a HOST context: QPSK rows
// that carry a text behind a 16-bit word, row q turned by i^q, come back as the text under hypothesis q; two pushes equal
// one; State / SetState carry a stream into a second object; in_counts are obeyed; more frames than cap throws; a
// configuration out of bounds is refused.  Prints "framesync-cxx ok" and exits 0.
#include <complex>
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

using cf = std::complex<float>;

// the word through q times (b0, b1) -> (!b1, b0): what the word looks like received as x i^q
static uint64_t turned(uint64_t word, unsigned bits, unsigned q) {
    uint64_t out = 0;
    for (unsigned k = 0; k < bits; k += 2) {
        unsigned b0 = (word >> (bits - 1 - k)) & 1, b1 = (word >> (bits - 2 - k)) & 1;
        for (unsigned t = 0; t < q; t++) {
            const unsigned old = b0;
            b0 = b1 ^ 1u, b1 = old;
        }
        out |= ((uint64_t)b0 << (bits - 1 - k)) | ((uint64_t)b1 << (bits - 2 - k));
    }
    return out;
}

int main() {
    using namespace hzsdr;
    Context ctx(0);
    const std::string text = "frames on the device";
    const unsigned W = 16, P = 8 * (unsigned)text.size();
    const size_t N = 300, R = 4, pitch = N + 3, at = 70;  // symbols
    const uint64_t word = 0xEB90;
    std::vector<int> bits(2 * N);
    for (size_t i = 0; i < 2 * N; i++) bits[i] = (int)((i * 2654435761u >> 7) & 1u);
    for (unsigned k = 0; k < W; k++) bits[2 * at + k] = (int)((word >> (W - 1 - k)) & 1);
    for (unsigned k = 0; k < P; k++) bits[2 * at + W + k] = (text[k / 8] >> (7 - k % 8)) & 1;
    std::vector<cf> x(R * pitch);
    for (size_t r = 0; r < R; r++)
        for (size_t n = 0; n < N; n++) {
            cf v((bits[2 * n] ? 1.0f : -1.0f) * (float)(1 + n % 5), (bits[2 * n + 1] ? 1.0f : -1.0f) * (float)(1 + n % 3));
            for (size_t t = 0; t < r; t++) v = cf(-v.imag(), v.real());  // times i
            x[r * pitch + n] = v;
        }
    stream::FrameSync::Config c;
    c.bits_per_symbol = 2, c.word_bits = W, c.payload_bits = P, c.thr = 0, c.holdoff = 20;
    for (unsigned q = 0; q < 4; q++) c.words.push_back(turned(word, W, q)), c.maps.push_back(q);
    const size_t start = at + W / 2;
    {
        stream::FrameSync f(ctx, HZSDR_FMT_C64, c, R);
        CHECK(f.Rows() == R && std::get<0>(f.Plan()) == 1 && std::get<1>(f.Plan()) == 64 && f.FrameBytes() == text.size());
        CHECK(std::get<3>(f.Plan()) == (HZSDR_FRAMESYNC_FORM_COMPLEX | HZSDR_FRAMESYNC_FORM_DIBIT));
        const auto rows = f.Push(x.data(), N, pitch);
        CHECK(rows.size() == R);
        for (size_t r = 0; r < R; r++) {
            bool seen = false;
            for (const auto &fr : rows[r])
                if (fr.position == start) {
                    seen = true;
                    CHECK(std::string(fr.bytes.begin(), fr.bytes.end()) == text && fr.distance == 0 && fr.hypothesis == r);
                }
            CHECK(seen);
        }
        const auto z = f.State();
        CHECK(f.Positions() == std::vector<uint64_t>(R, N) && z.positions == f.Positions() && z.history.size() == R * f.HistoryBytes());
        // two pushes, the second from a second object that takes the first one's state
        f.Reset();
        CHECK(f.Positions() == std::vector<uint64_t>(R, 0));
        stream::FrameSync g(ctx, HZSDR_FMT_C64, c, R);
        const auto head = f.Push(x.data(), 100, pitch);
        g.SetState(f.State());
        const auto tail = g.Push(x.data() + 100, N - 100, pitch);
        const auto z2 = g.State();
        CHECK(z2.positions == z.positions && z2.holds == z.holds && z2.history == z.history && z2.last == z.last);
        for (size_t r = 0; r < R; r++) {
            CHECK(head[r].size() + tail[r].size() == rows[r].size());
            for (size_t k = 0; k < rows[r].size(); k++) {
                const auto &fr = k < head[r].size() ? head[r][k] : tail[r][k - head[r].size()];
                CHECK(fr.bytes == rows[r][k].bytes && fr.position == rows[r][k].position && fr.hypothesis == rows[r][k].hypothesis);
            }
        }
        // in_counts: only row 2 consumes
        f.Reset();
        const std::vector<uint32_t> counts = {0, 0, (uint32_t)N, 0};
        const auto only = f.Push(x.data(), N, pitch, counts.data());
        CHECK(only[0].empty() && only[1].empty() && only[3].empty() && only[2].size() == rows[2].size());
        CHECK(f.Positions() == (std::vector<uint64_t>{0, 0, N, 0}));
    }
    {
        // a word that every run of ones matches, hold-off 1: more frames than cap throws
        stream::FrameSync::Config every;
        every.word_bits = 2, every.payload_bits = 2, every.words = {3}, every.maps = {0}, every.holdoff = 1;
        stream::FrameSync f(ctx, HZSDR_SYMSYNC_REAL_F32, every);
        std::vector<float> ones(50, 1.0f);
        try {
            f.Push(ones.data(), ones.size(), 0, nullptr, 4);
            CHECK(!"more frames than cap passed in silence");
        } catch (const std::length_error &) {
        }
        f.Reset();
        const auto all = f.Push(ones.data(), ones.size(), 0, nullptr, 64);
        CHECK(all[0].size() == 47 && all[0][0].position == 2 && all[0][46].position == 48 && all[0][0].bytes[0] == 0xC0);
    }
    try {
        stream::FrameSync::Config bad = c;
        bad.thr = 16;
        stream::FrameSync f(ctx, HZSDR_FMT_C64, bad, R);
        CHECK(!"thr = popcount(mask) accepted");
    } catch (const Error &e) {
        CHECK(e.status == HZSDR_ERR_INVALID_ARGUMENT);
    }
    try {
        stream::FrameSync f(ctx, 7, c);
        CHECK(!"an unknown kind accepted");
    } catch (const Error &e) {
        CHECK(e.status == HZSDR_ERR_FORMAT_UNKNOWN);
    }
    try {
        stream::FrameSync::Config bad = c;
        bad.maps.pop_back();
        stream::FrameSync f(ctx, HZSDR_FMT_C64, bad);
        CHECK(!"three maps for four words accepted");
    } catch (const std::invalid_argument &) {
    }
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("framesync-cxx ok\n");
    return 0;
}

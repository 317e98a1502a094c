// test_softframe.cpp -- hzsdr::stream::SoftFrames beside hzsdr::stream::FrameSync and in front of hzsdr::stream::Viterbi
// (go-sdr_amd/cxx/hzsdr.hpp) over the C ABI in a HOST context: a text through the K = 7 rate 1/2 code onto QPSK symbols of
// varying amplitude behind a 32-bit sync word, four rows received under the four rotations, pushed in two pieces that cut
// the payload; every frame's floats are served, their signs are the bits the FrameSync packed, and the soft-input Viterbi
// decodes them to the text with metric 0; the raw Push obeys counts and leaves the other slots; state, plan, positions
// and reset; a differential FrameSync configuration is refused.  Prints "softframe-cxx ok" and exits 0.
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

static unsigned parity(unsigned v) { return (unsigned)__builtin_popcount(v) & 1u; }

// every dibit (b0, b1) of the word, b0 the more significant, through m times (b0, b1) -> (b1, !b0)
static uint64_t map_dibits(uint64_t word, unsigned bits, unsigned m) {
    uint64_t out = 0;
    for (int k = (int)bits - 2; k >= 0; k -= 2) {
        unsigned b0 = (unsigned)(word >> (k + 1)) & 1u, b1 = (unsigned)(word >> k) & 1u;
        for (unsigned i = 0; i < m % 4; i++) {
            const unsigned t = b0;
            b0 = b1, b1 = t ^ 1u;
        }
        out |= ((uint64_t)b0 << (k + 1)) | ((uint64_t)b1 << k);
    }
    return out;
}

int main() {
    using namespace hzsdr;
    Context ctx(0);
    const std::string text = "softbits";
    const unsigned K = 7, W = 32;
    const uint64_t word = 0x1ACFFC1Dull;
    const size_t D = 8 * text.size(), T = D + K - 1, P = 2 * T, Ps = P / 2, R = 4, lead = 9, n = lead + W / 2 + Ps + 6;
    std::vector<unsigned> bits;  // the word, then the code bits
    for (unsigned k = 0; k < W; k++) bits.push_back((unsigned)(word >> (W - 1 - k)) & 1u);
    unsigned state = 0;
    for (size_t t = 0; t < T; t++) {
        const unsigned u = t < D ? ((unsigned)(uint8_t)text[t / 8] >> (7 - t % 8)) & 1u : 0u;
        const unsigned reg = (u << (K - 1)) | state;
        bits.push_back(parity(reg & 0171u));
        bits.push_back(parity(reg & 0133u));
        state = reg >> 1;
    }
    std::vector<std::complex<float>> x(R * n, std::complex<float>(0.5f, 0.5f));
    for (size_t r = 0; r < R; r++)
        for (size_t i = 0; i < bits.size() / 2; i++) {
            const float a = 0.3f + 0.01f * (float)((i * 7 + r) % 40);
            std::complex<float> v(bits[2 * i] ? a : -a, bits[2 * i + 1] ? a : -a);
            for (size_t q = 0; q < r; q++) v = {-v.imag(), v.real()};  // times i
            x[r * n + lead + i] = v;
        }
    stream::FrameSync::Config fc;
    fc.bits_per_symbol = 2, fc.word_bits = W, fc.payload_bits = (unsigned)P;
    for (unsigned q = 0; q < 4; q++) fc.words.push_back(map_dibits(word, W, (4 - q) % 4)), fc.maps.push_back(q);
    stream::Viterbi::Config vc;
    vc.data_bits = D, vc.scale = 64.0f;
    {
        stream::FrameSync fs(ctx, HZSDR_FMT_C64, fc, R);
        stream::SoftFrames sf(ctx, HZSDR_FMT_C64, fc, R);
        stream::Viterbi vd(ctx, HZSDR_VITERBI_SOFT_F32, vc, R);
        CHECK(sf.Rows() == R && sf.PayloadBits() == P && sf.HistoryFloats() == P - 2 && vd.ReceivedBits() == P);
        CHECK(std::get<0>(sf.Plan()) == 512 && std::get<2>(sf.Plan()) == (HZSDR_SOFTFRAME_FORM_COMPLEX | HZSDR_SOFTFRAME_FORM_DIBIT));
        const size_t cut = lead + W / 2 + Ps / 2;
        std::vector<std::complex<float>> a(R * cut), b(R * (n - cut));
        for (size_t r = 0; r < R; r++) {
            std::copy(x.begin() + (long)(r * n), x.begin() + (long)(r * n + cut), a.begin() + (long)(r * cut));
            std::copy(x.begin() + (long)(r * n + cut), x.begin() + (long)((r + 1) * n), b.begin() + (long)(r * (n - cut)));
        }
        const auto f0 = fs.Push(a.data(), cut);
        const auto s0 = sf.Push(a.data(), cut, f0);
        for (size_t r = 0; r < R; r++) CHECK(f0[r].empty() && s0[r].empty());
        const auto mid = sf.State();
        CHECK(mid.positions == std::vector<uint64_t>(R, cut) && mid.history.size() == R * (P - 2));
        const auto f1 = fs.Push(b.data(), n - cut);
        const auto s1 = sf.Push(b.data(), n - cut, f1);
        CHECK(sf.Positions() == std::vector<uint64_t>(R, n));
        std::vector<float> block(R * P, 0.0f);
        for (size_t r = 0; r < R; r++) {
            CHECK(f1[r].size() == 1 && s1[r].size() == 1);
            if (f1[r].size() != 1 || s1[r].size() != 1) continue;
            CHECK(f1[r][0].hypothesis == r && f1[r][0].position == lead + W / 2 && s1[r][0].status == HZSDR_SOFTFRAME_SERVED && s1[r][0].values.size() == P);
            for (size_t k = 0; k < P; k++) {
                const float v = s1[r][0].values[k];
                const unsigned bit = (f1[r][0].bytes[k / 8] >> (7 - k % 8)) & 1u;
                CHECK(bit == (std::signbit(v) ? 0u : 1u) && bit == bits[W + k]);
                CHECK(std::fabs(v) == 0.3f + 0.01f * (float)(((W / 2 + k / 2) * 7 + r) % 40));
            }
            std::copy(s1[r][0].values.begin(), s1[r][0].values.end(), block.begin() + (long)(r * P));
        }
        const auto decoded = vd.Decode(block.data(), 1);
        for (size_t r = 0; r < R; r++) {
            CHECK(decoded[r].size() == 1 && decoded[r][0].metric == 0);
            CHECK(std::string(decoded[r][0].bytes.begin(), decoded[r][0].bytes.end()) == text);
        }
        // the same second push through a bank that got the state, by the raw arrays: row 2 is told to emit nothing
        stream::SoftFrames other(ctx, HZSDR_FMT_C64, fc, R);
        other.SetState(mid);
        std::vector<uint64_t> pos(R);
        std::vector<uint32_t> info(R), counts(R, 1), status(R, 77);
        std::vector<float> out(R * (P + 3), -5.0f);
        for (size_t r = 0; r < R; r++) pos[r] = f1[r][0].position, info[r] = f1[r][0].distance | f1[r][0].hypothesis << 8;
        counts[2] = 0;
        other.Push(b.data(), n - cut, 0, nullptr, pos.data(), info.data(), counts.data(), 1, out.data(), P + 3, status.data());
        for (size_t r = 0; r < R; r++) {
            CHECK(status[r] == (r == 2 ? 77u : 0u));
            for (size_t k = 0; k < P + 3; k++) CHECK(out[r * (P + 3) + k] == (r == 2 || k >= P ? -5.0f : block[r * P + k]));
        }
        // a forged position: quiet NaNs and the status
        pos[0] = ~0ull, counts[2] = 1, info[1] = 4u << 8;
        other.Push(b.data(), 0, 0, nullptr, pos.data(), info.data(), counts.data(), 1, out.data(), P + 3, status.data());
        CHECK(status[0] == HZSDR_SOFTFRAME_OUTSIDE && status[1] == HZSDR_SOFTFRAME_NO_HYPOTHESIS && status[2] == HZSDR_SOFTFRAME_OUTSIDE);
        for (size_t k = 0; k < P; k++) CHECK(std::isnan(out[k]) && std::isnan(out[P + 3 + k]));
        other.Reset();
        CHECK(other.Positions() == std::vector<uint64_t>(R, 0));
        for (float v : other.State().history) CHECK(v == 0.0f);
    }
    try {
        stream::FrameSync::Config bad = fc;
        bad.bits_per_symbol = 1, bad.diff = 1;
        stream::SoftFrames s(ctx, HZSDR_FMT_C64, bad);
        CHECK(!"a differential configuration accepted");
    } catch (const std::invalid_argument &) {
    }
    try {
        stream::FrameSync::Config bad = fc;
        bad.payload_bits = 7;
        stream::SoftFrames s(ctx, HZSDR_FMT_C64, bad);
        CHECK(!"an odd payload at two bits per symbol accepted");
    } catch (const Error &e) {
        CHECK(e.status == HZSDR_ERR_INVALID_ARGUMENT);
    }
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("softframe-cxx ok\n");
    return 0;
}

// test_viterbi.cpp -- hzsdr::stream::Viterbi behind hzsdr::stream::FrameSync (go-sdr_amd/cxx/hzsdr.hpp) over the C ABI in
// a HOST context: real rows that carry, behind a 16-bit word, the K = 7 rate 1/2 code of a text and its CRC-16; the
// frames FrameSync::Push returns go into Viterbi::Decode as they are and come back as the text, with the flipped channel
// bits as the metric and the CRC ok; a block with counts is obeyed; soft input agrees; sizes and plan; a configuration
// out of bounds is refused.  Prints "viterbi-cxx ok" and exits 0.
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

int main() {
    using namespace hzsdr;
    Context ctx(0);
    const std::string text = "viterbi on rows";
    const unsigned K = 7, W = 16, C = 16;
    const size_t D = 8 * text.size() + C, T = D + K - 1, P = 2 * T, R = 3, NS = 700, pitch = NS + 2, at = 120;
    const uint64_t word = 0xEB90;
    // the data bits: the text and its CRC-16/CCITT-FALSE
    std::vector<int> u(D);
    unsigned reg = 0xFFFF;
    for (size_t k = 0; k < 8 * text.size(); k++) {
        u[k] = (text[k / 8] >> (7 - k % 8)) & 1;
        const unsigned top = ((reg >> 15) & 1u) ^ (unsigned)u[k];
        reg = (reg << 1) & 0xFFFFu;
        if (top) reg ^= 0x1021u;
    }
    for (unsigned k = 0; k < C; k++) u[8 * text.size() + k] = (int)((reg >> (15 - k)) & 1u);
    // the code bits, by the header's definition (the second output inverted)
    std::vector<int> code(P);
    unsigned state = 0;
    for (size_t t = 0; t < T; t++) {
        const unsigned r = ((t < D ? (unsigned)u[t] : 0u) << (K - 1)) | state;
        code[2 * t] = (int)parity(r & 0171u), code[2 * t + 1] = (int)(parity(r & 0133u) ^ 1u);
        state = r >> 1;
    }
    // row r: pseudo-random bits, the word and the code at symbol `at`, r channel bits of the code flipped
    std::vector<float> x(R * pitch);
    for (size_t r = 0; r < R; r++)
        for (size_t n = 0; n < NS; n++) {
            int bit = (int)((n * 2654435761u >> 9) & 1u);
            if (n >= at && n < at + W) bit = (int)((word >> (W - 1 - (n - at))) & 1);
            if (n >= at + W && n < at + W + P) {
                const size_t k = n - at - W;
                bit = code[k] ^ (int)(k % 97 == 5 && k / 97 < r);
            }
            x[r * pitch + n] = (bit ? 1.0f : -1.0f) * (float)(1 + n % 4);
        }
    stream::FrameSync::Config fc;
    fc.word_bits = W, fc.payload_bits = (unsigned)P, fc.thr = 0, fc.words = {word}, fc.maps = {0};
    stream::Viterbi::Config vc;
    vc.inv = 2, vc.data_bits = D, vc.crc_bits = C, vc.crc_poly = 0x1021, vc.crc_init = 0xFFFF;
    {
        stream::FrameSync f(ctx, HZSDR_SYMSYNC_REAL_F32, fc, R);
        stream::Viterbi v(ctx, HZSDR_VITERBI_BITS, vc, R);
        CHECK(v.Rows() == R && v.ReceivedBits() == P && v.FrameBytes() == f.FrameBytes() && v.Steps() == T && v.DataBytes() == (D + 7) / 8);
        CHECK(std::get<0>(v.Plan()) == 1 && std::get<1>(v.Plan()) == 1 && std::get<2>(v.Plan()) == T * 8 && std::get<3>(v.Plan()) == HZSDR_VITERBI_FORM_LDS);
        const auto frames = f.Push(x.data(), NS, pitch, nullptr, 8);
        const auto decoded = v.Decode(frames);
        CHECK(decoded.size() == R);
        for (size_t r = 0; r < R; r++) {
            CHECK(decoded[r].size() == frames[r].size());
            bool seen = false;
            for (size_t k = 0; k < frames[r].size(); k++)
                if (frames[r][k].position == at + W) {
                    seen = true;
                    const auto &d = decoded[r][k];
                    CHECK(std::string(d.bytes.begin(), d.bytes.begin() + (long)text.size()) == text && d.metric == r && d.crc_ok);
                }
            CHECK(seen);
        }
        // a block with counts: row 1 decodes nothing
        std::vector<uint8_t> block(R * 2 * v.FrameBytes(), 0);
        for (size_t r = 0; r < R; r++)
            for (const auto &fr : frames[r])
                if (fr.position == at + W) std::copy(fr.bytes.begin(), fr.bytes.end(), block.begin() + (long)(r * 2 * v.FrameBytes()));
        const std::vector<uint32_t> counts = {1, 0, 5};
        const auto some = v.Decode(block.data(), 2, 0, counts.data());
        CHECK(some[0].size() == 1 && some[1].empty() && some[2].size() == 2 && some[0][0].crc_ok && some[2][0].metric == 2);
        // soft input of magnitude 2: the same bytes, every flip costs 2
        stream::Viterbi s(ctx, HZSDR_VITERBI_SOFT_F32, vc, R);
        std::vector<float> soft(R * P);
        for (size_t r = 0; r < R; r++)
            for (size_t k = 0; k < P; k++) soft[r * P + k] = (code[k] ^ (int)(k % 97 == 5 && k / 97 < r)) ? 2.0f : -2.0f;
        const auto sd = s.Decode(soft.data(), 1);
        for (size_t r = 0; r < R; r++) CHECK(sd[r].size() == 1 && sd[r][0].bytes == some[r == 1 ? 0 : r][0].bytes && sd[r][0].metric == 2 * r && sd[r][0].crc_ok);
    }
    try {
        stream::Viterbi::Config bad = vc;
        bad.K = 10;
        stream::Viterbi v(ctx, HZSDR_VITERBI_BITS, bad);
        CHECK(!"K = 10 accepted");
    } catch (const Error &e) {
        CHECK(e.status == HZSDR_ERR_INVALID_ARGUMENT);
    }
    try {
        stream::Viterbi v(ctx, 7, vc);
        CHECK(!"an unknown kind accepted");
    } catch (const Error &e) {
        CHECK(e.status == HZSDR_ERR_FORMAT_UNKNOWN);
    }
    try {
        stream::Viterbi::Config bad = vc;
        bad.gens.clear();
        stream::Viterbi v(ctx, HZSDR_VITERBI_BITS, bad);
        CHECK(!"no generators accepted");
    } catch (const std::invalid_argument &) {
    }
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("viterbi-cxx ok\n");
    return 0;
}

// test_tuner.cpp -- hzsdr::stream::TunerBank (go-sdr_amd/cxx/hzsdr.hpp) over the C ABI in a HOST context: a stream that
// is zero but for one sample `a` at position j0 comes out of a tuner on a quarter-turn word (k * 2^30) as the taps turned
// by (-i)^(k j0), y_k[m] = a h[m D - j0] (-i)^(k j0) where that index exists and zero elsewhere -- every factor is on an
// axis, so the check is exact, output by output, with D above and at one and through the chunked form; retune moves a
// row; the read-outs have their lengths and entry 0 of a table is 1.  Prints "tuner-cxx ok" and exits 0.
#include <complex>
#include <cstdio>

#include "go-sdr_amd/cxx/hzsdr.hpp"

static int failures = 0;
#define CHECK(cond)                                                \
    do {                                                           \
        if (!(cond)) {                                             \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                            \
        }                                                          \
    } while (0)

typedef std::complex<float> cf;

static cf turned(cf v, size_t quarter_turns_back) {  // v (-i)^n
    for (size_t n = 0; n < quarter_turns_back % 4; n++) v = cf(v.imag(), -v.real());
    return v;
}

static void impulse(hzsdr::Context &ctx, size_t D, size_t Q, bool chunked) {
    using namespace hzsdr;
    const size_t N = 700, j0 = 333;
    const cf a(0.5f, -2.0f);
    std::vector<float> h(Q);
    for (size_t k = 0; k < Q; k++) h[k] = 0.0078125f * (float)(k % 89) - 0.25f;
    std::vector<cf> x(N);
    x[j0] = a;
    std::vector<uint32_t> words = {0u, 1u << 30, 2u << 30, 3u << 30, 0u};
    stream::TunerBank b(ctx, HZSDR_FMT_C64, words, h, D);
    CHECK(b.Tuners() == 5 && std::get<0>(b.Plan()) >= 32 && std::get<1>(b.Plan()) >= 32);
    CHECK(((std::get<2>(b.Plan()) & HZSDR_TUNER_FORM_CHUNKED) != 0) == chunked);
    b.Retune(4, {3u << 30});
    const size_t head = (N + D - 1) / D, total = (N - 1 + Q + D - 1) / D;
    CHECK(b.OutputsFor(N) == head);
    const std::vector<cf> p = b.Push(x.data(), N);
    CHECK(p.size() == 5 * head);
    CHECK(std::get<0>(b.Pending()) == N && std::get<1>(b.Pending()) == head && std::get<2>(b.Pending()) == total - head);
    const std::vector<cf> t = b.Flush();
    CHECK(t.size() == 5 * (total - head));
    CHECK(std::get<0>(b.Pending()) == 0 && std::get<1>(b.Pending()) == 0);
    for (size_t k = 0; k < 5; k++)
        for (size_t m = 0; m < total; m++) {
            const cf got = m < head ? p[k * head + m] : t[k * (total - head) + (m - head)];
            const bool in = m * D >= j0 && m * D - j0 < Q;
            const cf want = in ? turned(a * h[m * D - j0], (k == 4 ? 3 : k) * j0) : cf(0.0f, 0.0f);
            CHECK(got == want);
        }
    CHECK(b.Readout(HZSDR_TUNER_READ_TAPS, 1).size() == (Q + 1) / 2 * 2 && b.Readout(HZSDR_TUNER_READ_TAPS, 0)[Q - 1] == cf(h[Q - 1], 0.0f));
    CHECK(b.Readout(HZSDR_TUNER_READ_T2).size() == 2048 && b.Readout(HZSDR_TUNER_READ_T0).size() == 1024);
    CHECK(b.Readout(HZSDR_TUNER_READ_T1)[0] == cf(1.0f, 0.0f) && b.Readout(HZSDR_TUNER_READ_T2)[512] == cf(0.0f, -1.0f));
}

int main() {
    using namespace hzsdr;
    Context ctx(0);
    impulse(ctx, 3, 40, false);
    impulse(ctx, 1, 47, false);
    impulse(ctx, 256, 1024, true);
    impulse(ctx, 1, 1, false);
    try {
        stream::TunerBank bad(ctx, HZSDR_FMT_C64, {0u}, std::vector<float>(8, 1.0f), 257);
        CHECK(!"down above 256 accepted");
    } catch (const Error &e) {
        CHECK(e.status == HZSDR_ERR_INVALID_ARGUMENT);
    }
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("tuner-cxx ok\n");
    return 0;
}

// test_demod.cpp -- hzsdr::stream::Demodulator (go-sdr_amd/cxx/hzsdr.hpp) over the C ABI in a HOST context: the power
// detector of a stream that is zero but for one sample of power 4 comes out as the taps, y[m] = 4 h[m D - j0] where that
// index exists and zero elsewhere, checked output by output with D above and at one; two rows give two such responses;
// the bare FM detector of a quarter-turn-per-sample rotation reads pi / 2.  Prints "demod-cxx ok" and exits 0.
#include <cmath>
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

static void impulse(hzsdr::Context &ctx, size_t D, size_t Q) {
    using namespace hzsdr;
    const size_t N = 700, rows = 2, j0[2] = {5, 333};
    std::vector<float> h(Q);
    for (size_t k = 0; k < Q; k++) h[k] = 0.01f * (float)(k % 89) - 0.3f;
    std::vector<std::complex<float>> x(rows * N);
    for (size_t s = 0; s < rows; s++) x[s * N + j0[s]] = {0.0f, -2.0f};
    stream::Demodulator r(ctx, HZSDR_FMT_C64, HZSDR_DEMOD_POWER, h, D, rows);
    CHECK(r.Streams() == rows && r.Plan().first >= 128);
    const size_t head = (N + D - 1) / D, total = (N - 1 + Q + D - 1) / D;
    CHECK(r.OutputsFor(N) == head);
    const std::vector<float> a = r.Push(x.data(), N);
    CHECK(a.size() == rows * head);
    CHECK(std::get<0>(r.Pending()) == N && std::get<1>(r.Pending()) == head && std::get<2>(r.Pending()) == total - head);
    const std::vector<float> t = r.Flush();
    CHECK(t.size() == rows * (total - head));
    CHECK(std::get<0>(r.Pending()) == 0 && std::get<1>(r.Pending()) == 0);
    for (size_t s = 0; s < rows; s++)
        for (size_t m = 0; m < total; m++) {
            const float got = m < head ? a[s * head + m] : t[s * (total - head) + (m - head)];
            const bool in = m * D >= j0[s] && m * D - j0[s] < Q;
            CHECK(got == (in ? 4.0f * h[m * D - j0[s]] : 0.0f));
        }
}

int main() {
    using namespace hzsdr;
    Context ctx(0);
    impulse(ctx, 3, 40);
    impulse(ctx, 1, 47);
    impulse(ctx, 64, 1024);
    impulse(ctx, 1, 1);
    {
        // i^n: every step a quarter turn
        const std::complex<float> turn[4] = {{1, 0}, {0, 1}, {-1, 0}, {0, -1}};
        std::vector<std::complex<float>> x(64);
        for (size_t n = 0; n < x.size(); n++) x[n] = turn[n % 4];
        stream::Demodulator fm(ctx, HZSDR_FMT_C64, HZSDR_DEMOD_FM);
        const std::vector<float> d = fm.Push(x.data(), x.size());
        CHECK(d.size() == x.size() && fm.Flush().empty());
        for (size_t n = 1; n < d.size(); n++) CHECK(std::fabs(d[n] - 1.5707964f) <= 5e-7f);
    }
    try {
        stream::Demodulator bad(ctx, HZSDR_FMT_C64, HZSDR_DEMOD_FM, std::vector<float>(8, 1.0f), 65);
        CHECK(!"down above 64 accepted");
    } catch (const Error &e) {
        CHECK(e.status == HZSDR_ERR_INVALID_ARGUMENT);
    }
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("demod-cxx ok\n");
    return 0;
}

// test_resampler.cpp -- hzsdr::stream::Resampler (go-sdr_amd/cxx/hzsdr.hpp) over the C ABI in a HOST context: a single
// 1 at sample j0 comes out as the taps, y[m] = h[m D - j0 U] where that index exists and zero elsewhere, checked
// output by output for a ratio above and a ratio below one; two rows give two such responses.  Prints
// "resampler-cxx ok" and exits 0.
#include <cmath>
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

static void impulse(hzsdr::Context &ctx, size_t U, size_t D, size_t L) {
    using namespace hzsdr;
    const size_t N = 700, rows = 2, j0[2] = {5, 333};
    std::vector<float> h(L);
    for (size_t k = 0; k < L; k++) h[k] = 0.01f * (float)(k % 89) - 0.3f;
    std::vector<std::complex<float>> x(rows * N);
    for (size_t s = 0; s < rows; s++) x[s * N + j0[s]] = {1.0f, -2.0f};
    stream::Resampler r(ctx, HZSDR_FMT_C64, U, D, h, rows);
    CHECK(r.Streams() == rows && r.Plan().first >= 64);
    const size_t head = (N * U + D - 1) / D, total = ((N - 1) * U + L + D - 1) / D;
    CHECK(r.OutputsFor(N) == head);
    const Buffer a = r.Push(x.data(), N);
    CHECK(a.view.length == rows * head);
    CHECK(std::get<0>(r.Pending()) == N && std::get<1>(r.Pending()) == head && std::get<2>(r.Pending()) == total - head);
    const Buffer t = r.Flush();
    CHECK(t.view.length == rows * (total - head));
    CHECK(std::get<0>(r.Pending()) == 0 && std::get<1>(r.Pending()) == 0);
    for (size_t s = 0; s < rows; s++)
        for (size_t m = 0; m < total; m++) {
            const auto *p = m < head ? (const std::complex<float> *)a.view.data + s * head + m
                                     : (const std::complex<float> *)t.view.data + s * (total - head) + (m - head);
            const bool in = m * D >= j0[s] * U && m * D - j0[s] * U < L;
            const float g = in ? h[m * D - j0[s] * U] : 0.0f;
            CHECK(p->real() == g && p->imag() == -2.0f * g);
        }
}

int main() {
    using namespace hzsdr;
    Context ctx(0);
    impulse(ctx, 3, 2, 40);
    impulse(ctx, 2, 5, 47);
    impulse(ctx, 1, 1, 1);
    try {
        stream::Resampler bad(ctx, HZSDR_FMT_C64, 1025, 1, std::vector<float>(8, 1.0f));
        CHECK(!"up above 1024 accepted");
    } catch (const Error &e) {
        CHECK(e.status == HZSDR_ERR_INVALID_ARGUMENT);
    }
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("resampler-cxx ok\n");
    return 0;
}

// test_spectrum.cpp -- hzsdr::fft::Spectrum (go-sdr_amd/cxx/hzsdr.hpp) over the C ABI in a HOST context: a stream of i8
// samples that is zero except one impulse at each frame's first sample, amplitudes 2^-(1+s) (1 - 0.5j).  The transform
// of such a frame is the amplitude in every bin, and the squared magnitudes (times the window's w[0]^2 = 0.25 and the
// scale 2^-3) sum exactly in float32, so every bin of row r is known to the bit: in both kernel forms, in one push and
// in two.  A push that completes no row returns an empty vector.  Prints "spectrum-cxx ok" and exits 0.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

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
    const size_t N = 256, HOP = N + 37, K = 3, ROWS = 9, FRAMES = ROWS * K + 2;  // (9 rows: two workgroups of four and one row)
    const size_t LEN = (FRAMES - 1) * HOP + N + 50;  // (37 of the 50 fall into the skip gap, 13 are held)
    const float scale = 0.125f;
    std::vector<int8_t> x(2 * LEN, 0);
    std::vector<double> power(FRAMES);
    for (size_t j = 0; j < FRAMES; j++) {
        const int s = (int)(j % 5), i = 64 >> s, q = -(32 >> s);
        x[2 * j * HOP] = (int8_t)i;
        x[2 * j * HOP + 1] = (int8_t)q;
        power[j] = (double)(i * i + q * q) / (128.0 * 128.0);
    }
    std::vector<float> want(ROWS);
    for (size_t r = 0; r < ROWS; r++) {
        double sum = 0;
        for (size_t t = 0; t < K; t++) sum += 0.25 * power[r * K + t];
        want[r] = (float)(0.125 * sum);
        CHECK((double)want[r] == 0.125 * sum);  // (exact in float32)
    }
    std::vector<float> window(N, 1.0f);
    window[0] = 0.5f;
    auto samples = [&](size_t first, size_t count) { return Samples{HZSDR_FMT_I8, x.data() + 2 * first, count}; };
    auto check_rows = [&](const std::vector<float> &got, size_t r0, size_t rows) {
        CHECK(got.size() == rows * N);
        if (got.size() != rows * N) return;
        for (size_t r = 0; r < rows; r++)
            for (size_t k = 0; k < N; k++) CHECK(std::memcmp(&got[r * N + k], &want[r0 + r], 4) == 0);
    };

    fft::Spectrum sp(ctx, HZSDR_FMT_I8, N, HOP, K, window, scale, HZSDR_ORDER_ZERO_FIRST);
    CHECK(sp.Bins() == N);
    CHECK(sp.RowsFor(LEN) == ROWS && sp.RowsFor(N - 1) == 0 && sp.RowsFor(2 * HOP + N) == 1);
    for (int form : {HZSDR_SPECTRUM_FORM_ROW_WALK, HZSDR_SPECTRUM_FORM_FRAME_PARALLEL}) {
        sp.Reset();
        CHECK(sp.Pending() == std::make_pair((size_t)0, (size_t)0));
        sp.Options(form);
        check_rows(sp.Push(samples(0, LEN)), 0, ROWS);
        CHECK(sp.LastForm() == form);
        CHECK(sp.Pending() == std::make_pair((size_t)2, (size_t)13));
        // two pushes: the first ends one sample behind frame 1's start (one frame in the open row, one sample held)
        sp.Reset();
        const size_t cut = HOP + 1;
        const std::vector<float> none = sp.Push(samples(0, cut));
        CHECK(none.empty());
        CHECK(sp.Pending() == std::make_pair((size_t)1, (size_t)1));
        CHECK(sp.RowsFor(LEN - cut) == ROWS);
        check_rows(sp.Push(samples(cut, LEN - cut)), 0, ROWS);
        CHECK(sp.Pending() == std::make_pair((size_t)2, (size_t)13));
        CHECK(sp.Push(samples(0, 0)).empty());  // (an empty push)
    }
    {
        // a second push that starts in the skip gap behind a row's last frame
        sp.Reset();
        sp.Options(HZSDR_SPECTRUM_FORM_AUTO);
        const size_t cut = 2 * HOP + N + 10;
        check_rows(sp.Push(samples(0, cut)), 0, 1);
        CHECK(sp.Pending() == std::make_pair((size_t)0, (size_t)0));
        check_rows(sp.Push(samples(cut, LEN - cut)), 1, ROWS - 1);
        CHECK(sp.LastForm() == HZSDR_SPECTRUM_FORM_ROW_WALK || sp.LastForm() == HZSDR_SPECTRUM_FORM_FRAME_PARALLEL);
    }
    try {
        sp.Options(7);
        CHECK(!"an unknown kernel form accepted");
    } catch (const Error &e) {
        CHECK(e.status == HZSDR_ERR_INVALID_ARGUMENT);
    }
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("spectrum-cxx ok\n");
    return 0;
}

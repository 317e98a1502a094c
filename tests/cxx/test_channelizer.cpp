// test_channelizer.cpp -- hzsdr::fft::Channelizer (go-sdr_amd/cxx/hzsdr.hpp) over the C ABI in a HOST context: one
// shape in both layouts.  An impulse at stream position t0 gives y[j][k] = g[t0 - jD] exp(-2 pi i k t0 / M) for the
// frames that cover it, which is checked channel by channel; the channel-major result is the transpose, bit for bit.
// Prints "channelizer-cxx ok" and exits 0.
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

int main() {
    using namespace hzsdr;
    const size_t M = 256, P = 3, L = P * M, D = 100, frames = 9, n = (frames - 1) * D + L + 7, t0 = 613;
    Context ctx(0);
    std::vector<float> g(L);
    for (size_t i = 0; i < L; i++) g[i] = 0.001f * (float)(i % 97) + 0.25f;
    Buffer x(HZSDR_FMT_C64, n);
    ((std::complex<float> *)x.view.data)[t0] = {1.0f, 0.0f};
    fft::Channelizer fm(ctx, HZSDR_FMT_C64, M, g, D, HZSDR_ORDER_ZERO_FIRST, HZSDR_CHANNELIZER_FRAME_MAJOR);
    fft::Channelizer cm(ctx, HZSDR_FMT_C64, M, g, D, HZSDR_ORDER_ZERO_FIRST, HZSDR_CHANNELIZER_CHANNEL_MAJOR);
    CHECK(fm.FramesFor(n) == frames && fm.Channels() == M);
    const auto a = fm.Push(x.view);
    const auto b = cm.Push(x.view);
    CHECK(a.size() == frames * M && b.size() == frames * M);
    CHECK(fm.Pending().first == n - frames * D && fm.Pending().second == frames);
    const double pi = 3.14159265358979323846;
    for (size_t j = 0; j < frames; j++) {
        const bool covered = t0 >= j * D && t0 < j * D + L;
        const double amp = covered ? (double)g[t0 - j * D] : 0.0;
        for (size_t k = 0; k < M; k++) {
            const double ph = -2.0 * pi * (double)((k * t0) % M) / (double)M;
            const std::complex<double> want(amp * std::cos(ph), amp * std::sin(ph));
            CHECK(std::abs(std::complex<double>(a[j * M + k]) - want) <= 1e-5 * (amp + 1e-30));
            CHECK(std::memcmp(&a[j * M + k], &b[k * frames + j], sizeof(std::complex<float>)) == 0);
        }
    }
    try {
        fft::Channelizer bad(ctx, HZSDR_FMT_C64, M, g, M + 1);
        CHECK(!"hop above the channel count accepted");
    } catch (const Error &e) {
        CHECK(e.status == HZSDR_ERR_INVALID_ARGUMENT);
    }
    cm.Reset();
    CHECK(cm.Pending().first == 0 && cm.Pending().second == 0);
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("channelizer-cxx ok\n");
    return 0;
}

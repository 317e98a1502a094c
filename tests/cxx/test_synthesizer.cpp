// test_synthesizer.cpp -- hzsdr::fft::Synthesizer (go-sdr_amd/cxx/hzsdr.hpp) over the C ABI in a HOST context: one
// shape in both layouts.  A single value 1 in channel k0 of frame j0 gives x^[t] = g[t - j0 D] exp(+2 pi i k0 t / M)
// over the L positions the frame covers and zero elsewhere, which is checked position by position; the channel-major
// result is the same, bit for bit.  Prints "synthesizer-cxx ok" and exits 0.
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
    const size_t M = 256, P = 3, L = P * M, D = 100, frames = 9, j0 = 4, k0 = 201;
    Context ctx(0);
    std::vector<float> g(L);
    for (size_t i = 0; i < L; i++) g[i] = 0.001f * (float)(i % 97) + 0.25f;
    std::vector<std::complex<float>> fm_in(frames * M), cm_in(frames * M);
    fm_in[j0 * M + k0] = {1.0f, 0.0f};
    cm_in[k0 * frames + j0] = {1.0f, 0.0f};
    fft::Synthesizer fm(ctx, HZSDR_FMT_C64, M, g, D, HZSDR_ORDER_ZERO_FIRST, HZSDR_CHANNELIZER_FRAME_MAJOR);
    fft::Synthesizer cm(ctx, HZSDR_FMT_C64, M, g, D, HZSDR_ORDER_ZERO_FIRST, HZSDR_CHANNELIZER_CHANNEL_MAJOR);
    CHECK(fm.Channels() == M && fm.GroupFrames() >= 1);
    const Buffer a = fm.Push(fm_in), b = cm.Push(cm_in);
    CHECK(a.view.length == frames * D && b.view.length == frames * D);
    CHECK(fm.Pending().first == L - D && fm.Pending().second == frames);
    const Buffer at = fm.Flush(), bt = cm.Flush();
    CHECK(at.view.length == L - D && bt.view.length == L - D);
    CHECK(fm.Pending().first == 0 && fm.Pending().second == 0);
    const double pi = 3.14159265358979323846;
    for (size_t t = 0; t < (frames - 1) * D + L; t++) {
        const bool head = t < frames * D;
        const auto *pa = (const std::complex<float> *)(head ? a : at).view.data + (head ? t : t - frames * D);
        const auto *pb = (const std::complex<float> *)(head ? b : bt).view.data + (head ? t : t - frames * D);
        const bool covered = t >= j0 * D && t < j0 * D + L;
        const double amp = covered ? (double)g[t - j0 * D] : 0.0;
        const double ph = 2.0 * pi * (double)((k0 * t) % M) / (double)M;
        const std::complex<double> want(amp * std::cos(ph), amp * std::sin(ph));
        CHECK(std::abs(std::complex<double>(*pa) - want) <= 1e-5 * (amp + 1e-30));
        CHECK(std::memcmp(pa, pb, sizeof(std::complex<float>)) == 0);
    }
    try {
        fft::Synthesizer bad(ctx, HZSDR_FMT_C64, M, g, M + 1);
        CHECK(!"hop above the channel count accepted");
    } catch (const Error &e) {
        CHECK(e.status == HZSDR_ERR_INVALID_ARGUMENT);
    }
    cm.Push(cm_in);
    cm.Reset();
    CHECK(cm.Pending().first == 0 && cm.Pending().second == 0);
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("synthesizer-cxx ok\n");
    return 0;
}

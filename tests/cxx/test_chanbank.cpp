// test_chanbank.cpp -- hzsdr::fft::ChannelBank (go-sdr_amd/cxx/hzsdr.hpp) over the C ABI in a HOST context.  An impulse
// at stream position t0 gives y[j][k] = g[t0 - jD] exp(-2 pi i k t0 / M) for the frames that cover it, which is checked
// channel by channel for M = 100 and for the odd M = 7; the channel-major result is the transpose, bit for bit, and
// NegativeFirst is ZeroFirst moved by floor(M / 2) positions, bit for bit; the plan, the table and the taps have their
// shapes.  Prints "chanbank-cxx ok" and exits 0.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "go-sdr_amd/cxx/hzsdr.hpp"

static int failures = 0;
#define CHECK(cond)                                                \
    do {                                                           \
        if (!(cond)) {                                             \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                            \
        }                                                          \
    } while (0)

static void impulse(hzsdr::Context &ctx, size_t M, size_t P, size_t D, size_t t0) {
    using namespace hzsdr;
    const size_t L = P * M, frames = 70, n = (frames - 1) * D + L + D / 2;
    std::vector<float> g(L);
    for (size_t i = 0; i < L; i++) g[i] = 0.001f * (float)(i % 97) + 0.25f;
    Buffer x(HZSDR_FMT_C64, n);
    ((std::complex<float> *)x.view.data)[t0] = {1.0f, 0.0f};
    fft::ChannelBank fm(ctx, HZSDR_FMT_C64, M, g, D, HZSDR_ORDER_ZERO_FIRST, HZSDR_CHANNELIZER_FRAME_MAJOR);
    fft::ChannelBank cm(ctx, HZSDR_FMT_C64, M, g, D, HZSDR_ORDER_ZERO_FIRST, HZSDR_CHANNELIZER_CHANNEL_MAJOR);
    fft::ChannelBank nf(ctx, HZSDR_FMT_C64, M, g, D);
    CHECK(fm.FramesFor(n) == frames && fm.Channels() == M);
    CHECK(std::get<0>(fm.Plan()) == 64 && std::get<1>(fm.Plan()) >= 2 * M && std::get<1>(fm.Plan()) % 32 == 0);
    CHECK(((std::get<2>(fm.Plan()) & HZSDR_CHANBANK_FORM_A_LDS) != 0) == (M <= 32));
    CHECK(fm.Taps() == g);
    CHECK(fm.Table(M - 1).size() == (M + 1) / 2 * 2 && fm.Table(M - 1)[0] == std::complex<float>(1.0f, 0.0f));
    const auto a = fm.Push(x.view);
    const auto b = cm.Push(x.view);
    const auto c = nf.Push(x.view);
    CHECK(a.size() == frames * M && b.size() == frames * M && c.size() == frames * M);
    CHECK(fm.Pending().first == n - frames * D && fm.Pending().second == frames);
    const double pi = 3.14159265358979323846;
    for (size_t j = 0; j < frames; j++) {
        const bool covered = t0 >= j * D && t0 < j * D + L;
        const double amp = covered ? (double)g[t0 - j * D] : 0.0;
        for (size_t k = 0; k < M; k++) {
            const double ph = -2.0 * pi * (double)((k * t0) % M) / (double)M;
            const std::complex<double> want(amp * std::cos(ph), amp * std::sin(ph));
            CHECK(std::abs(std::complex<double>(a[j * M + k]) - want) <= 1e-6 * (amp + 1e-30));
            CHECK(std::memcmp(&a[j * M + k], &b[k * frames + j], sizeof(std::complex<float>)) == 0);
            CHECK(std::memcmp(&a[j * M + k], &c[j * M + (k + M / 2) % M], sizeof(std::complex<float>)) == 0);
        }
    }
    cm.Reset();
    CHECK(cm.Pending().first == 0 && cm.Pending().second == 0);
}

int main() {
    using namespace hzsdr;
    Context ctx(0);
    impulse(ctx, 100, 3, 37, 613);
    impulse(ctx, 7, 5, 7, 201);
    impulse(ctx, 32, 2, 1, 40);
    for (size_t m : {(size_t)1, (size_t)256})
        try {
            fft::ChannelBank bad(ctx, HZSDR_FMT_C64, m, std::vector<float>(4 * m, 1.0f), 1);
            CHECK(!"a channel count outside 2 ... 255 accepted");
        } catch (const Error &e) {
            CHECK(e.status == HZSDR_ERR_INVALID_ARGUMENT);
        }
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("chanbank-cxx ok\n");
    return 0;
}

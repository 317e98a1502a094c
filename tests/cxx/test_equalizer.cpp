// test_equalizer.cpp -- hzsdr::stream::Equalizer (go-sdr_amd/cxx/hzsdr.hpp) over the C ABI in a HOST context: a fresh bank
// with mu = 0 copies its rows exactly; two pushes equal one; State / SetState carry a stream into a second object;
// PushInPlace equals Push; counts stop a row and leave zeros behind it; a live CMA bank opens the eye of QPSK symbols
// through a two-tap channel (no wrong sign in the last quarter, where the bare symbols have many); real rows;
// parameters and geometry out of range are refused.
// Prints "equalizer-cxx ok" and exits 0.
#include <cmath>
#include <complex>
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

using cf = std::complex<float>;

int main() {
    using namespace hzsdr;
    Context ctx(0);
    const size_t N = 600, R = 3, pitch = N + 4, taps = 5;
    std::vector<cf> x(R * pitch);
    for (size_t r = 0; r < R; r++)
        for (size_t n = 0; n < N; n++) x[r * pitch + n] = {(float)(1 + (n * 11 + r) % 51), -(float)(2 + (n * 7 + 3 * r) % 37)};
    {
        stream::Equalizer f(ctx, HZSDR_FMT_C64, HZSDR_EQUALIZER_CMA, taps, 2, {0.0f, 1.0f}, R);
        CHECK(f.Rows() == R && std::get<0>(f.Plan()) == 1 && std::get<1>(f.Plan()) == 256);
        CHECK(std::get<2>(f.Plan()) == HZSDR_EQUALIZER_FORM_COMPLEX);
        // the centre tap alone: y[n] = x[n - 2]
        std::vector<float> track;
        const auto y = f.Push(x.data(), N, pitch, nullptr, &track);
        CHECK(y.size() == R * N && track.size() == R * N);
        for (size_t r = 0; r < R; r++)
            for (size_t n = 0; n < N; n++) CHECK(y[r * N + n] == (n < 2 ? cf(0.0f, 0.0f) : x[r * pitch + n - 2]));
        const auto z = f.State();
        CHECK(z.size() == R * (2 * taps - 1) * 2 && z[2 * 2] == 1.0f && z[0] == 0.0f && z[2 * taps] == x[N - 1].real() && z[2 * taps + 1] == x[N - 1].imag());
        // two pushes, the second from a second object that takes the first one's state
        f.Reset();
        CHECK(f.State()[2 * 2] == 1.0f && f.State()[2 * taps] == 0.0f);
        stream::Equalizer g(ctx, HZSDR_FMT_C64, HZSDR_EQUALIZER_CMA, taps, 2, {0.0f, 1.0f}, R);
        const auto head = f.Push(x.data(), 3, pitch);
        g.SetState(f.State());
        const auto tail = g.Push(x.data() + 3, N - 3, pitch);
        CHECK(g.State() == z);
        for (size_t r = 0; r < R; r++) {
            CHECK(std::memcmp(&head[r * 3], &y[r * N], 3 * sizeof(cf)) == 0);
            CHECK(std::memcmp(&tail[r * (N - 3)], &y[r * N + 3], (N - 3) * sizeof(cf)) == 0);
        }
        // in place, and counts: row 1 stops at 100 symbols
        std::vector<cf> w = x;
        const uint32_t counts[3] = {(uint32_t)N, 100, (uint32_t)N + 7};
        f.Reset();
        f.PushInPlace(w.data(), N, pitch, counts);
        g.Reset();
        const auto c = g.Push(x.data(), N, pitch, counts);
        for (size_t r = 0; r < R; r++) {
            const size_t m = r == 1 ? 100 : N;
            CHECK(std::memcmp(&w[r * pitch], &y[r * N], m * sizeof(cf)) == 0 && std::memcmp(&c[r * N], &y[r * N], m * sizeof(cf)) == 0);
            for (size_t n = m; n < pitch; n++) CHECK(w[r * pitch + n] == x[r * pitch + n]);
            for (size_t n = m; n < N; n++) CHECK(c[r * N + n] == cf(0.0f, 0.0f));
        }
        // symbols of the other kind are refused before the library is called
        try {
            std::vector<float> real(R * N, 1.0f);
            f.Push(real.data(), N);
            CHECK(!"float symbols accepted by a complex bank");
        } catch (const std::invalid_argument &) {
        }
    }
    {
        // QPSK through h = (1, 0.6 + 0.45i): CMA with 9 taps opens the eye inside 4000 symbols
        const size_t M = 4000;
        std::vector<cf> a(M), rx(M);
        uint32_t s = 12345;
        for (size_t n = 0; n < M; n++) {
            s = s * 1664525u + 1013904223u;
            a[n] = cf((s >> 30) & 1 ? 0.70710678f : -0.70710678f, (s >> 29) & 1 ? 0.70710678f : -0.70710678f);
            rx[n] = a[n] + (n ? cf(0.6f, 0.45f) * a[n - 1] : cf(0.0f, 0.0f));
        }
        stream::Equalizer f(ctx, HZSDR_FMT_C64, HZSDR_EQUALIZER_CMA, 9, 4, {0.01f, 1.0f});
        const auto y = f.Push(rx.data(), M);
        auto wrong = [&](const std::vector<cf> &v, size_t delay) {
            size_t best = M;
            for (int q = 0; q < 4; q++) {
                size_t bad = 0;
                for (size_t n = 3 * M / 4; n < M; n++) {
                    const cf u = v[n] * std::pow(cf(0.0f, 1.0f), q);
                    bad += (u.real() > 0) != (a[n - delay].real() > 0) || (u.imag() > 0) != (a[n - delay].imag() > 0);
                }
                best = bad < best ? bad : best;
            }
            return best;
        };
        CHECK(wrong(rx, 0) > 50 && wrong(y, 4) == 0);
        f.SetParams({0.0f, 1.0f});
        const auto taps_then = f.State();
        f.Push(rx.data(), 100);
        CHECK(std::memcmp(f.State().data(), taps_then.data(), 2 * 9 * sizeof(float)) == 0);  // (mu = 0: the taps hold)
    }
    {
        // a real row, decision-directed: two taps, w = (1, 0), history 0.25: one hand-computed step
        stream::Equalizer f(ctx, HZSDR_EQUALIZER_REAL_F32, HZSDR_EQUALIZER_DD_BPSK, 2, 0, {0.5f, 0.75f});
        f.SetState({1.0f, 0.0f, 0.25f});
        const float one = 0.5f;
        std::vector<float> track;
        const auto y = f.Push(&one, 1, 0, nullptr, &track);
        CHECK(y[0] == 0.5f && track[0] == 0.0625f && f.State() == std::vector<float>({1.0625f, 0.03125f, 0.5f}) && std::get<2>(f.Plan()) == 0);
    }
    try {
        stream::Equalizer bad(ctx, HZSDR_FMT_C64, HZSDR_EQUALIZER_CMA, 9, 4, {1.5f, 1.0f});
        CHECK(!"mu above 1 accepted");
    } catch (const Error &e) {
        CHECK(e.status == HZSDR_ERR_INVALID_ARGUMENT);
    }
    try {
        stream::Equalizer bad(ctx, HZSDR_EQUALIZER_REAL_F32, HZSDR_EQUALIZER_DD_QPSK, 9, 4, {0.1f, 1.0f});
        CHECK(!"DD_QPSK accepted for real rows");
    } catch (const Error &e) {
        CHECK(e.status == HZSDR_ERR_INVALID_ARGUMENT);
    }
    try {
        stream::Equalizer bad(ctx, HZSDR_FMT_C64, HZSDR_EQUALIZER_CMA, 9, 9, {0.1f, 1.0f});
        CHECK(!"centre == taps accepted");
    } catch (const Error &e) {
        CHECK(e.status == HZSDR_ERR_INVALID_ARGUMENT);
    }
    try {
        stream::Equalizer bad(ctx, 7, HZSDR_EQUALIZER_CMA, 9, 4, {0.1f, 1.0f});
        CHECK(!"kind 7 accepted");
    } catch (const Error &e) {
        CHECK(e.status == HZSDR_ERR_FORMAT_UNKNOWN);
    }
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("equalizer-cxx ok\n");
    return 0;
}

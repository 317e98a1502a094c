// test_agc.cpp -- hzsdr::stream::Agc (go-sdr_amd/cxx/hzsdr.hpp) over the C ABI in a HOST context: with the loop held still
// the outputs are the samples times g0 = 0.5, exactly, and the track is 0.5; two pushes equal one; State / SetState carry
// a stream into a second object; PushInPlace equals Push; a live loop brings complex tones at the levels 0.01 and 50 to
// within 5 % of ref, its state being ref over the level; real rows; parameters out of range are refused.
// Prints "agc-cxx ok" and exits 0.
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
    const size_t N = 600, R = 3, pitch = N + 4;
    std::vector<cf> x(R * pitch);
    for (size_t r = 0; r < R; r++)
        for (size_t n = 0; n < N; n++) x[r * pitch + n] = {(float)(1 + (n * 11 + r) % 51), -(float)(2 + (n * 7 + 3 * r) % 37)};
    const std::vector<float> still = {1.0f, 0.0f, 0.0f, 0.0f, 0.5f, 0.25f, 4.0f};
    {
        stream::Agc f(ctx, HZSDR_FMT_C64, still, R);
        CHECK(f.Rows() == R && std::get<0>(f.Plan()) == 1 && std::get<1>(f.Plan()) == 256);
        CHECK(std::get<2>(f.Plan()) == HZSDR_AGC_FORM_COMPLEX);
        std::vector<float> track;
        const auto y = f.Push(x.data(), N, pitch, &track);
        CHECK(y.size() == R * N && track.size() == R * N && f.Position() == N);
        for (size_t r = 0; r < R; r++)
            for (size_t n = 0; n < N; n++) CHECK(y[r * N + n] == 0.5f * x[r * pitch + n] && track[r * N + n] == 0.5f);
        const auto z = f.State();
        CHECK(z.size() == R && z[0] == 0.5f && z[R - 1] == 0.5f);
        // two pushes, the second from a second object that takes the first one's state
        f.Reset();
        CHECK(f.Position() == 0 && f.State()[0] == 0.5f);
        stream::Agc g(ctx, HZSDR_FMT_C64, still, R);
        const auto head = f.Push(x.data(), 77, pitch);
        g.SetState(f.State(), f.Position());
        const auto tail = g.Push(x.data() + 77, N - 77, pitch);
        CHECK(g.Position() == N && g.State() == z);
        for (size_t r = 0; r < R; r++) {
            CHECK(std::memcmp(&head[r * 77], &y[r * N], 77 * sizeof(cf)) == 0);
            CHECK(std::memcmp(&tail[r * (N - 77)], &y[r * N + 77], (N - 77) * sizeof(cf)) == 0);
        }
        // in place
        std::vector<cf> w = x;
        f.Reset();
        f.PushInPlace(w.data(), N, pitch);
        for (size_t r = 0; r < R; r++) {
            CHECK(std::memcmp(&w[r * pitch], &y[r * N], N * sizeof(cf)) == 0);
            for (size_t n = N; n < pitch; n++) CHECK(w[r * pitch + n] == cf(0.0f, 0.0f));
        }
        // samples of the other kind are refused before the library is called
        try {
            std::vector<float> real(R * N, 1.0f);
            f.Push(real.data(), N);
            CHECK(!"float samples accepted by a complex bank");
        } catch (const std::invalid_argument &) {
        }
    }
    {
        // tones at the levels 0.01 and 50, attack 0.1, decay 0.01: settled well inside 2000 samples
        const size_t M = 2000;
        const float level[2] = {0.01f, 50.0f};
        std::vector<cf> tone(2 * M);
        for (size_t r = 0; r < 2; r++)
            for (size_t n = 0; n < M; n++) tone[r * M + n] = std::polar(level[r], (float)std::fmod(0.37 * (double)n + 1.0, 2.0 * M_PI));
        stream::Agc f(ctx, HZSDR_FMT_C64, {1.0f, 0.1f, 0.01f, 0.0f, 1.0f, 1e-4f, 1e4f}, 2);
        std::vector<float> track;
        const auto y = f.Push(tone.data(), M, 0, &track);
        for (size_t r = 0; r < 2; r++) {
            double worst = 0.0;
            for (size_t n = 3 * M / 4; n < M; n++) worst = std::fmax(worst, std::fabs(std::abs(y[r * M + n]) - 1.0));
            CHECK(worst < 0.05 && std::fabs(f.State()[r] * level[r] - 1.0) < 0.05 && track[r * M] == 1.0f);
        }
        f.SetParams({1.0f, 0.1f, 0.01f, 0.0f, 1.0f, 0.5f, 2.0f});
        CHECK(f.Position() == M && std::fabs(f.State()[0] * level[0] - 1.0) < 0.05);  // (held to the new range behind the next sample)
    }
    {
        // real rows at the level 4, rates of 0.5: g = 1, 0.5, 0.25, 0.25, ...
        const size_t M = 300;
        std::vector<float> xr(M);
        for (size_t n = 0; n < M; n++) xr[n] = n % 3 ? 4.0f : -4.0f;
        stream::Agc f(ctx, HZSDR_AGC_REAL_F32, {1.0f, 0.5f, 0.5f, 0.0f, 1.0f, 0.125f, 8.0f});
        std::vector<float> track;
        const auto y = f.Push(xr.data(), M, 0, &track);
        for (size_t n = 0; n < M; n++) {
            const float gain = n == 0 ? 1.0f : n == 1 ? 0.5f : 0.25f;
            CHECK(track[n] == gain && y[n] == gain * xr[n]);
        }
        CHECK(std::get<2>(f.Plan()) == 0 && f.State()[0] == 0.25f);
    }
    try {
        stream::Agc bad(ctx, HZSDR_FMT_C64, {1.0f, 0.6f, 0.0f, 0.0f, 1.0f, 0.5f, 2.0f});
        CHECK(!"attack above 0.5 accepted");
    } catch (const Error &e) {
        CHECK(e.status == HZSDR_ERR_INVALID_ARGUMENT);
    }
    try {
        stream::Agc bad(ctx, 7, still);
        CHECK(!"an unknown kind accepted");
    } catch (const Error &e) {
        CHECK(e.status == HZSDR_ERR_FORMAT_UNKNOWN);
    }
    try {
        stream::Agc bad(ctx, HZSDR_FMT_C64, still, 2, true);
        CHECK(!"seven values for two rows accepted");
    } catch (const std::invalid_argument &) {
    }
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("agc-cxx ok\n");
    return 0;
}

// test_carrier.cpp -- hzsdr::stream::CarrierLoop (go-sdr_amd/cxx/hzsdr.hpp) over the C ABI in a HOST context: with the loop
// held still and a quarter turn per sample the outputs are the samples times (-i)^n, exactly, and the track is 0.25; two
// pushes equal one; State / SetState carry a stream into a second object; PushInPlace equals Push; a tone a little off
// frequency is pulled in: the track ends at its offset and the output at a constant phase; parameters out of range are
// refused.  Prints "carrier-cxx ok" and exits 0.
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

static cf turned(cf x, size_t n) {
    switch (n % 4) {
    case 0: return x;
    case 1: return {x.imag(), -x.real()};
    case 2: return {-x.real(), -x.imag()};
    default: return {-x.imag(), x.real()};
    }
}

int main() {
    using namespace hzsdr;
    Context ctx(0);
    const size_t N = 600, R = 3, pitch = N + 4;
    std::vector<cf> x(R * pitch);
    for (size_t r = 0; r < R; r++)
        for (size_t n = 0; n < N; n++) x[r * pitch + n] = {(float)(1 + (n * 11 + r) % 51), -(float)(2 + (n * 7 + 3 * r) % 37)};
    const std::vector<float> still = {0.0f, 0.0f, 0.25f, 0.25f, 0.25f};
    {
        stream::CarrierLoop f(ctx, HZSDR_CARRIER_BPSK, still, R);
        CHECK(f.Rows() == R && std::get<0>(f.Plan()) == 1 && std::get<1>(f.Plan()) == 256);
        CHECK(std::get<2>(f.Plan()) == HZSDR_CARRIER_BPSK * HZSDR_CARRIER_FORM_MODE);
        std::vector<float> track;
        const auto y = f.Push(x.data(), N, pitch, &track);
        CHECK(y.size() == R * N && track.size() == R * N && f.Position() == N);
        for (size_t r = 0; r < R; r++)
            for (size_t n = 0; n < N; n++) CHECK(y[r * N + n] == turned(x[r * pitch + n], n) && track[r * N + n] == 0.25f);
        const auto z = f.State();
        CHECK(z.size() == 2 * R && z[0] == (uint32_t)(N << 30) && z[1] == 1u << 30);
        // two pushes, the second from a second object that takes the first one's state
        f.Reset();
        CHECK(f.Position() == 0 && f.State()[0] == 0 && f.State()[1] == 1u << 30);
        stream::CarrierLoop g(ctx, HZSDR_CARRIER_BPSK, still, R);
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
    }
    {
        // a tone 0.003 cycles per sample off, a loop of 0.02: pulled in well inside 4000 samples
        const size_t M = 4000;
        const double off = 0.003, bw = 0.02, zeta = 0.7071, tn = bw / (zeta + 1.0 / (4.0 * zeta)), d = 1.0 + 2.0 * zeta * tn + tn * tn;
        const float alpha = (float)(4.0 * zeta * tn / d / (2.0 * M_PI)), beta = (float)(4.0 * tn * tn / d / (2.0 * M_PI));
        std::vector<cf> tone(M);
        for (size_t n = 0; n < M; n++) tone[n] = std::polar(1.0f, (float)std::fmod(2.0 * M_PI * off * (double)n + 1.0, 2.0 * M_PI));
        stream::CarrierLoop f(ctx, HZSDR_CARRIER_TONE, {alpha, beta, 0.0f, -0.01f, 0.01f});
        std::vector<float> track;
        const auto y = f.Push(tone.data(), M, 0, &track);
        double mean = 0.0, worst = 0.0;
        for (size_t n = 3 * M / 4; n < M; n++) {
            mean += track[n] / (double)(M / 4);
            worst = std::fmax(worst, std::fabs(std::arg(y[n])));
        }
        CHECK(std::fabs(mean - off) < 1e-6 && worst < 1e-3);
        CHECK(std::fabs((double)(int32_t)f.State()[1] / 4294967296.0 - off) < 1e-6);
        // the same loop, one set per row, by SetParams: the form cannot be told from the values, the count can
        f.SetParams({alpha, beta, 0.0f, -0.02f, 0.02f});
        CHECK(f.Position() == M);
    }
    try {
        stream::CarrierLoop bad(ctx, HZSDR_CARRIER_TONE, {0.2f, 0.0f, 0.0f, 0.0f, 0.0f});
        CHECK(!"alpha above 0.125 accepted");
    } catch (const Error &e) {
        CHECK(e.status == HZSDR_ERR_INVALID_ARGUMENT);
    }
    try {
        stream::CarrierLoop bad(ctx, 7, still);
        CHECK(!"an unknown mode accepted");
    } catch (const Error &e) {
        CHECK(e.status == HZSDR_ERR_INVALID_ARGUMENT);
    }
    try {
        stream::CarrierLoop bad(ctx, HZSDR_CARRIER_TONE, still, 2, true);
        CHECK(!"five values for two rows accepted");
    } catch (const std::invalid_argument &) {
    }
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("carrier-cxx ok\n");
    return 0;
}

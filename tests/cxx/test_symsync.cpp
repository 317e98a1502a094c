// test_symsync.cpp -- hzsdr::stream::SymbolSync (go-sdr_amd/cxx/hzsdr.hpp) over the C ABI in a HOST context: with the loop
// held still, 4 samples per symbol read samples out and 5 read midpoints of the cubic; three rows with clocks of their
// own give three counts; two pushes equal one; a complex row is two real ones; State / SetState carry a stream into a
// second object; parameters that crowd two strobes into a sample are refused.  Prints "symsync-cxx ok" and exits 0.
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

int main() {
    using namespace hzsdr;
    Context ctx(0);
    const size_t N = 600;
    std::vector<float> x(N);
    // integers of one sign, 60 ... 110: no symbol below is a small difference of large terms
    for (size_t n = 0; n < N; n++) x[n] = (float)(60 + (n * 11) % 51);
    {
        stream::SymbolSync f(ctx, HZSDR_SYMSYNC_REAL_F32, {4.0f, 0.0f, 0.0f, 0.0f});
        CHECK(f.Rows() == 1 && std::get<0>(f.Plan()) == 1 && std::get<1>(f.Plan()) == 256 && std::get<2>(f.Plan()) == 0);
        CHECK(f.MaxSymbols(N) == N / 4 + 2 && f.MaxSymbols(0) == 0);
        const auto y = f.Push(x.data(), N);
        CHECK(y.size() == 1 && y[0].size() == N / 4 && f.Position() == N);
        for (size_t k = 0; k < y[0].size(); k++) CHECK(y[0][k] == x[4 * k]);
        // two pushes, the second from a second object that takes the first one's state
        f.Reset();
        stream::SymbolSync g(ctx, HZSDR_SYMSYNC_REAL_F32, {4.0f, 0.0f, 0.0f, 0.0f});
        const auto head = f.Push(x.data(), 77);
        const std::vector<float> z = f.State();
        CHECK(z.size() == 8 && z[1] == 2.0f);
        g.SetState(z, f.Position());
        const auto tail = g.Push(x.data() + 77, N - 77);
        CHECK(g.Position() == N && head[0].size() + tail[0].size() == y[0].size());
        CHECK(std::memcmp(head[0].data(), y[0].data(), head[0].size() * 4) == 0);
        CHECK(std::memcmp(tail[0].data(), y[0].data() + head[0].size(), tail[0].size() * 4) == 0);
    }
    {
        // 5 samples per symbol: symbol k is the cubic half way between x[5 k] and x[5 k + 1]
        stream::SymbolSync f(ctx, HZSDR_SYMSYNC_REAL_F32, {5.0f, 0.0f, 0.0f, 0.0f});
        const auto y = f.Push(x.data(), N);
        CHECK(y[0].size() == N / 5);
        for (size_t k = 1; k < y[0].size(); k++) {
            const size_t i = 5 * k;
            const double want = (-(double)x[i - 1] + 9.0 * x[i] + 9.0 * x[i + 1] - (double)x[i + 2]) / 16.0;
            // within 4 float32 ulps of its own value (31 ... 128 here)
            const float w = (float)want;
            CHECK(want > 31.0 && std::fabs(y[0][k] - want) <= 4.0 * (std::nextafter(w, 1e9f) - w));
        }
    }
    {
        // three rows, a clock each: 4, 8 and 16 samples per symbol
        const size_t R = 3, pitch = N + 4;
        std::vector<float> rows(R * pitch, 0.0f), par;
        for (size_t r = 0; r < R; r++) {
            std::memcpy(&rows[r * pitch], x.data(), N * 4);
            par.insert(par.end(), {(float)(4 << r), 0.0f, 0.0f, 0.0f});
        }
        stream::SymbolSync f(ctx, HZSDR_SYMSYNC_REAL_F32, par, R, true);
        CHECK(std::get<2>(f.Plan()) == HZSDR_SYMSYNC_FORM_PER_ROW);
        const auto y = f.Push(rows.data(), N, pitch);
        CHECK(y.size() == R);
        for (size_t r = 0; r < R; r++) {
            const size_t sps = (size_t)4 << r;
            CHECK(y[r].size() == (N - 1 - sps / 2) / sps + 1);  // symbol k is found at sample sps k + sps / 2
            for (size_t k = 0; k < y[r].size(); k++) CHECK(y[r][k] == x[sps * k + sps / 2 - 2]);
        }
    }
    {
        // a complex row with the loop held still is two real rows
        std::vector<std::complex<float>> c(N);
        std::vector<float> im(N);
        for (size_t n = 0; n < N; n++) c[n] = {x[n], im[n] = x[N - 1 - n]};
        stream::SymbolSync fc(ctx, HZSDR_FMT_C64, {4.0f, 0.0f, 0.0f, 0.0f}), fi(ctx, HZSDR_SYMSYNC_REAL_F32, {4.0f, 0.0f, 0.0f, 0.0f});
        CHECK(std::get<2>(fc.Plan()) == HZSDR_SYMSYNC_FORM_COMPLEX && fc.State().size() == 13);
        const auto y = fc.PushComplex(c.data(), N);
        const auto yi = fi.Push(im.data(), N);
        CHECK(y[0].size() == N / 4 && yi[0].size() == N / 4);
        for (size_t k = 0; k < y[0].size(); k++) CHECK(y[0][k].real() == x[4 * k] && y[0][k].imag() == yi[0][k]);
    }
    try {
        stream::SymbolSync bad(ctx, HZSDR_SYMSYNC_REAL_F32, {2.25f, 0.0f, 0.13f, 0.0f});
        CHECK(!"two strobes in a sample accepted");
    } catch (const Error &e) {
        CHECK(e.status == HZSDR_ERR_INVALID_ARGUMENT);
    }
    try {
        stream::SymbolSync bad(ctx, HZSDR_FMT_I16, {4.0f, 0.0f, 0.0f, 0.0f});
        CHECK(!"int16 rows accepted");
    } catch (const Error &e) {
        CHECK(e.status == HZSDR_ERR_FORMAT_UNKNOWN);
    }
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("symsync-cxx ok\n");
    return 0;
}

// test_iir.cpp -- hzsdr::stream::IirBank (go-sdr_amd/cxx/hzsdr.hpp) over the C ABI in a HOST context: the impulse response
// of a one-pole section with a pole at 0.5 is 2^-n exactly, through the denormals to +0; three rows with cascades of
// their own give three such responses; two pushes equal one; a complex row is two real ones; State / SetState carry a
// stream into a second object.  Prints "iir-cxx ok" and exits 0.
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
    const size_t N = 200;
    {
        // y[n] = x[n] + 0.5 y[n - 1]
        stream::IirBank f(ctx, HZSDR_IIR_REAL_F32, {1.0f, 0.0f, 0.0f, -0.5f, 0.0f});
        CHECK(f.Rows() == 1 && f.Sections() == 1 && std::get<1>(f.Plan()) == 256 && std::get<2>(f.Plan()) == 0);
        std::vector<float> x(N, 0.0f);
        x[0] = 1.0f;
        const std::vector<float> y = f.Push(x.data(), N);
        CHECK(y.size() == N && f.Position() == N);
        for (size_t n = 0; n < N; n++) {
            const float want = n < 150 ? std::ldexp(1.0f, -(int)n) : 0.0f;
            CHECK(std::memcmp(&y[n], &want, 4) == 0);
        }
        CHECK(y[149] > 0.0f && y[149] < 1.2e-38f);  // a denormal, kept
    }
    {
        // three rows, a pole each: 0.5, -0.5 and 0.25; the second push continues the first
        const size_t R = 3, pitch = N + 4;
        const float pole[R] = {0.5f, -0.5f, 0.25f};
        std::vector<float> sec;
        for (size_t r = 0; r < R; r++) sec.insert(sec.end(), {1.0f, 0.0f, 0.0f, -pole[r], 0.0f});
        stream::IirBank f(ctx, HZSDR_IIR_REAL_F32, sec, R, true);
        CHECK(std::get<2>(f.Plan()) == HZSDR_IIR_FORM_PER_ROW && f.Sections() == 1);
        std::vector<float> x(R * pitch, 0.0f);
        for (size_t r = 0; r < R; r++) x[r * pitch] = 3.0f;
        const std::vector<float> a = f.Push(x.data(), 70, pitch), b = f.Push(x.data() + 70, N - 70, pitch);
        CHECK(a.size() == R * 70 && b.size() == R * (N - 70) && f.Position() == N);
        for (size_t r = 0; r < R; r++) {
            float want = 3.0f;
            for (size_t n = 0; n < 40; n++, want *= pole[r]) CHECK(a[r * 70 + n] == want);
        }
        f.Reset();
        const std::vector<float> whole = f.Push(x.data(), N, pitch);
        for (size_t r = 0; r < R; r++) {
            CHECK(std::memcmp(&whole[r * N], &a[r * 70], 70 * 4) == 0);
            CHECK(std::memcmp(&whole[r * N + 70], &b[r * (N - 70)], (N - 70) * 4) == 0);
        }
    }
    {
        // a complex row is two real rows; the state moves a stream into a second object
        const std::vector<float> sec = {0.2f, 0.3f, 0.1f, -0.9f, 0.5f, 1.0f, -1.0f, 0.0f, -0.8f, 0.0f};
        std::vector<std::complex<float>> x(N);
        std::vector<float> re(N), im(N);
        for (size_t n = 0; n < N; n++) x[n] = {re[n] = std::sin(0.1f * n), im[n] = 0.25f + std::cos(0.37f * n)};
        stream::IirBank fc(ctx, HZSDR_FMT_C64, sec), fr(ctx, HZSDR_IIR_REAL_F32, sec), fi(ctx, HZSDR_IIR_REAL_F32, sec);
        CHECK(std::get<2>(fc.Plan()) == HZSDR_IIR_FORM_COMPLEX && fc.Sections() == 2);
        const std::vector<std::complex<float>> y = fc.PushComplex(x.data(), N);
        const std::vector<float> yr = fr.Push(re.data(), N), yi = fi.Push(im.data(), N);
        for (size_t n = 0; n < N; n++) CHECK(y[n].real() == yr[n] && y[n].imag() == yi[n]);
        stream::IirBank first(ctx, HZSDR_IIR_REAL_F32, sec), second(ctx, HZSDR_IIR_REAL_F32, sec);
        const std::vector<float> head = first.Push(re.data(), 77);
        const std::vector<float> z = first.State();
        CHECK(z.size() == 4);
        second.SetState(z, first.Position());
        const std::vector<float> tail = second.Push(re.data() + 77, N - 77);
        CHECK(second.Position() == N);
        CHECK(std::memcmp(head.data(), yr.data(), 77 * 4) == 0 && std::memcmp(tail.data(), yr.data() + 77, (N - 77) * 4) == 0);
    }
    try {
        stream::IirBank bad(ctx, HZSDR_IIR_REAL_F32, std::vector<float>(45, 0.5f));
        CHECK(!"nine sections accepted");
    } catch (const Error &e) {
        CHECK(e.status == HZSDR_ERR_INVALID_ARGUMENT);
    }
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("iir-cxx ok\n");
    return 0;
}

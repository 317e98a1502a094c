// demod_ref.cpp -- the bit-exact restatement of the demodulator bank (include/hzsdr_demod.h) over csrc/hz_demod_math.h,
// the header the kernel evaluates: built with g++ -O2 -ffp-contract=off, it computes the bits the device must produce.
//
//   demod_ref sweep             the error E of demod_angle against float64 atan2 of the same float32 pair: x = 1 with y
//                               every float32 in [0, 1] (every ratio), carried into all eight octants; both axes and the
//                               zeros; 2^24 seeded pairs with exponents over the whole range.  Prints "E <value>".
//   demod_ref run CASES OUT     CASES: records of int32 mode, D, Q, int64 N, Q float32 taps, N complex64 samples (already
//                               converted).  OUT: per record int64 count, then the count float32 outputs of the whole
//                               stream (pushes and flush: m < ceil((N - 1 + Q) / D), nothing for N = 0).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "hz_demod_math.h"

using namespace hz::dm;

static float bits_f(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}

static uint64_t splitmix(uint64_t &s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct Worst {
    double e = 0;
    float y = 0, x = 0;
    void take(float yy, float xx) { take(yy, xx, atan2((double)yy, (double)xx)); }
    void take(float yy, float xx, double want) {
        const double v = fabs((double)demod_angle(yy, xx) - want);
        if (!(v <= e)) e = v, y = yy, x = xx;  // (a NaN is taken, and reported)
    }
    void merge(const Worst &o) {
        if (!(o.e <= e)) *this = o;
    }
};

static int sweep() {
    const unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    const uint32_t one = 0x3f800000u;  // y = bits 0 ... one: every float32 in [0, 1]
    std::vector<Worst> w(nt);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; t++)
        th.emplace_back([&, t] {
            Worst &m = w[t];
            for (uint64_t b = t; b <= one; b += nt) {
                const float y = bits_f((uint32_t)b);
                // the eight octants of the ratio, (+-1, +-y) and (+-y, +-1): one float64 atan2 and its reflections (exact
                // identities; their float64 rounding, 4e-16, is nine orders below E)
                const double a = atan2((double)y, 1.0), pi = 3.14159265358979323846, h = pi / 2;
                m.take(y, 1.0f, a), m.take(-y, 1.0f, -a), m.take(y, -1.0f, pi - a), m.take(-y, -1.0f, a - pi);
                m.take(1.0f, y, h - a), m.take(1.0f, -y, h + a), m.take(-1.0f, y, a - h), m.take(-1.0f, -y, -h - a);
            }
            uint64_t s = 0x5DEECE66Dull + t;
            for (uint64_t k = t; k < (1ull << 24); k += nt) {
                // sign, exponent (0: denormals ... 254) and fraction at random, of both
                uint64_t r = splitmix(s);
                const uint32_t a = (uint32_t)r, c = (uint32_t)(r >> 32);
                const uint32_t ea = (a >> 23) & 0xff, ec = (c >> 23) & 0xff;
                m.take(bits_f(ea == 255 ? a & ~(1u << 23) : a), bits_f(ec == 255 ? c & ~(1u << 23) : c));
            }
        });
    for (auto &x : th) x.join();
    Worst all;
    for (auto &m : w) all.merge(m);
    // both axes and the zeros, at a few magnitudes
    const float mags[] = {bits_f(1), 1e-38f, 1e-20f, 1.0f, 3.0f, 1e20f, 3e38f};
    for (float v : mags)
        for (float z : {0.0f, -0.0f}) all.take(z, v), all.take(z, -v), all.take(v, z), all.take(-v, z);
    int bad = 0;
    for (float y : {0.0f, -0.0f})
        for (float x : {0.0f, -0.0f}) {
            const float r = demod_angle(y, x);
            uint32_t u;
            memcpy(&u, &r, 4);
            bad += u != 0;
        }
    if (bad) {
        printf("angle(+-0, +-0) is not +0\n");
        return 1;
    }
    printf("worst pair y=%a x=%a\n", all.y, all.x);
    printf("E %.6e\n", all.e);
    return 0;
}

static int run(const char *cases, const char *outp) {
    FILE *f = fopen(cases, "rb"), *o = fopen(outp, "wb");
    if (!f || !o) return 2;
    int32_t hd[3];
    while (fread(hd, 4, 3, f) == 3) {
        const int mode = hd[0];
        const int64_t D = hd[1], Q = hd[2];
        int64_t N;
        if (fread(&N, 8, 1, f) != 1) return 3;
        std::vector<float> h(Q);
        std::vector<c32> x(N);
        if (fread(h.data(), 4, Q, f) != (size_t)Q || fread(x.data(), 8, N, f) != (size_t)N) return 3;
        std::vector<float> d(N);
        for (int64_t n = 0; n < N; n++) d[n] = demod_detect(mode, x[n], n ? x[n - 1] : c32{0.0f, 0.0f});
        const int64_t count = N ? (N - 1 + Q + D - 1) / D : 0;
        std::vector<float> y(count);
        for (int64_t m = 0; m < count; m++) {
            float acc = 0.0f;
            for (int64_t q = 0; q < Q; q++) {
                const int64_t n = m * D - q;
                acc = demod_term(acc, h[q], n >= 0 && n < N ? d[n] : 0.0f);
            }
            y[m] = acc;
        }
        fwrite(&count, 8, 1, o);
        fwrite(y.data(), 4, count, o);
    }
    fclose(f);
    return fclose(o) ? 4 : 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "sweep")) return sweep();
    if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
    fprintf(stderr, "usage: demod_ref sweep | demod_ref run CASES OUT\n");
    return 64;
}

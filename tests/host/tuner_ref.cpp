// tuner_ref.cpp -- the bit-exact restatement of the tuner bank (include/hzsdr_tuner.h): steps 2 and 3 of the contract
// written out as float32 fused steps over csrc/hz_tuner_math.h, the header the kernel takes cmul and the phase split
// from.  Built with g++ -O2 -ffp-contract=off, it computes the bits the device must produce.
//
//   tuner_ref run CASES OUT
//       CASES: records of int32 K, D, Q, given; int64 N; K uint32 words; Q float32 taps; then, where given = 1, the
//              operands as read out of the library -- K * Qp complex64 modulated taps, the tables T2 (2048), T1 (2048),
//              T0 (1024) -- and where given = 0 nothing: the program makes them by its OWN copy of step 1 (below, not
//              the header's); then N complex64 samples (already converted).
//       OUT:   per record int64 count, then K rows of count complex64 outputs of the whole stream (pushes and flush:
//              m < ceil((N - 1 + Q) / D), nothing for N = 0), then the K * Qp modulated taps and the 5120 table entries
//              that were used.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "hz_tuner_math.h"

using namespace hz::tn;

// ---- step 1, this program's own copy -------------------------------------------------------------------
// cos and sin of 2 pi u / 2^32 in float64 behind an exact reduction of the integer phase to [0, pi/4]
static void unit(uint32_t u, double *c, double *s) {
    const double two_pi = 6.283185307179586476925286766559;
    const uint32_t quad = u >> 30, r = u << 2 >> 2;
    const bool mirror = r > (1u << 29);
    const double t = (double)(mirror ? (1u << 30) - r : r) * (two_pi / 4294967296.0);
    double a = cos(t), b = sin(t);
    if (r == 0) a = 1.0, b = 0.0;
    const double cr = mirror ? b : a, sr = mirror ? a : b;
    const double cs[4] = {cr, 0.0 - sr, 0.0 - cr, sr}, sn[4] = {sr, cr, 0.0 - sr, 0.0 - cr};
    *c = cs[quad], *s = sn[quad];
}

static c32 own_tap(float h, uint32_t w, uint32_t q) {
    double c, s;
    unit((uint32_t)((uint64_t)w * q), &c, &s);
    return c32{(float)((double)h * c), (float)((double)h * s)};
}

static c32 own_table(uint32_t phase) {
    double c, s;
    unit(phase, &c, &s);
    return c32{(float)c, (float)(0.0 - s)};
}

static int run(const char *cases, const char *outp) {
    FILE *f = fopen(cases, "rb"), *o = fopen(outp, "wb");
    if (!f || !o) return 2;
    int32_t hd[4];
    while (fread(hd, 4, 4, f) == 4) {
        const int64_t K = hd[0], D = hd[1], Q = hd[2], Qp = (Q + 1) / 2 * 2;
        const bool given = hd[3] != 0;
        int64_t N;
        if (fread(&N, 8, 1, f) != 1) return 3;
        std::vector<uint32_t> w(K);
        std::vector<float> h(Qp, 0.0f);
        std::vector<c32> G(K * Qp), tab(kTables), x(N);
        if (fread(w.data(), 4, K, f) != (size_t)K || fread(h.data(), 4, Q, f) != (size_t)Q) return 3;
        if (given) {
            if (fread(G.data(), 8, K * Qp, f) != (size_t)(K * Qp) || fread(tab.data(), 8, kTables, f) != kTables) return 3;
        } else {
            for (int64_t k = 0; k < K; k++)
                for (int64_t q = 0; q < Qp; q++) G[k * Qp + q] = q < Q ? own_tap(h[q], w[k], (uint32_t)q) : c32{0.0f, 0.0f};
            for (uint32_t i = 0; i < kT2; i++) tab[i] = own_table(i << 21);
            for (uint32_t i = 0; i < kT1; i++) tab[kT2 + i] = own_table(i << 10);
            for (uint32_t i = 0; i < kT0; i++) tab[kT2 + kT1 + i] = own_table(i);
        }
        if (fread(x.data(), 8, N, f) != (size_t)N) return 3;
        const int64_t count = N ? (N - 1 + Q + D - 1) / D : 0;
        std::vector<c32> y(K * count);
        for (int64_t k = 0; k < K; k++) {
            const uint32_t step = w[k] * (uint32_t)D;  // (w D) mod 2^32
            uint32_t p = 0;                            // the running phase word of output m
            for (int64_t m = 0; m < count; m++, p += step) {
                c32 acc{0.0f, 0.0f};
                for (int64_t q = 0; q < Qp; q++) {  // ALL Qp terms, out-of-stream samples as +0
                    const int64_t n = m * D - q;
                    acc = tuner_term(acc, G[k * Qp + q], n >= 0 && n < N ? x[n] : c32{0.0f, 0.0f});
                }
                y[k * count + m] = tuner_rotate(acc, p, tab.data());
            }
        }
        fwrite(&count, 8, 1, o);
        fwrite(y.data(), 8, K * count, o);
        fwrite(G.data(), 8, K * Qp, o);
        fwrite(tab.data(), 8, kTables, o);
    }
    fclose(f);
    return fclose(o) ? 4 : 0;
}

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
    fprintf(stderr, "usage: tuner_ref run CASES OUT\n");
    return 64;
}

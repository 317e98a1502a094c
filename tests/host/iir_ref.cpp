// iir_ref.cpp -- the bit-exact restatement of the IIR bank (include/hzsdr_iir.h) over csrc/hz_iir_math.h, the header the
// kernel evaluates: built with g++ -O2 -ffp-contract=off, it computes the bits the device must produce.
//
//   iir_ref run CASES OUT     CASES: records of int32 S, planes (1 real, 2 complex), segments, per_row (0 / 1), int64 R, N;
//                             then per segment int64 start and its coefficients (S * 5 float32, or R * S * 5 when
//                             per_row): the cascade in force from sample `start` on (the first segment starts at 0; a
//                             later one is a hzsdr_iir_set_sections between two pushes); then R rows of N samples,
//                             float32 or (re, im) pairs, already converted.
//                             OUT: per record the R * N outputs in the same layout, then the state behind them:
//                             R * S * 2 * planes float32 -- row, section, z1 / z2, re / im.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "hz_iir_math.h"

using namespace hz::im;

static int run(const char *cases, const char *outp) {
    FILE *f = fopen(cases, "rb"), *o = fopen(outp, "wb");
    if (!f || !o) return 2;
    int32_t hd[4];
    while (fread(hd, 4, 4, f) == 4) {
        const int S = hd[0], PL = hd[1], segs = hd[2], per_row = hd[3];
        int64_t dim[2];
        if (fread(dim, 8, 2, f) != 2) return 3;
        const int64_t R = dim[0], N = dim[1];
        if (S < 1 || S > 8 || PL < 1 || PL > 2 || segs < 1 || R < 1 || N < 0) return 5;
        const size_t per = (size_t)(per_row ? R : 1) * S * kCoefs;
        std::vector<int64_t> start(segs);
        std::vector<std::vector<float>> coef(segs, std::vector<float>(per));
        for (int g = 0; g < segs; g++)
            if (fread(&start[g], 8, 1, f) != 1 || fread(coef[g].data(), 4, per, f) != per) return 3;
        std::vector<float> x((size_t)R * N * PL), z((size_t)R * S * 2 * PL, 0.0f);
        if (fread(x.data(), 4, x.size(), f) != x.size()) return 3;
        for (int64_t r = 0; r < R; r++)
            for (int p = 0; p < PL; p++) {
                int g = 0;
                for (int64_t n = 0; n < N; n++) {
                    while (g + 1 < segs && start[g + 1] <= n) g++;
                    const float *c = coef[g].data() + (per_row ? (size_t)r * S * kCoefs : 0);
                    float v = x[((size_t)r * N + n) * PL + p];
                    for (int s = 0; s < S; s++) {
                        float *zs = &z[(((size_t)r * S + s) * 2) * PL + p];
                        v = iir_step(c + s * kCoefs, v, zs[0], zs[PL]);
                    }
                    x[((size_t)r * N + n) * PL + p] = v;
                }
            }
        fwrite(x.data(), 4, x.size(), o);
        fwrite(z.data(), 4, z.size(), o);
    }
    fclose(f);
    return fclose(o) ? 4 : 0;
}

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
    fprintf(stderr, "usage: iir_ref run CASES OUT\n");
    return 64;
}

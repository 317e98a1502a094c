// symsync_ref.cpp -- the bit-exact restatement of the symbol-timing recovery bank (include/hzsdr_symsync.h) over
// csrc/hz_symsync_math.h, the header the kernel evaluates, with the constants of csrc/hz_symsync_plan.h: built with
// g++ -O2 -ffp-contract=off, it computes the bits the device must produce.
//
//   symsync_ref run CASES OUT   CASES: records of int32 planes (1 real, 2 complex), segments, per_row (0 / 1), has_state
//                               (0 / 1), int64 R, N; then per segment int64 start and its parameters (4 float32 sps,
//                               limit, g_mu, g_omega, or R * 4 when per_row): the parameters in force from sample `start`
//                               on (the first segment starts at 0; a later one is a hzsdr_symsync_set_params between two
//                               pushes); then, when has_state, the state to start from (hzsdr_symsync_get_state's layout:
//                               R * 8 float32, or R * 13 for complex rows), else the initial state; then R rows of N
//                               samples, float32 or (re, im) pairs.
//                               OUT: per record R uint32 counts; R rows of N / 2 + 2 symbols in the input's layout, +0
//                               behind a row's count; the state behind them; one uint32, the number of steps that left
//                               the counter below 0 (the definition says none).
//   symsync_ref derive SETS OUT SETS: sets of 4 float32.  OUT: per set int32 accepted (0 / 1), float32 h0, hmin, hmax,
//                               float64 hmin - g_mu.
//   symsync_ref bound N AMIN    prints max_symbols(N, AMIN).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hz_symsync_math.h"
#include "hz_symsync_plan.h"

using namespace hz;

template <int PL>
static uint32_t row(const std::vector<std::vector<float>> &par, const std::vector<int64_t> &start, int per_row, int64_t r, int64_t N, const float *x,
                    float *z, float *y, uint32_t *count) {
    sm::State<PL> s{};
    s.c = z[sp::kStC], s.h = z[sp::kStH], s.flag = z[sp::kStFlag] != 0.0f ? 1u : 0u;
    for (int p = 0; p < PL; p++) {
        s.yp[p] = z[sp::state_index(0, sp::kStYp, p, PL)], s.ym[p] = z[sp::state_index(0, sp::kStYm, p, PL)];
        s.x1[p] = z[sp::state_index(0, sp::kStX1, p, PL)], s.x2[p] = z[sp::state_index(0, sp::kStX2, p, PL)];
        s.x3[p] = z[sp::state_index(0, sp::kStX3, p, PL)];
    }
    uint32_t k = 0, negative = 0;
    size_t g = 0;
    sm::Loop loop = sp::derive(par[0].data() + (per_row ? r * sp::kParams : 0)).loop;
    for (int64_t n = 0; n < N; n++) {
        while (g + 1 < par.size() && start[g + 1] <= n) loop = sp::derive(par[++g].data() + (per_row ? r * sp::kParams : 0)).loop;
        float v[PL];
        if (sm::sync_step<PL>(s, loop, x + n * PL, v)) {
            for (int p = 0; p < PL; p++) y[(size_t)k * PL + p] = v[p];
            k++;
        }
        if (s.c < 0.0f) negative++;
    }
    z[sp::kStC] = s.c, z[sp::kStH] = s.h, z[sp::kStFlag] = s.flag ? 1.0f : 0.0f;
    for (int p = 0; p < PL; p++) {
        z[sp::state_index(0, sp::kStYp, p, PL)] = s.yp[p], z[sp::state_index(0, sp::kStYm, p, PL)] = s.ym[p];
        z[sp::state_index(0, sp::kStX1, p, PL)] = s.x1[p], z[sp::state_index(0, sp::kStX2, p, PL)] = s.x2[p];
        z[sp::state_index(0, sp::kStX3, p, PL)] = s.x3[p];
    }
    *count = k;
    return negative;
}

static int run(const char *cases, const char *outp) {
    FILE *f = fopen(cases, "rb"), *o = fopen(outp, "wb");
    if (!f || !o) return 2;
    int32_t hd[4];
    while (fread(hd, 4, 4, f) == 4) {
        const int PL = hd[0], segs = hd[1], per_row = hd[2], has_state = hd[3];
        int64_t dim[2];
        if (fread(dim, 8, 2, f) != 2) return 3;
        const int64_t R = dim[0], N = dim[1];
        if (PL < 1 || PL > 2 || segs < 1 || R < 1 || N < 0) return 5;
        const size_t per = (size_t)(per_row ? R : 1) * sp::kParams, zrow = sp::state_row_floats(PL), cap = (size_t)N / 2 + 2;
        std::vector<int64_t> start(segs);
        std::vector<std::vector<float>> par(segs, std::vector<float>(per));
        for (int g = 0; g < segs; g++) {
            if (fread(&start[g], 8, 1, f) != 1 || fread(par[g].data(), 4, per, f) != per) return 3;
            for (size_t q = 0; q < per; q += sp::kParams)
                if (sp::check_params(par[g].data() + q)) return 6;
        }
        std::vector<float> z((size_t)R * zrow, 0.0f), x((size_t)R * N * PL), y((size_t)R * cap * PL, 0.0f);
        if (has_state) {
            if (fread(z.data(), 4, z.size(), f) != z.size()) return 3;
        } else {
            for (int64_t r = 0; r < R; r++) z[r * zrow + sp::kStH] = sp::derive(par[0].data() + (per_row ? r * sp::kParams : 0)).h0;
        }
        if (fread(x.data(), 4, x.size(), f) != x.size()) return 3;
        std::vector<uint32_t> counts(R);
        uint32_t negative = 0;
        for (int64_t r = 0; r < R; r++) {
            const float *xr = x.data() + (size_t)r * N * PL;
            float *zr = z.data() + r * zrow, *yr = y.data() + (size_t)r * cap * PL;
            negative += PL == 2 ? row<2>(par, start, per_row, r, N, xr, zr, yr, &counts[r]) : row<1>(par, start, per_row, r, N, xr, zr, yr, &counts[r]);
        }
        fwrite(counts.data(), 4, counts.size(), o);
        fwrite(y.data(), 4, y.size(), o);
        fwrite(z.data(), 4, z.size(), o);
        fwrite(&negative, 4, 1, o);
    }
    fclose(f);
    return fclose(o) ? 4 : 0;
}

static int derive(const char *sets, const char *outp) {
    FILE *f = fopen(sets, "rb"), *o = fopen(outp, "wb");
    if (!f || !o) return 2;
    float q[4];
    while (fread(q, 4, 4, f) == 4) {
        const int32_t ok = sp::check_params(q) == nullptr;
        // (derive is defined for any four values; what it gives for refused ones is not used)
        const sp::Derived d = sp::derive(q);
        const float v[3] = {d.h0, d.loop.hmin, d.loop.hmax};
        const double least = sp::least_advance(q);
        fwrite(&ok, 4, 1, o), fwrite(v, 4, 3, o), fwrite(&least, 8, 1, o);
    }
    fclose(f);
    return fclose(o) ? 4 : 0;
}

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "derive")) return derive(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "bound")) {
        printf("%llu\n", (unsigned long long)sp::max_symbols(strtoull(argv[2], nullptr, 10), strtod(argv[3], nullptr)));
        return 0;
    }
    fprintf(stderr, "usage: symsync_ref run CASES OUT | derive SETS OUT | bound N AMIN\n");
    return 64;
}

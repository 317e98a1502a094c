// agc_ref.cpp -- the bit-exact restatement of the AGC bank (include/hzsdr_agc.h) over csrc/hz_agc_math.h, the header
// the kernel evaluates, with the constants of csrc/hz_agc_plan.h: built with g++ -O2 -ffp-contract=off, it computes the
// bits the device must produce.
//
//   agc_ref run CASES OUT      CASES: records of int32 complex (0 / 1), segments, per_row (0 / 1), has_state (0 / 1),
//                              int64 R, N; then per segment int64 start and its parameters (7 float32 ref, attack,
//                              decay, floor, g0, gmin, gmax, or R * 7 when per_row): the parameters in force from
//                              sample `start` on (the first segment starts at 0; a later one is a hzsdr_agc_set_params
//                              between two pushes); then, when has_state, the gains to start from (R float32), else
//                              the initial state; then R rows of N float32 (real) or (re, im) pairs (complex).
//                              OUT: per record R rows of N outputs of the input's type; R rows of N float32 track
//                              values; the R gains behind them; six int64, the samples of the record that took each
//                              branch of the header's step: attack (e < 0, the gain moved), decay (e >= 0, the gain
//                              moved), the clip at -1, the gate, the clamp at gmin, the clamp at gmax.
//   agc_ref derive SETS OUT    SETS: sets of 7 float32.  OUT: per set int32 accepted (0 / 1), float32 iref.
//
// The kernel's step is cut in two (agc_drive off the walk, agc_step on it: hz_agc_math.h) with the gate riding in the
// walk's input as a NaN.  Every sample is ALSO put through agc_step_plain, the header's step word for word; the
// program ends with status 7 where the two differ in a bit.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hz_agc_math.h"
#include "hz_agc_plan.h"

using namespace hz;

static bool same_bits(float a, float b) { return memcmp(&a, &b, 4) == 0; }

enum { kAttack, kDecay, kClip, kGate, kGmin, kGmax, kBranches };

// what the header's step does with (g, a), branch by branch
static void count(float g, float a, const am::Loop &k, int64_t *c) {
    const float b = a * k.iref;
    float e = fmaf(-b, g, 1.0f);
    if (e < -1.0f) c[kClip]++, e = -1.0f;
    const float r = e < 0.0f ? k.attack : k.decay;
    float s = r * e;
    if (a < k.floor) c[kGate]++;
    if (s != s || a < k.floor)
        s = 0.0f;
    else
        c[e < 0.0f ? kAttack : kDecay]++;
    const float gn = fmaf(g, s, g);
    if (gn < k.gmin) c[kGmin]++;
    if (gn > k.gmax) c[kGmax]++;
}

template <typename S>
static bool row(const std::vector<std::vector<float>> &par, const std::vector<int64_t> &start, int per_row, int64_t r, int64_t N, const S *x, float *z,
                S *y, float *track, int64_t *branches) {
    float g = *z;
    size_t seg = 0;
    am::Loop k = ap::derive(par[0].data() + (per_row ? r * ap::kParams : 0));
    for (int64_t n = 0; n < N; n++) {
        while (seg + 1 < par.size() && start[seg + 1] <= n) k = ap::derive(par[++seg].data() + (per_row ? r * ap::kParams : 0));
        const float a = am::agc_level(x[n]);
        y[n] = am::agc_apply(x[n], g);
        track[n] = g;
        count(g, a, k, branches);
        const float plain = am::agc_step_plain(g, a, k);
        g = am::agc_step(g, am::agc_drive(a, k.iref, k.floor), k);
        if (!same_bits(g, plain) && !(g != g && plain != plain)) return false;
    }
    *z = g;
    return true;
}

static int run(const char *cases, const char *outp) {
    FILE *f = fopen(cases, "rb"), *o = fopen(outp, "wb");
    if (!f || !o) return 2;
    int32_t hd[4];
    while (fread(hd, 4, 4, f) == 4) {
        const int cplx = hd[0], segs = hd[1], per_row = hd[2], has_state = hd[3];
        int64_t dim[2];
        if (fread(dim, 8, 2, f) != 2) return 3;
        const int64_t R = dim[0], N = dim[1];
        if (cplx < 0 || cplx > 1 || segs < 1 || R < 1 || N < 0) return 5;
        const size_t per = (size_t)(per_row ? R : 1) * ap::kParams, width = cplx ? 2 : 1;
        std::vector<int64_t> start(segs);
        std::vector<std::vector<float>> par(segs, std::vector<float>(per));
        for (int g = 0; g < segs; g++) {
            if (fread(&start[g], 8, 1, f) != 1 || fread(par[g].data(), 4, per, f) != per) return 3;
            for (size_t q = 0; q < per; q += ap::kParams)
                if (ap::check_params(par[g].data() + q)) return 6;
        }
        std::vector<float> z((size_t)R), x((size_t)R * N * width), y((size_t)R * N * width), tr((size_t)R * N);
        if (has_state) {
            if (fread(z.data(), 4, z.size(), f) != z.size()) return 3;
        } else {
            for (int64_t r = 0; r < R; r++) z[r] = ap::initial_gain(par[0].data() + (per_row ? r * ap::kParams : 0));
        }
        if (fread(x.data(), 4, x.size(), f) != x.size()) return 3;
        int64_t branches[kBranches] = {0};
        for (int64_t r = 0; r < R; r++) {
            const size_t at = (size_t)r * N;
            const bool ok = cplx ? row(par, start, per_row, r, N, (const dm::c32 *)x.data() + at, &z[r], (dm::c32 *)y.data() + at, tr.data() + at, branches)
                                 : row(par, start, per_row, r, N, x.data() + at, &z[r], y.data() + at, tr.data() + at, branches);
            if (!ok) return 7;
        }
        fwrite(y.data(), 4, y.size(), o);
        fwrite(tr.data(), 4, tr.size(), o);
        fwrite(z.data(), 4, z.size(), o);
        fwrite(branches, 8, kBranches, o);
    }
    fclose(f);
    return fclose(o) ? 4 : 0;
}

static int derive(const char *sets, const char *outp) {
    FILE *f = fopen(sets, "rb"), *o = fopen(outp, "wb");
    if (!f || !o) return 2;
    float q[ap::kParams];
    while (fread(q, 4, ap::kParams, f) == ap::kParams) {
        const int32_t ok = ap::check_params(q) == nullptr;
        const float iref = ok ? ap::derive(q).iref : 0.0f;
        fwrite(&ok, 4, 1, o), fwrite(&iref, 4, 1, o);
    }
    fclose(f);
    return fclose(o) ? 4 : 0;
}

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "derive")) return derive(argv[2], argv[3]);
    fprintf(stderr, "usage: agc_ref run CASES OUT | derive SETS OUT\n");
    return 64;
}

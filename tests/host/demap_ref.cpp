// demap_ref.cpp -- the restatement of the demapper bank (include/hzsdr_demap.h) over csrc/hz_demap_math.h, symbol by
// symbol: one frame at a time, every point's distance in a plain array, the two minima of every bit by a loop over the
// labels, the values of a frame in a plain array, then the outputs one by one -- no threads, no blocks, no tree.  It
// computes the bits the device must produce.
//
//   demap_ref run CASES OUT    CASES: records of
//                                uint32 kind, m, S, N, has_perm, has_flip, n_gains, rows; float32 points[2 M | M | 0];
//                                uint32 perm[N] (has_perm); uint8 flip[ceil(N / 8)] (has_flip); float32 gains[n_gains];
//                                int64 R, cap; int32 has_counts; (R uint32 counts); R * cap dense frames of W float32.
//                              OUT: per record R * cap * N uint32 bit patterns; slots from min(count, cap) up are zero.
//   demap_ref check SETS OUT   SETS: records of the eight uint32, then uint32 npoints, nperm, ngains and float32
//                                points[npoints], uint32 perm[nperm], float32 gains[ngains] (flip is not validated).
//                              OUT: per set int32 accepted (0 / 1).
//   demap_ref call SETS OUT    SETS: records of uint64 kind, m, S, N (= S m), in, out (addresses), in_stride, out_stride,
//                                cap, rows.  OUT: per record int32 0 (accepted), 1 (invalid argument), 2 (destination
//                                too small): hz_demap_plan.h's check of a call.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hz_demap_math.h"
#include "hz_demap_plan.h"

using namespace hz;

struct Head {
    dmp::Config q;
    uint32_t has_flip;
};

static bool read_head(FILE *f, Head &h) {
    uint32_t v[8];
    if (fread(v, 4, 8, f) != 8) return false;
    h.q = dmp::Config{(int)v[0], v[1], v[2], v[3], false, v[4] != 0, v[6], v[7]};
    h.has_flip = v[5];
    return true;
}

static uint32_t point_floats(const dmp::Config &q) { return q.kind == dmp::kLlrF32 ? 0u : (q.kind == dmp::kC64 ? 2u : 1u) << q.m; }

// one frame: W floats -> N bit patterns
static void demap(const dmp::Config &q, const std::vector<float> &pts, const std::vector<uint32_t> &perm, const std::vector<uint8_t> &flip, float g,
                  const float *x, uint32_t *out) {
    const uint32_t m = (uint32_t)q.m, S = (uint32_t)q.S, N = (uint32_t)q.N, M = 1u << m;
    std::vector<float> L((size_t)S * m), d(M);
    for (uint32_t s = 0; s < S; s++) {
        if (q.kind == dmp::kLlrF32) {
            L[s] = x[s] * g;
            continue;
        }
        const bool cplx = q.kind == dmp::kC64;
        const float xr = cplx ? x[2 * s] : x[s], xi = cplx ? x[2 * s + 1] : 0.0f;
        for (uint32_t p = 0; p < M; p++) d[p] = cplx ? dm::dist(xr, xi, pts[2 * p], pts[2 * p + 1]) : dm::dist_real(xr, pts[p]);
        for (uint32_t j = 0; j < m; j++) {
            float d0 = INFINITY, d1 = INFINITY;
            for (uint32_t p = 0; p < M; p++) {
                float &side = dm::bit_of(p, m, j) ? d1 : d0;
                if (d[p] < side) side = d[p];
            }
            L[(size_t)s * m + j] = (xr != xr || xi != xi) ? dm::float_of(dm::kNanBits) : dm::llr(d0, d1, g);
        }
    }
    for (uint32_t k = 0; k < N; k++) {
        const uint32_t at = q.has_perm ? perm[k] : k;
        const float v = at == dm::kErased ? dm::float_of(dm::kNanBits) : L[at];
        const uint32_t fb = flip.empty() ? 0u : (uint32_t)(flip[k >> 3] >> (7u - (k & 7u))) & 1u;
        out[k] = dm::stored(v, fb);
    }
}

static int run(const char *cases, const char *outp) {
    FILE *f = fopen(cases, "rb"), *o = fopen(outp, "wb");
    if (!f || !o) return 2;
    Head h;
    while (read_head(f, h)) {
        dmp::Config &q = h.q;
        const uint32_t np = dmp::known(q.kind) && q.m <= dmp::kMaxBits ? point_floats(q) : 0;
        q.has_points = np != 0;
        if (!dmp::known(q.kind) || dmp::check_config(q)) return 6;
        std::vector<float> pts(np), gains(q.n_gains);
        std::vector<uint32_t> perm(q.has_perm ? q.N : 0);
        std::vector<uint8_t> flip(h.has_flip ? (q.N + 7) / 8 : 0);
        if (np && fread(pts.data(), 4, np, f) != np) return 3;
        if (!perm.empty() && fread(perm.data(), 4, perm.size(), f) != perm.size()) return 3;
        if (!flip.empty() && fread(flip.data(), 1, flip.size(), f) != flip.size()) return 3;
        if (fread(gains.data(), 4, gains.size(), f) != gains.size()) return 3;
        if (dmp::check_arrays(q, pts.data(), perm.data(), gains.data())) return 6;
        int64_t dim[2];
        int32_t has_counts;
        if (fread(dim, 8, 2, f) != 2 || fread(&has_counts, 4, 1, f) != 1) return 3;
        const int64_t R = dim[0], cap = dim[1];
        if (R < 1 || cap < 1 || (uint64_t)R != q.rows) return 6;
        const dmp::Geom g = dmp::geom(q);
        std::vector<uint32_t> counts((size_t)R, (uint32_t)cap);
        if (has_counts && fread(counts.data(), 4, R, f) != (size_t)R) return 3;
        std::vector<float> in((size_t)R * cap * g.W);
        if (fread(in.data(), 4, in.size(), f) != in.size()) return 3;
        std::vector<uint32_t> out((size_t)R * cap * g.N, 0);
        for (int64_t r = 0; r < R; r++)
            for (int64_t fr = 0; fr < cap && fr < (int64_t)counts[r]; fr++)
                demap(q, pts, perm, flip, gains[q.n_gains > 1 ? r : 0], in.data() + ((size_t)r * cap + fr) * g.W, out.data() + ((size_t)r * cap + fr) * g.N);
        fwrite(out.data(), 4, out.size(), o);
    }
    fclose(f);
    return fclose(o) ? 4 : 0;
}

static int check(const char *sets, const char *outp) {
    FILE *f = fopen(sets, "rb"), *o = fopen(outp, "wb");
    if (!f || !o) return 2;
    Head h;
    while (read_head(f, h)) {
        uint32_t len[3];
        if (fread(len, 4, 3, f) != 3) return 3;
        std::vector<float> pts(len[0]), gains(len[2]);
        std::vector<uint32_t> perm(len[1]);
        if (fread(pts.data(), 4, len[0], f) != len[0] || fread(perm.data(), 4, len[1], f) != len[1] || fread(gains.data(), 4, len[2], f) != len[2]) return 3;
        dmp::Config &q = h.q;
        q.has_points = len[0] != 0;
        int32_t ok = dmp::known(q.kind) && dmp::check_config(q) == nullptr;
        if (ok) ok = len[0] == point_floats(q) && len[1] == (q.has_perm ? q.N : 0) && len[2] == q.n_gains;
        if (ok) ok = dmp::check_arrays(q, pts.data(), perm.data(), gains.data()) == nullptr;
        fwrite(&ok, 4, 1, o);
    }
    fclose(f);
    return fclose(o) ? 4 : 0;
}

static int call(const char *sets, const char *outp) {
    FILE *f = fopen(sets, "rb"), *o = fopen(outp, "wb");
    if (!f || !o) return 2;
    uint64_t v[10];
    while (fread(v, 8, 10, f) == 10) {
        const dmp::Config q{(int)v[0], v[1], v[2], v[3], v[0] != (uint64_t)dmp::kLlrF32, false, 1, v[9]};
        if (!dmp::known(q.kind) || dmp::check_config(q)) return 6;
        const dmp::Geom g = dmp::geom(q);
        const dbp::Call c{(uintptr_t)v[4], (uintptr_t)v[5], (size_t)v[6], g.W, (size_t)v[7], g.N, (size_t)v[8], (size_t)v[9], true};
        const char *why = nullptr;
        const int32_t rc = dmp::check_run(g, c, &why);
        if ((rc != dbp::kOk) != (why != nullptr)) return 7;
        fwrite(&rc, 4, 1, o);
    }
    fclose(f);
    return fclose(o) ? 4 : 0;
}

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "call")) return call(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "check")) return check(argv[2], argv[3]);
    fprintf(stderr, "usage: demap_ref run CASES OUT | check SETS OUT | call SETS OUT\n");
    return 64;
}

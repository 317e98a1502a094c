// equalizer_ref.cpp -- the bit-exact restatement of the equalizer bank (include/hzsdr_equalizer.h) over
// csrc/hz_equalizer_math.h, the header the kernel evaluates, with the constants and the state's layout of
// csrc/hz_equalizer_plan.h: built with g++ -O2 -ffp-contract=off, it computes the bits the device must produce.
//
//   equalizer_ref run CASES OUT    CASES: records of int32 complex (0 / 1), mode, per_row (0 / 1), has_state (0 / 1),
//                                  has_counts (0 / 1), 0; int64 R, W, N, c; the parameters (2 float32 mu, level, or R * 2
//                                  when per_row); then, when has_state, the state to start from (R rows of (2 N - 1)
//                                  float32, twice that for complex rows), else the initial state; then, when has_counts,
//                                  R uint32 counts (row r consumes min(count, W) symbols), else every row consumes W;
//                                  then R rows of W float32 (real) or (re, im) pairs (complex).
//                                  OUT: per record R rows of W outputs of the input's type and R rows of W float32 track
//                                  values (zeros behind a row's count); the state behind them.
//   equalizer_ref check SETS OUT   SETS: records of float32 mu, level, int32 taps, centre, mode, complex.
//                                  OUT: per record int32 parameters accepted (0 / 1), int32 geometry accepted (0 / 1).
//
// The sum of the products is the header's butterfly over an array of Np entries, all entries at once; the program ends
// with status 7 where the entries of a finite sum do not end equal bit for bit.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hz_equalizer_math.h"
#include "hz_equalizer_plan.h"

using namespace hz;

// one row: `cnt` symbols of x through the equalizer; z is the row's state
template <int PL>
static bool row(int mode, const em::Loop &k, uint32_t N, int64_t cnt, const float *x, float *z, float *y, float *track) {
    const uint32_t Np = ep::pow2_up(N);
    std::vector<float> X((size_t)N * PL), p((size_t)Np * PL), q((size_t)Np * PL);
    for (int64_t n = 0; n < cnt; n++) {
        for (int c = 0; c < PL; c++) X[c] = x[n * PL + c];
        for (uint32_t i = 1; i < N; i++)
            for (int c = 0; c < PL; c++) X[i * PL + c] = z[ep::state_history(i - 1, c, N, PL)];
        for (uint32_t i = 0; i < Np; i++) {
            float w[PL], xi[PL], pi[PL] = {};
            if (i < N) {
                for (int c = 0; c < PL; c++) w[c] = z[ep::state_tap(i, c, PL)], xi[c] = X[i * PL + c];
                em::eq_product<PL>(w, xi, pi);
            }
            for (int c = 0; c < PL; c++) p[i * PL + c] = pi[c];
        }
        for (uint32_t s = 1; s < Np; s <<= 1) {
            for (uint32_t i = 0; i < Np; i++)
                for (int c = 0; c < PL; c++) q[i * PL + c] = p[i * PL + c] + p[(i ^ s) * PL + c];
            p.swap(q);
        }
        float yy[PL], e[PL], g[PL];
        for (int c = 0; c < PL; c++) yy[c] = p[c];
        for (uint32_t i = 1; i < Np; i++)
            for (int c = 0; c < PL; c++)
                if (std::isfinite(yy[c]) && memcmp(&p[i * PL + c], &yy[c], 4) != 0) return false;
        em::eq_error<PL>(mode, yy, k.level, e);
        em::eq_gain<PL>(k.mu, e, g);
        for (uint32_t i = 0; i < N; i++) {
            float w[PL], xi[PL];
            for (int c = 0; c < PL; c++) w[c] = z[ep::state_tap(i, c, PL)], xi[c] = X[i * PL + c];
            em::eq_update<PL>(w, g, xi);
            for (int c = 0; c < PL; c++) z[ep::state_tap(i, c, PL)] = w[c];
        }
        for (int c = 0; c < PL; c++) y[n * PL + c] = yy[c];
        track[n] = em::eq_track<PL>(e);
        for (uint32_t i = 0; i + 1 < N; i++)
            for (int c = 0; c < PL; c++) z[ep::state_history(i, c, N, PL)] = X[i * PL + c];
    }
    return true;
}

static int run(const char *cases, const char *outp) {
    FILE *f = fopen(cases, "rb"), *o = fopen(outp, "wb");
    if (!f || !o) return 2;
    int32_t hd[6];
    while (fread(hd, 4, 6, f) == 6) {
        const int cplx = hd[0], mode = hd[1], per_row = hd[2], has_state = hd[3], has_counts = hd[4];
        int64_t dim[4];
        if (fread(dim, 8, 4, f) != 4) return 3;
        const int64_t R = dim[0], W = dim[1], N = dim[2], c = dim[3];
        if (cplx < 0 || cplx > 1 || R < 1 || W < 0 || ep::check_geom(N, c, mode, cplx != 0)) return 5;
        const uint32_t pl = cplx ? 2 : 1, rowz = ep::state_row_floats((uint32_t)N, pl);
        const size_t per = (size_t)(per_row ? R : 1) * ep::kParams;
        std::vector<float> par(per);
        if (fread(par.data(), 4, per, f) != per) return 3;
        for (size_t q = 0; q < per; q += ep::kParams)
            if (ep::check_params(par.data() + q)) return 6;
        std::vector<float> z((size_t)R * rowz, 0.0f), x((size_t)R * W * pl), y((size_t)R * W * pl, 0.0f), tr((size_t)R * W, 0.0f);
        std::vector<uint32_t> cnt((size_t)R, (uint32_t)W);
        if (has_state) {
            if (fread(z.data(), 4, z.size(), f) != z.size()) return 3;
        } else {
            for (int64_t r = 0; r < R; r++) z[(size_t)r * rowz + ep::state_tap((uint32_t)c, 0, pl)] = 1.0f;
        }
        if (has_counts && fread(cnt.data(), 4, cnt.size(), f) != cnt.size()) return 3;
        if (fread(x.data(), 4, x.size(), f) != x.size()) return 3;
        for (int64_t r = 0; r < R; r++) {
            const em::Loop k = ep::derive(par.data() + (per_row ? r * ep::kParams : 0));
            const int64_t n = cnt[r] < (uint64_t)W ? (int64_t)cnt[r] : W;
            const size_t at = (size_t)r * W;
            const bool ok = cplx ? row<2>(mode, k, (uint32_t)N, n, x.data() + at * 2, z.data() + (size_t)r * rowz, y.data() + at * 2, tr.data() + at)
                                 : row<1>(mode, k, (uint32_t)N, n, x.data() + at, z.data() + (size_t)r * rowz, y.data() + at, tr.data() + at);
            if (!ok) return 7;
        }
        fwrite(y.data(), 4, y.size(), o);
        fwrite(tr.data(), 4, tr.size(), o);
        fwrite(z.data(), 4, z.size(), o);
    }
    fclose(f);
    return fclose(o) ? 4 : 0;
}

static int check(const char *sets, const char *outp) {
    FILE *f = fopen(sets, "rb"), *o = fopen(outp, "wb");
    if (!f || !o) return 2;
    struct Rec {
        float q[2];
        int32_t taps, centre, mode, cplx;
    } rec;
    while (fread(&rec, sizeof rec, 1, f) == 1) {
        const int32_t ok[2] = {ep::check_params(rec.q) == nullptr, ep::check_geom(rec.taps, rec.centre, rec.mode, rec.cplx != 0) == nullptr};
        fwrite(ok, 4, 2, o);
    }
    fclose(f);
    return fclose(o) ? 4 : 0;
}

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "check")) return check(argv[2], argv[3]);
    fprintf(stderr, "usage: equalizer_ref run CASES OUT | check SETS OUT\n");
    return 64;
}

// carrier_ref.cpp -- the bit-exact restatement of the carrier recovery bank (include/hzsdr_carrier.h) over
// csrc/hz_carrier_math.h, the header the kernel evaluates, with the constants of csrc/hz_carrier_plan.h: built with
// g++ -O2 -ffp-contract=off, it computes the bits the device must produce.
//
//   carrier_ref run CASES OUT   CASES: records of int32 mode, segments, per_row (0 / 1), has_state (0 / 1), int64 R, N;
//                               then per segment int64 start and its parameters (5 float32 alpha, beta, f0, fmin, fmax,
//                               or R * 5 when per_row): the parameters in force from sample `start` on (the first
//                               segment starts at 0; a later one is a hzsdr_carrier_set_params between two pushes);
//                               then, when has_state, the state to start from (R * 2 uint32: theta, F), else the
//                               initial state; then R rows of N (re, im) pairs.
//                               OUT: per record R rows of N outputs (re, im); R rows of N float32 track values; the
//                               state behind them.
//   carrier_ref derive SETS OUT SETS: sets of 5 float32.  OUT: per set int32 accepted (0 / 1), float32 alpha_w, beta_w,
//                               int32 F0, Fmin, Fmax.
//   carrier_ref unit STRIDE THREADS   walks the phase words 0, STRIDE, 2 STRIDE, ... below 2^32 (STRIDE = 1: all of
//                               them), and the axes, the diagonals and their neighbours, against float64, on THREADS
//                               threads (16 at most), and prints the largest |(c, s) - exact| of car_unit and of the
//                               tuner's three-table rotator with the words they occur at, then the number of axis words
//                               at which car_unit is not exactly 0 and 1 in magnitude.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "hz_carrier_math.h"
#include "hz_carrier_plan.h"

using namespace hz;

template <int MODE>
static void row(const std::vector<std::vector<float>> &par, const std::vector<int64_t> &start, int per_row, int64_t r, int64_t N, const float *x,
                uint32_t *z, float *y, float *track) {
    cm::State s{z[0], (int32_t)z[1]};
    size_t g = 0;
    cm::Loop loop = cp::derive(par[0].data() + (per_row ? r * cp::kParams : 0));
    for (int64_t n = 0; n < N; n++) {
        while (g + 1 < par.size() && start[g + 1] <= n) loop = cp::derive(par[++g].data() + (per_row ? r * cp::kParams : 0));
        tn::c32 v;
        track[n] = cm::car_step<MODE>(s, loop, tn::c32{x[2 * n], x[2 * n + 1]}, &v);
        y[2 * n] = v.re, y[2 * n + 1] = v.im;
    }
    z[0] = s.theta, z[1] = (uint32_t)s.f;
}

static int run(const char *cases, const char *outp) {
    FILE *f = fopen(cases, "rb"), *o = fopen(outp, "wb");
    if (!f || !o) return 2;
    int32_t hd[4];
    while (fread(hd, 4, 4, f) == 4) {
        const int mode = hd[0], segs = hd[1], per_row = hd[2], has_state = hd[3];
        int64_t dim[2];
        if (fread(dim, 8, 2, f) != 2) return 3;
        const int64_t R = dim[0], N = dim[1];
        if (mode < 0 || mode >= (int)cp::kModes || segs < 1 || R < 1 || N < 0) return 5;
        const size_t per = (size_t)(per_row ? R : 1) * cp::kParams;
        std::vector<int64_t> start(segs);
        std::vector<std::vector<float>> par(segs, std::vector<float>(per));
        for (int g = 0; g < segs; g++) {
            if (fread(&start[g], 8, 1, f) != 1 || fread(par[g].data(), 4, per, f) != per) return 3;
            for (size_t q = 0; q < per; q += cp::kParams)
                if (cp::check_params(par[g].data() + q)) return 6;
        }
        std::vector<uint32_t> z((size_t)R * cp::kStateWords, 0u);
        std::vector<float> x((size_t)R * N * 2), y((size_t)R * N * 2), tr((size_t)R * N);
        if (has_state) {
            if (fread(z.data(), 4, z.size(), f) != z.size()) return 3;
        } else {
            for (int64_t r = 0; r < R; r++) z[cp::state_index(r, 1)] = (uint32_t)cp::derive(par[0].data() + (per_row ? r * cp::kParams : 0)).f0;
        }
        if (fread(x.data(), 4, x.size(), f) != x.size()) return 3;
        for (int64_t r = 0; r < R; r++) {
            const float *xr = x.data() + (size_t)r * N * 2;
            uint32_t *zr = z.data() + r * cp::kStateWords;
            float *yr = y.data() + (size_t)r * N * 2, *tr_r = tr.data() + (size_t)r * N;
            if (mode == cm::kTone)
                row<cm::kTone>(par, start, per_row, r, N, xr, zr, yr, tr_r);
            else if (mode == cm::kBpsk)
                row<cm::kBpsk>(par, start, per_row, r, N, xr, zr, yr, tr_r);
            else
                row<cm::kQpsk>(par, start, per_row, r, N, xr, zr, yr, tr_r);
        }
        fwrite(y.data(), 4, y.size(), o);
        fwrite(tr.data(), 4, tr.size(), o);
        fwrite(z.data(), 4, z.size(), o);
    }
    fclose(f);
    return fclose(o) ? 4 : 0;
}

static int derive(const char *sets, const char *outp) {
    FILE *f = fopen(sets, "rb"), *o = fopen(outp, "wb");
    if (!f || !o) return 2;
    float q[5];
    while (fread(q, 4, 5, f) == 5) {
        const int32_t ok = cp::check_params(q) == nullptr;
        cm::Loop k{0.0f, 0.0f, 0, 0, 0};
        if (ok) k = cp::derive(q);  // (llrint of a refused value may not fit an int32)
        const float w[2] = {k.aw, k.bw};
        const int32_t fr[3] = {k.f0, k.fmin, k.fmax};
        fwrite(&ok, 4, 1, o), fwrite(w, 4, 2, o), fwrite(fr, 4, 3, o);
    }
    fclose(f);
    return fclose(o) ? 4 : 0;
}

struct Worst {
    double car = 0.0, tab = 0.0;
    uint32_t car_at = 0, tab_at = 0;
    uint64_t words = 0;
};

static void measure(uint32_t p, const tn::c32 *tab, Worst &w) {
    double ec, es;
    tn::tuner_unit(p, &ec, &es);
    float c, s;
    cm::car_unit(p, &c, &s);
    const double dc = (double)c - ec, ds = (double)s - es, d = sqrt(dc * dc + ds * ds);
    if (d > w.car) w.car = d, w.car_at = p;
    const tn::c32 r = tn::tuner_rotate(tn::c32{1.0f, 0.0f}, p, tab);  // exp(-2 pi i p / 2^32)
    const double tc = (double)r.re - ec, ts = (double)r.im + es, t = sqrt(tc * tc + ts * ts);
    if (t > w.tab) w.tab = t, w.tab_at = p;
    w.words++;
}

static int unit(uint64_t stride, unsigned threads) {
    if (stride < 1 || threads < 1 || threads > 16) return 64;
    std::vector<tn::c32> tab(tn::kTables);
    for (uint32_t i = 0; i < tn::kT2; i++) tab[i] = tn::tuner_table(i, 21);
    for (uint32_t i = 0; i < tn::kT1; i++) tab[tn::kT2 + i] = tn::tuner_table(i, 10);
    for (uint32_t i = 0; i < tn::kT0; i++) tab[tn::kT2 + tn::kT1 + i] = tn::tuner_table(i, 0);
    const uint64_t count = ((1ull << 32) + stride - 1) / stride;
    std::vector<Worst> worst(threads + 1);
    std::vector<std::thread> pool;
    for (unsigned th = 0; th < threads; th++)
        pool.emplace_back([&, th] {
            const uint64_t lo = count * th / threads, hi = count * (th + 1) / threads;
            for (uint64_t k = lo; k < hi; k++) measure((uint32_t)(k * stride), tab.data(), worst[th]);
        });
    for (auto &t : pool) t.join();
    // the axes, the diagonals (where the quadrant changes) and their neighbours
    uint32_t bad_axes = 0;
    for (uint32_t e = 0; e < 8; e++) {
        for (int32_t d = -64; d <= 64; d++) measure(e * 0x20000000u + (uint32_t)d, tab.data(), worst[threads]);
        if (e % 2 == 0) {
            float c, s;
            cm::car_unit(e * 0x20000000u, &c, &s);
            const float big = e % 4 == 0 ? fabsf(c) : fabsf(s), small = e % 4 == 0 ? s : c;
            const float sign = e == 0 || e == 2 ? 1.0f : -1.0f;
            if (big != 1.0f || small != 0.0f || (e % 4 == 0 ? c : s) != sign) bad_axes++;
        }
    }
    Worst w;
    for (const Worst &v : worst) {
        if (v.car > w.car) w.car = v.car, w.car_at = v.car_at;
        if (v.tab > w.tab) w.tab = v.tab, w.tab_at = v.tab_at;
        w.words += v.words;
    }
    printf("%llu %.9e %u %.9e %u %u\n", (unsigned long long)w.words, w.car, w.car_at, w.tab, w.tab_at, bad_axes);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "derive")) return derive(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "unit")) return unit(strtoull(argv[2], nullptr, 10), (unsigned)strtoul(argv[3], nullptr, 10));
    fprintf(stderr, "usage: carrier_ref run CASES OUT | derive SETS OUT | unit STRIDE THREADS\n");
    return 64;
}

// plane0_window.cpp -- mm2::plane0_window (hz_firmm2_plan.h) under AddressSanitizer + UndefinedBehaviorSanitizer:
// the per-plane matrix loop of the persistent-pass kernel (hz_firmm2.h, kPlane) multiplies digit plane 0 only on the
// step pairs [p0_lo, p0_hi), so every nonzero plane-0 digit of every table the chain can build must be read by pairs
// inside that window only.  Built by tests/test_plane0_window.py:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I go-sdr_amd/csrc -I include
//         tests/host/plane0_window.cpp go-sdr_amd/csrc/hz_host.cpp -o plane0_window
// Random tap counts, factors 8 and 16, filters (windowed sincs, decaying exponentials peaked at either end, a sinc
// over a floor, random taps), both byte scales (u8 1/127.5, i8 1/128), the chain's shift S and smaller ones, random
// modulations (clock step and Shift frequency) -- and taps placed ON the bound: coefficients of 127 (2^16 + 2^8 + 1)
// and one unit either side, the edge of the three-digit balanced range.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "hz_firmm_plan.h"
#include "hzsdr.h"

using namespace hz;

static uint64_t rng_state = 0x2545F4914F6CDD1Dull;
static uint64_t rnd() {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static double urand() { return (double)(rnd() >> 11) / 9007199254740992.0; }

#define REQUIRE(c)                                                                                  \
    do {                                                                                            \
        if (!(c)) {                                                                                 \
            fprintf(stderr, "%s:%d: REQUIRE(%s) failed (iteration %d)\n", __FILE__, __LINE__, #c, it); \
            exit(1);                                                                                \
        }                                                                                           \
    } while (0)

int main(int argc, char **argv) {
    const int iters = argc > 1 ? atoi(argv[1]) : 400;
    const double kW = 65536.0 + 256.0 + 1.0;
    long long checked = 0, nonzero = 0, on_bound = 0, windows_all = 0, windows_part = 0, windows_none = 0;
    for (int it = 0; it < iters; it++) {
        const int D = (rnd() & 1) ? 8 : 16;
        const int nt = 16 + (int)(rnd() % 1500);
        const double scale = (rnd() & 1) ? 1.0 / 127.5 : 1.0 / 128.0;
        std::vector<double> taps(2 * nt);
        const int kind = (int)(rnd() % 5);
        const double cut = 0.01 + 0.2 * urand(), decay = 5.0 + 200.0 * urand(), rot = urand() * 6.0;
        for (int k = 0; k < nt; k++) {
            const double c = k - (nt - 1) / 2.0;
            const double sinc = c == 0 ? 1.0 : sin(M_PI * 2 * cut * c) / (M_PI * 2 * cut * c);
            const double ham = 0.54 - 0.46 * cos(2 * M_PI * k / (nt - 1));
            double re = 0, im = 0;
            if (kind == 0) re = 2 * cut * sinc * ham;
            else if (kind == 1) re = exp(-k / decay) * cos(rot * k), im = exp(-k / decay) * sin(rot * k);
            else if (kind == 2) re = exp(-(nt - 1 - k) / decay);
            else if (kind == 3) re = 2 * cut * sinc * ham + 0.02;
            else re = urand() - 0.5, im = (urand() - 0.5) * urand();
            taps[2 * k] = re, taps[2 * k + 1] = im;
        }
        int S = mm::digit_shift(taps.data(), (size_t)nt, scale);
        if (rnd() % 3 == 0) S -= (int)(rnd() % 4);  // (a smaller shift keeps |q| <= 2^30)
        // taps ON the bound: |h| scale 2^S = 127 W + {-1, -1/2, 0, 1/2, 1}, at a random phase
        if (rnd() & 1) {
            const int nb = 1 + (int)(rnd() % 6);
            for (int b = 0; b < nb; b++) {
                const int k = (int)(rnd() % (uint64_t)nt);
                const double m = 127.0 * kW + 0.5 * ((int)(rnd() % 5) - 2);
                const double v = ldexp(m / scale, -S), ph = (rnd() & 1) ? 0.0 : urand() * 2 * M_PI;
                taps[2 * k] = v * cos(ph), taps[2 * k + 1] = v * sin(ph);
                on_bound++;
            }
        }
        const unsigned off = (unsigned)(nt - 1 + 7) / 8 * 8;
        mm2::Geom g2 = mm2::make_geom(nt, D, off, S);
        mm2::plane0_window(g2, D, taps.data(), scale);
        const int np = g2.ks / 2;
        REQUIRE(0 <= g2.p0_lo && g2.p0_lo <= g2.p0_hi && g2.p0_hi <= np);
        if (g2.p0_lo == 0 && g2.p0_hi == np) windows_all++;
        else if (g2.p0_lo == g2.p0_hi) windows_none++;
        else windows_part++;
        mm::Geom g{};
        g.ntaps = g2.ntaps, g.w0 = g2.w0, g.ks = g2.ks, g.ne = g2.ne, g.e0 = g2.e0, g.shift = g2.shift, g.off = g2.off;
        const int runs = 4;
        for (int r = 0; r < runs; r++) {
            const double step = r == 0 ? 0.0 : 1.0 / (1e6 + urand() * 6e7);
            const double omega = r == 0 ? 0.0 : (urand() - 0.5) * 2 * M_PI * 3e7;
            const std::vector<uint8_t> tab = mm::digit_table(g, D, taps.data(), scale, step, omega, scale != 1.0 / 128.0, true);
            for (int E = 0; E < g.ne; E++)
                for (int pout = 0; pout < 2; pout++)
                    for (int e = 0; e < 16; e++) {
                        checked++;
                        // T[f][E][part][pl]: plane 0 = f 0, pl 0
                        if (tab[((((size_t)0 * g.ne + E) * 2 + pout) * 2 + 0) * 16 + e] == 0) continue;
                        nonzero++;
                        // every pair that reads entry E: E = (D / 8) i - kq - 4 t + e0
                        for (int t = 0; t < np; t++)
                            for (int i = 0; i < mm2::kT; i++)
                                for (int kq = 0; kq < 4; kq++)
                                    if ((D / 8) * i - kq - 4 * t + g.e0 == E) REQUIRE(t >= g2.p0_lo && t < g2.p0_hi);
                    }
        }
    }
    printf("plane0_window ok: %d filters, %lld plane-0 bytes checked, %lld nonzero, %lld taps on the bound; windows: %lld all pairs, %lld part, %lld none\n",
           iters, checked, nonzero, on_bound, windows_all, windows_part, windows_none);
    return 0;
}

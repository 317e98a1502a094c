// hz_tuner_math.h -- the arithmetic of the tuner bank (include/hzsdr_tuner.h) that is not the matrix product, HIP-free:
// the complex product of the rotator, the split of a phase word into its three table indices, the rotator itself and
// the four-fma term of step 2 as the host restatement evaluates it.  It compiles as __host__ __device__ under hipcc and
// as plain C++17 under g++ (-ffp-contract=off); the kernel of hz_tuner.hip and tests/host/tuner_ref.cpp evaluate the
// rotator of every output from this header, so that the host build and the device build compute the same bits.
//
// Nothing here calls libm or the device's math library: IEEE float32 *, each rounded by itself, and fmaf where a fused
// step is written out.  The tables and the modulated taps are host-made (tuner_unit below, float64) and come in as data.
#pragma once
#include <stdint.h>
#include <math.h>

#include "hz_plan.h"

#if defined(__clang__)
#define HZ_TM_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define HZ_TM_NO_CONTRACT
#endif

namespace hz {
namespace tn {

struct c32 {
    float re, im;
};

// p = a 2^21 + b 2^10 + c: 11, 11 and 10 bits
constexpr uint32_t kT2 = 2048, kT1 = 2048, kT0 = 1024;
constexpr uint32_t kTables = kT2 + kT1 + kT0;  // T2 at 0, T1 at kT2, T0 at kT2 + kT1 of one array
HZ_HD uint32_t tuner_a(uint32_t p) { return p >> 21; }
HZ_HD uint32_t tuner_b(uint32_t p) { return (p >> 10) & 2047u; }
HZ_HD uint32_t tuner_c(uint32_t p) { return p & 1023u; }

// cmul(u, v): the inner products rounded by themselves, the outer step fused
HZ_HD c32 tuner_cmul(c32 u, c32 v) {
    HZ_TM_NO_CONTRACT
    const float ii = u.im * v.im, ir = u.im * v.re;
    c32 r;
    r.re = __builtin_fmaf(u.re, v.re, -ii);
    r.im = __builtin_fmaf(u.re, v.im, ir);
    return r;
}

// y = cmul(s, cmul(cmul(T2[a], T1[b]), T0[c])) of the phase word p; tab: the three tables in one array
HZ_HD c32 tuner_rotate(c32 s, uint32_t p, const c32 *tab) {
    const c32 r = tuner_cmul(tuner_cmul(tab[tuner_a(p)], tab[kT2 + tuner_b(p)]), tab[kT2 + kT1 + tuner_c(p)]);
    return tuner_cmul(s, r);
}

// one q of step 2 as a chain of four fused steps: THE expression the matrix product must reproduce
HZ_HD c32 tuner_term(c32 acc, c32 g, c32 a) {
    acc.re = __builtin_fmaf(g.re, a.re, acc.re);
    acc.re = __builtin_fmaf(-g.im, a.im, acc.re);
    acc.im = __builtin_fmaf(g.im, a.re, acc.im);
    acc.im = __builtin_fmaf(g.re, a.im, acc.im);
    return acc;
}

// Host only from here on: step 1 and the tables.
// (cos, sin) of 2 pi u / 2^32 in float64.  The integer phase is first reduced, exactly, to the first half quadrant, so
// that the values on the axes and the diagonals' symmetries are exact: cos = 1, sin = 0 at u = 0, cos = -1, sin = 0 at
// u = 2^31.
inline void tuner_unit(uint32_t u, double *c, double *s) {
    const uint32_t quad = u >> 30, r = u & 0x3fffffffu;  // the angle is quad * pi/2 + r * 2 pi / 2^32
    const double k = 6.283185307179586476925286766559 / 4294967296.0;
    double cr, sr;
    if (r <= 0x20000000u) {
        cr = cos(r * k), sr = sin(r * k);
    } else {  // the mirror at pi/4: r' = 2^30 - r
        cr = sin((0x40000000u - r) * k), sr = cos((0x40000000u - r) * k);
    }
    if (r == 0) cr = 1.0, sr = 0.0;
    switch (quad) {
    case 0: *c = cr, *s = sr; break;
    case 1: *c = 0.0 - sr, *s = cr; break;
    case 2: *c = 0.0 - cr, *s = 0.0 - sr; break;
    default: *c = sr, *s = 0.0 - cr; break;
    }
}
// G_k[q] of step 1
inline c32 tuner_tap(float h, uint32_t w, uint32_t q) {
    double c, s;
    tuner_unit(w * q, &c, &s);  // (wrapping: the integer phase modulo 2^32)
    return c32{(float)((double)h * c), (float)((double)h * s)};
}
// entry i of a table whose step is 2^shift phase units: exp(-2 pi i (i << shift) / 2^32)
inline c32 tuner_table(uint32_t i, int shift) {
    double c, s;
    tuner_unit(i << shift, &c, &s);
    return c32{(float)c, (float)(0.0 - s)};
}

}  // namespace tn
}  // namespace hz

// hz_demod_math.h -- the arithmetic of the demodulator bank (include/hzsdr_demod.h), HIP-free: the separately rounded
// product with the conjugate, the library's own float32 arctangent, the four detectors and the one-fma term of the
// post-filter.  It compiles as __host__ __device__ under hipcc and as plain C++17 under g++ (-ffp-contract=off), and
// every path -- the kernel of hz_demod.hip and the restatement of tests/host/demod_ref.cpp -- evaluates the expression
// of each output from this header, so that the host build and the device build compute the same bits.
//
// Nothing here calls libm or the device's math library: the operations are IEEE float32 +, -, *, / and sqrt, each
// correctly rounded by itself (no contraction: the pragma below, and the build's -ffp-contract=off), fabs / copysign as
// bit operations, and fmaf where a fused step is written out.
//
// demod_angle(y, x), the angle of x + iy in (-pi, pi]:
//       t = min(|x|, |y|) / max(|x|, |y|)                  one correctly rounded division, t in [0, 1]
//       s = t * t
//       r = fmaf(P(s), s * t, t)                            atan t = t + t s P(s), P of degree 7 by Horner in fmaf
//       r = PIO2 - r   where |y| > |x|                      one float32 subtraction from float32 pi/2
//       r = PI - r     where x < 0                          one float32 subtraction from float32 pi
//       r = copysign(r, y)
// with angle(+-0, +-0) = +0 and t = 1 or 0 where the larger magnitude is infinite.  P's coefficients are the float32
// roundings of a weighted least-squares fit iterated to equal ripple (1.3e-8 of approximation error in exact
// arithmetic); the rest of the error is float32 rounding, above all that of the last subtraction (half an ulp of a
// result in [2, 4), 1.2e-7) and of float32 pi itself (8.7e-8).
//
// The error E, MEASURED by tests/host/demod_ref.cpp against float64 atan2 of the same float32 pair -- every float32
// ratio (x = 1, y every float32 in [0, 1]) in all eight octants, both axes, and 2^24 random pairs with exponents over
// the whole range:
//       E = 2.673684e-7 rad  (the bound asserted by tests/test_demod_cpu.py is 2^-21 = 4.77e-7, two ulps of the largest result)
#pragma once

#include "hz_plan.h"

#if defined(__clang__)
#define HZ_DM_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define HZ_DM_NO_CONTRACT
#endif

namespace hz {
namespace dm {

struct c32 {
    float re, im;
};

constexpr float kPi = 3.14159274101257324f, kPiO2 = 1.57079637050628662f;
// atan t = t + t s P(s), s = t^2, on [0, 1]
constexpr float kAtan[8] = {-3.333298564e-01f, 1.999039650e-01f,  -1.418597549e-01f, 1.057393029e-01f,
                            -7.366702706e-02f, 4.112181813e-02f, -1.513251010e-02f, 2.622237895e-03f};

// a * conj(b), every operation rounded by itself
HZ_HD c32 demod_mul_conj(c32 a, c32 b) {
    HZ_DM_NO_CONTRACT
    const float rr = a.re * b.re, ii = a.im * b.im, ir = a.im * b.re, ri = a.re * b.im;
    c32 p;
    p.re = rr + ii;
    p.im = ir - ri;
    return p;
}

HZ_HD float demod_angle(float y, float x) {
    HZ_DM_NO_CONTRACT
    const float ax = __builtin_fabsf(x), ay = __builtin_fabsf(y);
    const bool steep = ay > ax;
    const float mx = steep ? ay : ax, mn = steep ? ax : ay;
    if (mx == 0.0f) return 0.0f;
    float t = mn / mx;
    if (mx == __builtin_inff()) t = mn == mx ? 1.0f : 0.0f;
    const float s = t * t;
    float p = kAtan[7];
    p = __builtin_fmaf(p, s, kAtan[6]);
    p = __builtin_fmaf(p, s, kAtan[5]);
    p = __builtin_fmaf(p, s, kAtan[4]);
    p = __builtin_fmaf(p, s, kAtan[3]);
    p = __builtin_fmaf(p, s, kAtan[2]);
    p = __builtin_fmaf(p, s, kAtan[1]);
    p = __builtin_fmaf(p, s, kAtan[0]);
    const float u = s * t;
    float r = __builtin_fmaf(p, u, t);
    if (steep) r = kPiO2 - r;
    if (x < 0.0f) r = kPi - r;
    return __builtin_copysignf(r, y);
}

HZ_HD float demod_power(c32 a) {
    HZ_DM_NO_CONTRACT
    const float rr = a.re * a.re, ii = a.im * a.im;
    return rr + ii;
}

HZ_HD float demod_envelope(c32 a) { return __builtin_sqrtf(demod_power(a)); }
HZ_HD float demod_phase(c32 a) { return demod_angle(a.im, a.re); }
// a = c(x[n]), b = c(x[n - 1])
HZ_HD float demod_fm(c32 a, c32 b) {
    const c32 p = demod_mul_conj(a, b);
    return demod_angle(p.im, p.re);
}

constexpr int kFm = 1, kPhase = 2, kEnvelope = 3, kPower = 4;  // HZSDR_DEMOD_*

// d[n] of `mode` from a = c(x[n]) and b = c(x[n - 1]) (read by FM alone)
HZ_HD float demod_detect(int mode, c32 a, c32 b) {
    switch (mode) {
    case kFm: return demod_fm(a, b);
    case kPhase: return demod_phase(a);
    case kEnvelope: return demod_envelope(a);
    default: return demod_power(a);
    }
}

// one term of the post-filter: THE expression every path evaluates
HZ_HD float demod_term(float acc, float h, float d) { return __builtin_fmaf(h, d, acc); }

}  // namespace dm
}  // namespace hz

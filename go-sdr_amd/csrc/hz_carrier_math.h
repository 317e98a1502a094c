// hz_carrier_math.h -- the arithmetic of the carrier recovery bank (include/hzsdr_carrier.h), HIP-free: the oscillator's
// unit vector out of a 32-bit phase word, the three phase detectors and one step of the second-order loop.  It compiles
// as __host__ __device__ under hipcc and as plain C++17 under g++ (-ffp-contract=off), and both the kernel of
// hz_carrier.hip and the restatement of tests/host/carrier_ref.cpp evaluate every output, every track value and every
// state word through car_step, so that the host build and the device build compute the same bits.  Nothing here calls
// libm or the device's math library, and nothing reads a table: integer steps, int <-> float conversions, fmaf,
// products, comparisons.  The complex product is the tuner's (hz_tuner_math.h, tuner_cmul).
//
// The step is written without a branch: the detector is a template parameter, the clip and the clamp are selections.
//
// car_unit against float64 (tuner_unit) over ALL 2^32 phase words, the largest |(c, s) - exact| (tests/host/carrier_ref.cpp,
// mode `unit`):  car_unit 1.294e-07 (at p = 0x1f2b5db0);  the tuner's three-table rotator, measured by the same program
// over the same words, 1.605e-07 (at p = 0x5a55c4aa).  On the four axes car_unit is exactly (+-1, 0) and (0, +-1).
//
// Properties (restated in include/hzsdr_carrier.h):
//   - denormals are kept: neither build flushes them;
//   - a NaN sample gives a NaN output for THAT sample and moves the row on as a sample of zero error does: the error
//     is NaN, to_i32 of NaN is 0, so F stays (the clamp apart) and theta advances by F: a NaN stays in its sample as
//     well as in its row.  An infinity clips to an error of +-1 or to a NaN;
//   - no value of a row reaches another row, an address or a trip count.
#pragma once

#include <math.h>
#include <stdint.h>

#include "hz_plan.h"
#include "hz_tuner_math.h"

#if defined(__clang__)
#define HZ_CM_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define HZ_CM_NO_CONTRACT
#endif

namespace hz {
namespace cm {

enum { kTone = 0, kBpsk = 1, kQpsk = 2 };  // HZSDR_CARRIER_TONE / _BPSK / _QPSK

// the loop's constants of one row, as the kernel sees them (derived by hz_carrier_plan.h, derive)
struct Loop {
    float aw, bw;               // alpha 2^32, beta 2^32: phase units per unit error
    int32_t f0, fmin, fmax;     // phase units per sample
};

// the kept state of one row
struct State {
    uint32_t theta;  // 2^32 to the turn
    int32_t f;       // phase units per sample
};

constexpr float kRad = 0x1.921fb6p-30f;  // 2 pi / 2^32
// cos a = 1 + z C(z), sin a = a + a z S(z), z = a^2, |a| <= pi / 4: weighted least squares towards the least
// largest error, float64, rounded to float32 (the polynomials' own error: 5.4e-11 and 1.8e-9, far below the rounding)
constexpr float kC0 = -0x1.000000p-1f, kC1 = 0x1.55553ep-5f, kC2 = -0x1.6c087ep-10f, kC3 = 0x1.993430p-16f;
constexpr float kS0 = -0x1.555540p-3f, kS1 = 0x1.1105b4p-7f, kS2 = -0x1.98da64p-13f;

// (cos, sin) of 2 pi p / 2^32.  The phase is cut into the quadrant NEAREST to it and a remainder in [-2^29, 2^29),
// a = remainder 2 pi / 2^32 in [-pi / 4, pi / 4); the quadrant is applied by exchange and sign.
HZ_HD void car_unit(uint32_t p, float *c, float *s) {
    HZ_CM_NO_CONTRACT
    const uint32_t pq = p + 0x20000000u, quad = pq >> 30;
    const int32_t rem = (int32_t)(pq & 0x3fffffffu) - 0x20000000;
    const float a = (float)rem * kRad;
    const float z = a * a;
    float pc = __builtin_fmaf(kC3, z, kC2);
    pc = __builtin_fmaf(pc, z, kC1);
    pc = __builtin_fmaf(pc, z, kC0);
    const float ca = __builtin_fmaf(z, pc, 1.0f);
    float ps = __builtin_fmaf(kS2, z, kS1);
    ps = __builtin_fmaf(ps, z, kS0);
    const float az = a * z;
    const float sa = __builtin_fmaf(az, ps, a);
    const bool swap = (quad & 1u) != 0u;
    const float cq = swap ? sa : ca, sq = swap ? ca : sa;
    *c = ((quad + 1u) & 2u) != 0u ? -cq : cq;  // quadrants 1 and 2
    *s = (quad & 2u) != 0u ? -sq : sq;         // quadrants 2 and 3
}

// v != v ? 0 : (int32_t) v, truncating toward zero; |v| <= 2^29 by the parameter check (hz_carrier_plan.h)
HZ_HD int32_t to_i32(float v) { return v != v ? 0 : (int32_t)v; }

template <int MODE> HZ_HD float car_detect(float yr, float yi) {
    HZ_CM_NO_CONTRACT
    float e;
    if (MODE == kTone)
        e = yi;
    else if (MODE == kBpsk)
        e = yr * yi;
    else
        e = (yr < 0.0f ? -yi : yi) - (yi < 0.0f ? -yr : yr);
    return e < -1.0f ? -1.0f : (e > 1.0f ? 1.0f : e);
}

// one sample x through the row's loop: y is the output, the return value the frequency estimate behind this sample
// in cycles per sample.  The sum F + dF is formed modulo 2^32: it cannot leave int32 for a state the loop itself made
// (hz_carrier_plan.h), and a state that hzsdr_carrier_set_state brought wraps as the phase does.
template <int MODE> HZ_HD float car_step(State &st, const Loop &k, tn::c32 x, tn::c32 *y) {
    HZ_CM_NO_CONTRACT
    float c, s;
    car_unit(st.theta, &c, &s);
    const tn::c32 v = tn::tuner_cmul(x, tn::c32{c, -s});
    *y = v;
    const float e = car_detect<MODE>(v.re, v.im);
    const int32_t df = to_i32(k.bw * e), dth = to_i32(k.aw * e);
    int32_t f = (int32_t)((uint32_t)st.f + (uint32_t)df);
    f = f < k.fmin ? k.fmin : f;
    f = f > k.fmax ? k.fmax : f;
    st.f = f;
    st.theta = st.theta + (uint32_t)f + (uint32_t)dth;
    return (float)f * 0x1p-32f;
}

}  // namespace cm
}  // namespace hz

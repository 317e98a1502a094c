// hz_agc_math.h -- the arithmetic of the AGC bank (include/hzsdr_agc.h), HIP-free: the level of a sample, the walk's
// input made of it, one step of the multiplicative gain loop and the output product.  It compiles as
// __host__ __device__ under hipcc and as plain C++17 under g++ (-ffp-contract=off), and both the kernel of hz_agc.hip
// and the restatement of tests/host/agc_ref.cpp evaluate every output, every track value and every state word through
// these functions, so that the host build and the device build compute the same bits.  Nothing here calls libm or the
// device's math library: IEEE float32 *, sqrt and fmaf, each correctly rounded by itself, comparisons and selections.
// The complex level is the demodulator bank's envelope (hz_demod_math.h, demod_envelope).
//
// The step of the header, cut where the gain's history enters:
//   agc_level   a = |x|                                          \  no g in them: the kernel evaluates them with
//   agc_drive   b = a * iref, or a NaN where a < floor           /  lane = sample, off the walk
//   agc_step    e, the clip, r, s, g' and the two clamps         the walk: g -> g, the only loop-carried chain
//   agc_apply   y = x * g                                        lane = sample again, g being the gain BEFORE the step
// The gate rides in b as a NaN: e = fmaf(-NaN, g, 1) is a NaN, no comparison with a NaN holds, so r = decay,
// s = decay * NaN is a NaN and the selection `s != s ? 0 : s` that a NaN SAMPLE needs anyway gives s = 0.  That is
// the header's `(s != s || a < floor) ? 0 : s` for every a, b and g (a NaN level is not under the floor and makes a NaN
// b by itself), and the walk carries no second comparison.  agc_step_plain below is the header's step word for word;
// tests/host/agc_ref.cpp evaluates both at every sample and refuses to go on where their bits differ.
//
// The step is written without a branch: clip, rate, gate and clamps are selections.
//
// Properties (restated in include/hzsdr_agc.h):
//   - denormals are kept: neither build flushes them;
//   - a NaN sample gives a NaN output for THAT sample and holds the gain; an infinity gives e = -1 (fmaf(-inf, g, 1) is
//     -inf for a gain above 0);
//   - a NaN gain stays: fmaf(NaN, s, NaN) is a NaN, and neither clamp's comparison holds for it;
//   - no value of a row reaches another row, an address or a trip count.
#pragma once

#include <stdint.h>

#include "hz_plan.h"
#include "hz_demod_math.h"

#if defined(__clang__)
#define HZ_AM_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define HZ_AM_NO_CONTRACT
#endif

namespace hz {
namespace am {

// the loop's constants of one row, as the kernel sees them (derived by hz_agc_plan.h, derive); g0 stays on the host
struct Loop {
    float iref;           // (float)(1 / (double) ref)
    float attack, decay;  // the rate towards a lower and towards a higher gain
    float floor;          // the hang gate: levels under it hold the gain
    float gmin, gmax;
};

HZ_HD float agc_level(float x) { return __builtin_fabsf(x); }
HZ_HD float agc_level(dm::c32 x) { return dm::demod_envelope(x); }

// the walk's input of a sample of level a: the level in units of ref, a NaN under the gate
HZ_HD float agc_drive(float a, float iref, float floor) {
    HZ_AM_NO_CONTRACT
    const float b = a * iref;
    return a < floor ? __builtin_nanf("") : b;
}

// one sample through the row's loop: the gain behind it, from the gain g applied to it and its drive b
HZ_HD float agc_step(float g, float b, const Loop &k) {
    HZ_AM_NO_CONTRACT
    float e = __builtin_fmaf(-b, g, 1.0f);
    e = e < -1.0f ? -1.0f : e;
    const float r = e < 0.0f ? k.attack : k.decay;
    float s = r * e;
    s = s != s ? 0.0f : s;
    const float gn = __builtin_fmaf(g, s, g);
    return gn < k.gmin ? k.gmin : (gn > k.gmax ? k.gmax : gn);
}

// the header's step word for word, from the level a itself: what agc_step(g, agc_drive(a, ...), k) must equal
HZ_HD float agc_step_plain(float g, float a, const Loop &k) {
    HZ_AM_NO_CONTRACT
    const float b = a * k.iref;
    float e = __builtin_fmaf(-b, g, 1.0f);
    e = e < -1.0f ? -1.0f : e;
    const float r = e < 0.0f ? k.attack : k.decay;
    float s = r * e;
    s = (s != s || a < k.floor) ? 0.0f : s;
    const float gn = __builtin_fmaf(g, s, g);
    return gn < k.gmin ? k.gmin : (gn > k.gmax ? k.gmax : gn);
}

HZ_HD float agc_apply(float x, float g) {
    HZ_AM_NO_CONTRACT
    return x * g;
}
HZ_HD dm::c32 agc_apply(dm::c32 x, float g) {
    HZ_AM_NO_CONTRACT
    dm::c32 y;
    y.re = x.re * g;
    y.im = x.im * g;
    return y;
}

}  // namespace am
}  // namespace hz

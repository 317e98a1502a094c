// hz_agc_plan.h -- the host arithmetic of the AGC bank (include/hzsdr_agc.h), HIP-free so that tests/host/agc_plan.cpp
// can run it under the sanitizers.  The bank is a row-wave bank: how the rows are dealt to waves, the tile and its
// address maps are hz_rowwave_plan.h, with the reasons.  Here: the tile's planes and the LDS request, the validation of
// a row's parameters and the derivation of its constants, and why no step can overflow.
//
// The planes.  Plane kGainPlane = 0 holds the walk's input b when the walk begins and the gain applied to each sample
// when it ends: the walk reads and writes this plane alone, whatever the kind.  The samples lie behind it, untouched
// between the loader and the storer: plane 1 (real rows), planes 1 and 2 (re, im).  The LDS request is
// (1 + planes) T P floats: at most 3 * 256 * 9 * 4 bytes, the carrier bank's figure.
//
// The bounds.  Accepted are finite values with 2^-64 <= ref <= 2^64, 0 <= attack, decay <= 0.5, 0 <= floor and
// 2^-64 <= gmin <= g0 <= gmax <= 2^64.  Then
//   - iref = (float)(1 / (double) ref) lies in [2^-64, 2^64]: the quotient of 1 by a power of two is exact, and
//     rounding is monotonic.  It is a normal float32 above zero;
//   - g is g0 at first and the result of the two clamps behind every sample, so gmin <= g <= gmax.  Behind
//     hzsdr_agc_set_params g still lies in the OLD range, which is inside [2^-64, 2^64] as every range is;
//   - a >= 0 or a NaN (a magnitude), so b = a * iref >= 0, infinite or a NaN, and -b g <= 0: e = fmaf(-b, g, 1) <= 1,
//     rounding being monotonic and 1 a float32.  The clip holds e >= -1.  So e lies in [-1, 1] or is a NaN;
//   - r is attack or decay, in [0, 0.5]: s = r e lies in [-0.5, 0.5] or is a NaN, which the selection turns to 0;
//   - g' = fmaf(g, s, g) = g (1 + s) rounded once lies in [0.5 g, 1.5 g] (monotonic again: 0.5 g and 1.5 g are
//     float32s or round inwards of 1.5 * 2^64 < 2^128): above 2^-65, a normal float32, and finite.  The clamps bring it
//     back into [gmin, gmax].
// No step of the LOOP can overflow or reach zero, whatever the samples.  Two values outside the loop can be infinite
// by the input's doing and are defined so: the level of a complex sample whose squares overflow (an infinity: e = -1,
// the loudest sample there is), and the output x g of a sample above 2^128 / g, an infinity in its own sample.
// Only hzsdr_agc_set_state can bring a g from outside: a finite one is clamped behind the next sample, a NaN stays, and
// an infinity or a zero is held by the gate's selection where -b g is a NaN, else clamped.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "hz_rowwave_plan.h"
#include "hz_agc_math.h"

namespace hz {
namespace ap {

using rw::kMaxRows, rw::kLanes, rw::kWaves, rw::kMaxGroup, rw::kSteps, rw::kLdsBudget;
using rw::wave_first_row, rw::wave_row_count, rw::tile_slot, rw::move_slot, rw::walk_slot;

constexpr uint32_t kParams = 7;  // ref, attack, decay, floor, g0, gmin, gmax
constexpr int kRealF32 = 32, kC64 = 1;  // HZSDR_AGC_REAL_F32, HZSDR_FMT_C64
constexpr uint32_t kGainPlane = 0;   // b before the walk, the applied gain behind it
constexpr uint32_t kSamplePlane = 1; // the sample: this plane (real), this and the next (re, im)
constexpr float kLow = 0x1p-64f, kHigh = 0x1p64f;

struct Geom : rw::Geom {  // (planes: the samples' alone, as in every row-wave bank)
    size_t lds_bytes;
};

// rows: 1 ... kMaxRows
inline Geom agc_geom(uint32_t rows, bool complex_rows) {
    Geom g{rw::geom(rows, complex_rows), 0};
    g.lds_bytes = (size_t)(1u + g.planes) * g.T * g.P * 4;
    return g;
}

// nullptr when the seven values make a loop, else what is wrong with them
inline const char *check_params(const float *q) {
    for (uint32_t k = 0; k < kParams; k++)
        if (!isfinite(q[k])) return "a parameter is not finite";
    if (!(q[0] >= kLow && q[0] <= kHigh)) return "2^-64 <= ref <= 2^64";
    if (!(q[1] >= 0.0f && q[1] <= 0.5f)) return "0 <= attack <= 0.5";
    if (!(q[2] >= 0.0f && q[2] <= 0.5f)) return "0 <= decay <= 0.5";
    if (!(q[3] >= 0.0f)) return "0 <= floor";
    if (!(q[5] >= kLow && q[5] <= q[4] && q[4] <= q[6] && q[6] <= kHigh)) return "2^-64 <= gmin <= g0 <= gmax <= 2^64";
    return nullptr;
}

// (ref, attack, decay, floor, g0, gmin, gmax) -> the row's constants; iref in float64
inline am::Loop derive(const float *q) {
    am::Loop k;
    k.iref = (float)(1.0 / (double)q[0]);
    k.attack = q[1], k.decay = q[2], k.floor = q[3];
    k.gmin = q[5], k.gmax = q[6];
    return k;
}
inline float initial_gain(const float *q) { return q[4]; }

}  // namespace ap
}  // namespace hz

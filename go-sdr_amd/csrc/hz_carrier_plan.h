// hz_carrier_plan.h -- the host arithmetic of the carrier recovery bank (include/hzsdr_carrier.h), HIP-free so that
// tests/host/carrier_plan.cpp can run it under the sanitizers.  The bank is a row-wave bank: how the rows are dealt to
// waves, the tile and its address maps are hz_rowwave_plan.h, with the reasons.  Here: the track plane and the LDS
// request, the derivation and validation of a row's loop constants, and the indices of the kept state.
//
// The bounds.  Accepted are finite values with 0 <= alpha, beta <= 0.125 and -0.25 <= fmin <= f0 <= fmax <= 0.25.  Then
//   - alpha_w = (float)(alpha 2^32) <= 2^29 and beta_w likewise: 0.125 * 2^32 = 2^29 is a float32, and rounding is
//     monotonic.  The error is clipped to [-1, 1] (or is a NaN), so each of the products beta_w e and alpha_w e is one
//     float32 product of magnitude at most 2^29 (or a NaN): to_i32 is defined, and |dF|, |dtheta| <= 2^29;
//   - Fmin, F0, Fmax = llrint(f 2^32) lie in [-2^30, 2^30] and keep their order (llrint is monotonic);
//   - F is F0 at first and the result of the clamp behind every sample, so Fmin <= F <= Fmax, and
//     |F + dF| <= 2^30 + 2^29 < 2^31: the sum of step 4 stays inside int32.  Behind hzsdr_carrier_set_params F still
//     lies in the OLD range, which is inside [-2^30, 2^30] as every range is: the same bound holds;
//   - theta is a uint32 that wraps by definition.
// Only hzsdr_carrier_set_state can bring an F from outside; the step forms the sum modulo 2^32 (hz_carrier_math.h), so
// that such a state wraps and nothing is undefined.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "hz_rowwave_plan.h"
#include "hz_carrier_math.h"

namespace hz {
namespace cp {

using rw::kMaxRows, rw::kLanes, rw::kWaves, rw::kMaxGroup, rw::kSteps, rw::kLdsBudget;
using rw::wave_first_row, rw::wave_row_count, rw::tile_slot, rw::move_slot, rw::walk_slot;

constexpr uint32_t kParams = 5;  // alpha, beta, f0, fmin, fmax
constexpr uint32_t kModes = 3;
constexpr uint32_t kStateWords = 2;  // theta, F
constexpr uint32_t kTrackPlane = 2;  // the track's plane of the tile, behind re and im

struct Geom : rw::Geom {
    size_t lds_bytes;
};

// rows: 1 ... kMaxRows; track: the third plane is asked for
inline Geom carrier_geom(uint32_t rows, bool track) {
    Geom g{rw::geom(rows, true), 0};
    g.lds_bytes = (size_t)(g.planes + (track ? 1u : 0u)) * g.T * g.P * 4;
    return g;
}

// nullptr when the five values make a loop, else what is wrong with them
inline const char *check_params(const float *q) {
    for (uint32_t k = 0; k < kParams; k++)
        if (!isfinite(q[k])) return "a parameter is not finite";
    if (!(q[0] >= 0.0f && q[0] <= 0.125f)) return "0 <= alpha <= 0.125";
    if (!(q[1] >= 0.0f && q[1] <= 0.125f)) return "0 <= beta <= 0.125";
    if (!(q[3] >= -0.25f && q[3] <= q[2] && q[2] <= q[4] && q[4] <= 0.25f)) return "-0.25 <= fmin <= f0 <= fmax <= 0.25";
    return nullptr;
}

// (alpha, beta, f0, fmin, fmax) -> alpha_w, beta_w = (float)(gain 2^32), F0, Fmin, Fmax = llrint(f 2^32), in float64
inline cm::Loop derive(const float *q) {
    const double two32 = 4294967296.0;
    cm::Loop k;
    k.aw = (float)((double)q[0] * two32);
    k.bw = (float)((double)q[1] * two32);
    k.f0 = (int32_t)llrint((double)q[2] * two32);
    k.fmin = (int32_t)llrint((double)q[3] * two32);
    k.fmax = (int32_t)llrint((double)q[4] * two32);
    return k;
}

// ---- the kept state (include/hzsdr_carrier.h): row-major, per row theta, F (the int32's bits) ----
HZ_HD size_t state_index(size_t row, uint32_t word) { return row * kStateWords + word; }
inline size_t state_words(uint32_t rows) { return (size_t)rows * kStateWords; }

}  // namespace cp
}  // namespace hz

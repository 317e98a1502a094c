/*
 * hzsdr_agc.h -- the AGC bank of libhzsdr_hip: a level-independent gain loop over one row, or over many rows at once,
 * one output per input of the input's type.  It is the next member of the family of hzsdr_tuner.h, hzsdr_iir.h,
 * hzsdr_carrier.h and hzsdr_symsync.h and stands between them: a tuner channel of unknown and drifting level goes in,
 * a row at the level `ref` comes out, and the carrier recovery bank and the symbol-timing bank, whose detectors are
 * amplitude-dependent, run at the loop gains they were designed for.  What it leaves to others: a level measured in a
 * filter of its own (the loop IS the level detector: ref / g is the row's level), look-ahead, a squelch output.
 *
 * The entries live beside hzsdr.h and the other headers (same conventions, same status codes, same context).  The
 * reference has no AGC: the definition below is the contract, restated under tests/.
 *
 * Input: `rows` = R rows, 1 <= R <= 8192, of n samples each.
 * Kind: HZSDR_AGC_REAL_F32 (real float32 rows: the demodulator's or the IIR bank's block as it is) or HZSDR_FMT_C64
 * (complex64 rows: the tuner bank's, the resampler's or the carrier bank's block as it is).
 * Parameters: seven finite float32 values ref, attack, decay, floor, g0, gmin, gmax -- the level to hold, the rate
 * towards a lower gain and the rate towards a higher gain (per sample, as a fraction of the gain), the hang gate, the
 * initial gain and its range -- either one set shared by all rows (7 values) or one per row (R * 7 values, row-major),
 * with
 *       2^-64 <= ref <= 2^64,   0 <= attack <= 0.5,   0 <= decay <= 0.5,   0 <= floor,
 *       2^-64 <= gmin <= g0 <= gmax <= 2^64.
 * From them, computed in float64:  iref = (float)(1.0 / (double) ref).
 *
 * State of a row: one float32, the gain g.  At create and reset g = g0, position 0.  For every input sample x, in
 * order, every operation ONE float32 operation, no contraction beyond the two fmaf written out:
 *       a  = |x|              real: fabsf(x);  complex: sqrtf(x.re * x.re + x.im * x.im), the demodulator bank's envelope
 *       b  = a * iref
 *       y  = x * g            real: x * g;  complex: (x.re * g, x.im * g)                 the output
 *       track = g             where a track output was asked for: the gain APPLIED to this sample (ref / track is
 *                             the row's level as the loop sees it)
 *       e  = fmaf(-b, g, 1)   = 1 - |y| / ref up to rounding
 *       e  = e < -1 ? -1 : e
 *       r  = e < 0 ? attack : decay
 *       s  = r * e
 *       s  = (s != s || a < floor) ? 0 : s        a NaN error, or a level under the gate: the gain holds
 *       g' = fmaf(g, s, g)                        multiplicative: g (1 + r e), a factor in [0.5, 1.5]
 *       g  = g' < gmin ? gmin : (g' > gmax ? gmax : g')
 * The loop is multiplicative so that its settling time in samples does not depend on the input's level: from a level
 * A times too low the gain grows by (1 + decay) per sample, ln A / ln(1 + decay) samples, and then closes the last
 * 5 % in ln 20 / decay; from a level A times too high the clipped error shrinks it by (1 - attack) per sample.  (An
 * additive loop g += r (ref - |y|) has a loop gain proportional to the level.)  hz.agc_rates turns time constants in
 * samples into the two rates.
 * `floor` is the hang gate: a row that falls silent keeps its gain instead of winding up to gmax on noise.  floor = 0
 * disables it.
 * No step of the loop can overflow or reach zero: e lies in [-1, 1] (b g >= 0 and the clip), |s| <= 0.5,
 * g' lies in [0.5 g, 1.5 g] with g in [2^-64, 2^64] (csrc/hz_agc_plan.h derives it).  Outside the loop, the level of a
 * complex sample whose squares overflow is an infinity (e = -1), and an output x g above the float32 range is an
 * infinity in its own sample.
 * Denormals are kept; nothing is flushed to zero.
 * A NaN in a sample gives a NaN output for THAT sample and nothing else: e and s are NaN, s becomes 0 and g holds (which
 * bits the NaN has is not part of the contract).  An infinite sample gives an infinite (or, complex with a zero
 * component, partly NaN) output for its sample and e = -1.  A NaN gain brought by hzsdr_agc_set_state stays: every
 * output of the row is a NaN until a set_state or a reset replaces it.
 * Bit parity with the host restatement of tests/host/agc_ref.cpp over csrc/hz_agc_math.h: outputs, track and state.
 * Invariance: outputs, track and state do not depend on how the stream is cut into pushes, on the memory space, on R, on
 * any pitch, on the other rows' contents, on whether the track is asked for, on in place or not, or on shared versus
 * per-row parameters of equal values.
 * Speed: the loop is sequential along a row, so ONE row runs at one lane's rate; the parallelism is across the rows.
 * Layout:
 *   - row r of the input starts r * in_stride SAMPLES into `in`; row r's outputs start r * out_stride samples into
 *     `out`, row r's track r * track_stride float32 into `track`; the strides are ignored when R = 1;
 *   - the state, as hzsdr_agc_get_state / _set_state move it, is one float32 per row, the gain.
 */
#ifndef HZSDR_AGC_H
#define HZSDR_AGC_H

#include "hzsdr.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hzsdr_agc hzsdr_agc;

/* the input kind of real float32 rows (the IIR and the symbol-timing bank's value); complex rows are HZSDR_FMT_C64 */
#define HZSDR_AGC_REAL_F32 32

#define HZSDR_AGC_MAX_ROWS 8192
#define HZSDR_AGC_PARAMS 7

/* hzsdr_agc_plan's `form`: _PER_ROW: every row has parameters of its own (they are per lane; without it they are
 * wave-uniform scalars); _COMPLEX: complex64 rows. */
#define HZSDR_AGC_FORM_PER_ROW 1
#define HZSDR_AGC_FORM_COMPLEX 2

/* A bank over `rows` rows of `kind` with the parameters `params`: 7 float32 host values ref, attack, decay, floor, g0,
 * gmin, gmax, or rows * 7 when per_row is not zero (free to go when this returns).  The state is the initial one, the
 * position 0.  HZSDR_ERR_FORMAT_UNKNOWN for another kind; HZSDR_ERR_INVALID_ARGUMENT for rows out of range, null
 * params, a parameter that is not finite or out of its range. */
int hzsdr_agc_create(hzsdr_ctx *ctx, int kind, const float *params, int per_row, size_t rows, hzsdr_agc **out);
/* Run all n samples of every row through the loop.  Row r's outputs go to out + r * out_stride, n of them; columns
 * from n up to out_stride are left untouched.  `out` may be `in` (with out_stride == in_stride when rows > 1): the rows
 * are levelled in place; otherwise the two must not overlap.  `track`, when not null, takes n float32 per row at
 * track + r * track_stride; it is in the context's memory space as `out` is.
 * HZSDR_ERR_DST_TOO_SMALL when rows > 1 and out_stride, or track_stride with a track, is below n;
 * HZSDR_ERR_INVALID_ARGUMENT for rows > 1 with in_stride < n, null in or out with n > 0: decided before anything is
 * launched, the state is unchanged.
 * Stream-ordered on the context's stream; HOST contexts stage `in`, `out` and `track`. */
int hzsdr_agc_push(hzsdr_agc *a, const void *in, size_t n, size_t in_stride, void *out, size_t out_stride, float *track, size_t track_stride);
/* Exchange the parameters between two pushes, in the same form and count as create; g and the position stay (g is
 * held to the new range BEHIND the next sample: that sample still sees the gain it had).  Everything is validated
 * before anything changes. */
int hzsdr_agc_set_params(hzsdr_agc *a, const float *params);
/* Copy the state (one gain per row) into the host array `state` of `cap` floats, behind every push so far.
 * HZSDR_ERR_DST_TOO_SMALL when cap is below rows. */
int hzsdr_agc_get_state(hzsdr_agc *a, float *state, size_t cap);
/* Replace the state by the host array `state` of exactly `rows` floats and set the position.  The values are taken as
 * they are. */
int hzsdr_agc_set_state(hzsdr_agc *a, const float *state, size_t count, uint64_t position);
/* Samples consumed per row since create, reset or the position given to set_state. */
int hzsdr_agc_position(const hzsdr_agc *a, uint64_t *position);
/* The rows one wave owns (the last wave may own fewer; wave w owns rows [w * rows_per_wave, ...)), the samples of a
 * tile and the form (HZSDR_AGC_FORM_*), so that tests can aim at edges. */
int hzsdr_agc_plan(const hzsdr_agc *a, size_t *rows_per_wave, size_t *tile_samples, int *form);
/* Back to position 0 with the initial state (g = g0 of the parameters in force); the parameters stay. */
int hzsdr_agc_reset(hzsdr_agc *a);
int hzsdr_agc_free(hzsdr_agc *a);

#ifdef __cplusplus
}
#endif

#endif /* HZSDR_AGC_H */

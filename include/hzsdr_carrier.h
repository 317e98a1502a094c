/*
 * hzsdr_carrier.h -- the carrier recovery bank of libhzsdr_hip: a second-order loop around a numerically controlled
 * oscillator over one complex64 row, or over many rows at once, one derotated complex64 output per input.  It is the
 * next member of the family of hzsdr_tuner.h, hzsdr_iir.h and hzsdr_symsync.h and takes their complex64 rows as they
 * are: a tuner channel that is never exactly on frequency goes in, a row whose residual carrier offset and phase the
 * loop has removed comes out, and hzsdr_symsync.h makes coherent soft symbols of it.  The detectors are
 * AMPLITUDE-DEPENDENT, as the Gardner detector is: the AGC bank of hzsdr_agc.h in front brings the rows to unit symbol
 * amplitude (or scale the gains by the amplitude -- by its square for BPSK).  What it leaves to others:
 * decision-directed detectors for 8PSK or QAM, a lock indicator.
 *
 * The entries live beside hzsdr.h and the other headers (same conventions, same status codes, same context).  The
 * reference has no carrier recovery: the definition below is the contract, restated under tests/.
 *
 * Input: `rows` = R rows, 1 <= R <= 8192, of n complex64 samples each.
 * Mode: the phase detector, one for all rows: HZSDR_CARRIER_TONE, _BPSK or _QPSK.
 * Parameters: five finite float32 values alpha, beta, f0, fmin, fmax -- the proportional and the integral gain in turns
 * per unit error, the initial frequency and its range in cycles per sample -- either one set shared by all rows (5
 * values) or one per row (R * 5 values, row-major), with 0 <= alpha, beta <= 0.125 and
 * -0.25 <= fmin <= f0 <= fmax <= 0.25.  From them, each computed in float64:
 *       alpha_w = (float)(alpha 2^32),  beta_w = (float)(beta 2^32),  F0, Fmin, Fmax = llrint(f 2^32).
 *
 * State of a row: theta, a uint32 phase, 2^32 to the turn, and F, an int32 frequency in phase units per sample.  At
 * create and reset theta = 0, F = F0, position 0.  For every input sample x, in order:
 *       (c, s) = car_unit(theta)
 *       y = x (c - i s):  y.re = fmaf(x.re, c, -(x.im * -s)),  y.im = fmaf(x.re, -s, x.im * c)        the output
 *       e = y.im                                                      HZSDR_CARRIER_TONE: a pilot, a residual
 *                                                                     carrier, FM by PLL
 *           y.re * y.im                                               HZSDR_CARRIER_BPSK
 *           (y.re < 0 ? -y.im : y.im) - (y.im < 0 ? -y.re : y.re)     HZSDR_CARRIER_QPSK
 *       e = e < -1 ? -1 : (e > 1 ? 1 : e)
 *       dF = to_i32(beta_w * e);  dtheta = to_i32(alpha_w * e)        each ONE float32 product;
 *                                                                     to_i32(v) = v != v ? 0 : (int32_t) v
 *       F = min(Fmax, max(Fmin, F + dF))                              in int32
 *       theta = theta + (uint32) F + (uint32) dtheta                  wrapping
 *       track = (float) F * 2^-32                                     where a track output was asked for: the
 *                                                                     frequency estimate behind this sample, in
 *                                                                     cycles per sample
 *   car_unit(p), without a table and without libm (csrc/hz_carrier_math.h has the coefficients, as hex floats):
 *       pq = p + 2^29 (wrapping);  quad = pq >> 30;  rem = (int32)(pq & 0x3fffffff) - 2^29
 *       a = (float) rem * (float)(2 pi / 2^32);  z = a * a
 *       cos a = fmaf(z, C(z), 1), C a cubic;  sin a = fmaf(a * z, S(z), a), S a quadratic; both by Horner's rule in fmaf
 *       quad 0: (cos a, sin a);  1: (-sin a, cos a);  2: (-cos a, -sin a);  3: (sin a, -cos a)
 *     On the four axes the values are exactly 0 and 1 in magnitude.  Its largest error against float64 over all 2^32
 *     phase words is 1.294e-07, the tuner bank's three-table rotator's 1.605e-07.
 * No step can overflow: |beta_w e|, |alpha_w e| <= 2^29, |F| <= 2^30, |F + dF| < 2^31 (csrc/hz_carrier_plan.h derives
 * it).  A state that hzsdr_carrier_set_state brings from outside these bounds wraps modulo 2^32.
 * Denormals are kept; nothing is flushed to zero.
 * A NaN in a sample gives a NaN output for THAT sample and nothing else: e is NaN, dF = dtheta = 0, F stays and theta
 * moves on by F, as it does for a sample of zero error.  A NaN stays in its sample as well as in its row (which bits
 * the NaN has is not part of the contract).  An infinity gives an output of infinities or NaNs for its sample and an
 * error of -1, +1 or NaN.
 * Bit parity with the host restatement of tests/host/carrier_ref.cpp over csrc/hz_carrier_math.h: outputs, track and
 * state.
 * Invariance: outputs, track and state do not depend on how the stream is cut into pushes, on the memory space, on R, on
 * any pitch, on the other rows' contents, on whether the track is asked for, on in place or not, or on shared versus
 * per-row parameters of equal values.
 * Speed: the loop is sequential along a row, so ONE row runs at one lane's rate; the parallelism is across the rows.
 * Layout:
 *   - row r of the input starts r * in_stride SAMPLES into `in`; row r's outputs start r * out_stride complex64 into
 *     `out`, row r's track r * track_stride float32 into `track`; the strides are ignored when R = 1;
 *   - the state, as hzsdr_carrier_get_state / _set_state move it, is row-major: per row the two uint32 words theta and
 *     F (the int32's bits).  F * 2^-32 is the measured offset in cycles per sample.
 */
#ifndef HZSDR_CARRIER_H
#define HZSDR_CARRIER_H

#include "hzsdr.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hzsdr_carrier hzsdr_carrier;

#define HZSDR_CARRIER_TONE 0
#define HZSDR_CARRIER_BPSK 1
#define HZSDR_CARRIER_QPSK 2

#define HZSDR_CARRIER_MAX_ROWS 8192

/* hzsdr_carrier_plan's `form`: _PER_ROW: every row has parameters of its own (they are per lane; without it they are
 * wave-uniform scalars), plus the mode times HZSDR_CARRIER_FORM_MODE. */
#define HZSDR_CARRIER_FORM_PER_ROW 1
#define HZSDR_CARRIER_FORM_MODE 2

/* A bank over `rows` complex64 rows with the detector `mode` and the parameters `params`: 5 float32 host values alpha,
 * beta, f0, fmin, fmax, or rows * 5 when per_row is not zero (free to go when this returns).  The state is the initial
 * one, the position 0.  HZSDR_ERR_INVALID_ARGUMENT for an unknown mode, rows out of range, null params, a parameter
 * that is not finite or out of its range. */
int hzsdr_carrier_create(hzsdr_ctx *ctx, int mode, const float *params, int per_row, size_t rows, hzsdr_carrier **out);
/* Run all n samples of every row through the loop.  Row r's outputs go to out + r * out_stride, n of them; columns
 * from n up to out_stride are left untouched.  `out` may be `in` (with out_stride == in_stride when rows > 1): the rows
 * are derotated in place; otherwise the two must not overlap.  `track`, when not null, takes n float32 per row at
 * track + r * track_stride; it is in the context's memory space as `out` is.
 * HZSDR_ERR_DST_TOO_SMALL when rows > 1 and out_stride, or track_stride with a track, is below n;
 * HZSDR_ERR_INVALID_ARGUMENT for rows > 1 with in_stride < n, null in or out with n > 0: decided before anything is
 * launched, the state is unchanged.
 * Stream-ordered on the context's stream; HOST contexts stage `in`, `out` and `track`. */
int hzsdr_carrier_push(hzsdr_carrier *c, const void *in, size_t n, size_t in_stride, void *out, size_t out_stride, float *track,
                       size_t track_stride);
/* Exchange the parameters between two pushes, in the same form and count as create; theta, F and the position stay (F
 * is held to the new range at the next sample).  Everything is validated before anything changes. */
int hzsdr_carrier_set_params(hzsdr_carrier *c, const float *params);
/* Copy the state (the layout above) into the host array `state` of `cap` words, behind every push so far.
 * HZSDR_ERR_DST_TOO_SMALL when cap is below rows * 2. */
int hzsdr_carrier_get_state(hzsdr_carrier *c, uint32_t *state, size_t cap);
/* Replace the state by the host array `state` of exactly rows * 2 words and set the position.  The values are taken
 * as they are. */
int hzsdr_carrier_set_state(hzsdr_carrier *c, const uint32_t *state, size_t count, uint64_t position);
/* Samples consumed per row since create, reset or the position given to set_state. */
int hzsdr_carrier_position(const hzsdr_carrier *c, uint64_t *position);
/* The rows one wave owns (the last wave may own fewer; wave w owns rows [w * rows_per_wave, ...)), the samples of a
 * tile and the form (HZSDR_CARRIER_FORM_*), so that tests can aim at edges. */
int hzsdr_carrier_plan(const hzsdr_carrier *c, size_t *rows_per_wave, size_t *tile_samples, int *form);
/* Back to position 0 with the initial state (theta = 0, F = F0 of the parameters in force); the parameters stay. */
int hzsdr_carrier_reset(hzsdr_carrier *c);
int hzsdr_carrier_free(hzsdr_carrier *c);

#ifdef __cplusplus
}
#endif

#endif /* HZSDR_CARRIER_H */

/*
 * hzsdr_iir.h -- the IIR bank of libhzsdr_hip: a cascade of biquads over one row, or over many rows at once, real or
 * complex.  It is the next member of the family of hzsdr_channelizer.h, hzsdr_resampler.h, hzsdr_demod.h and
 * hzsdr_tuner.h and takes their rows as they are: the demodulator's real float32 block (FM de-emphasis, a DC blocker
 * behind an envelope detector, a CTCSS notch, a one-pole smoother that turns the power detector into a squelch
 * level) and any complex block (a DC blocker in front of the FM detector of a direct-conversion front end).
 *
 * The entries live beside hzsdr.h and the other headers (same conventions, same status codes, same context).  The
 * reference has no recursive filter: the definition below is the contract, restated under tests/.
 *
 * Input: `rows` = R rows, 1 <= R <= 8192, of n samples each, of one of two kinds:
 *   - complex: a source format of hzsdr.h (u8, i8, i16, c64; iq.go:110-126), converted by hzsdr_convert's c(.)
 *     (iq_c64.go:77-117); the output is complex64;
 *   - real: HZSDR_IIR_REAL_F32, float32 in and float32 out.
 * Cascade: S sections, 1 <= S <= 8, each five finite float32 coefficients b0 b1 b2 a1 a2 in that order, a0 = 1
 * divided out by the caller.  Either one cascade shared by all rows (S * 5 values) or one per row (R * S * 5 values,
 * row-major: row, section, coefficient).
 * Section step, transposed direct form II, every operation ONE float32 operation rounded by itself:
 *       y  = fmaf(b0, x, z1)
 *       t  = fmaf(b1, x, z2)
 *       z1 = fmaf(-a1, y, t)
 *       u  = b2 * x
 *       z2 = fmaf(-a2, y, u)
 *   - section s + 1 takes section s's y as its x; the last y is the output;
 *   - z1 = z2 = +0 at position 0 (create, reset);
 *   - a complex row is two such recursions, re and im, with the same real coefficients;
 *   - one output per input: no decimation, nothing to flush.
 * Denormals are kept (a decaying tail runs through them to +0); nothing is flushed to zero.
 * Bit parity (with the host restatement of tests/host/iir_ref.cpp over csrc/hz_iir_math.h) is defined for finite
 * inputs whose states stay finite.  A NaN or an infinity propagates as one, its bits are not part of the contract,
 * and IT POISONS ITS ROW -- the state keeps it -- until hzsdr_iir_reset or hzsdr_iir_set_state; the other rows are
 * not touched by it.
 * Invariance: the bits do not depend on how the stream is cut into pushes, on the memory space, on R, on either pitch
 * or on the other rows' contents, on shared versus per-row coefficients of equal values, or on the run.
 * Speed: the definition is exact and sequential along a row, so ONE row runs at one lane's rate whatever its length;
 * the parallelism is across the rows.  There is no block form: it would change the rounding.
 * Layout:
 *   - row r of the input starts r * in_stride SAMPLES into `in`; row r of the output starts r * out_stride samples
 *     (float32 or complex64) into `out`; both strides are ignored when R = 1;
 *   - the state, as hzsdr_iir_get_state / _set_state move it, is R * S * 2 floats for real rows, index
 *     (r * S + s) * 2 + z with z = 0 for z1 and 1 for z2, and R * S * 4 floats for complex rows, index
 *     ((r * S + s) * 2 + z) * 2 + p with p = 0 for re and 1 for im: row, section, z1 / z2, re / im.
 */
#ifndef HZSDR_IIR_H
#define HZSDR_IIR_H

#include "hzsdr.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hzsdr_iir hzsdr_iir;

/* The input kind of real float32 rows, beside the four source formats of hzsdr.h (1 ... 4). */
#define HZSDR_IIR_REAL_F32 32

#define HZSDR_IIR_MAX_SECTIONS 8
#define HZSDR_IIR_MAX_ROWS 8192

/* hzsdr_iir_plan's `form`: a sum of these.  _PER_ROW: every row has a cascade of its own (the coefficients are per
 * lane; without it they are wave-uniform scalars).  _COMPLEX: two recursions per row. */
#define HZSDR_IIR_FORM_PER_ROW 1
#define HZSDR_IIR_FORM_COMPLEX 2

/* A bank over `rows` rows of kind_or_format samples with the cascade `sections`: n_sections * 5 float32 host values,
 * or rows * n_sections * 5 when per_row is not zero (free to go when this returns).  The state is zero, the position 0.
 * HZSDR_ERR_INVALID_ARGUMENT for n_sections or rows out of range, a non-finite coefficient, null sections;
 * HZSDR_ERR_FORMAT_UNKNOWN for a kind that is neither a source format nor HZSDR_IIR_REAL_F32. */
int hzsdr_iir_create(hzsdr_ctx *ctx, int kind_or_format, const float *sections, size_t n_sections, int per_row, size_t rows,
                     hzsdr_iir **out);
/* Filter all n samples of every row: *written = n outputs per row, float32 for real rows and complex64 otherwise;
 * columns [n, out_stride) of a row are left untouched.  in == out with equal strides is allowed for HZSDR_IIR_REAL_F32
 * and HZSDR_FMT_C64 (the rows are filtered in place).  HZSDR_ERR_DST_TOO_SMALL when out_cap is below n, or when
 * rows > 1 and out_stride is below n; HZSDR_ERR_INVALID_ARGUMENT for rows > 1 with in_stride < n, and for in == out
 * with another format or unequal strides: decided before anything is launched, the state is unchanged.
 * Stream-ordered on the context's stream; HOST contexts stage `in` and `out` (pitched rows by a 2-D copy). */
int hzsdr_iir_push(hzsdr_iir *iir, const void *in, size_t n, size_t in_stride, void *out, size_t out_cap, size_t out_stride,
                   size_t *written);
/* Exchange the coefficients between two pushes; the state and the position stay, so that a notch is retuned without
 * a click.  `sections` as for create, with the SAME n_sections and form.  Everything is validated before anything
 * changes: HZSDR_ERR_INVALID_ARGUMENT for another count, a non-finite coefficient, null sections. */
int hzsdr_iir_set_sections(hzsdr_iir *iir, const float *sections, size_t n_sections);
/* Copy the state (the layout above) into the host array `state` of `cap` floats, behind every push so far.
 * HZSDR_ERR_DST_TOO_SMALL when cap is below the state's floats. */
int hzsdr_iir_get_state(hzsdr_iir *iir, float *state, size_t cap);
/* Replace the state by the host array `state` of exactly the state's `count` floats and set the position.  The values
 * are taken as they are (this is how a poisoned row is healed). */
int hzsdr_iir_set_state(hzsdr_iir *iir, const float *state, size_t count, uint64_t position);
/* Samples consumed per row since create, reset or the position given to set_state. */
int hzsdr_iir_position(const hzsdr_iir *iir, uint64_t *position);
/* The rows one wave owns (the last wave may own fewer; wave w owns rows [w * rows_per_wave, ...)), the samples of a
 * tile (tile t of a push holds its samples [t * tile_samples, (t + 1) * tile_samples)) and the form (HZSDR_IIR_FORM_*),
 * so that tests can aim at edges. */
int hzsdr_iir_plan(const hzsdr_iir *iir, size_t *rows_per_wave, size_t *tile_samples, int *form);
/* Back to position 0 with a zero state; the coefficients stay. */
int hzsdr_iir_reset(hzsdr_iir *iir);
int hzsdr_iir_free(hzsdr_iir *iir);

#ifdef __cplusplus
}
#endif

#endif /* HZSDR_IIR_H */

/*
 * hzsdr_equalizer.h -- the adaptive equalizer bank of libhzsdr_hip: an N-tap linear equalizer at the symbol rate over one
 * row of soft symbols, or over many rows at once, adapted blind (the constant modulus algorithm) or on its own decisions
 * (decision-directed LMS), one output per symbol consumed, of the input's type.  It is the next member of the family of
 * hzsdr_tuner.h, hzsdr_iir.h, hzsdr_agc.h, hzsdr_carrier.h and hzsdr_symsync.h and stands between the symbol-timing
 * bank and the frame sync bank: hzsdr_symsync_push's (symbols, counts) go in as they are, the equalized symbols and the
 * SAME counts go on into hzsdr_framesync_push or hzsdr_softframe_push, with no host read in between.  It removes the
 * inter-symbol interference that multipath, a mismatched matched filter or a receiver's IF ripple leave in the symbols.
 * What it leaves to others: fractionally spaced (T/2) input, trained (known-symbol) adaptation, decision feedback, tap
 * leakage.
 *
 * The entries live beside hzsdr.h and the other headers (same conventions, same status codes, same context).  The
 * reference has no equalizer: the definition below is the contract, restated under tests/.
 *
 * Input: `rows` = R rows, 1 <= R <= 8192, of up to n soft symbols each, one sample per symbol.
 * Kind: HZSDR_EQUALIZER_REAL_F32 (real float32 rows, real taps) or HZSDR_FMT_C64 (complex64 rows, complex taps).
 * Counts: `in_counts`, when not null, is one uint32 per row in the context's memory space -- the symbol-timing bank's
 * `counts` as they are.  Row r consumes min(in_counts[r], n) symbols (n with in_counts null) and writes as many outputs;
 * the columns behind a row's count are left untouched and the counts are not rewritten: the frame sync bank reads the
 * same array next to this bank's output.  Nothing depends on a position, so none is offered.
 * Geometry, fixed at create: N taps, 1 <= N <= 64; a centre index c, 0 <= c < N; a mode, HZSDR_EQUALIZER_CMA,
 * HZSDR_EQUALIZER_DD_BPSK or HZSDR_EQUALIZER_DD_QPSK (complex rows only).
 * Parameters: two finite float32 values mu, level -- the step, and the CMA modulus squared or the decisions' amplitude
 * per component in the DD modes -- either one set shared by all rows (2 values) or one per row (R * 2 values,
 * row-major), with
 *       0 <= mu <= 1,   2^-64 <= level <= 2^64.
 *
 * State of a row: the taps w[0 ... N-1], then the N - 1 latest inputs, newest first.  At create and reset w[c] = 1,
 * every other tap is +0 and the inputs before the stream's start are +0.  For every new symbol x of a COMPLEX row, in
 * order, with X[0] = x, X[i] the i-th previous input and Np = N rounded up to a power of two, every operation ONE float32
 * operation, no contraction beyond the fmaf written out:
 *   1. the products, for i < N
 *          p[i].re = fmaf(-w[i].im, X[i].im, w[i].re * X[i].re)
 *          p[i].im = fmaf( w[i].im, X[i].re, w[i].re * X[i].im)
 *      and p[i] = (+0, +0) for N <= i < Np;
 *   2. the sum, a butterfly: for s = 1, 2, 4, ... < Np,  p[i] = p[i] + p[i ^ s]  componentwise, over all i at once; then
 *      y = p[0] (all entries are equal bit for bit, since float addition commutes);
 *   3. the error
 *          CMA:       c = level - fmaf(y.im, y.im, y.re * y.re),   e = (c * y.re, c * y.im)
 *          DD_QPSK:   e = (copysignf(level, y.re) - y.re, copysignf(level, y.im) - y.im)
 *          DD_BPSK:   e = (copysignf(level, y.re) - y.re, -y.im)
 *      each component clipped as  v < -1 ? -1 : (v > 1 ? 1 : v),  then  g = (mu * e.re, mu * e.im);
 *   4. the update, for i < N, w[i] += g conj(X[i]):
 *          w.re = fmaf( g.im, X.im, fmaf(g.re, X.re, w.re))
 *          w.im = fmaf(-g.re, X.im, fmaf(g.im, X.re, w.im))
 *   5. the output is y, the value BEFORE the update;
 *   6. track, where a track output was asked for, is fmaf(e.im, e.im, e.re * e.re) of the clipped error;
 *   7. the history moves on by one.
 * REAL rows take the same steps with scalars: p[i] = w[i] * X[i]; CMA e = (level - y * y) * y; DD (HZSDR_EQUALIZER_DD_BPSK)
 * e = copysignf(level, y) - y; w[i] = fmaf(g, X[i], w[i]); track = e * e.
 * With mu = 0 and taps brought by hzsdr_equalizer_set_state the bank is a fixed FIR over many rows; the taps read by
 * hzsdr_equalizer_get_state are the inverse-channel estimate.
 * Denormals are kept; nothing is flushed to zero.
 * Bit parity with the host restatement of tests/host/equalizer_ref.cpp over csrc/hz_equalizer_math.h: outputs, track
 * and state, while the row's inputs, taps and outputs are finite.  A NaN, an infinity or a diverged CMA row garbles its
 * own row, until a reset or a set_state, and nothing else: not another row, not a store behind a row's count, not a
 * trip count.
 * Invariance: outputs, track and state do not depend on how the stream is cut into pushes (pushes shorter than N - 1 and
 * of 0 symbols included), on the memory space, on R, on any pitch, on the other rows or their counts, on whether the track
 * is asked for, on in place or not, or on shared versus per-row parameters of equal values.
 * Speed: the loop is sequential along a row, but the taps of a row are dealt to the lanes of a wave (lane = tap), so a
 * symbol costs about the same whatever N is; the rows run side by side.
 * Layout:
 *   - row r of the input starts r * in_stride SYMBOLS into `in`; row r's outputs start r * out_stride symbols into
 *     `out`, row r's track r * track_stride float32 into `track`; the strides are ignored when R = 1;
 *   - the state, as hzsdr_equalizer_get_state / _set_state move it, is row-major, (2 N - 1) float32 per real row and
 *     twice that per complex row, whose entries are (re, im) pairs.
 */
#ifndef HZSDR_EQUALIZER_H
#define HZSDR_EQUALIZER_H

#include "hzsdr.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hzsdr_equalizer hzsdr_equalizer;

/* the input kind of real float32 rows (the other banks' value); complex rows are HZSDR_FMT_C64 */
#define HZSDR_EQUALIZER_REAL_F32 32

#define HZSDR_EQUALIZER_MAX_ROWS 8192
#define HZSDR_EQUALIZER_MAX_TAPS 64
#define HZSDR_EQUALIZER_PARAMS 2

/* the modes */
#define HZSDR_EQUALIZER_CMA 0
#define HZSDR_EQUALIZER_DD_BPSK 1
#define HZSDR_EQUALIZER_DD_QPSK 2

/* hzsdr_equalizer_plan's `form`: _PER_ROW: every row has parameters of its own; _COMPLEX: complex64 rows. */
#define HZSDR_EQUALIZER_FORM_PER_ROW 1
#define HZSDR_EQUALIZER_FORM_COMPLEX 2

/* A bank over `rows` rows of `kind` with `taps` taps, the centre tap `centre`, the mode `mode` and the parameters
 * `params`: 2 float32 host values mu, level, or rows * 2 when per_row is not zero (free to go when this returns).  The
 * state is the initial one.  HZSDR_ERR_FORMAT_UNKNOWN for another kind; HZSDR_ERR_INVALID_ARGUMENT for rows, taps,
 * centre or mode out of range, HZSDR_EQUALIZER_DD_QPSK with real rows, null params, a parameter that is not finite or
 * out of its range. */
int hzsdr_equalizer_create(hzsdr_ctx *ctx, int kind, int mode, size_t taps, size_t centre, const float *params, int per_row, size_t rows,
                           hzsdr_equalizer **out);
/* Run min(in_counts[r], n) symbols of every row r (n with in_counts null) through the equalizer.  Row r's outputs go
 * to out + r * out_stride; the columns behind the row's count are left untouched.  `out` may be `in` (with
 * out_stride == in_stride when rows > 1): the rows are equalized in place; otherwise the two must not overlap.
 * `track`, when not null, takes the squared clipped error of every symbol at track + r * track_stride, in the same
 * ragged layout; it is in the context's memory space as `out` and `in_counts` are.
 * HZSDR_ERR_DST_TOO_SMALL when rows > 1 and out_stride, or track_stride with a track, is below n;
 * HZSDR_ERR_INVALID_ARGUMENT for rows > 1 with in_stride < n, null in or out with n > 0, in place with unequal
 * strides: decided before anything is launched, the state is unchanged.
 * Stream-ordered on the context's stream; HOST contexts stage `in`, `in_counts`, `out` and `track`. */
int hzsdr_equalizer_push(hzsdr_equalizer *q, const void *in, size_t n, size_t in_stride, const uint32_t *in_counts, void *out, size_t out_stride,
                         float *track, size_t track_stride);
/* Exchange the parameters between two pushes, in the same form and count as create; the state stays.  Everything is
 * validated before anything changes. */
int hzsdr_equalizer_set_params(hzsdr_equalizer *q, const float *params);
/* Copy the state into the host array `state` of `cap` floats, behind every push so far.  HZSDR_ERR_DST_TOO_SMALL when
 * cap is below rows * (2 * taps - 1) (complex rows: twice that). */
int hzsdr_equalizer_get_state(hzsdr_equalizer *q, float *state, size_t cap);
/* Replace the state by the host array `state` of exactly that many floats.  The values are taken as they are. */
int hzsdr_equalizer_set_state(hzsdr_equalizer *q, const float *state, size_t count);
/* The rows one wave owns (the last wave may own fewer; wave w owns rows [w * rows_per_wave, ...)), the symbols of a
 * tile and the form (HZSDR_EQUALIZER_FORM_*), so that tests can aim at edges. */
int hzsdr_equalizer_plan(const hzsdr_equalizer *q, size_t *rows_per_wave, size_t *tile_symbols, int *form);
/* Back to the initial state (w[centre] = 1, everything else +0); the parameters stay. */
int hzsdr_equalizer_reset(hzsdr_equalizer *q);
int hzsdr_equalizer_free(hzsdr_equalizer *q);

#ifdef __cplusplus
}
#endif

#endif /* HZSDR_EQUALIZER_H */

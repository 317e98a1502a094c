/*
 * hzsdr_symsync.h -- the symbol-timing recovery bank of libhzsdr_hip: soft symbols at the symbol rate out of one row, or
 * out of many rows at once, real or complex.  It is the next member of the family of hzsdr_channelizer.h,
 * hzsdr_resampler.h, hzsdr_demod.h, hzsdr_tuner.h and hzsdr_iir.h and takes their rows as they are: the demodulator's or
 * the IIR bank's real float32 block (an FM-detected GMSK or FSK channel: AIS, PMR, POCSAG) and any complex64 block (a
 * BPSK or QPSK carrier).  What it leaves to others: the matched filter in front of it, the carrier (hzsdr_carrier.h),
 * and the decisions, the sync-word search and the frames: the frame sync bank (hzsdr_framesync.h) takes this bank's
 * symbols and counts as they are, on the device.
 *
 * The entries live beside hzsdr.h and the other headers (same conventions, same status codes, same context).  The
 * reference has no timing recovery: the definition below is the contract, restated under tests/.
 *
 * Input: `rows` = R rows, 1 <= R <= 8192, of n samples each, of one of two kinds:
 *   - real: HZSDR_SYMSYNC_REAL_F32, float32 in and float32 symbols out;
 *   - complex: HZSDR_FMT_C64, complex64 in and complex64 symbols out.
 * Parameters: four finite float32 values sps, limit, g_mu, g_omega -- the nominal samples per symbol, the relative
 * range of the period, the two loop gains -- either one set shared by all rows (4 values) or one per row (R * 4
 * values, row-major), with 2 < sps <= 256, 0 <= limit <= 0.25, g_mu >= 0, g_omega >= 0.  From them, each computed in
 * float64 and rounded to float32:  h0 = sps / 2,  hmin = h0 (1 - limit),  hmax = h0 (1 + limit);  and hmin - g_mu,
 * evaluated in float32, must be at least 1: then a sample holds at most one strobe and the counter stays at 0 or above.
 *
 * The loop is a Gardner timing-error detector around a 4-point cubic Lagrange interpolator, advanced once per input
 * sample, every operation ONE float32 operation rounded by itself.  State of a real row: the counter c, the half-period
 * estimate h, flag (0: the next strobe is the mid-symbol one, 1: the symbol one), y_prev, y_mid, and the three latest
 * samples x1, x2, x3, newest first.  At create and reset c = 0, h = h0, flag = 0, everything else +0, position 0.
 * Step for the new sample x0:
 *       if (c < 1) {                                  a strobe lies in [n - 2, n - 1), at the fraction mu = c
 *           y = interp(x3, x2, x1, x0, c)
 *           if (flag == 0) { y_mid = y; adv = h; }
 *           else {
 *               e = (y_prev - y) * y_mid
 *               e = e < -1 ? -1 : (e > 1 ? 1 : e)
 *               h = fmaf(g_omega, e, h);  h = h < hmin ? hmin : (h > hmax ? hmax : h)
 *               adv = fmaf(g_mu, e, h)
 *               emit y;  y_prev = y
 *           }
 *           flag ^= 1;  c = c + adv
 *       }
 *       c = c - 1;  x3 = x2;  x2 = x1;  x1 = x0
 *   interp, between x2 (mu = 0) and x1 (mu = 1):
 *       c3 = fmaf(0.5f, x2 - x1, (1/6.f) * (x0 - x3))
 *       c2 = fmaf(0.5f, x1 + x3, -x2)
 *       c1 = ((x1 - 0.5f * x2) - (1/3.f) * x3) - (1/6.f) * x0
 *       y  = fmaf(fmaf(fmaf(c3, mu, c2), mu, c1), mu, x2)
 *   - a complex row keeps (re, im) pairs for y_prev, y_mid, x1, x2, x3, interpolates re and im separately, and
 *     e = fmaf(y_prev.im - y.im, y_mid.im, (y_prev.re - y.re) * y_mid.re);
 *   - this sign of e locks on the symbol centres (the opposite one locks on the transitions);
 *   - the latency is two samples; there is nothing to flush.
 * Denormals are kept; nothing is flushed to zero.
 * Bit parity (with the host restatement of tests/host/symsync_ref.cpp over csrc/hz_symsync_math.h: symbols, counts and
 * state) is defined for finite inputs.  A NaN or an infinity may silence or garble ITS OWN ROW until
 * hzsdr_symsync_reset or hzsdr_symsync_set_state; its bits are not part of the contract.  It never touches another row,
 * never makes the kernel write outside a row's capacity (every store is guarded by out_cap, and counts[r] never
 * exceeds it) and never changes a trip count: the walk is a fixed loop over the samples.
 * Invariance: symbols, counts and state do not depend on how the stream is cut into pushes, on the memory space, on R,
 * on either pitch, on the other rows' contents, or on shared versus per-row parameters of equal values.
 * Speed: the loop is sequential along a row, so ONE row runs at one lane's rate; the parallelism is across the rows.
 * Output bound: two symbol strobes are at least 2 (hmin - g_mu) apart, so a push of n samples writes at most
 *       floor(n / (2 amin)) + 2
 * symbols per row (0 for n = 0), amin the smallest hmin - g_mu over the rows, taken in float64 less a relative margin
 * of 2^-20 for the float32 counter: hzsdr_symsync_max_symbols.
 * Layout:
 *   - row r of the input starts r * in_stride SAMPLES into `in`; row r's symbols start r * out_stride symbols (float32
 *     or complex64) into `out`; both strides are ignored when R = 1;
 *   - the state, as hzsdr_symsync_get_state / _set_state move it, is row-major: per row c, h, flag (0.0 or 1.0; any
 *     other value counts as 1), y_prev, y_mid, x1, x2, x3 -- 8 floats for a real row, 13 for a complex one, whose five
 *     sample-valued entries are (re, im) pairs.  h is how a caller reads the measured symbol rate: 2 h samples.
 */
#ifndef HZSDR_SYMSYNC_H
#define HZSDR_SYMSYNC_H

#include "hzsdr.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hzsdr_symsync hzsdr_symsync;

/* The input kind of real float32 rows: the SAME value as HZSDR_IIR_REAL_F32 (hzsdr_iir.h), so that one constant names
 * the demodulator's and the IIR bank's block all along the chain. */
#define HZSDR_SYMSYNC_REAL_F32 32

#define HZSDR_SYMSYNC_MAX_ROWS 8192

/* hzsdr_symsync_plan's `form`: a sum of these.  _PER_ROW: every row has parameters of its own (they are per lane;
 * without it they are wave-uniform scalars).  _COMPLEX: (re, im) rows. */
#define HZSDR_SYMSYNC_FORM_PER_ROW 1
#define HZSDR_SYMSYNC_FORM_COMPLEX 2

/* A bank over `rows` rows of `kind` samples with the parameters `params`: 4 float32 host values sps, limit, g_mu,
 * g_omega, or rows * 4 when per_row is not zero (free to go when this returns).  The state is the initial one, the
 * position 0.  HZSDR_ERR_INVALID_ARGUMENT for rows out of range, null params, a parameter that is not finite or out of
 * its range, hmin - g_mu below 1; HZSDR_ERR_FORMAT_UNKNOWN for a kind that is neither HZSDR_SYMSYNC_REAL_F32 nor
 * HZSDR_FMT_C64 (nothing upstream hands this stage u8, i8 or i16 rows). */
int hzsdr_symsync_create(hzsdr_ctx *ctx, int kind, const float *params, int per_row, size_t rows, hzsdr_symsync **out);
/* Run all n samples of every row through the loop.  Row r's symbols go to out + r * out_stride; counts[r] (uint32,
 * `rows` of them, in the context's memory space as `out` is) is the number written for row r by THIS push; columns
 * from counts[r] up to out_stride are left untouched.  *max_written, when not null, is the largest count (the call
 * then waits for the stream).  n = 0 writes counts of 0.  `out` must not overlap `in`.
 * HZSDR_ERR_DST_TOO_SMALL when out_cap is below hzsdr_symsync_max_symbols(n), or when rows > 1 and out_stride is
 * below it; HZSDR_ERR_INVALID_ARGUMENT for rows > 1 with in_stride < n, null in, out or counts with n > 0: decided
 * before anything is launched, the state is unchanged.
 * Stream-ordered on the context's stream; HOST contexts stage `in`, `out` and `counts`. */
int hzsdr_symsync_push(hzsdr_symsync *s, const void *in, size_t n, size_t in_stride, void *out, size_t out_cap, size_t out_stride,
                       uint32_t *counts, size_t *max_written);
/* The output bound above for a push of n samples. */
int hzsdr_symsync_max_symbols(const hzsdr_symsync *s, size_t n, size_t *bound);
/* Exchange the parameters between two pushes, in the same form and count as create; the state and the position stay
 * (h is held to the new range at the next symbol).  Everything is validated before anything changes.
 * The bound of the NEW parameters holds for the pushes that follow: one mid-symbol advance may still be the old h,
 * which is at least 1 as every accepted h is, so one interval between two symbols may be as short as 1 + amin, and
 * the "+ 2" of the bound covers one such interval in a push (tests/host/symsync_plan.cpp walks it). */
int hzsdr_symsync_set_params(hzsdr_symsync *s, const float *params);
/* Copy the state (the layout above) into the host array `state` of `cap` floats, behind every push so far.
 * HZSDR_ERR_DST_TOO_SMALL when cap is below the state's floats. */
int hzsdr_symsync_get_state(hzsdr_symsync *s, float *state, size_t cap);
/* Replace the state by the host array `state` of exactly the state's `count` floats and set the position.  The values
 * are taken as they are (this is how a silenced row is healed). */
int hzsdr_symsync_set_state(hzsdr_symsync *s, const float *state, size_t count, uint64_t position);
/* Samples consumed per row since create, reset or the position given to set_state. */
int hzsdr_symsync_position(const hzsdr_symsync *s, uint64_t *position);
/* The rows one wave owns (the last wave may own fewer; wave w owns rows [w * rows_per_wave, ...)), the samples of a
 * tile and the form (HZSDR_SYMSYNC_FORM_*), so that tests can aim at edges. */
int hzsdr_symsync_plan(const hzsdr_symsync *s, size_t *rows_per_wave, size_t *tile_samples, int *form);
/* Back to position 0 with the initial state; the parameters stay. */
int hzsdr_symsync_reset(hzsdr_symsync *s);
int hzsdr_symsync_free(hzsdr_symsync *s);

#ifdef __cplusplus
}
#endif

#endif /* HZSDR_SYMSYNC_H */

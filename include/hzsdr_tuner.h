/*
 * hzsdr_tuner.h -- the tuner bank of libhzsdr_hip: K digital down-converters at arbitrary centre frequencies over ONE
 * pass of one IQ stream, a shared prototype filter and a decimation.  It is the front end for channels that do not lie
 * on the channelizer's grid; its output is the channel-major block (K rows with a pitch) that hzsdr_resampler.h and
 * hzsdr_demod.h take as it is (streams = K).
 *
 * The entries live beside hzsdr.h and the other five headers (same conventions, same status codes, same context).
 * The reference has no such operator: the definition below is the contract, restated under tests/.
 *
 * Parameters:
 *   - tuners = K, 1 <= K <= 256;
 *   - words[k] = w_k, a uint32_t per tuner: tuner k is centred on f_k = w_k fs / 2^32, words at or above 2^31 are the
 *     negative frequencies;
 *   - down = D, 1 <= D <= 256;
 *   - taps = h[0 .. Q), float32 host values, all finite, 1 <= Q <= 1024, shared by all tuners; Qp is Q rounded up to
 *     even and h[q] = +0 for Q <= q < Qp;
 *   - c(.) is hzsdr_convert's conversion to complex64 (iq_c64.go:77-117); source formats are u8, i8, i16 and c64; the
 *     output is complex64, K rows;
 *   - positions count from create or reset.  A sample before position 0 is +0 + 0i, and so is, for flush, a sample
 *     behind the last one pushed.
 * Meaning:
 *       z_k[n] = c(x[n]) exp(-2 pi i w_k n / 2^32)         y_k[m] = sum_q h[q] z_k[m D - q]
 *   Shift(-f_k) with phase zero at stream position 0, the FIR h, every D-th output: the orientation of the
 *   channelizer's channel k.
 * Arithmetic, in three steps:
 *   1. The modulated taps, made on the host at create and on retune:
 *          G_k[q] = RN32(h[q] cos t) + i RN32(h[q] sin t),  t = 2 pi ((w_k q) mod 2^32) / 2^32
 *      The integer phase is exact; cos, sin and the product are float64 (cos and sin evaluated behind an exact
 *      reduction of the integer phase to the first half quadrant, so that they are exact on the axes), one rounding to
 *      float32.  G_k[q] = +0 + 0i for q >= Q.  hzsdr_tuner_readout hands them back; the bit-exact restatement takes them
 *      as given.
 *   2. The matrix product.  Per (k, m), from +0, q ascending over ALL Qp terms (padding tap and out-of-stream samples
 *      included), four fused steps per q, with a = c(x[m D - q]) and g = G_k[q]:
 *          re = fma(g.re, a.re, re)    re = fma(-g.im, a.im, re)    im = fma(g.im, a.re, im)    im = fma(g.re, a.im, im)
 *      As a real product: row 2k of A is (g.re, -g.im) interleaved over q, row 2k + 1 is (g.im, g.re); column m of B is
 *      (a.re, a.im) interleaved over q; the inner dimension 2 Qp is a multiple of 4.  It runs on
 *      v_mfma_f32_16x16x4_f32, whose result is this k-ordered chain of float32 fused multiply-adds.
 *   3. The rotator.  p = (w_k m D) mod 2^32, kept by the host as a running uint32 for a push's first output and
 *      advanced per output in wrapping uint32 arithmetic.  p = a 2^21 + b 2^10 + c (11, 11 and 10 bits); three host-made
 *      tables of complex64, each the float64 value rounded once, entry 0 exactly 1 + 0i:
 *          T2[a] = exp(-2 pi i a / 2^11)    T1[b] = exp(-2 pi i b / 2^22)    T0[c] = exp(-2 pi i c / 2^32)
 *          r = cmul(cmul(T2[a], T1[b]), T0[c])        y = cmul(s, r),  s the sum of step 2
 *          cmul(u, v).re = fma(u.re, v.re, -(u.im * v.im))    cmul(u, v).im = fma(u.re, v.im, u.im * v.re)
 *      the inner products rounded by themselves (csrc/hz_tuner_math.h).
 * Counts, the demodulator's:
 *   - after N samples the outputs m < ceil(N / D) have been written;
 *   - flush writes ceil(N / D) <= m < ceil((N - 1 + Q) / D) and resets (N = 0 writes nothing).
 * Invariance: the bits of row k do not depend on how the stream is cut into pushes, on the memory space, on the
 * output pitch, on the run, or on the other tuners, their number and their order.  The object keeps the last Q - 1
 * converted samples between pushes.
 * Layout: row k of the output starts k * out_stride complex64 values into `out`; out_stride is ignored when K = 1.
 */
#ifndef HZSDR_TUNER_H
#define HZSDR_TUNER_H

#include "hzsdr.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hzsdr_tuner hzsdr_tuner;

/* hzsdr_tuner_plan's `form`: a sum of these.  _CHUNKED: the window of a tile's outputs under the whole filter is past
 * the LDS budget (large D under a long filter); the inner dimension is staged in chunks of q, the accumulators carried
 * through them.  _TRANSPOSED: the window in LDS is stored as D rows (sample w in row w mod D); whenever D > 1. */
#define HZSDR_TUNER_FORM_CHUNKED 1
#define HZSDR_TUNER_FORM_TRANSPOSED 2

/* hzsdr_tuner_readout's `what` */
#define HZSDR_TUNER_READ_TAPS 1 /* G of tuner `index`: Qp complex64 */
#define HZSDR_TUNER_READ_T2 2   /* 2048 complex64; `index` is ignored for the tables */
#define HZSDR_TUNER_READ_T1 3   /* 2048 complex64 */
#define HZSDR_TUNER_READ_T0 4   /* 1024 complex64 */

/* A bank of `tuners` tuners at `words` (host values) over src_format samples (iq.go:110-126) with the prototype
 * filter `taps` (n_taps float32 host values) and the decimation `down`; words and taps are free to go when this
 * returns.  The modulated taps, the tables and the held samples (zero) are prepared here.
 * HZSDR_ERR_INVALID_ARGUMENT for tuners, down or n_taps out of range, a non-finite tap, null words or taps;
 * HZSDR_ERR_FORMAT_UNKNOWN for an unknown format. */
int hzsdr_tuner_create(hzsdr_ctx *ctx, int src_format, const uint32_t *words, size_t tuners, size_t down, const float *taps,
                       size_t n_taps, hzsdr_tuner **out);
/* Consume all n_in samples and write the outputs they complete, *written per row (hzsdr_tuner_outputs_for's count), as
 * complex64; columns [written, out_stride) of a row are left untouched.  HZSDR_ERR_DST_TOO_SMALL when out_cap is
 * below the count, or when tuners > 1 and out_stride is below the count: decided before anything is launched, the state
 * is unchanged.  Stream-ordered on the context's stream; HOST contexts stage `in` and `out` (pitched rows by a 2-D
 * copy). */
int hzsdr_tuner_push(hzsdr_tuner *t, const void *in, size_t n_in, void *out, size_t out_cap, size_t out_stride, size_t *written);
/* Write the outputs that still depend on samples pushed (hzsdr_tuner_pending's flush_outputs per row), the samples
 * behind the last one taken as zero, and go back to stream position 0.  HZSDR_ERR_DST_TOO_SMALL as for push; the state
 * is unchanged then. */
int hzsdr_tuner_flush(hzsdr_tuner *t, void *out, size_t out_cap, size_t out_stride, size_t *written);
/* The outputs per row a push of n_in samples would write now. */
int hzsdr_tuner_outputs_for(const hzsdr_tuner *t, size_t n_in, size_t *count);
/* Samples consumed, the index m of the next output, and the outputs per row a flush would write now. */
int hzsdr_tuner_pending(const hzsdr_tuner *t, uint64_t *consumed, uint64_t *next_output, size_t *flush_outputs);
/* The tile of one workgroup -- tile_outputs outputs (tile i of a push holds the push's outputs
 * [i * tile_outputs, (i + 1) * tile_outputs)) times tile_rows rows of the real matrix A, two per tuner -- and the
 * kernel form this object runs (HZSDR_TUNER_FORM_*), so that tests can aim at tile edges. */
int hzsdr_tuner_plan(const hzsdr_tuner *t, size_t *tile_outputs, size_t *tile_rows, int *form);
/* Replace the words of tuners [first, first + count) and rebuild their modulated taps; in effect from the next push on.
 * The stream position and the held samples are untouched and the phase stays referred to stream position 0: a retune
 * to the same word changes no bit.  HZSDR_ERR_INVALID_ARGUMENT for a range outside the bank or null words. */
int hzsdr_tuner_set_words(hzsdr_tuner *t, size_t first, size_t count, const uint32_t *words);
/* Copy one of the host-made operands (HZSDR_TUNER_READ_*) to `dst`, a HOST buffer of `cap` complex64 values:
 * HZSDR_ERR_DST_TOO_SMALL when it has more, HZSDR_ERR_INVALID_ARGUMENT for an unknown `what` or a tuner outside the
 * bank. */
int hzsdr_tuner_readout(const hzsdr_tuner *t, int what, size_t index, void *dst, size_t cap);
/* Back to stream position 0: nothing consumed, output 0 next, held samples zero.  The words stay. */
int hzsdr_tuner_reset(hzsdr_tuner *t);
int hzsdr_tuner_free(hzsdr_tuner *t);

#ifdef __cplusplus
}
#endif

#endif /* HZSDR_TUNER_H */

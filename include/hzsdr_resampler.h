/*
 * hzsdr_resampler.h -- the polyphase rational resampler of libhzsdr_hip: the
 * rate of one stream, or of many rows at once, changed by the ratio U/D.  It
 * is the third member of the polyphase family, after the channelizer of
 * hzsdr_channelizer.h and the synthesis bank of hzsdr_synthesizer.h, and takes
 * the channelizer's channel-major output (M rows with a pitch) as it is: a
 * channel row comes out at fs/hop, which is seldom the rate a demodulator or
 * an audio sink wants.
 *
 * The entries live beside hzsdr.h and the other three headers (same
 * conventions, same status codes, same context).  The reference has no
 * resampler: the definition below, scipy.signal.upfirdn's convention, is the
 * contract, restated in float64 under tests/.
 *
 * Parameters:
 *   - up = U, down = D, 1 <= U, D <= 1024; they need not be coprime and are
 *     NOT reduced;
 *   - taps = h[0 .. L), float32 host values, all finite, 1 <= L <= 65536;
 *     Q = ceil(L / U) <= 256 taps per phase; h[k] = +0.0f for k >= L;
 *   - streams = R, 1 <= R <= 8192; every stream shares h and the stream
 *     position;
 *   - c(.) is hzsdr_convert's conversion to complex64 (iq_c64.go:77-117);
 *     source formats are u8, i8, i16 and c64; the output is complex64;
 *   - positions count from create or reset.  A sample before position 0 is
 *     +0 + 0i.  For flush, so is a sample behind the last one pushed.
 * Output:
 *       phi_m = (m * D) mod U        i_m = floor(m * D / U)
 *       y[m]  = sum_{q = 0}^{Q - 1} h[phi_m + q * U] * c(x[i_m - q])
 *   i.e. upfirdn(h, x, U, D): zero-stuff by U, filter with h, keep every D-th.
 * Arithmetic:
 *   - each term is one __fmaf_rn(h, x, acc) per component; q ascends, starting
 *     from +0;
 *   - ALL Q terms are evaluated, padding taps and out-of-stream samples
 *     included (a skipped term can differ in the sign of zero, and non-finite
 *     samples would poison differently).
 * Counts:
 *   - after N samples in total the outputs m < M(N) = ceil(N * U / D) have
 *     been written;
 *   - flush writes the outputs M(N) <= m < ceil(((N - 1) * U + L) / D) and
 *     resets (the range is empty when L - U is too small; N = 0 writes
 *     nothing): a whole stream has exactly upfirdn's length -- except that
 *     with L < U the pushes alone may have written M(N), up to
 *     ceil((U - L) / D) more, the last ones sums of padding taps only, +0.
 * Invariance: the bits do not depend on how the stream is cut into pushes, on
 * the memory space, on the number of streams or the pitch, or on the run.
 * Layout:
 *   - row s of the input starts s * in_stride SAMPLES into `in`; row s of the
 *     output starts s * out_stride complex64 values into `out`; both strides
 *     are ignored when R = 1.
 */
#ifndef HZSDR_RESAMPLER_H
#define HZSDR_RESAMPLER_H

#include "hzsdr.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hzsdr_resampler hzsdr_resampler;

/* hzsdr_resampler_plan's `form`: a sum of these.  Without _DIRECT a workgroup
 * stages its tile's input window in LDS; with it every lane reads its samples
 * from memory (D/U so large that the window of one tile does not fit).
 * Without _TAPS_GLOBAL the polyphase table is in LDS; with it the table is
 * read from memory (it is past the LDS budget).  _TAPS_UNIFORM: U divides D,
 * every output has phase 0, and the table's one row is read as scalars common
 * to a wave (neither from LDS nor lane by lane).  _WINDOW_PADDED: the window
 * in LDS has one empty slot behind every 32 samples (D/U is 2 or more; never
 * together with _DIRECT). */
#define HZSDR_RESAMPLER_FORM_DIRECT 1
#define HZSDR_RESAMPLER_FORM_TAPS_GLOBAL 2
#define HZSDR_RESAMPLER_FORM_TAPS_UNIFORM 4
#define HZSDR_RESAMPLER_FORM_WINDOW_PADDED 8

/* A resampler by up/down over `streams` rows of src_format samples
 * (iq.go:110-126) with the filter `taps` (n_taps float32 host values, free to
 * go when this returns).  The polyphase table, the held tails (zero) and the
 * kernel form are prepared here.  HZSDR_ERR_INVALID_ARGUMENT for up, down,
 * n_taps, ceil(n_taps / up) or streams out of range, a non-finite tap, null
 * taps; HZSDR_ERR_FORMAT_UNKNOWN for an unknown format. */
int hzsdr_resampler_create(hzsdr_ctx *ctx, int src_format, size_t up, size_t down, const float *taps, size_t n_taps,
                           size_t streams, hzsdr_resampler **out);
/* Consume all n_in samples of every row and write the outputs they complete,
 * *written per row (hzsdr_resampler_outputs_for's count), as complex64;
 * columns [written, out_stride) of a row are left untouched.
 * HZSDR_ERR_DST_TOO_SMALL when out_cap is below the count, or when streams > 1
 * and out_stride is below the count: decided before anything is launched, the
 * state is unchanged.  HZSDR_ERR_INVALID_ARGUMENT for streams > 1 with
 * in_stride < n_in.  Stream-ordered on the context's stream; HOST contexts
 * stage `in` and `out` (pitched rows by a 2-D copy). */
int hzsdr_resampler_push(hzsdr_resampler *r, const void *in, size_t n_in, size_t in_stride, void *out, size_t out_cap,
                         size_t out_stride, size_t *written);
/* Write the outputs that still depend on samples pushed (hzsdr_resampler_pending's
 * flush_outputs per row), the samples behind the last one taken as zero, and
 * go back to stream position 0.  HZSDR_ERR_DST_TOO_SMALL as for push; the
 * state is unchanged then. */
int hzsdr_resampler_flush(hzsdr_resampler *r, void *out, size_t out_cap, size_t out_stride, size_t *written);
/* The outputs per row a push of n_in samples would write now. */
int hzsdr_resampler_outputs_for(const hzsdr_resampler *r, size_t n_in, size_t *count);
/* Samples consumed per row, the index m of the next output, and the outputs a
 * flush would write now. */
int hzsdr_resampler_pending(const hzsdr_resampler *r, uint64_t *consumed, uint64_t *next_output, size_t *flush_outputs);
/* The outputs one workgroup writes (tile t of a push holds the push's outputs
 * [t * tile_outputs, (t + 1) * tile_outputs)) and the kernel form this object
 * runs (HZSDR_RESAMPLER_FORM_*), so that tests can aim at tile edges. */
int hzsdr_resampler_plan(const hzsdr_resampler *r, size_t *tile_outputs, int *form);
/* Back to stream position 0: nothing consumed, output 0 next, tails zero. */
int hzsdr_resampler_reset(hzsdr_resampler *r);
int hzsdr_resampler_free(hzsdr_resampler *r);

#ifdef __cplusplus
}
#endif

#endif /* HZSDR_RESAMPLER_H */

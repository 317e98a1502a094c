/*
 * hzsdr_demod.h -- the demodulator bank of libhzsdr_hip: FM, phase, envelope
 * or power of one stream, or of many rows at once, followed by a real
 * post-filter and a decimation.  It is the next member of the family of
 * hzsdr_channelizer.h, hzsdr_synthesizer.h and hzsdr_resampler.h and takes the
 * channelizer's channel-major block (M rows with a pitch) and the resampler's
 * output rows as they are, so that a capture split into channels never leaves
 * the device to have a phase difference taken.
 *
 * The entries live beside hzsdr.h and the other four headers (same
 * conventions, same status codes, same context).  The reference has no
 * demodulator: the definition below is the contract, restated under tests/.
 *
 * Parameters:
 *   - mode is one of HZSDR_DEMOD_FM, _PHASE, _ENVELOPE, _POWER;
 *   - down = D, 1 <= D <= 64;
 *   - taps = h[0 .. Q), float32 host values, all finite, 1 <= Q <= 1024;
 *   - streams = R, 1 <= R <= 8192; every stream shares h and the stream
 *     position;
 *   - c(.) is hzsdr_convert's conversion to complex64 (iq_c64.go:77-117);
 *     source formats are u8, i8, i16 and c64; the output is REAL float32;
 *   - positions count from create or reset.  A sample before position 0 is
 *     +0 + 0i.
 * Detector, one value d[n] per input sample, in float32, every operation
 * rounded by itself (no contraction), with a = c(x[n]) and b = c(x[n - 1]):
 *   - FM:        p.re = (a.re * b.re) + (a.im * b.im)
 *                p.im = (a.im * b.re) - (a.re * b.im)       p = a * conj(b)
 *                d[n] = angle(p.im, p.re)
 *   - PHASE:     d[n] = angle(a.im, a.re)
 *   - ENVELOPE:  d[n] = sqrt((a.re * a.re) + (a.im * a.im)), the square root
 *                correctly rounded
 *   - POWER:     d[n] = (a.re * a.re) + (a.im * a.im)
 *   angle(y, x) is the library's own float32 arctangent, written out operation
 *   by operation in csrc/hz_demod_math.h (within 2^-21 rad of atan2; its
 *   measured error is recorded there).  angle(+-0, +-0) = +0, so d[0] of FM
 *   needs no special case, and a zero sample gives d = +0 in every mode.
 * Output:
 *       y[m] = sum_{q = 0}^{Q - 1} h[q] * d[m * D - q]
 *   - each term is one __fmaf_rn(h, d, acc); q ascends, starting from +0;
 *   - ALL Q terms are evaluated; d[n] = +0 for n < 0.
 *   The default of the host layers, taps [1.0] with D = 1, is the bare
 *   detector.  The FM gain fs / (2 pi deviation) is folded into the taps by
 *   the caller.
 * Counts:
 *   - after N samples per row the outputs m < ceil(N / D) have been written;
 *   - flush writes the outputs ceil(N / D) <= m < ceil((N - 1 + Q) / D), with
 *     d[n] = +0 for n >= N, and resets (N = 0 writes nothing): a whole stream
 *     has upfirdn(h, d, 1, D)'s length.
 * Invariance: the bits do not depend on how the stream is cut into pushes, on
 * the memory space, on the number of streams or either pitch, or on the run.
 * The object keeps the last Q converted samples of every row and recomputes d
 * from them; it never stores d across pushes.
 * Layout:
 *   - row s of the input starts s * in_stride SAMPLES into `in`; row s of the
 *     output starts s * out_stride floats into `out`; both strides are ignored
 *     when R = 1.
 */
#ifndef HZSDR_DEMOD_H
#define HZSDR_DEMOD_H

#include "hzsdr.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hzsdr_demod hzsdr_demod;

#define HZSDR_DEMOD_FM 1
#define HZSDR_DEMOD_PHASE 2
#define HZSDR_DEMOD_ENVELOPE 3
#define HZSDR_DEMOD_POWER 4

/* hzsdr_demod_plan's `form`: a sum of these.  A workgroup of 256 lanes stages
 * its tile's detector values in LDS, each computed once, and every lane owns
 * tile_outputs / 256 outputs.  _HALF_TILE: the window of 256 outputs is past
 * the LDS budget (D of 63 or 64 under a long filter), tile_outputs is 128 and
 * the upper half of the lanes only fills the window.  _TRANSPOSED: the window
 * is stored as D rows (value w in row w mod D), which keeps the lanes of one
 * read on distinct banks; it is set whenever D > 1. */
#define HZSDR_DEMOD_FORM_HALF_TILE 1
#define HZSDR_DEMOD_FORM_TRANSPOSED 2

/* A demodulator of `mode` over `streams` rows of src_format samples
 * (iq.go:110-126) with the post-filter `taps` (n_taps float32 host values,
 * free to go when this returns) and the decimation `down`.  The held tails
 * (zero) and the kernel form are prepared here.  HZSDR_ERR_INVALID_ARGUMENT
 * for mode, down, n_taps or streams out of range, a non-finite tap, null
 * taps; HZSDR_ERR_FORMAT_UNKNOWN for an unknown format. */
int hzsdr_demod_create(hzsdr_ctx *ctx, int src_format, int mode, size_t down, const float *taps, size_t n_taps, size_t streams,
                       hzsdr_demod **out);
/* Consume all n_in samples of every row and write the outputs they complete,
 * *written per row (hzsdr_demod_outputs_for's count), as float32; columns
 * [written, out_stride) of a row are left untouched.
 * HZSDR_ERR_DST_TOO_SMALL when out_cap is below the count, or when streams > 1
 * and out_stride is below the count: decided before anything is launched, the
 * state is unchanged.  HZSDR_ERR_INVALID_ARGUMENT for streams > 1 with
 * in_stride < n_in.  Stream-ordered on the context's stream; HOST contexts
 * stage `in` and `out` (pitched rows by a 2-D copy). */
int hzsdr_demod_push(hzsdr_demod *d, const void *in, size_t n_in, size_t in_stride, float *out, size_t out_cap, size_t out_stride,
                     size_t *written);
/* Write the outputs that still depend on samples pushed (hzsdr_demod_pending's
 * flush_outputs per row), the detector values behind the last sample taken as
 * zero, and go back to stream position 0.  HZSDR_ERR_DST_TOO_SMALL as for
 * push; the state is unchanged then. */
int hzsdr_demod_flush(hzsdr_demod *d, float *out, size_t out_cap, size_t out_stride, size_t *written);
/* The outputs per row a push of n_in samples would write now. */
int hzsdr_demod_outputs_for(const hzsdr_demod *d, size_t n_in, size_t *count);
/* Samples consumed per row, the index m of the next output, and the outputs a
 * flush would write now. */
int hzsdr_demod_pending(const hzsdr_demod *d, uint64_t *consumed, uint64_t *next_output, size_t *flush_outputs);
/* The outputs one workgroup writes (tile t of a push holds the push's outputs
 * [t * tile_outputs, (t + 1) * tile_outputs)) and the kernel form this object
 * runs (HZSDR_DEMOD_FORM_*), so that tests can aim at tile edges. */
int hzsdr_demod_plan(const hzsdr_demod *d, size_t *tile_outputs, int *form);
/* Back to stream position 0: nothing consumed, output 0 next, tails zero. */
int hzsdr_demod_reset(hzsdr_demod *d);
int hzsdr_demod_free(hzsdr_demod *d);

#ifdef __cplusplus
}
#endif

#endif /* HZSDR_DEMOD_H */

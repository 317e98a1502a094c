/*
 * hzsdr_channelizer.h -- the polyphase channelizer of libhzsdr_hip: one wide
 * IQ stream split into M equally spaced channels, every channel filtered by
 * the same prototype and decimated by the hop D, in one pass over the raw
 * samples (a weighted fold of L = P*M samples into M values, then one M-point
 * forward transform per output frame: O(L + M log M) per frame).
 *
 * The entries live beside hzsdr.h and hzsdr_spectrum.h (same conventions, same
 * status codes, same context) until the Go binding takes them up.  Each
 * declaration cites the reference interface (file:line under the go-sdr
 * checkout) it relates to.
 *
 * Definitions (stream positions t count from the first sample pushed since
 * create or reset; c(.) is hzsdr_convert's conversion to complex64; g is the
 * prototype of L = P*M float32 values, 1 <= P <= 32; D is the hop, 1 <= D <= M):
 *   - frame j exists once samples [jD, jD + L) have been pushed;
 *   - y[j][k] = sum_{i=0}^{L-1} g[i] * c(x[jD + i]) * exp(-2 pi i k (jD + i) / M),
 *     k = 0 .. M-1: channel k is Shift(-k fs / M) with phase zero at stream
 *     position 0, then the FIR whose impulse response is g reversed, then every
 *     D-th output; the output rate is fs / D.  g[i] multiplies the sample at
 *     frame offset i;
 *   - computed as a fold indexed by absolute time modulo M, then one forward
 *     transform (the sign convention of fft.Forward, fft/fft.go:32-35):
 *       u_j[r] = sum_{p=0}^{P-1} g[i_p] * c(x[jD + i_p]),  i_p = ((r - jD) mod M) + pM
 *       y[j][.] = FFT_M(u_j)
 *     the fold in float32, p ascending, starting from +0, one fused
 *     multiply-add per component and term; the rotation jD mod M is integer
 *     state carried across pushes and applied to the indices of the loads;
 *   - HZSDR_CHANNELIZER_FRAME_MAJOR:   out[f * M + pos(k)], rows of M complex64;
 *     HZSDR_CHANNELIZER_CHANNEL_MAJOR: out[pos(k) * out_stride + f], one
 *     contiguous complex64 stream per channel; columns [frames_written,
 *     out_stride) of every row are left untouched;
 *   - pos(k) = k for HZSDR_ORDER_ZERO_FIRST and (k + M/2) mod M for
 *     HZSDR_ORDER_NEGATIVE_FIRST (FrequencySlice.Shift, fft/result.go:82-97).
 * The output bits do not depend on how the stream is cut into pushes, on the
 * memory space, on the output layout or on the run.
 */
#ifndef HZSDR_CHANNELIZER_H
#define HZSDR_CHANNELIZER_H

#include "hzsdr_spectrum.h" /* HZSDR_ORDER_* */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hzsdr_channelizer hzsdr_channelizer;

/* output layout */
#define HZSDR_CHANNELIZER_FRAME_MAJOR 0
#define HZSDR_CHANNELIZER_CHANNEL_MAJOR 1

/* A channelizer of src_format samples (iq.go:110-126) into `channels` = M
 * channels (the transform of fft.Planner, fft/fft.go:42-48; M a power of two,
 * 256 .. 8192) with the prototype `taps` (n_taps = P*M float32 host values,
 * 1 <= P <= 32) and frames `hop` samples apart (1 <= hop <= M).  `order`:
 * HZSDR_ORDER_* (fft.Order, fft/result.go:34-47); `layout`:
 * HZSDR_CHANNELIZER_FRAME_MAJOR or _CHANNEL_MAJOR.  The transform's tables and
 * the device copy of the taps are prepared here.
 * HZSDR_ERR_INVALID_ARGUMENT for M outside the range or not a power of two,
 * n_taps == 0, not a multiple of M or above 32*M, hop == 0 or above M, a bad
 * order or layout, null taps; HZSDR_ERR_FORMAT_UNKNOWN for an unknown format. */
int hzsdr_channelizer_create(hzsdr_ctx *ctx, int src_format, size_t channels, const float *taps, size_t n_taps,
                             size_t hop, int order, int layout, hzsdr_channelizer **out);
/* Consume n_in samples of `in` (all of them) and write every frame that
 * completes during the push to `out` (complex64; the bins of fft.Forward,
 * fft/fft.go:32-35, in the channelizer's order and layout; out_stride is the
 * row pitch in complex64 values of the channel-major layout and is ignored
 * for frame-major).  The samples the next frame still needs stay on the
 * device.  HZSDR_ERR_DST_TOO_SMALL when out_frames_cap, or the channel-major
 * out_stride, is below the frames the push completes: checked before anything
 * is launched; the state is unchanged.  Stream-ordered on the context's
 * stream; HOST contexts stage `in` and `out`.
 * HZSDR_ERR_INVALID_ARGUMENT ("the push is too long") for n_in above 2^62, here and in frames_for. */
int hzsdr_channelizer_push(hzsdr_channelizer *c, const void *in, size_t n_in, void *out, size_t out_frames_cap,
                           size_t out_stride, size_t *frames_written);
/* The frames a push of n_in samples would write now. */
int hzsdr_channelizer_frames_for(const hzsdr_channelizer *c, size_t n_in, size_t *frames);
/* Samples held for the next frame, and the index j of the next frame. */
int hzsdr_channelizer_pending(const hzsdr_channelizer *c, size_t *samples_held, uint64_t *frame_index);
/* Back to stream position 0: no samples held, frame 0 next, rotation 0. */
int hzsdr_channelizer_reset(hzsdr_channelizer *c);
int hzsdr_channelizer_free(hzsdr_channelizer *c);

#ifdef __cplusplus
}
#endif

#endif /* HZSDR_CHANNELIZER_H */

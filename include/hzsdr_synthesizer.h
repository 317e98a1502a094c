/*
 * hzsdr_synthesizer.h -- the polyphase synthesis bank of libhzsdr_hip: M
 * channels put back into one wide IQ stream, the adjoint of the channelizer
 * of hzsdr_channelizer.h (one M-point backward transform per input frame, then
 * a weighted overlap-add of L = P*M values: O(L + M log M) per frame).  It is
 * what a transmit path (hackrf/tx.go:86, pluto/tx.go:153, the Writer of
 * writer.go:31-44 behind stream.ConvertWriter, stream/convert.go:58-77) needs
 * in front of it to send many carriers at once, and what turns channelized,
 * edited frames back into a stream.
 *
 * The entries live beside hzsdr.h, hzsdr_spectrum.h and hzsdr_channelizer.h
 * (same conventions, same status codes, same context) until the Go binding
 * takes them up.  Each declaration cites the reference interface (file:line
 * under the go-sdr checkout) it relates to.
 *
 * Definitions:
 *   - M is the channel count, a power of two, 256 .. 8192; g is the prototype
 *     of L = P*M float32 values, 1 <= P <= 32; D is the hop, 1 <= D <= M;
 *     output positions t count from create or reset;
 *   - input frame j holds Y[j][k], k = 0 .. M-1 (ZeroFirst index), stored at
 *     pos(k) exactly as the channelizer writes it:
 *       HZSDR_CHANNELIZER_FRAME_MAJOR:   in[f * M + pos(k)];
 *       HZSDR_CHANNELIZER_CHANNEL_MAJOR: in[pos(k) * in_stride + f];
 *     pos(k) = k for HZSDR_ORDER_ZERO_FIRST and (k + M/2) mod M for
 *     HZSDR_ORDER_NEGATIVE_FIRST (FrequencySlice.Shift, fft/result.go:82-97);
 *   - w_j[r] = sum_k Y[j][k] * exp(+2 pi i k r / M)   (the sign convention of
 *     fft.Backward, fft/fft.go:32-35, unnormalised)
 *     x^[t]  = sum_{j : 0 <= t - jD < L} g[t - jD] * w_j[t mod M]
 *     i.e. channel k is zero-stuffed by D, filtered by g and Shift(+k fs / M)
 *     with phase zero at position 0, and the channels are summed.  With the
 *     same (g, M, D) this is the adjoint of the channelizer's definition;
 *   - the sum over j runs in float32, j ascending from +0, one
 *     __fmaf_rn(g, w, acc) per component and term;
 *   - the destination format (c64 | u8 | i8 | i16) is applied to the finished
 *     sum with hzsdr_convert's c64 -> dst arithmetic (iq_c64.go:77-117; the
 *     identity for c64); out-of-range values behave as hzsdr_convert does: the
 *     caller scales the taps, there is no scale parameter.
 * Streaming:
 *   - a push of F frames writes exactly F*D samples, positions
 *     [F0 D, (F0 + F) D); the L - D partial sums behind them stay on the
 *     device; the rotation (the next frame's first position mod M) is running
 *     integer state, never a product with the stream length;
 *   - flush writes the L - D held partial sums, the stream's tail, and resets:
 *     a whole stream of F frames yields (F - 1) D + L samples;
 *   - the output bits do not depend on how the frames are cut into pushes, on
 *     the memory space, on the input layout or order, on the run, or on how the
 *     implementation groups frames internally.
 */
#ifndef HZSDR_SYNTHESIZER_H
#define HZSDR_SYNTHESIZER_H

#include "hzsdr_channelizer.h" /* HZSDR_CHANNELIZER_*_MAJOR, HZSDR_ORDER_* */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hzsdr_synthesizer hzsdr_synthesizer;

/* A synthesis bank of `channels` = M channels (the transform of fft.Planner,
 * fft/fft.go:42-48, run Backward; M a power of two, 256 .. 8192) into
 * dst_format samples (iq.go:110-126) with the prototype `taps` (n_taps = P*M
 * float32 host values, 1 <= P <= 32) and input frames `hop` output samples
 * apart (1 <= hop <= M).  `order`: HZSDR_ORDER_* (fft.Order,
 * fft/result.go:34-47); `layout`: HZSDR_CHANNELIZER_FRAME_MAJOR or
 * _CHANNEL_MAJOR, the layout of the frames pushed.  The transform's tables,
 * the device copy of the taps and the held partial sums are prepared here.
 * HZSDR_ERR_INVALID_ARGUMENT for M outside the range or not a power of two,
 * n_taps == 0, not a multiple of M or above 32*M, hop == 0 or above M, a bad
 * order or layout, null taps; HZSDR_ERR_FORMAT_UNKNOWN for an unknown format. */
int hzsdr_synthesizer_create(hzsdr_ctx *ctx, int dst_format, size_t channels, const float *taps, size_t n_taps,
                             size_t hop, int order, int layout, hzsdr_synthesizer **out);
/* Consume n_frames frames of M complex64 values (the bins fft.Backward takes,
 * fft/fft.go:32-35, in the synthesizer's order and layout; in_stride is the
 * row pitch in complex64 values of the channel-major layout, at least
 * n_frames, and is ignored for frame-major) and write the n_frames * hop
 * samples they complete to `out` in the destination format (a Writer's
 * Write, writer.go:31-44).  HZSDR_ERR_DST_TOO_SMALL when out_cap (in samples)
 * is below n_frames * hop: checked before anything is launched; the state is
 * unchanged.  HZSDR_ERR_INVALID_ARGUMENT for a channel-major in_stride below
 * n_frames.  A push of no frames writes nothing.  Stream-ordered on the
 * context's stream; HOST contexts stage `frames` and `out`. */
int hzsdr_synthesizer_push(hzsdr_synthesizer *s, const void *frames, size_t n_frames, size_t in_stride, void *out,
                           size_t out_cap, size_t *samples_written);
/* Write the held partial sums (L - hop samples once a frame has been pushed,
 * none before), the tail of the stream, and go back to stream position 0
 * (the end of a transmission: WriteCloser.Close, writer.go:46-49).
 * HZSDR_ERR_DST_TOO_SMALL when out_cap is below the held count; the state is
 * unchanged. */
int hzsdr_synthesizer_flush(hzsdr_synthesizer *s, void *out, size_t out_cap, size_t *samples_written);
/* Partial sums held behind the samples written, and the index j of the next
 * frame. */
int hzsdr_synthesizer_pending(const hzsdr_synthesizer *s, size_t *samples_held, uint64_t *frame_index);
/* The frames one internal launch group takes: a push of more frames is
 * processed in groups of at most this many, with the same bits as any other
 * cut (fft.Plan.Transform once per group of frames, fft/fft.go:52-59). */
int hzsdr_synthesizer_group_frames(const hzsdr_synthesizer *s, size_t *frames);
/* Back to stream position 0: nothing held, frame 0 next, rotation 0. */
int hzsdr_synthesizer_reset(hzsdr_synthesizer *s);
int hzsdr_synthesizer_free(hzsdr_synthesizer *s);

#ifdef __cplusplus
}
#endif

#endif /* HZSDR_SYNTHESIZER_H */

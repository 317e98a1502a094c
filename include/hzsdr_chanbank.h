/*
 * hzsdr_chanbank.h -- the channel bank of libhzsdr_hip: the polyphase channelizer for the SMALL channel counts, any
 * M from 2 to 255, powers of two or not (8, 16 or 64 sub-bands of a dongle's capture, 100 FM channels of 200 kHz, 12 or
 * 25 channels of a PMR or AIS block).  hzsdr_channelizer.h takes over at M = 256.  Below 256 the transform is one
 * float32 matrix product -- the DFT matrix times a tile of folded frames -- so one kernel serves every M and its
 * results are pinned bit for bit to a host restatement.
 *
 * The entries live beside hzsdr.h and the other six headers (same conventions, same status codes, same context).
 * The reference has no such operator: the definition below is the contract, restated under tests/.
 *
 * Parameters:
 *   - channels = M, any integer with 2 <= M <= 255; Mp is M rounded up to even;
 *   - taps = g[0 .. L), float32 host values, L = P M, 1 <= P <= 32;
 *   - hop = D, 1 <= D <= M;
 *   - order: HZSDR_ORDER_ZERO_FIRST or HZSDR_ORDER_NEGATIVE_FIRST (hzsdr_spectrum.h); layout:
 *     HZSDR_CHANNELIZER_FRAME_MAJOR or HZSDR_CHANNELIZER_CHANNEL_MAJOR (hzsdr_channelizer.h);
 *   - c(.) is hzsdr_convert's conversion to complex64 (iq_c64.go:77-117); source formats are u8, i8, i16 and c64; the
 *     output is complex64;
 *   - stream positions t count from the first sample pushed since create or reset.
 * Meaning, exactly the channelizer's:
 *   - frame j exists once samples [jD, jD + L) have been pushed;
 *   - y[j][k] = sum_{i=0}^{L-1} g[i] c(x[jD + i]) exp(-2 pi i k (jD + i) / M), k = 0 .. M-1: channel k is
 *     Shift(-k fs / M) with phase zero at stream position 0, then the FIR whose impulse response is g reversed, then
 *     every D-th output; the output rate is fs / D;
 *   - the object keeps the samples the next frame needs (converted, fewer than L) and the rotation jD mod M;
 *   - there is no flush.
 * Arithmetic, in three steps:
 *   1. The fold, as in hzsdr_channelizer.h:
 *          u_j[r] = sum_{p=0}^{P-1} g[i_p] c(x[jD + i_p]),  i_p = ((r - jD) mod M) + pM,  0 <= r < M
 *      in float32, p ascending, from +0, one fused multiply-add per component and term; u_j[r] = +0 + 0i for
 *      M <= r < Mp.  The rotation jD mod M is integer state carried across pushes and applied to the indices of the
 *      loads.
 *   2. The DFT table, made on the host at create:
 *          W[k][r] = RN32(cos t) - i RN32(sin t),  t = 2 pi ((k r) mod M) / M
 *      The integer phase is exact; cos and sin are float64, evaluated behind an exact integer reduction of the phase
 *      to the first half quadrant, one rounding to float32.  Entries on the axes are therefore exact: n = (k r) mod M
 *      = 0 gives exactly 1 + 0i, 4 n = M exactly 0 - 1i, 2 n = M exactly -1 + 0i, 4 n = 3 M exactly 0 + 1i.
 *      W[k][r] = +0 + 0i for r >= M.  hzsdr_chanbank_readout hands the table back; the bit-exact restatement takes it
 *      as given.
 *   3. The product.  Per (j, k), from +0, r ascending over ALL Mp terms (padding included), four fused steps per r,
 *      with w = W[k][r] and a = u_j[r]:
 *          re = fma(w.re, a.re, re)    re = fma(-w.im, a.im, re)    im = fma(w.im, a.re, im)    im = fma(w.re, a.im, im)
 *      As a real product: row 2k of A is (w.re, -w.im) interleaved over r, row 2k + 1 is (w.im, w.re); column j of B
 *      is (a.re, a.im) interleaved over r; the inner dimension 2 Mp is a multiple of 4.  It runs on
 *      v_mfma_f32_16x16x4_f32, whose result is this k-ordered chain of float32 fused multiply-adds.
 * Output position:
 *   - pos(k) = k for HZSDR_ORDER_ZERO_FIRST;
 *   - pos(k) = (k + floor(M / 2)) mod M for HZSDR_ORDER_NEGATIVE_FIRST: ascending signed frequency, position 0 at
 *     -floor(M / 2) fs / M.  For odd M this is numpy's fftshift; it is NOT FrequencySlice.Shift's half swap
 *     (fft/result.go:91-94), which leaves an odd slice's last bin where it is.  For even M the two agree.
 * Layouts:
 *   - HZSDR_CHANNELIZER_FRAME_MAJOR:   out[f * M + pos(k)], rows of M complex64, out_stride is ignored;
 *   - HZSDR_CHANNELIZER_CHANNEL_MAJOR: out[pos(k) * out_stride + f], one contiguous complex64 stream per channel;
 *     columns [frames_written, out_stride) of every row are left untouched.
 * Invariance: the bits of a frame do not depend on how the stream is cut into pushes, on the memory space, on the
 * layout, the order or the pitch, on the run, or on which column of which tile the frame lands in.
 */
#ifndef HZSDR_CHANBANK_H
#define HZSDR_CHANBANK_H

#include "hzsdr_channelizer.h" /* HZSDR_ORDER_*, HZSDR_CHANNELIZER_FRAME_MAJOR, _CHANNEL_MAJOR */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hzsdr_chanbank hzsdr_chanbank;

/* hzsdr_chanbank_plan's `form`.  _A_LDS: the real matrix A is staged in LDS beside the folded frames (small M);
 * otherwise every k-step loads it from device memory. */
#define HZSDR_CHANBANK_FORM_A_LDS 1

/* hzsdr_chanbank_readout's `what` */
#define HZSDR_CHANBANK_READ_DFT 1  /* row `index` = k of W: Mp complex64 */
#define HZSDR_CHANBANK_READ_TAPS 2 /* the prototype: L float32; `index` is ignored */

/* A channel bank of src_format samples (iq.go:110-126) into `channels` = M channels, 2 <= M <= 255, with the
 * prototype `taps` (n_taps = P*M float32 host values, 1 <= P <= 32, free to go when this returns) and frames `hop`
 * samples apart (1 <= hop <= M).  The DFT table, the matrix A and the device copy of the taps are prepared here.
 * HZSDR_ERR_INVALID_ARGUMENT for M outside 2 .. 255 (256 belongs to hzsdr_channelizer.h), n_taps == 0, not a multiple
 * of M or above 32*M, hop == 0 or above M, a bad order or layout, null taps; HZSDR_ERR_FORMAT_UNKNOWN for an unknown
 * format. */
int hzsdr_chanbank_create(hzsdr_ctx *ctx, int src_format, size_t channels, const float *taps, size_t n_taps, size_t hop,
                          int order, int layout, hzsdr_chanbank **out);
/* Consume n_in samples of `in` (all of them) and write every frame that completes during the push to `out`
 * (complex64, in the bank's order and layout; out_stride is the row pitch in complex64 values of the channel-major
 * layout and is ignored for frame-major).  The samples the next frame still needs stay on the device.
 * HZSDR_ERR_DST_TOO_SMALL when out_frames_cap, or the channel-major out_stride, is below the frames the push
 * completes: decided before anything is launched; the state is unchanged.  Stream-ordered on the context's stream;
 * HOST contexts stage `in` and `out` (pitched rows by a 2-D copy). */
int hzsdr_chanbank_push(hzsdr_chanbank *c, const void *in, size_t n_in, void *out, size_t out_frames_cap, size_t out_stride,
                        size_t *frames_written);
/* The frames a push of n_in samples would write now. */
int hzsdr_chanbank_frames_for(const hzsdr_chanbank *c, size_t n_in, size_t *frames);
/* Samples held for the next frame, and the index j of the next frame. */
int hzsdr_chanbank_pending(const hzsdr_chanbank *c, size_t *samples_held, uint64_t *frame_index);
/* The tile of one workgroup -- tile_frames consecutive frames of a push (tile i holds the push's frames
 * [i * tile_frames, (i + 1) * tile_frames)) times tile_rows rows of the real matrix A, two per channel and the padding
 * rows behind them -- and the kernel form this object runs (HZSDR_CHANBANK_FORM_*), so that tests can aim at tile
 * edges. */
int hzsdr_chanbank_plan(const hzsdr_chanbank *c, size_t *tile_frames, size_t *tile_rows, int *form);
/* Copy one of the host-made operands (HZSDR_CHANBANK_READ_*) to `dst`, a HOST buffer of `cap` elements (complex64 for
 * _DFT, float32 for _TAPS): HZSDR_ERR_DST_TOO_SMALL when the operand has more, HZSDR_ERR_INVALID_ARGUMENT for an
 * unknown `what` or a row outside the table. */
int hzsdr_chanbank_readout(const hzsdr_chanbank *c, int what, size_t index, void *dst, size_t cap);
/* Back to stream position 0: no samples held, frame 0 next, rotation 0. */
int hzsdr_chanbank_reset(hzsdr_chanbank *c);
int hzsdr_chanbank_free(hzsdr_chanbank *c);

#ifdef __cplusplus
}
#endif

#endif /* HZSDR_CHANBANK_H */

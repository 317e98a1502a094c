/*
 * hzsdr_covar.h -- the array side of libhzsdr_hip beyond the weighted sum: the covariance bank, which turns N coherent
 * channels into their spatial covariance matrices block by block, and the beam scan, which maps such matrices (or a
 * caller's inverse or noise projector) over a grid of weight vectors.  Bartlett, Capon and MUSIC need nothing else from
 * the sample stream; hzsdr_beamform and hzsdr_beamform_angles (hzsdr.h) take the steering angle as given, these two
 * objects find it.
 *
 * The entries live beside hzsdr.h and the other seven headers (same conventions, same status codes, same context).
 * The reference has neither object: the definitions below are the contract, restated under tests/.
 *
 * ---- The covariance bank ----
 * Parameters:
 *   - channels = N, 2 <= N <= 16; block = B snapshots per matrix, 1 <= B <= 2^24; blocks do not overlap: block b covers
 *     stream positions [bB, (b+1)B), counted from the first snapshot pushed since create, reset or flush;
 *   - c(.) is hzsdr_convert's conversion to complex64 (iq_c64.go:77-117); source formats are u8, i8, i16 and c64; all N
 *     rows share the format and the stream position.
 * Meaning:
 *   R_b[i][j] = sum_n a_i[n] conj(a_j[n]),  a_i[n] = c(x_i[n]),  n over the block; N x N complex64, row-major,
 *   unnormalised.
 * Arithmetic, which fixes the bits:
 *   - v_{2i} = Re a_i, v_{2i+1} = Im a_i: 2N real rows;
 *   - the block's snapshots are cut into segments of 256 at block-relative positions [256 s, 256 s + 256); a segment
 *     that the block or a flush ends early is padded with +0 + 0i and all 256 terms are evaluated;
 *   - segment sums: g_s[p][q] = the chain acc = fmaf(v_p[n], v_q[n], acc) from +0, n ascending over the segment (64
 *     steps of v_mfma_f32_16x16x4_f32, k-slot j of step t being snapshot 4 t + j);
 *   - block sum: the pairwise tree over the block's nseg = ceil(n_present / 256) segments: T(lo, hi) = g_lo when
 *     hi - lo = 1, else T(lo, mid) + T(mid, hi) with mid = lo + the largest power of two strictly below hi - lo; one
 *     float32 addition per node, left operand first.  The shape depends on nseg alone;
 *   - combine: R[i][j].re = G[2i][2j] + G[2i+1][2j+1], R[i][j].im = G[2i+1][2j] - G[2i][2j+1], one rounding each.
 *   R is exactly Hermitian, its diagonal's imaginary parts are +0, and an entry depends on its two channels only.
 * Invariance: the bits of R_b do not depend on how the stream is cut into pushes (cuts inside a segment and inside a
 * group of four included), on the memory space, on which of the two input entries is used or on either pitch, on the
 * number of blocks in a push, on the run, or on the other channels, their number and their order.
 *
 * ---- The beam scan ----
 *   p[b][g] = Re sum_i w_i sum_j Q_b[i][j] conj(w_j)  for G weight vectors w (as hzsdr_beamform_angles makes them) and
 *   any N x N complex64 matrices Q_b; with Q = R this is the power of the beam hzsdr_beamform forms with w.
 * Arithmetic: i ascending, inside it j ascending, from +0; with u = conj(w_j):
 *   t.re = fmaf(Q.re, u.re, t.re)  t.re = fmaf(-Q.im, u.im, t.re)  t.im = fmaf(Q.im, u.re, t.im)  t.im = fmaf(Q.re, u.im, t.im)
 *   then p = fmaf(w_i.re, t.re, p), p = fmaf(-w_i.im, t.im, p).
 */
#ifndef HZSDR_COVAR_H
#define HZSDR_COVAR_H

#include "hzsdr.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hzsdr_covar hzsdr_covar;
typedef struct hzsdr_scan hzsdr_scan;

/* hzsdr_covar_plan's `form`: one accumulator tile (N <= 8) or the tiles (0,0), (0,1), (1,1) (N <= 16) */
#define HZSDR_COVAR_FORM_ONE_TILE 1
#define HZSDR_COVAR_FORM_THREE_TILES 2

#define HZSDR_SCAN_MAX_VECTORS 65536

/* A covariance bank over `channels` = N rows of src_format samples (iq.go:110-126), `block` = B snapshots per matrix.
 * HZSDR_ERR_INVALID_ARGUMENT for N outside 2 .. 16 or B outside 1 .. 2^24; HZSDR_ERR_FORMAT_UNKNOWN for an unknown
 * format. */
int hzsdr_covar_create(hzsdr_ctx *ctx, int src_format, size_t channels, size_t block, hzsdr_covar **out);
/* Consume n_in snapshots of every row -- row i starts i * in_stride samples into `in`: the channel-major block that the
 * channel bank, the tuner bank and the resampler write, taken as it is -- and write every block that completes during
 * the push: block b of the push starts b * out_stride complex64 values into `out` (out_stride >= N^2; ignored when at
 * most one block is written; the values behind N^2 of a wider pitch are left untouched).  The open block's group sums
 * and the open segment's snapshots stay on the device.  HZSDR_ERR_DST_TOO_SMALL when out_blocks_cap is below the blocks
 * the push completes, or out_stride below N^2 with more than one: decided before anything is launched, the state is
 * unchanged.  HZSDR_ERR_INVALID_ARGUMENT for in_stride < n_in or a null buffer.  Stream-ordered on the context's
 * stream; HOST contexts stage `in` and `out`.  A long push is launched in rounds, all device memory it needs being
 * there before the first: after HZSDR_ERR_OUT_OF_MEMORY the state is unchanged; after HZSDR_ERR_HIP (a failed launch
 * or copy) the stream position is undefined and hzsdr_covar_reset starts over. */
int hzsdr_covar_push(hzsdr_covar *c, const void *in, size_t n_in, size_t in_stride, void *out, size_t out_blocks_cap, size_t out_stride,
                     size_t *blocks_written);
/* The same push from N separate buffers, as hzsdr_beamform takes them: the same bits.  HZSDR_ERR_INVALID_ARGUMENT for a
 * null row. */
int hzsdr_covar_push_channels(hzsdr_covar *c, const void *const *channels, size_t n_in, void *out, size_t out_blocks_cap, size_t out_stride,
                              size_t *blocks_written);
/* Write the open block if it holds at least one snapshot -- as defined above, with the present snapshots only -- and
 * go back to stream position 0.  With nothing open, nothing is written. */
int hzsdr_covar_flush(hzsdr_covar *c, void *out, size_t out_blocks_cap, size_t *blocks_written);
/* The blocks a push of n_in snapshots would write now. */
int hzsdr_covar_blocks_for(const hzsdr_covar *c, size_t n_in, size_t *blocks);
/* Snapshots consumed per row, the index of the open block, the snapshots it holds. */
int hzsdr_covar_pending(const hzsdr_covar *c, uint64_t *consumed, uint64_t *next_block, size_t *open_snapshots);
/* The segment length (256), the segments one workgroup sums where an aligned group of them lies inside the push
 * (elsewhere one), and the kernel form (HZSDR_COVAR_FORM_*), so that tests can aim at tile edges. */
int hzsdr_covar_plan(const hzsdr_covar *c, size_t *segment, size_t *group_segments, int *form);
/* Back to stream position 0 with nothing open. */
int hzsdr_covar_reset(hzsdr_covar *c);
int hzsdr_covar_free(hzsdr_covar *c);

/* A beam scan over `count` = G weight vectors of `channels` = N complex64 HOST values each (G x N, row-major; free to
 * go when this returns), 1 <= G <= 65536, 2 <= N <= 16. */
int hzsdr_scan_create(hzsdr_ctx *ctx, size_t channels, const void *weights, size_t count, hzsdr_scan **out);
/* p[b][g] for n_mats matrices (at most 65535), matrix b starting b * mat_stride complex64 values into `mats`
 * (mat_stride >= N^2), to out[b * out_stride + g], float32 (out_stride >= G; both pitches are ignored for one matrix);
 * `out` holds out_cap float32 values.  HZSDR_ERR_DST_TOO_SMALL when it is too small.  Stream-ordered; HOST contexts
 * stage both buffers. */
int hzsdr_scan_run(hzsdr_scan *s, const void *mats, size_t n_mats, size_t mat_stride, void *out, size_t out_cap, size_t out_stride);
int hzsdr_scan_free(hzsdr_scan *s);

#ifdef __cplusplus
}
#endif

#endif /* HZSDR_COVAR_H */

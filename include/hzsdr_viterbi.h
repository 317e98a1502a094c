/*
 * hzsdr_viterbi.h -- the Viterbi decoder bank of libhzsdr_hip: convolutionally coded frame bits to data bits, a path
 * metric and an optional CRC verdict per frame, over many rows of frames at once.  It is the next member of the family of
 * hzsdr_tuner.h, hzsdr_iir.h, hzsdr_agc.h, hzsdr_carrier.h, hzsdr_symsync.h and hzsdr_framesync.h and stands behind the
 * last of them: it takes the frame sync bank's `out` block and its device-side `counts` as they are, with no host read in
 * between.  What it leaves to others: tail-biting codes; decoding ONE continuous coded stream across frame boundaries;
 * soft outputs of the decoder; bit unstuffing; descrambling and the outer Reed-Solomon code of a concatenated link, which
 * are the Reed-Solomon decoder bank's (hzsdr_rs.h takes `out` and the counts as they are).  The soft INPUT block
 * (HZSDR_VITERBI_SOFT_F32) is what the soft frame bank writes beside the frame sync bank (hzsdr_softframe.h).
 *
 * The entries live beside hzsdr.h and the other headers (same conventions, same status codes, same context).  The
 * reference has no decoder: the definition below is the contract, restated under tests/ (tests/host/viterbi_ref.cpp over
 * csrc/hz_viterbi_math.h state by state, tests/viterbi_ref.py in numpy over whole arrays, and exhaustively for short
 * frames).  Everything is integer arithmetic after one defined quantisation: the kernel, the host program and the numpy
 * restatement agree exactly.
 *
 * Code.  Constraint length K, 3 <= K <= 9, S = 2^(K-1) states; rate 1/n mother code, n = 2, 3 or 4; generators
 * g[0 ... n-1], K-bit words, not zero, whose most significant bit multiplies the newest input bit; an inversion mask
 * `inv` of n bits (CCSDS inverts its second output).  `state` holds the previous K - 1 input bits, the most recent in
 * bit K - 2.  With reg = (u[t] << (K-1)) | state the outputs are c_j[t] = parity(reg & g[j]) ^ ((inv >> j) & 1),
 * j = 0 ... n-1, sent in that order; the next state is reg >> 1.  The encoder starts in state 0.
 *
 * Puncturing.  A pattern of Lp bits, n <= Lp <= 64, Lp a multiple of n, first bit = most significant.  Mother-code bit
 * m = t * n + j of a frame is transmitted iff pattern bit m mod Lp is 1.  Every group of n has at least one 1: no
 * trellis step is blind.  An all-ones pattern of length n means no puncturing.
 *
 * Termination.  HZSDR_VITERBI_TAIL: D data bits are followed by K - 1 zero input bits, T = D + K - 1 steps, and the
 * survivor is the one ending in state 0.  HZSDR_VITERBI_TRUNCATED: T = D, and the survivor is the end state of smallest
 * metric, ties to the smallest state number.
 *
 * Sizes.  1 <= D, T <= 8192.  N is the number of transmitted positions among the T * n mother bits, N <= 8192 =
 * HZSDR_FRAMESYNC_MAX_PAYLOAD: a frame sync payload fits as it is.  FB = ceil(N / 8), DB = ceil(D / 8).
 *
 * Input.  HZSDR_VITERBI_BITS: packed hard bits, most significant bit first, FB bytes per frame slot; frame f of row r
 * is at in + r * in_stride + f * FB BYTES: the frame sync bank's `out` block.  Bit 1 gives q = +1, bit 0 gives q = -1.
 * HZSDR_VITERBI_SOFT_F32: one float32 per received position, sign bit clear meaning 1 as in the frame sync bank; frame f
 * of row r is at float r * in_stride + f * N;  q = (int) rintf(fminf(fmaxf(x * scale, -127), 127)), a NaN gives q = 0
 * (an erasure); `scale` is a finite positive float32 given at create (it is not read for HZSDR_VITERBI_BITS).  Each
 * operation is one float32 operation, so q is the same everywhere; +-infinity gives +-127, -0 gives 0.
 * in_counts is uint32[R] in the context's memory space, or null for "every row has cap": row r decodes
 * min(in_counts[r], cap) frames (the frame sync bank's counts may exceed cap).
 *
 * Metric.  A punctured position costs 0.  A transmitted position of value q under the hypothesised code bit c costs
 * |q| when q != 0 and (q > 0) != (c == 1), else 0.  A branch costs the sum over its n positions.  Path metrics are
 * exact non-negative integers: metric[0] = 0 at t = 0, every other state starts at INF = 2^30; INF plus the largest
 * reachable cost (127 * 4 * 8192) neither wraps in uint32 nor reaches below a real metric.
 *
 * Add-compare-select.  New state s' has input u = s' >> (K-2) and the predecessors p_b = ((s' & (S/2 - 1)) << 1) | b,
 * b = 0, 1.  Its new metric is the minimum over b of metric[p_b] + cost(p_b, u); the decision d[t][s'] is the b of the
 * minimum, TIES TO b = 0.  Traceback from the end state s, t = T - 1 down to 0: u[t] = s >> (K-2), then
 * s = ((s & (S/2 - 1)) << 1) | d[t][s].  The output is u[0 ... D-1], most significant bit first in DB bytes, pad bits 0.
 *
 * CRC (crc_bits C = 0: none).  C = 8, 16, 24 or 32, C < D; poly, init, xorout below 2^C.  Over u[0 ... D-C-1] in stream
 * order: reg = init; per bit top = ((reg >> (C-1)) & 1) ^ bit, reg = (reg << 1) & (2^C - 1), reg ^= poly if top; at the
 * end reg ^= xorout.  The frame is "ok" iff reg equals u[D-C ... D-1] read first bit = most significant.  No reflect
 * switches: a reflected CRC over a link that sends each byte least significant bit first is this register over the
 * received bit order.  The data bits are emitted either way.
 *
 * Output of a call, for frame f < min(in_counts[r], cap) of row r:  out + r * out_stride + f * DB bytes hold the
 * decoded bits;  info[r * cap + f] = final metric | crc_ok << 31 (the metric is below 2^23; for hard input it is the
 * number of channel bit errors corrected; the flag is 0 when C = 0).  Slots from min(in_counts[r], cap) up are left
 * untouched in out and in info, and so are a frame's neighbouring bytes when DB is no multiple of 8.  The bank keeps NO
 * state between calls: frames are independent.
 *
 * Invariance: a frame's bytes and info do not depend on R, on either stride, on cap or the frame's slot, on the memory
 * space, on how frames are grouped into waves or on any other frame's contents (NaNs, infinities and all-erasure frames
 * included).
 * Speed: one wave runs a frame's T add-compare-select steps one after the other, lane = state, and then walks the
 * survivor back, so ONE frame is bound by one wave's dependent chain: 490 cycles per trellis step, forward and traceback
 * together, 216 us for K = 7, D = 1024, measured.  Many frames are bound by the instruction issue of the waves that share
 * a SIMD: 65536 such frames take 6.3 ms, 10.7 Gbit/s of decoded data, measured; K = 5 decodes 27.6 Gbit/s and K = 9
 * 2.1 Gbit/s at 8192 frames, measured.
 */
#ifndef HZSDR_VITERBI_H
#define HZSDR_VITERBI_H

#include "hzsdr.h"
#include "hzsdr_framesync.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hzsdr_viterbi hzsdr_viterbi;

#define HZSDR_VITERBI_MAX_ROWS 8192
#define HZSDR_VITERBI_MIN_K 3
#define HZSDR_VITERBI_MAX_K 9
#define HZSDR_VITERBI_MAX_RATE 4
#define HZSDR_VITERBI_MAX_PATTERN 64
#define HZSDR_VITERBI_MAX_BITS 8192
#define HZSDR_VITERBI_MAX_FRAMES 4194304

/* input kinds */
#define HZSDR_VITERBI_BITS 1
#define HZSDR_VITERBI_SOFT_F32 32
/* terminations */
#define HZSDR_VITERBI_TAIL 0
#define HZSDR_VITERBI_TRUNCATED 1
/* hzsdr_viterbi_plan's `form`: where a wave keeps a frame's decisions: in its LDS, or in a device scratch of the bank */
#define HZSDR_VITERBI_FORM_LDS 1
#define HZSDR_VITERBI_FORM_SCRATCH 2

/* A bank over `rows` rows of frames: kind, K, n, the host array gens[n] (free to go when this returns), inv, the
 * puncture pattern of pattern_bits bits, the termination, D = data_bits, scale, and the CRC (crc_bits 0: none) as above.
 * HZSDR_ERR_FORMAT_UNKNOWN for another kind; HZSDR_ERR_INVALID_ARGUMENT for anything outside the bounds above (K, n, a
 * zero or too wide generator, inv or a pattern with bits above its width, a pattern group without a 1, D, T or N above
 * 8192, a scale that is not finite and positive with soft input, a CRC width other than 0, 8, 16, 24, 32 or not below
 * D, CRC parameters above the width), rows out of 1 ... 8192, null gens. */
int hzsdr_viterbi_create(hzsdr_ctx *ctx, int kind, unsigned K, unsigned n, const unsigned *gens, unsigned inv, uint64_t pattern,
                         unsigned pattern_bits, int termination, size_t data_bits, float scale, unsigned crc_bits, uint32_t crc_poly,
                         uint32_t crc_init, uint32_t crc_xorout, size_t rows, hzsdr_viterbi **out);
/* Decode min(in_counts[r], cap) frames of every row.  in, in_counts, out and info are in the context's memory space;
 * in_stride is in BYTES (HZSDR_VITERBI_BITS) or floats (HZSDR_VITERBI_SOFT_F32), out_stride in bytes, both ignored when
 * rows = 1; info takes rows * cap entries.  HZSDR_ERR_DST_TOO_SMALL when rows > 1 and out_stride is below cap * DB;
 * HZSDR_ERR_INVALID_ARGUMENT for cap = 0, rows * cap above 2^22, rows > 1 with in_stride below cap * FB (cap * N floats),
 * null in, out or info: decided before anything is launched, nothing is written.
 * Stream-ordered on the context's stream; HOST contexts stage every array. */
int hzsdr_viterbi_decode(hzsdr_viterbi *v, const void *in, size_t in_stride, const uint32_t *in_counts, size_t cap, uint8_t *out,
                         size_t out_stride, uint32_t *info);
/* N received positions, FB = ceil(N / 8), T trellis steps and DB = ceil(D / 8) of a frame (null: not wanted). */
int hzsdr_viterbi_sizes(const hzsdr_viterbi *v, size_t *N, size_t *FB, size_t *T, size_t *DB);
/* The frames one wave decodes side by side (64 / S, at least 1), the states a lane owns (S / 64, at least 1), the bytes
 * of one frame's decisions and where they live (HZSDR_VITERBI_FORM_*), so that tests can aim at edges. */
int hzsdr_viterbi_plan(const hzsdr_viterbi *v, size_t *frames_per_wave, size_t *states_per_lane, size_t *decision_bytes, int *form);
int hzsdr_viterbi_free(hzsdr_viterbi *v);

#ifdef __cplusplus
}
#endif

#endif /* HZSDR_VITERBI_H */

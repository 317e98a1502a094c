/*
 * hzsdr_demap.h -- the demapper bank of libhzsdr_hip: frames of received symbols to per-bit soft values in the order
 * and with the signs a decoder expects, over many rows of frames at once.  It stands between the soft frame bank
 * (hzsdr_softframe.h) and the decoder banks (hzsdr_viterbi.h, hzsdr_ldpc.h): it takes the soft frame bank's float32
 * block and the device-side counts as they are -- with complex rows and B = 2 a frame's P floats are its P / 2 complex
 * symbols re, im, re, im ..., the frame's rotation hypothesis already undone; with real rows and B = 1 they are its real
 * symbols -- and writes the block the decoders read, with no host read in between.  It does the two things that keep a
 * signal other than plain BPSK / QPSK away from the decoders: max-log soft values for constellations of up to 8 bits per
 * symbol (8PSK, 16/64/256-QAM, APSK, the four levels of 4-FSK), and, on the soft values, the bit deinterleaver, the
 * depuncturer (holes become erasures) and the derandomiser (CCSDS 131.0-B randomises the LDPC codeword).
 *
 * Not in scope: exact (log-sum) LLRs; combining repeated positions (rate matching with soft combining); rotations that
 * are not multiples of 90 degrees, such as 8PSK's 45 degree ambiguity (the frame sync bank's four hypotheses do not
 * resolve them); differential modes; a separable fast path for square QAM (the contract permits one: any evaluation
 * that gives the same bits is allowed); changing the gain after create.
 *
 * The entries live beside hzsdr.h and the other headers (same conventions, same status codes, same context).  The
 * reference has no such stage: the definition below is the contract, restated under tests/ (tests/host/demap_ref.cpp
 * over csrc/hz_demap_math.h symbol by symbol, tests/demap_ref.py in numpy over whole arrays).  Every step is ONE float32
 * operation, so the kernel, the host program and numpy agree on every bit.
 *
 * Kinds.  HZSDR_DEMAP_C64: a symbol is a pair of float32 (xr, xi), the points are complex.  HZSDR_DEMAP_REAL_F32: one
 * float32 per symbol, the points are real (PAM, 4-FSK levels).  HZSDR_DEMAP_LLR_F32: one float32 that is a per-bit value
 * already, m = 1 and no points; only gain, order and sign are applied (BPSK / QPSK frames that need a deinterleaver or a
 * derandomiser).
 *
 * Constellation.  m bits per symbol, 1 <= m <= 8, M = 2^m points: a host array at create (free to go afterwards) of
 * M pairs (pr, pi) for C64, of M floats for REAL_F32; every point is finite.  Point p carries the label p: bit j of a
 * symbol (0 is the first) is (p >> (m - 1 - j)) & 1.
 *
 * Frame.  S symbols, 1 <= S <= 8192, S * m <= 16384 = HZSDR_DEMAP_MAX_LLRS (a frame's values fit in 64 KiB of LDS);
 * N output floats, 1 <= N <= 8192 (the decoders' limit).  Input frame f of row r is at float r * in_stride + f * W,
 * W = 2 S for C64 and S otherwise; output frame f of row r is at float r * out_stride + f * N.  Row r handles
 * min(in_counts[r], cap) frames, a null in_counts means cap; in_counts is uint32[R] in the context's memory space.
 * 1 <= R <= 8192, R * cap <= 2^22.
 *
 * Per symbol s, every step ONE float32 operation, denormals kept (the unit is built with -ffp-contract=off):
 *   dr = xr - pr,  di = xi - pi,  d_p = (dr * dr) + (di * di): two multiplies and one add, not fused;
 *   REAL_F32: d_p = dr * dr;
 *   for bit j: d0 = the minimum of d_p over the points whose bit j is 0, d1 over those whose bit j is 1;
 *   L[s * m + j] = (d0 - d1) * g.
 * A positive value says 1 (the family's rule: sign bit clear means 1), so the hard decision of L is the nearest point's
 * bit wherever d0 != d1.  If xr or xi is a NaN all m values of the symbol are erasures.  LLR_F32: L[s] = x * g.
 * No d_p is a NaN or -0 once the input has no NaN, so the minima do not depend on the order they are taken in: the
 * definition names values, not storage or order.
 *
 * Gain.  g is a finite positive float32, shared by the rows (n_gains = 1) or one per row (n_gains = rows); for max-log
 * LLRs it is 1 / (2 sigma^2).
 *
 * Order, holes and sign.  perm is an optional uint32[N]: out[k] = L[perm[k]], perm[k] < S * m, or HZSDR_DEMAP_ERASED
 * (0xFFFFFFFF) for a hole; repeats are allowed.  Without perm N must equal S * m and the order is kept.  flip is
 * optional: N packed bits, most significant bit first; where bit k is 1 the sign bit of out[k] is flipped on the bit
 * pattern.  Last, any NaN is stored as the quiet NaN 0x7FC00000 -- an erased input, a hole, inf - inf --, which is the
 * soft frame bank's erasure and the decoders' q = 0.  Every entry of perm is validated at create, before it can index
 * anything.
 *
 * Slots from min(in_counts[r], cap) up are left untouched, and so are the floats between a row's cap frames and the next
 * row.  The bank keeps NO state between calls.
 *
 * Invariance: a frame's floats do not depend on R, on either stride, on cap or the frame's slot, on the memory space, on
 * how frames are grouped into workgroups or on any other frame's contents.
 *
 * Speed: a workgroup takes G frames side by side, each on T threads (hzsdr_demap_plan), lane = symbol, the points read
 * as wave-uniform scalars; the S * m values go to LDS and leave in k order (perm gather, flip, canonical NaN), so stores
 * are whole segments whatever the permutation.  Per symbol the kernel makes 2 subtractions, 2 multiplies and 1 add per
 * point (2 and 1 for real points) and then the minima: m * M point by point, about 3 M in the two-sided tree over blocks
 * of 32 points that HZSDR_DEMAP_FORM_TREE reports, used from m = 7 on (DESIGN.md section 4 counts both per m).  On the
 * MI355X, 32768 frames of S = 2048 from HBM, beside the library's own device copy of the bytes read plus written: LLR_F32
 * 186 us (2.1 of the copy), C64 with m = 2 267 us (1.5; 251 Gsymbols/s), m = 4 691 us (2.6; 97), m = 6 925 us (3.5; 73),
 * m = 8 2811 us (10.5; 24 Gsymbols/s), REAL_F32 with m = 2 270 us (2.0), all measured; a block interleaver as perm adds
 * 7 ... 45 %; one frame takes 9 ... 12 us up to m = 6 and 24.5 us at m = 8, measured.  Both forms of the minima were
 * timed: at m = 8 the tree takes 2811 us where point by point takes 4881, at m = 6 1077 where point by point takes 925;
 * m = 7 was not measured (profiles/demap_time.txt).
 */
#ifndef HZSDR_DEMAP_H
#define HZSDR_DEMAP_H

#include "hzsdr.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hzsdr_demap hzsdr_demap;

#define HZSDR_DEMAP_MAX_ROWS 8192
#define HZSDR_DEMAP_MAX_BITS 8
#define HZSDR_DEMAP_MAX_SYMBOLS 8192
#define HZSDR_DEMAP_MAX_LLRS 16384
#define HZSDR_DEMAP_MAX_OUT 8192
#define HZSDR_DEMAP_MAX_FRAMES 4194304
#define HZSDR_DEMAP_ERASED 0xFFFFFFFFu

/* kinds (C64 is HZSDR_FMT_C64, REAL_F32 is HZSDR_SYMSYNC_REAL_F32: the frame sync and soft frame banks' kinds) */
#define HZSDR_DEMAP_C64 1
#define HZSDR_DEMAP_REAL_F32 32
#define HZSDR_DEMAP_LLR_F32 33
/* hzsdr_demap_plan's `form`, a sum of: several frames share a workgroup; a perm gathers the output; the minima are
 * taken by the two-sided tree (else point by point and bit by bit) */
#define HZSDR_DEMAP_FORM_GROUPED 1
#define HZSDR_DEMAP_FORM_PERM 2
#define HZSDR_DEMAP_FORM_TREE 4

/* A bank over `rows` rows of frames: kind, m = bits_per_symbol, the host array `points` (2 M floats re, im for C64, M
 * floats for REAL_F32, null for LLR_F32), S = symbols, perm (uint32[received] or null), N = received, flip
 * (ceil(N / 8) bytes or null), gains[n_gains]; all host arrays are free to go when this returns.
 * HZSDR_ERR_FORMAT_UNKNOWN for another kind; HZSDR_ERR_INVALID_ARGUMENT for m outside 1 ... 8, LLR_F32 with m != 1 or
 * with points, a null or non-finite point, S, N or S * m out of range, a perm entry that is neither below S * m nor
 * HZSDR_DEMAP_ERASED, no perm with N != S * m, n_gains that is neither 1 nor rows, null gains, a gain that is not finite
 * and positive, rows outside 1 ... 8192. */
int hzsdr_demap_create(hzsdr_ctx *ctx, int kind, unsigned bits_per_symbol, const float *points, size_t symbols, const uint32_t *perm,
                       size_t received, const uint8_t *flip, const float *gains, size_t n_gains, size_t rows, hzsdr_demap **out);
/* Demap min(in_counts[r], cap) frames of every row.  in, in_counts and out are in the context's memory space; the
 * strides are in floats and are ignored when rows = 1.  HZSDR_ERR_DST_TOO_SMALL when rows > 1 and out_stride is below
 * cap * N; HZSDR_ERR_INVALID_ARGUMENT for cap = 0, rows * cap above 2^22, rows > 1 with in_stride below cap * W, null in
 * or out, in and out ranges that overlap: decided before anything is launched, nothing is written.
 * Stream-ordered on the context's stream; HOST contexts stage every array. */
int hzsdr_demap_run(hzsdr_demap *d, const float *in, size_t in_stride, const uint32_t *in_counts, size_t cap, float *out, size_t out_stride);
/* S symbols, W input floats, m bits per symbol and N output floats of a frame (null: not wanted). */
int hzsdr_demap_sizes(const hzsdr_demap *d, size_t *S, size_t *W, size_t *m, size_t *N);
/* The frames one workgroup takes side by side, the threads a frame has, the LDS bytes of one frame's values and the form
 * (a sum of HZSDR_DEMAP_FORM_*), so that tests can aim at edges. */
int hzsdr_demap_plan(const hzsdr_demap *d, size_t *frames_per_group, size_t *threads_per_frame, size_t *frame_lds_bytes, int *form);
int hzsdr_demap_free(hzsdr_demap *d);

#ifdef __cplusplus
}
#endif

#endif /* HZSDR_DEMAP_H */

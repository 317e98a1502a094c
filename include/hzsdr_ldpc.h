/*
 * hzsdr_ldpc.h -- the LDPC decoder bank of libhzsdr_hip: soft or hard frames of a binary low-density parity-check code
 * to data bits, the number of unsatisfied checks, the iterations run and a verdict per frame, over many rows of frames at
 * once.  It is a sibling of hzsdr_viterbi.h and stands where that bank stands: it takes the soft frame bank's float32
 * block (hzsdr_softframe.h) or the frame sync bank's `out` block (hzsdr_framesync.h) and their device-side counts as they
 * are, with no host read in between.  What it leaves to others: layered schedules; non-binary codes; shortening by known
 * bits; rate matching; the outer BCH code of DVB-S2; soft outputs of the decoder.  Symbols of more than two bits, bit
 * interleaving, punctured positions inside a frame and a randomiser on the codeword (CCSDS 131.0-B) are undone in front of
 * this bank by the demapper bank (hzsdr_demap.h), whose output block is this bank's input.  It ships no standard's tables: the
 * Python layer expands a quasi-cyclic base table (the form in which CCSDS 131.0-B, DVB-S2, 802.11n and 5G publish their
 * codes) into the compressed form below.
 *
 * The entries live beside hzsdr.h and the other headers (same conventions, same status codes, same context).  The
 * reference has no decoder: the definition below is the contract, restated under tests/ (tests/host/ldpc_ref.cpp over
 * csrc/hz_ldpc_math.h edge by edge, tests/ldpc_ref.py in numpy over whole arrays).  Everything is integer arithmetic
 * after one defined quantisation: the kernel, the host program and the numpy restatement agree exactly.
 *
 * Code.  The parity-check matrix H of m checks over n variables in check-major compressed form: row_ptr is uint32[m + 1]
 * with row_ptr[0] = 0 and row_ptr[m] = E = edges; col is uint32[E], the variables of check c at col[row_ptr[c] ...
 * row_ptr[c + 1] - 1], STRICTLY ASCENDING inside a check.  1 <= m <= 16384, 2 <= n <= 16384, E <= 65536; every check has
 * degree 2 ... 64, every variable degree 1 ... 64.  Edge e = (c, v) is entry e of col.
 *
 * Frame.  N received positions, 1 <= N <= 8192 = HZSDR_FRAMESYNC_MAX_PAYLOAD (a frame sync payload fits as it is), occupy
 * the variables head ... head + N - 1, head + N <= n; every other variable is punctured, q = 0 (a trailing punctured
 * block as in AR4JA, or a leading one).  D data bits, 1 <= D <= n, are the variables 0 ... D - 1.  FB = ceil(N / 8),
 * DB = ceil(D / 8).
 *
 * Input.  HZSDR_LDPC_SOFT_F32: one float32 per received position, sign bit clear meaning 1; frame f of row r is at float
 * r * in_stride + f * N: the soft frame bank's block.  q = (int) rintf(fminf(fmaxf(x * scale, -127), 127)), a NaN gives
 * q = 0 (an erasure): the Viterbi bank's quantiser, operation for operation, each ONE float32 operation, so q is the same
 * everywhere; +-infinity gives +-127, -0 gives 0.  `scale` is a finite positive float32 given at create.
 * HZSDR_LDPC_BITS: packed hard bits, most significant bit first, FB bytes per frame slot, frame f of row r at
 * in + r * in_stride + f * FB BYTES: the frame sync bank's `out` block.  Bit 1 gives q = +level, bit 0 gives q = -level,
 * `level` in 1 ... 127 given at create.  (`scale` is not read for BITS, `level` not for SOFT_F32.)
 * in_counts is uint32[R] in the context's memory space, or null for "every row has cap": row r decodes
 * min(in_counts[r], cap) frames (the frame sync bank's counts may exceed cap).  1 <= R <= 8192, R * cap <= 2^22.
 *
 * Decision: flooding min-sum in integers.  Parameters at create: max_iters in 1 ... 255; a = norm in 1 ... 16, the
 * normalisation a / 16; beta = offset in 0 ... 126.  A positive value says "1".  The message r_e of every edge starts at
 * 0 and P[v] = q[v].  hard[v] = 1 iff P[v] > 0; u is the number of checks whose hard bits have odd parity.  If u = 0 the
 * frame leaves with iters = 0.  Otherwise, for it = 1 ... max_iters:
 *   1. for every edge e = (c, v):  t_e = clamp(P[v] - r_e, -127, 127), P and r of the previous iteration;
 *   2. for every check c:  par = the xor of (t_e > 0) over its edges;  m1 <= m2 the two smallest |t_e|;  an edge gets
 *      mag = m2 if it is the FIRST edge, in col order, that attains m1, and mag = m1 otherwise;
 *      mag' = max(((mag * a) >> 4) - beta, 0);  r_e = +mag' if par ^ (t_e > 0) is 1, and -mag' otherwise;
 *   3. P[v] = q[v] + the sum of r_e over the variable's edges, an exact integer sum (|P| <= 127 * 65 fits in int16);
 *      hard and u anew; stop when u = 0.
 * `iters` is the number of iterations run.  The definition names values, not storage.
 *
 * Output of a call, for frame f < min(in_counts[r], cap) of row r:  out + r * out_stride + f * DB bytes hold
 * hard[0 ... D-1] of the last iteration run, most significant bit first, pad bits 0;
 * info[r * cap + f] = u | iters << 16 | (u == 0) << 31  (u <= 16384, iters <= 255).  Slots from min(in_counts[r], cap) up
 * are left untouched in out and in info, and so are a frame's neighbouring bytes.  The bank keeps NO state between calls.
 *
 * Invariance: a frame's bytes and info do not depend on R, on either stride, on cap or the frame's slot, on the memory
 * space, on how frames are grouped into workgroups or on any other frame's contents (frames that are all NaN, infinity
 * or -0 included).
 *
 * Speed: a workgroup decodes G frames side by side, each on T threads (hzsdr_ldpc_plan), a frame's q, P and messages in
 * LDS from the first load to the packed store; an iteration is a pass over the checks and a pass over the variables with
 * two barriers, 4 LDS reads and 2 writes of state per edge (DESIGN.md section 4 counts them).  ONE frame of a (3, 6)
 * code of n = 2048 takes 3.4 us per iteration, measured, bound by the barriers and the latency of the dependent LDS
 * accesses; 32768 such frames (D = 1024) decode 13.7 Gbit/s where they converge in about 3 iterations and 4.2 Gbit/s
 * where every frame runs 20, measured, beside the Viterbi bank's 10.7 Gbit/s (K = 7, D = 1024), the family's yardstick;
 * the largest frames (n = 16384, half of it punctured, tables through the cache) decode 3.1 and 2.0 Gbit/s, measured
 * (profiles/ldpc_time.txt).
 */
#ifndef HZSDR_LDPC_H
#define HZSDR_LDPC_H

#include "hzsdr.h"
#include "hzsdr_framesync.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hzsdr_ldpc hzsdr_ldpc;

#define HZSDR_LDPC_MAX_ROWS 8192
#define HZSDR_LDPC_MAX_CHECKS 16384
#define HZSDR_LDPC_MAX_VARIABLES 16384
#define HZSDR_LDPC_MAX_EDGES 65536
#define HZSDR_LDPC_MAX_DEGREE 64
#define HZSDR_LDPC_MAX_BITS 8192
#define HZSDR_LDPC_MAX_ITERS 255
#define HZSDR_LDPC_MAX_FRAMES 4194304

/* input kinds */
#define HZSDR_LDPC_BITS 1
#define HZSDR_LDPC_SOFT_F32 32
/* hzsdr_ldpc_plan's `form`: where a workgroup reads the code's edge tables: its LDS beside the frames, or the cache */
#define HZSDR_LDPC_FORM_TABLES_LDS 1
#define HZSDR_LDPC_FORM_TABLES_CACHE 2

/* A bank over `rows` rows of frames: kind; the code, checks = m, variables = n, the host arrays row_ptr[m + 1] and
 * col[edges] (free to go when this returns); head, received = N and data_bits = D; scale (SOFT_F32) and level (BITS);
 * max_iters, norm = a and offset = beta, all as above.  HZSDR_ERR_FORMAT_UNKNOWN for another kind;
 * HZSDR_ERR_INVALID_ARGUMENT for anything outside the bounds above (m, n, edges, row_ptr[0] != 0, a row pointer that
 * descends or disagrees with edges, a degree out of 2 ... 64 or 1 ... 64, a column >= n or not above its predecessor,
 * head + N > n, N or D out of range, a scale that is not finite and positive with soft input, a level out of 1 ... 127
 * with hard input, max_iters, norm, offset), rows out of 1 ... 8192, null row_ptr or col.  No field taken from the
 * arrays indexes memory before it is checked. */
int hzsdr_ldpc_create(hzsdr_ctx *ctx, int kind, size_t checks, size_t variables, const uint32_t *row_ptr, const uint32_t *col, size_t edges,
                      size_t head, size_t received, size_t data_bits, float scale, unsigned level, unsigned max_iters, unsigned norm,
                      unsigned offset, size_t rows, hzsdr_ldpc **out);
/* Decode min(in_counts[r], cap) frames of every row.  in, in_counts, out and info are in the context's memory space;
 * in_stride is in BYTES (HZSDR_LDPC_BITS) or floats (HZSDR_LDPC_SOFT_F32), out_stride in bytes, both ignored when
 * rows = 1; info takes rows * cap entries.  HZSDR_ERR_DST_TOO_SMALL when rows > 1 and out_stride is below cap * DB;
 * HZSDR_ERR_INVALID_ARGUMENT for cap = 0, rows * cap above 2^22, rows > 1 with in_stride below cap * FB (cap * N floats),
 * null in, out or info: decided before anything is launched, nothing is written.
 * Stream-ordered on the context's stream; HOST contexts stage every array. */
int hzsdr_ldpc_decode(hzsdr_ldpc *l, const void *in, size_t in_stride, const uint32_t *in_counts, size_t cap, uint8_t *out, size_t out_stride,
                      uint32_t *info);
/* N received positions, FB = ceil(N / 8), the code's n, m and E, and DB = ceil(D / 8) of a frame (null: not wanted). */
int hzsdr_ldpc_sizes(const hzsdr_ldpc *l, size_t *N, size_t *FB, size_t *n, size_t *m, size_t *E, size_t *DB);
/* The frames one workgroup decodes side by side, the threads a frame has, the LDS bytes of one frame's state (q, P and
 * the messages) and where the edge tables are read (HZSDR_LDPC_FORM_*), so that tests can aim at edges. */
int hzsdr_ldpc_plan(const hzsdr_ldpc *l, size_t *frames_per_group, size_t *threads_per_frame, size_t *frame_lds_bytes, int *form);
int hzsdr_ldpc_free(hzsdr_ldpc *l);

#ifdef __cplusplus
}
#endif

#endif /* HZSDR_LDPC_H */

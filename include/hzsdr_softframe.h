/*
 * hzsdr_softframe.h -- the soft frame bank of libhzsdr_hip: the payload FLOATS of the frames a frame sync bank found,
 * over one row of soft symbols or over many rows at once.  It is the next member of the family of hzsdr_tuner.h,
 * hzsdr_iir.h, hzsdr_agc.h, hzsdr_carrier.h, hzsdr_symsync.h, hzsdr_framesync.h, hzsdr_viterbi.h and hzsdr_rs.h and
 * runs BESIDE the frame sync bank: it sees the same symbol rows in the same pushes, takes that bank's device-side
 * positions, info and counts of the push as they are, and writes every accepted frame's P payload floats through the
 * frame's hypothesis map in the layout the Viterbi bank's soft input (HZSDR_VITERBI_SOFT_F32) reads: frame f of row r
 * at float r * out_stride + f * P, sign bit clear meaning 1.  Nothing is read by the host in between.  What it leaves to
 * others: a soft form of the frame sync bank's differential decodings (diff != 0 there has NO soft counterpart here:
 * pair this bank with diff = 0 banks only); level normalisation (hzsdr_agc.h in front, the decoder's `scale` behind);
 * int8 soft values.  Symbols of more than two bits, bit deinterleaving, depuncturing and derandomising of the soft values
 * are the demapper bank's (hzsdr_demap.h), which takes this bank's block as it is.
 *
 * The entries live beside hzsdr.h and the other headers (same conventions, same status codes, same context).  The
 * reference has no such stage: the definition below is the contract, restated under tests/ (tests/host/softframe_ref.cpp
 * over csrc/hz_softframe_plan.h push by push, tests/softframe_ref.py in numpy over whole streams).
 *
 * Rows, B, P, hypotheses and maps are those of hzsdr_framesync_create: R rows, 1 <= R <= 8192, of kind
 * HZSDR_SYMSYNC_REAL_F32 or HZSDR_FMT_C64; B = 1 for real rows, B = 1 (Re only) or B = 2 for complex rows; P payload
 * bits, B <= P <= 8192, P a multiple of B; H hypotheses, 1 <= H <= 4, with maps[H].  Ps = P / B is a payload's symbols;
 * the bank keeps the last Kh = Ps - 1 symbols of every row, because a frame's payload almost always began in an earlier
 * push.
 * Input of a push: in, n, in_stride and in_counts are what hzsdr_framesync_push got; positions (uint64 [R * cap]), info
 * (uint32 [R * cap]) and counts (uint32 [R]) are what it wrote; cap is the same.  Row r consumes c = min(in_counts[r], n)
 * symbols, the stream's symbols p0 ... p1 - 1 with p1 = p0 + c, and emits min(counts[r], cap) frames.
 *
 * A frame's floats.  A row's stream of decision floats is the floats themselves (real rows), the Re parts (complex rows,
 * B = 1) or re, im, re, im ... (complex rows, B = 2): B per symbol.  With s = positions[r * cap + f] and
 * h = (info[r * cap + f] >> 8) & 0xFF, float k of the frame is float s * B + k of that stream through map maps[h]:
 *   B = 1: map 0 copies the 32 bits, map 1 copies them with the sign bit flipped;
 *   B = 2: map q applies (x0, x1) -> (x1, x0 with its sign bit flipped) q times to every pair.
 * Sign flips are on the bit pattern and no arithmetic is done on the values: NaN payloads, -0 and infinities pass
 * through exactly.
 * Equivalence: the frame sync bank decides 1 where a float's sign bit is clear and maps the decided bits by the same
 * maps, so THE SIGN OF EMITTED FLOAT k DECIDES THE BIT THE FRAME SYNC BANK PACKED AT PLACE k of the same frame (bit
 * 7 - k % 8 of byte k / 8 is 1 iff the sign bit of float k is clear), for diff = 0.  The hard frame is the soft frame's
 * signs.
 *
 * Window.  A frame is served when h < H, s + Kh >= p0 and s + Ps <= p1: its payload ends in this push and began inside
 * what the bank holds.  Every frame the frame sync bank emits in the same push passes this.  Otherwise all P floats are
 * the quiet NaN 0x7FC00000, which the Viterbi bank treats as erasures.  status[r * cap + f] is 0 when served, 2 when
 * h >= H, else 1 (outside the window).  No value read from positions, info, counts or in_counts indexes memory without
 * this test: forged arrays give NaN frames and a status, never an access outside the bank's history and the push's input.
 * Slots from min(counts[r], cap) up stay untouched in out and status, and so do the floats between a row's cap * P and
 * out_stride.
 *
 * State of a row: the symbols consumed and the decision floats of the last Kh symbols (Kh * B floats; complex rows with
 * B = 1 keep Re only), zero where the stream had not begun.  hzsdr_softframe_get_state / _set_state move it as uint64
 * positions and float32 history, oldest first, bit for bit (NaN payloads included).  A push with n = 0, or a row whose
 * count is 0, leaves that row's state as it is.
 *
 * Invariance: floats, status and state do not depend on how the stream is cut into pushes, on the memory space, on R, on
 * either stride, on cap (up to what is stored) or on the other rows.  The stage moves bit patterns: the kernel, the
 * host program and the numpy restatement agree on every bit.
 * Speed: the stage is a copy, and its yardstick is the library's device copy of the bytes it writes.  Measured
 * (tools/softframe_time.py, profiles/softframe_time.txt), gather and carry of a push together: ONE frame of 2048 floats
 * 16.1 us (real rows) and 15.4 us (two bits per symbol), two launches, beside 8.5 us of one copy launch; 8192 rows x 4
 * frames of 2048 floats (268 MB written, the inputs from HBM) 189.7 us on real rows, 2.18 times the copy's 86.9 us, and
 * 154.2 us at two bits per symbol, 1.77 times: one float per lane against one 8-byte pair per lane.  Loads wider than
 * that were not tried.
 */
#ifndef HZSDR_SOFTFRAME_H
#define HZSDR_SOFTFRAME_H

#include "hzsdr.h"
#include "hzsdr_symsync.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hzsdr_softframe hzsdr_softframe;

#define HZSDR_SOFTFRAME_MAX_ROWS 8192
#define HZSDR_SOFTFRAME_MAX_PAYLOAD 8192
#define HZSDR_SOFTFRAME_MAX_HYPOTHESES 4
#define HZSDR_SOFTFRAME_MAX_SLOTS (1u << 22) /* rows * cap of a push */

/* status of a frame slot */
#define HZSDR_SOFTFRAME_SERVED 0
#define HZSDR_SOFTFRAME_OUTSIDE 1
#define HZSDR_SOFTFRAME_NO_HYPOTHESIS 2

/* hzsdr_softframe_plan's `form`: _COMPLEX: complex64 rows; _DIBIT: B = 2 */
#define HZSDR_SOFTFRAME_FORM_COMPLEX 1
#define HZSDR_SOFTFRAME_FORM_DIBIT 2

/* A bank over `rows` rows of `kind` (HZSDR_SYMSYNC_REAL_F32 or HZSDR_FMT_C64): B = bits_per_symbol, P = payload_bits,
 * H = hyps with the host array maps[H] (free to go when this returns), all as hzsdr_framesync_create takes them.
 * Positions are 0, the history is zero.  HZSDR_ERR_FORMAT_UNKNOWN for another kind; HZSDR_ERR_INVALID_ARGUMENT for
 * anything outside the bounds above, a map that B does not have, rows out of range. */
int hzsdr_softframe_create(hzsdr_ctx *ctx, int kind, unsigned bits_per_symbol, unsigned payload_bits, unsigned hyps, const unsigned *maps,
                           size_t rows, hzsdr_softframe **out);
/* Serve min(counts[r], cap) frames of every row, then run min(in_counts[r], n) symbols of every row into the history.
 * All arrays are in the context's memory space; in_counts may be null ("every row has n"); out takes cap frames of P
 * floats per row, out_stride FLOATS from one row to the next (ignored when rows = 1); status takes rows * cap entries.
 * cap may be 0: the history advances only.
 * HZSDR_ERR_DST_TOO_SMALL when rows > 1 and out_stride is below cap * P; HZSDR_ERR_INVALID_ARGUMENT for rows > 1 with
 * in_stride < n, rows * cap above 2^22, n above 2^31 - 16, null in with n > 0, null positions, info, counts, out or
 * status with cap > 0: decided before anything is launched, the state is unchanged and nothing is written.
 * Stream-ordered on the context's stream; HOST contexts stage every array. */
int hzsdr_softframe_push(hzsdr_softframe *f, const void *in, size_t n, size_t in_stride, const uint32_t *in_counts, const uint64_t *positions,
                         const uint32_t *info, const uint32_t *counts, size_t cap, float *out, size_t out_stride, uint32_t *status);
/* Copy the state into host arrays of rows_cap >= rows entries (history: rows * history_floats floats), behind every
 * push so far.  HZSDR_ERR_DST_TOO_SMALL when rows_cap is below rows.  history may be null when there is none (P = B). */
int hzsdr_softframe_get_state(hzsdr_softframe *f, uint64_t *positions, float *history, size_t rows_cap);
/* Replace the state by host arrays of exactly `rows` entries; positions are at most 2^62 - 1. */
int hzsdr_softframe_set_state(hzsdr_softframe *f, const uint64_t *positions, const float *history, size_t rows);
/* Symbols consumed per row since create, reset or set_state, into a host array of rows_cap >= rows entries. */
int hzsdr_softframe_positions(hzsdr_softframe *f, uint64_t *positions, size_t rows_cap);
/* The floats a workgroup of the gather moves per step (one frame per workgroup, ceil(P / step_floats) steps), the
 * history floats per row (Kh * B) and the form (HZSDR_SOFTFRAME_FORM_*), so that tests can aim at edges. */
int hzsdr_softframe_plan(const hzsdr_softframe *f, size_t *step_floats, size_t *history_floats, int *form);
/* Back to position 0 with a zero history. */
int hzsdr_softframe_reset(hzsdr_softframe *f);
int hzsdr_softframe_free(hzsdr_softframe *f);

#ifdef __cplusplus
}
#endif

#endif /* HZSDR_SOFTFRAME_H */

/*
 * hzsdr_framesync.h -- the frame sync bank of libhzsdr_hip: hard decisions, a sync-word search and the frames' payload
 * bits over one row of soft symbols, or over many rows at once.  It is the next member of the family of hzsdr_tuner.h,
 * hzsdr_iir.h, hzsdr_agc.h, hzsdr_carrier.h and hzsdr_symsync.h and stands behind the last of them: it takes the
 * symbol-timing bank's (symbols, counts) as they are, on the device, and this is where the data rate falls from symbols
 * to packets -- where a receive chain hands over to the CPU.  What it leaves to others: decoding a convolutionally
 * coded payload and its CRC (hzsdr_viterbi.h takes `out` and `counts` as they are); bit unstuffing (hzsdr_hdlc.h stands
 * where this bank stands on HDLC-framed links); descrambling and every other word of a protocol; soft outputs (hzsdr_softframe.h runs beside this bank, takes `positions`, `info` and
 * `counts` as they are and writes the frames' payload floats); a sync word longer than 64 bits.
 *
 * The entries live beside hzsdr.h and the other headers (same conventions, same status codes, same context).  The
 * reference has no frame sync: the definition below is the contract, restated under tests/ (tests/host/framesync_ref.cpp
 * over csrc/hz_framesync_math.h bit by bit, tests/framesync_ref.py in numpy position by position).
 *
 * Rows: R rows, 1 <= R <= 8192, of kind HZSDR_SYMSYNC_REAL_F32 (one float32 per symbol) or HZSDR_FMT_C64.  A bank has B
 * bits per symbol: B = 1 for real rows, B = 1 (Re only) or B = 2 for complex rows.  A complex row with B = 2 is read as
 * its interleaved floats re, im, re, im ..., one decision per float.
 * Input of a push: row r starts r * in_stride SYMBOLS into `in`; n is the symbols a row may hold; in_counts is
 * uint32[R] in the context's memory space, or null for "every row has n".  Row r consumes min(in_counts[r], n) symbols
 * and nothing beyond, so every row has a position of its own.  in_counts is what hzsdr_symsync_push wrote, taken as it
 * is, with no host read in between.
 *
 * Decisions.  For the i-th float of a row since create or reset, the raw decision d[i] is 1 when the float32's sign bit
 * is clear, else 0: taken from the bit pattern, so -0 decides 0 and a NaN decides by its sign bit and stays in its own
 * bit.  With `diff` (B = 1 only): 0: b[i] = d[i];  1: b[i] = d[i] ^ d[i-1];  2: b[i] = 1 ^ d[i] ^ d[i-1] (NRZI as AIS and
 * HDLC use it);  d[-1] = 0.
 *
 * Search.  A sync word of W bits, B <= W <= 64, W a multiple of B, given with the first-received bit as the most
 * significant of the W bits; a mask of the same form (not zero, don't-care bits 0) and a threshold thr < popcount(mask);
 * H hypotheses, 1 <= H <= 4, each a word words[h] and a payload map maps[h].  For a window ending at bit e, with
 * e >= W - 1 and e + 1 a multiple of B:
 *       dist_h(e) = popcount((b[e-W+1 ... e] ^ words[h]) & mask)
 * e is a candidate when the smallest dist_h is <= thr; its hypothesis is the one of smallest distance, ties to the
 * smallest h.  Bits before position 0 do not exist: an all-zero history never matches an all-zero word.
 *
 * Hold-off.  Per row a uint64 `hold`, in symbols, 0 at create.  Candidates are taken in ascending e, each when bit
 * e + P has been delivered (a candidate whose payload is still open has not been looked at, and leaves `hold` as it
 * is).  A candidate with payload start s = (e + 1) / B is accepted iff s >= hold; then hold = s + holdoff,
 * 1 <= holdoff <= 2^31.  This is the only sequential step, and it runs over candidates, not over samples.
 *
 * Frame.  An accepted candidate yields P payload bits, B <= P <= 8192, P a multiple of B:  p[k] = map_h(b)[e + 1 + k].
 * Maps for B = 1: 0 identity, 1 inverted.  Maps for B = 2, q = 0 ... 3: apply q times (b0, b1) -> (b1, !b0) to every
 * dibit -- the received symbol times (-i)^q, with b0 from Re and b1 from Im.  The frame is emitted by the push that
 * delivers bit e + P.  Nothing is flushed: a frame still open at the end of a stream is not emitted.
 *
 * Output of a push, for the f-th frame accepted in row r, f from 0 in every push:
 *   - out: p[k] in byte k / 8, bit 7 - k % 8, of out + r * out_stride + f * FB BYTES, FB = ceil(P / 8), pad bits 0;
 *   - positions[r * cap + f] = s, uint64;   info[r * cap + f] = dist | h << 8, uint32;
 *   - counts[r] is the number of frames accepted in this push, stored or not: only f < cap is stored, so a loss shows
 *     as counts[r] > cap; slots from min(counts[r], cap) up are left untouched;
 *   - *max_count, when not null, returns the largest count, and the call then waits, as hzsdr_symsync_push does.
 *
 * State of a row: the symbols consumed, `hold`, the last K = W + P - 1 bits, and (diff != 0) the last raw decision.
 * hzsdr_framesync_get_state / _set_state move it as uint64 positions (symbols), uint64 holds, ceil(K / 8) history bytes
 * per row -- history bit k, oldest first, in byte k / 8, bit 7 - k % 8, zero where the stream had not begun -- and one
 * byte per row for the last raw decision.
 *
 * Invariance: frames, positions, info, counts and state do not depend on how the stream is cut into pushes (n = 0 and
 * rows whose count is 0 included), on the memory space, on R, on either stride, on cap (up to what is stored) or on the
 * other rows' contents.  Everything is integer arithmetic on decided bits: the kernel, the host program and the numpy
 * restatement agree exactly.
 * Speed: the stage reads every input byte once and writes almost nothing.  A wave owns a row, so ONE row is bound by one
 * wave's instruction latency: 148 Msymbols/s for real rows, 70 Msymbols/s at two bits per symbol, measured; 8192 rows
 * read 1.6 TB/s, 1.8 times the time of a device copy of the same bytes.  Splitting a long row over
 * waves is not done.
 */
#ifndef HZSDR_FRAMESYNC_H
#define HZSDR_FRAMESYNC_H

#include "hzsdr.h"
#include "hzsdr_symsync.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hzsdr_framesync hzsdr_framesync;

#define HZSDR_FRAMESYNC_MAX_ROWS 8192
#define HZSDR_FRAMESYNC_MAX_WORD 64
#define HZSDR_FRAMESYNC_MAX_PAYLOAD 8192
#define HZSDR_FRAMESYNC_MAX_HYPOTHESES 4

/* hzsdr_framesync_plan's `form`: _COMPLEX: complex64 rows; _DIBIT: B = 2; _DIFF: a differential decoding */
#define HZSDR_FRAMESYNC_FORM_COMPLEX 1
#define HZSDR_FRAMESYNC_FORM_DIBIT 2
#define HZSDR_FRAMESYNC_FORM_DIFF 4

/* A bank over `rows` rows of `kind` (HZSDR_SYMSYNC_REAL_F32 or HZSDR_FMT_C64): B = bits_per_symbol, W = word_bits, the
 * mask, thr, H = hyps with the host arrays words[H] and maps[H] (free to go when this returns), P = payload_bits, diff
 * and holdoff as above.  Positions and holds are 0, the history empty.  HZSDR_ERR_FORMAT_UNKNOWN for another kind;
 * HZSDR_ERR_INVALID_ARGUMENT for anything outside the bounds above, a word or mask with bits above W, a map that B does
 * not have, rows out of range. */
int hzsdr_framesync_create(hzsdr_ctx *ctx, int kind, unsigned bits_per_symbol, unsigned word_bits, uint64_t mask, unsigned thr, unsigned hyps,
                           const uint64_t *words, const unsigned *maps, unsigned payload_bits, int diff, uint64_t holdoff, size_t rows,
                           hzsdr_framesync **out);
/* Run min(in_counts[r], n) symbols of every row through the bank.  out, positions, info and counts are in the
 * context's memory space; out takes cap frames of FB bytes per row, out_stride BYTES from one row to the next (ignored
 * when rows = 1); positions and info take rows * cap entries.  cap may be 0: the frames are counted only.
 * HZSDR_ERR_DST_TOO_SMALL when rows > 1 and out_stride is below cap * FB; HZSDR_ERR_INVALID_ARGUMENT for rows > 1 with
 * in_stride < n, n above 2^31 - 16, null in or counts with n > 0, null out, positions or info with n > 0 and cap > 0:
 * decided before anything is launched, the state is unchanged.
 * Stream-ordered on the context's stream; HOST contexts stage every array. */
int hzsdr_framesync_push(hzsdr_framesync *f, const void *in, size_t n, size_t in_stride, const uint32_t *in_counts, uint8_t *out, size_t cap,
                         size_t out_stride, uint64_t *positions, uint32_t *info, uint32_t *counts, size_t *max_count);
/* Copy the state into host arrays of rows_cap >= rows entries (history: rows * ceil(K / 8) bytes), behind every push
 * so far.  HZSDR_ERR_DST_TOO_SMALL when rows_cap is below rows. */
int hzsdr_framesync_get_state(hzsdr_framesync *f, uint64_t *positions, uint64_t *holds, uint8_t *history, uint8_t *last, size_t rows_cap);
/* Replace the state by host arrays of exactly `rows` entries.  History bits are taken as they are, pad bits ignored. */
int hzsdr_framesync_set_state(hzsdr_framesync *f, const uint64_t *positions, const uint64_t *holds, const uint8_t *history, const uint8_t *last,
                              size_t rows);
/* Symbols consumed per row since create, reset or set_state, into a host array of rows_cap >= rows entries. */
int hzsdr_framesync_positions(hzsdr_framesync *f, uint64_t *positions, size_t rows_cap);
/* The rows one wave owns (the last wave may own fewer; wave w owns rows [w * rows_per_wave, ...)), the bits of a tile,
 * the words of the history ring and the form (HZSDR_FRAMESYNC_FORM_*), so that tests can aim at edges. */
int hzsdr_framesync_plan(const hzsdr_framesync *f, size_t *rows_per_wave, size_t *tile_bits, size_t *ring_words, int *form);
/* Back to position 0 with an empty history, hold 0 and last decision 0. */
int hzsdr_framesync_reset(hzsdr_framesync *f);
int hzsdr_framesync_free(hzsdr_framesync *f);

#ifdef __cplusplus
}
#endif

#endif /* HZSDR_FRAMESYNC_H */

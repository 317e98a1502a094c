/*
 * hzsdr_hdlc.h -- the HDLC deframer bank of libhzsdr_hip: hard decisions, the flags and aborts of an HDLC bit stream, and
 * the frames between two flags with their stuffed bits deleted and their FCS checked, over one row of soft symbols or
 * over many rows at once.  It is the next member of the family of hzsdr_tuner.h, hzsdr_iir.h, hzsdr_agc.h,
 * hzsdr_carrier.h, hzsdr_symsync.h, hzsdr_equalizer.h and hzsdr_framesync.h and stands where the last of them stands,
 * for the links that one does not fit: AIS, AX.25 / APRS and every other HDLC-framed channel has no fixed length, no
 * sync word beyond the 8-bit flag 01111110, and bit stuffing inside the frame.  It takes the symbol-timing bank's
 * (symbols, counts) as they are, on the device, and this is where the data rate falls from symbols to packets.  What it
 * leaves to others: what the bytes of a frame mean (addresses, AIS message types); descrambling (G3RUH); soft outputs.
 *
 * The entries live beside hzsdr.h and the other headers (same conventions, same status codes, same context).  The
 * reference has no HDLC: the definition below is the contract, restated under tests/ (tests/host/hdlc_ref.cpp over
 * csrc/hz_hdlc_math.h bit by bit, tests/hdlc_ref.py in numpy over whole arrays, and there a textbook bit-serial decoder).
 *
 * Rows, input, decisions: the frame sync bank's, with one bit per symbol.  R rows, 1 <= R <= 8192, of kind
 * HZSDR_SYMSYNC_REAL_F32 (one float32 per symbol) or HZSDR_FMT_C64 (Re only).  Row r starts r * in_stride SYMBOLS into
 * `in`; n is the symbols a row may hold; in_counts is uint32[R] in the context's memory space, or null for "every row
 * has n"; row r consumes min(in_counts[r], n) symbols and nothing beyond.  The raw decision d[i] of the i-th symbol of a
 * row since create or reset is 1 when the float32's sign bit is clear (-0 decides 0, a NaN by its sign bit).  With
 * `diff`: 0: b[i] = d[i];  1: b[i] = d[i] ^ d[i-1];  2: b[i] = 1 ^ d[i] ^ d[i-1] (NRZI, what AIS and AX.25 send);
 * d[-1] = 0.  b[i] is the i-th bit of the row; bits before position 0 are taken as 0.
 *
 * Events.  Two kinds, each a test of the 8 bits b[i-7 ... i]: a FLAG at i when they are 0,1,1,1,1,1,1,0; an ABORT at i
 * when they are 0,1,1,1,1,1,1,1 -- the seventh 1 of a run, so a longer run gives one abort.  Two flags may share their
 * 0: their events are 7 bits apart.  At create and reset the "previous event" is an abort at -1.
 *
 * Frames.  For two consecutive events e1 < e2 that are both flags the raw span is b[e1+1 ... e2-8], empty when
 * e2 - e1 <= 8; every other pair of events yields nothing.  Inside a span bit i is stuffed when b[i] = 0 and
 * b[i-5 ... i-1] are all 1: runs inside a span never pass 5 (a sixth 1 would have ended in an event) and the bit before
 * a span is the flag's 0, so this is a local test.  The frame's bits are the span's bits with the stuffed ones deleted,
 * in order; u is their number.  The frame is well-formed when u is a multiple of 8 and min_bytes <= u / 8 <= max_bytes,
 * 1 <= min_bytes <= max_bytes <= 1024, min_bytes > fcs / 8.  A span above Lmax = 8 max_bytes + floor(8 max_bytes / 5)
 * raw bits cannot be well-formed, so the bank keeps Lmax + 8 bits of history and no more.
 * On every stream a compliant transmitter sends this is the textbook bit-serial decoder (a ones counter that drops the 0
 * behind five 1s, closes a frame at a flag and discards it at an abort).  On garbage it is simply total: every bit
 * string has exactly one list of frames, the same however it is cut.
 *
 * FCS.  `fcs` is 0, 16 or 32.  For 16 the register c starts at 0xFFFF; per frame bit in order
 * c = (c >> 1) ^ (((c ^ bit) & 1) ? 0x8408 : 0); the frame is good iff c = 0xF0B8 at the end (CRC-16/X.25 over the frame
 * including its FCS).  For 32 the same step with 0xEDB88320 from 0xFFFFFFFF, good iff c = 0xDEBB20E3.  For 0 every
 * well-formed frame is good.  keep_bad = 0: only good frames are emitted; keep_bad = 1: every well-formed frame, with
 * its verdict.
 *
 * Output of a push, for the f-th frame emitted in row r -- frames in ascending e2, f from 0 in every push, a frame
 * emitted by the push that delivers bit e2:
 *   - out: the frame's u / 8 bytes, FCS included, at out + r * out_stride + f * max_bytes BYTES; msb_first = 0 (HDLC's
 *     own order): frame bit k in byte k / 8, bit k % 8;  msb_first = 1: bit 7 - k % 8 (the order the frame sync bank
 *     packs).  Bytes of the slot from u / 8 up are left untouched;
 *   - positions[r * cap + f] = e1 + 1, uint64;   info[r * cap + f] = u / 8 | good << 31, uint32;
 *   - counts[r] is the number of frames emitted in this push, stored or not: only f < cap is stored, so a loss shows
 *     as counts[r] > cap; slots from min(counts[r], cap) up are left untouched;
 *   - *max_count, when not null, returns the largest count, and the call then waits, as hzsdr_framesync_push does.
 * Nothing is flushed: a frame still open at the end of a stream is not emitted.
 *
 * State of a row: the symbols consumed, the previous event's kind and position, the last K = Lmax + 8 bits, and
 * (diff != 0) the last raw decision.  hzsdr_hdlc_get_state / _set_state move it in the frame sync bank's conventions:
 * uint64 positions (symbols); uint64 events, the previous event's position PLUS ONE (0 at create: the abort at -1; for a
 * flag the first bit of the span behind it); one byte per row for its kind (HZSDR_HDLC_EVENT_ABORT or _FLAG);
 * ceil(K / 8) history bytes per row -- history bit k, oldest first, in byte k / 8, bit 7 - k % 8, zero where the stream
 * had not begun -- and one byte per row for the last raw decision.
 *
 * Invariance: frames, positions, info, counts and state do not depend on how the stream is cut into pushes (n = 0 and
 * rows whose count is 0 included), on the memory space, on R, on either stride, on cap (up to what is stored) or on the
 * other rows' contents.  Everything is integer arithmetic on decided bits: the kernel, the host program and the numpy
 * restatement agree exactly.
 * Speed: DESIGN.md section 4 has the measurements (tools/hdlc_time.py, profiles/hdlc_time.txt).
 */
#ifndef HZSDR_HDLC_H
#define HZSDR_HDLC_H

#include "hzsdr.h"
#include "hzsdr_symsync.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hzsdr_hdlc hzsdr_hdlc;

#define HZSDR_HDLC_MAX_ROWS 8192
#define HZSDR_HDLC_MAX_BYTES 1024

#define HZSDR_HDLC_EVENT_ABORT 0
#define HZSDR_HDLC_EVENT_FLAG 1

/* hzsdr_hdlc_plan's `form`: _COMPLEX: complex64 rows; _DIFF: a differential decoding; the FCS; the two options */
#define HZSDR_HDLC_FORM_COMPLEX 1
#define HZSDR_HDLC_FORM_DIFF 4
#define HZSDR_HDLC_FORM_FCS16 8
#define HZSDR_HDLC_FORM_FCS32 16
#define HZSDR_HDLC_FORM_MSB_FIRST 32
#define HZSDR_HDLC_FORM_KEEP_BAD 64

/* A bank over `rows` rows of `kind` (HZSDR_SYMSYNC_REAL_F32 or HZSDR_FMT_C64) with diff, fcs, min_bytes, max_bytes,
 * msb_first and keep_bad as above.  Positions are 0, the history empty, the previous event an abort at -1.
 * HZSDR_ERR_FORMAT_UNKNOWN for another kind; HZSDR_ERR_INVALID_ARGUMENT for anything outside the bounds above, rows out
 * of range. */
int hzsdr_hdlc_create(hzsdr_ctx *ctx, int kind, int diff, unsigned fcs, unsigned min_bytes, unsigned max_bytes, int msb_first, int keep_bad, size_t rows,
                      hzsdr_hdlc **out);
/* Run min(in_counts[r], n) symbols of every row through the bank.  out, positions, info and counts are in the
 * context's memory space; out takes cap slots of max_bytes bytes per row, out_stride BYTES from one row to the next
 * (ignored when rows = 1); positions and info take rows * cap entries.  cap may be 0: the frames are counted only.
 * HZSDR_ERR_DST_TOO_SMALL when rows > 1 and out_stride is below cap * max_bytes; HZSDR_ERR_INVALID_ARGUMENT for rows > 1
 * with in_stride < n, n above 2^31 - 16, null in or counts with n > 0, null out, positions or info with n > 0 and
 * cap > 0: decided before anything is launched, the state is unchanged.
 * Stream-ordered on the context's stream; HOST contexts stage every array. */
int hzsdr_hdlc_push(hzsdr_hdlc *f, const void *in, size_t n, size_t in_stride, const uint32_t *in_counts, uint8_t *out, size_t cap, size_t out_stride,
                    uint64_t *positions, uint32_t *info, uint32_t *counts, size_t *max_count);
/* Copy the state into host arrays of rows_cap >= rows entries (history: rows * ceil(K / 8) bytes), behind every push
 * so far.  HZSDR_ERR_DST_TOO_SMALL when rows_cap is below rows. */
int hzsdr_hdlc_get_state(hzsdr_hdlc *f, uint64_t *positions, uint64_t *events, uint8_t *kinds, uint8_t *history, uint8_t *last, size_t rows_cap);
/* Replace the state by host arrays of exactly `rows` entries.  History bits are taken as they are, pad bits ignored.
 * HZSDR_ERR_INVALID_ARGUMENT for a position above 2^62, an event above its row's position, a kind or last above 1. */
int hzsdr_hdlc_set_state(hzsdr_hdlc *f, const uint64_t *positions, const uint64_t *events, const uint8_t *kinds, const uint8_t *history,
                         const uint8_t *last, size_t rows);
/* Symbols consumed per row since create, reset or set_state, into a host array of rows_cap >= rows entries. */
int hzsdr_hdlc_positions(hzsdr_hdlc *f, uint64_t *positions, size_t rows_cap);
/* The rows one wave owns, the bits of a tile, the words of the history ring and the form (HZSDR_HDLC_FORM_*), so that
 * tests can aim at edges.  The tiles whose loads travel together (the chunk) are 16. */
int hzsdr_hdlc_plan(const hzsdr_hdlc *f, size_t *rows_per_wave, size_t *tile_bits, size_t *ring_words, int *form);
/* Back to position 0 with an empty history, the previous event an abort at -1 and last decision 0. */
int hzsdr_hdlc_reset(hzsdr_hdlc *f);
int hzsdr_hdlc_free(hzsdr_hdlc *f);

#ifdef __cplusplus
}
#endif

#endif /* HZSDR_HDLC_H */

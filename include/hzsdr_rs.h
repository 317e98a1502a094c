/*
 * hzsdr_rs.h -- the Reed-Solomon decoder bank of libhzsdr_hip: frames of interleaved Reed-Solomon codewords over GF(2^8)
 * to corrected data bytes and a verdict per frame, over many rows of frames at once.  It is the next member of the family
 * of hzsdr_tuner.h, hzsdr_iir.h, hzsdr_agc.h, hzsdr_carrier.h, hzsdr_symsync.h, hzsdr_framesync.h and hzsdr_viterbi.h and
 * stands behind the last of them: it takes the Viterbi bank's `out` block (or, for links without an inner code, the frame
 * sync bank's) and the device-side `counts` as they are, with no host read in between, and does what concatenated links
 * (CCSDS telemetry, DVB-S, most amateur satellite downlinks) put behind the inner code: the pseudo-randomiser, the
 * symbol-interleaved Reed-Solomon outer code and the dual-basis symbol map.  What it leaves to others: erasure decoding;
 * soft decisions; encoding on the device; symbol sizes other than 8 bits; block or convolutional (Forney) interleavers
 * across frames.
 *
 * The entries live beside hzsdr.h and the other headers (same conventions, same status codes, same context).  The
 * reference has no decoder: the definition below is the contract.  It names no algorithm, so the kernel, a host
 * restatement (tests/host/rs_ref.cpp over csrc/hz_rs_math.h), a numpy restatement written independently
 * (tests/rs_ref.py: a linear solve for the error values) and an exhaustive nearest-codeword search agree exactly.
 *
 * Field.  GF(2^8) by a 9-bit field polynomial `gfpoly` with bit 8 set, primitive (0x187: CCSDS; 0x11D: DVB and most
 * others).  alpha is the element 0x02.
 *
 * Code.  n symbols per codeword, `nroots` parity symbols, 2 <= nroots <= 64, nroots < n <= 255; k = n - nroots data
 * symbols, t = floor(nroots / 2) (an odd nroots is allowed).  The first root index `fcr` is below 255; the root spacing
 * `prim` has 1 <= prim <= 254 and gcd(prim, 255) = 1.  Symbol p of a codeword, p = 0 the first, is the coefficient of
 * x^(n-1-p); a word c is a codeword iff c(alpha^(prim (fcr + j))) = 0 for j = 0 ... nroots - 1.  Codewords are
 * systematic: k data symbols first, then nroots parity symbols.  A shortened code is just n < 255: no padding is stored
 * anywhere.  CCSDS: (0x187, fcr 112, prim 11, nroots 32 or 16, n 255); DVB: (0x11D, 0, 1, 16, 204).
 *
 * Frame.  `interleave` I = 1 ... 8.  A frame is F = I n bytes; codeword i owns the frame bytes i, i + I, i + 2 I, ...
 * (CCSDS symbol interleaving).
 *
 * Per-byte preparation, for frame byte m, in this order:  b ^= scramble[m mod scramble_len] (scramble_len 0: none,
 * otherwise 1 ... 2040, a host array given at create);  v = in_map[b] (a 256-byte host table, or null for identity).
 *
 * Decision per codeword (bounded distance).  If a codeword exists that differs from the received word v in at most t of
 * its n positions, it is unique: it is the result, and e is the number of positions changed.  Otherwise the codeword
 * FAILS and its symbols pass through unchanged.  Nothing here names Berlekamp-Massey, Chien or Forney: any correct
 * errors-only decoder realises it, one that also fails where the locator has a degree above t, fewer distinct roots
 * among the n valid positions than its degree, or a root in the shortened region.
 *
 * Output of a call, for frame f < min(in_counts[r], cap) of row r:  the first I k bytes of the corrected frame, in frame
 * order, each as out_map[v] (null: identity), at out + r * out_stride + f * out_pitch;  info[r * cap + f] =
 * E | nfail << 16 | ok << 31 with E the sum of e over the frame's decoded codewords, nfail the number of failed
 * codewords and ok = (nfail == 0), in the bit where the Viterbi bank puts crc_ok.  Slots from a row's count up, and the
 * bytes behind I k inside a slot, are left untouched.  `out` may equal `in` with equal strides and pitches (in place);
 * otherwise the two must not overlap.  The bank keeps NO state between calls.
 *
 * Input.  Frame f of row r is at in + r * in_stride + f * in_pitch bytes, in_pitch >= F: the Viterbi bank's DB and the
 * frame sync bank's FB both fit.  in_counts is uint32[R] in the context's memory space, or null for "every row has
 * cap"; values above cap are clamped.  rows is 1 ... 8192 and rows * cap at most 2^22.
 *
 * Invariance: a frame's bytes and info do not depend on R, on strides, pitches, cap or the frame's slot, on the memory
 * space, on in place or not, on the grouping into waves or on any other frame's contents.
 *
 * Speed: one workgroup of I waves decodes a frame, wave i codeword i, lane j syndrome j.  ONE CCSDS 255/223 codeword
 * takes 24.8 us clean, 47.1 us with 8 and 57.7 us with 16 errors, measured: one wave's dependent chain, 255 Horner
 * steps of two dependent LDS reads each and then the 32 Berlekamp-Massey iterations.  65536 such codewords take 284 us
 * clean, 412 Gbit/s of data, measured -- not memory (0.11 TB/s moved) but the syndrome loop of the waves a compute unit
 * holds, three byte reads from LDS per symbol and wave; 929 us with 8 errors each (126 Gbit/s) and 1329 us with 16
 * (88 Gbit/s), measured: the instruction issue of the field multiplies of Berlekamp-Massey, Chien and Forney.  Four
 * codewords interleaved run at the same rates (273, 925, 1325 us per 65536 codewords), measured.  The Viterbi bank in
 * front delivers 10.7 Gbit/s at K = 7 (hzsdr_viterbi.h): this bank is never the slower of the two (DESIGN.md section 4,
 * profiles/rs_time.txt).
 */
#ifndef HZSDR_RS_H
#define HZSDR_RS_H

#include "hzsdr.h"
#include "hzsdr_viterbi.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hzsdr_rs hzsdr_rs;

#define HZSDR_RS_MAX_ROWS 8192
#define HZSDR_RS_MIN_ROOTS 2
#define HZSDR_RS_MAX_ROOTS 64
#define HZSDR_RS_MAX_N 255
#define HZSDR_RS_MAX_INTERLEAVE 8
#define HZSDR_RS_MAX_SCRAMBLE 2040
#define HZSDR_RS_MAX_FRAMES 4194304

/* A bank over `rows` rows of frames.  in_map and out_map are host tables of 256 bytes or null; scramble is a host array
 * of scramble_len bytes (null with scramble_len 0); all three are free to go when this returns.
 * HZSDR_ERR_INVALID_ARGUMENT for anything outside the bounds above: a gfpoly without bit 8, with bits above it or not
 * primitive, nroots out of 2 ... 64, n out of nroots + 1 ... 255, fcr above 254, prim out of 1 ... 254 or sharing a factor
 * with 255, interleave out of 1 ... 8, scramble_len above 2040 or not zero with a null scramble, rows out of 1 ... 8192. */
int hzsdr_rs_create(hzsdr_ctx *ctx, unsigned gfpoly, unsigned fcr, unsigned prim, unsigned nroots, unsigned n, unsigned interleave,
                    const uint8_t *in_map, const uint8_t *out_map, const uint8_t *scramble, size_t scramble_len, size_t rows, hzsdr_rs **out);
/* Decode min(in_counts[r], cap) frames of every row.  in, in_counts, out and info are in the context's memory space;
 * strides and pitches are in bytes, the strides ignored when rows = 1; info takes rows * cap entries.
 * HZSDR_ERR_DST_TOO_SMALL when rows > 1 and out_stride is below cap * out_pitch; HZSDR_ERR_INVALID_ARGUMENT for cap = 0,
 * rows * cap above 2^22, null in, out or info, in_pitch below F, out_pitch below I k, rows > 1 with in_stride below
 * cap * in_pitch, out = in with other strides or pitches, and in and out overlapping in part: decided before anything is
 * launched, nothing is written.  Stream-ordered on the context's stream; HOST contexts stage every array (rows go up
 * before they come back, so that untouched bytes stay). */
int hzsdr_rs_decode(hzsdr_rs *rs, const uint8_t *in, size_t in_stride, size_t in_pitch, const uint32_t *in_counts, size_t cap, uint8_t *out,
                    size_t out_stride, size_t out_pitch, uint32_t *info);
/* k data symbols and t correctable symbols per codeword, F = I n frame bytes and I k data bytes (null: not wanted). */
int hzsdr_rs_sizes(const hzsdr_rs *rs, size_t *k, size_t *t, size_t *frame_bytes, size_t *data_bytes);
/* The waves of a workgroup (I: one per codeword of a frame), its LDS request in bytes, the workgroups a compute unit
 * holds at once (32 / I: the wave slots, not the LDS, set it) and the grid's size at most, so that tests can aim at edges. */
int hzsdr_rs_plan(const hzsdr_rs *rs, size_t *waves_per_group, size_t *lds_bytes, size_t *groups_per_cu, size_t *max_groups);
int hzsdr_rs_free(hzsdr_rs *rs);

#ifdef __cplusplus
}
#endif

#endif /* HZSDR_RS_H */

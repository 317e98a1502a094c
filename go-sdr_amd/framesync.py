"""The frame sync bank (include/hzsdr_framesync.h): hard decisions, a sync-word search and the frames' payload bits out
of one row of soft symbols, or out of many rows, real or complex.

    words, maps = hz.sync_hypotheses(0x1ACFFC1D, 32, 2, "rotate")       # what a Costas loop leaves open: four rotations
    fs = ctx.frame_sync(hz.FMT_C64, 32, words, maps, payload_bits=168, bits_per_symbol=2, thr=2, rows=100)
    frames, positions, info, counts = fs.push(*ts.push(cr.push(rows)))  # the symbol-timing bank's (symbols, counts) as they are
    for payloads, starts, dist_h in fs.ragged(frames, positions, info, counts): ...   # host arrays, one triple per row

A float decides 1 when its sign bit is clear.  A window of W bits is a candidate when its distance to the nearest of
up to four words, under the mask, is at most thr; candidates are taken in ascending order and accepted outside the
hold-off of the one before; an accepted one yields P payload bits through its hypothesis's map (B = 1: identity or
inverted; B = 2: the four rotations), packed most significant bit first.  A frame is emitted by the push that delivers
its last bit.  Positions, the hold-off and the last W + P - 1 bits carry from push to push, per row, so frames,
positions, info, counts and state do not depend on how the stream is cut, on the memory space, on the number of rows, on
either pitch or on the other rows.  counts[r] above `cap` says that row r lost frames in this push.

Not here: decoding a convolutionally coded payload and its CRC (include/hzsdr_viterbi.h, Context.viterbi: it takes
frames and counts as push returns them); bit unstuffing (include/hzsdr_hdlc.h, Context.hdlc: the bank that stands here
on HDLC-framed links); descrambling; soft outputs (include/hzsdr_softframe.h,
Context.soft_frames: the bank beside this one, it takes positions, info and counts as push returns them); sync words
above 64 bits.
"""
import ctypes as C

import numpy as np

from . import ErrInvalidArgument, FMT_C64, _is_torch, lib
from ._frames import BitRingBank
from ._capi import (FRAMESYNC_FORM_COMPLEX, FRAMESYNC_FORM_DIBIT, FRAMESYNC_FORM_DIFF, FRAMESYNC_MAX_HYPOTHESES, FRAMESYNC_MAX_PAYLOAD,
                    FRAMESYNC_MAX_ROWS, FRAMESYNC_MAX_WORD)

_PU64, _PU8 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)


def pack_bits(bits):
    """bits (..., P) of 0 / 1 -> uint8 (..., ceil(P / 8)): bit k in byte k / 8, bit 7 - k % 8, pad bits 0"""
    return np.packbits(np.asarray(bits, np.uint8), axis=-1)


def unpack_bits(frames, count):
    """uint8 (..., FB) -> the first `count` bits (..., count) of 0 / 1"""
    return np.unpackbits(np.asarray(frames, np.uint8), axis=-1)[..., :int(count)]


def _map_dibits(word, bits, q):
    """every dibit (b0, b1) of the `bits`-bit word, b0 the more significant, through q times (b0, b1) -> (b1, !b0)"""
    out = 0
    for k in range(bits - 2, -1, -2):
        b0, b1 = (word >> (k + 1)) & 1, (word >> k) & 1
        for _ in range(q % 4):
            b0, b1 = b1, b0 ^ 1
        out |= (b0 << (k + 1)) | (b1 << k)
    return out


def sync_hypotheses(word, word_bits, bits_per_symbol=1, ambiguity="none"):
    """(words, maps) for the sync word `word` (the first-received bit the most significant of its word_bits bits) under
    what the carrier recovery leaves open: "none" (one hypothesis), "invert" (B = 1: the word and its complement, the
    payload of the second inverted back) or "rotate" (B = 2: words[q] is the word under the inverse of map q, so that a
    stream received as x * i^q hits with h = q and its payload comes out as sent)."""
    word, W, B = int(word), int(word_bits), int(bits_per_symbol)
    if not (1 <= W <= FRAMESYNC_MAX_WORD and 0 <= word < (1 << W)) or B not in (1, 2) or W % B:
        raise ValueError("sync_hypotheses: a word of 1 ... 64 bits, a multiple of the bits per symbol")
    if ambiguity == "none":
        return [word], [0]
    if ambiguity == "invert" and B == 1:
        return [word, word ^ ((1 << W) - 1)], [0, 1]
    if ambiguity == "rotate" and B == 2:
        return [_map_dibits(word, W, (4 - q) % 4) for q in range(4)], [0, 1, 2, 3]
    raise ValueError('sync_hypotheses: ambiguity is "none", "invert" (1 bit per symbol) or "rotate" (2 bits per symbol)')


class FrameSync(BitRingBank):
    """hzsdr_framesync: push(symbols, counts) -> (frames, positions, info, counts).  `kind` is SYMSYNC_REAL_F32 (float32
    rows) or FMT_C64 (complex64 rows, bits_per_symbol 1 -- Re only -- or 2).  One row takes (n,) symbols; `rows` = R > 1
    takes (R, n) with unit stride along a row and any row pitch.  `words` and `maps` are the hypotheses (sync_hypotheses
    builds them); `mask` defaults to all word_bits bits, `holdoff` to one frame's symbols.  numpy in a HOST context; torch
    tensors on the context's device, written on the context's stream, in a DEVICE context (positions are int64, info and
    counts int32 there: the same bits as the ABI's unsigned types)."""
    _c, _noun, _extent = "framesync", "frame sync", "FB"

    def __init__(self, ctx, kind, word_bits, words, maps, payload_bits, bits_per_symbol=1, mask=None, thr=0, diff=0, holdoff=None, rows=1):
        self._open(ctx, kind, rows)
        self.W, self.P, self.B = int(word_bits), int(payload_bits), int(bits_per_symbol)
        words, maps = [int(w) for w in np.atleast_1d(words)], [int(m) for m in np.atleast_1d(maps)]
        if len(words) != len(maps) or not 1 <= len(words) <= FRAMESYNC_MAX_HYPOTHESES:
            raise ErrInvalidArgument("frame sync: 1 ... 4 hypotheses, a map for every word")
        if min(words + maps + [self.W, self.P, self.B, int(thr), int(diff)]) < 0 or max(words) >= 1 << 64:
            raise ErrInvalidArgument("frame sync: words, maps, sizes, thr and diff are not negative")
        self.words, self.maps, self.thr, self.diff = words, maps, int(thr), int(diff)
        self.mask = ((1 << self.W) - 1 if 0 < self.W <= 64 else 0) if mask is None else int(mask)
        self.holdoff = max(1, (self.W + self.P) // max(self.B, 1)) if holdoff is None else int(holdoff)
        if not (0 <= self.mask < 1 << 64 and 0 <= self.holdoff < 1 << 64):
            raise ErrInvalidArgument("frame sync: mask and holdoff are uint64 values")
        self.frame_bytes, self.history_bytes = (self.P + 7) // 8, (self.W + self.P - 1 + 7) // 8
        w, m = (C.c_uint64 * len(words))(*words), (C.c_uint * len(maps))(*maps)
        ctx._ck(lib.hzsdr_framesync_create(ctx._h, self.kind, self.B, self.W, self.mask, self.thr, len(words), w, m, self.P, self.diff, self.holdoff,
                                           self.rows, C.byref(self._h)))

    def plan(self):
        """(rows per wave, bits per tile, words of the history ring, form): the form is a sum of FRAMESYNC_FORM_COMPLEX,
        FRAMESYNC_FORM_DIBIT and FRAMESYNC_FORM_DIFF."""
        return self._plan()

    def push(self, symbols, counts=None, cap=4, out=None):
        """Run the symbols of every row through the bank -> (frames, positions, info, counts).  `counts`, when given, is
        what SymbolSync.push returned beside the symbols: row r consumes min(counts[r], n) of its n symbols; without it
        every row consumes n.  frames is uint8 (rows, cap, FB), positions (rows, cap) the payloads' first symbols, info
        (rows, cap) dist | h << 8, counts (rows,) the frames accepted in this push: above cap where a row lost some.
        Slots from a row's count up hold what the destination held (a new one is zero).  `out`, when given, is such a
        tuple (frames, positions, info, counts) to write into; frames may be a view with a row pitch above cap * FB."""
        return self._push(symbols, counts, cap, out)

    def ragged(self, frames, positions, info, counts):
        """A push's results -> a list of `rows` host triples (frames (k, FB), positions (k,) uint64, info (k,) uint32),
        k = min(counts[r], cap) (this waits for the device in a DEVICE context)."""
        if _is_torch(frames):
            frames, positions, info, counts = (t.cpu().numpy() for t in (frames, positions, info, counts))
        cap = frames.shape[1]
        out = []
        for r, c in enumerate(np.asarray(counts).reshape(-1).view(np.uint32)):
            k = min(int(c), cap)
            out.append((frames[r, :k].copy(), positions[r, :k].copy().view(np.uint64), info[r, :k].copy().view(np.uint32)))
        return out

    def state(self):
        """(positions uint64 (rows,), holds uint64 (rows,), history uint8 (rows, ceil(K / 8)), last uint8 (rows,)):
        the symbols consumed, the hold-offs in symbols, the last K = W + P - 1 bits oldest first and most significant bit
        first, the last raw decisions; behind every push so far."""
        R = self.rows
        p, h, y, d = np.empty(R, np.uint64), np.empty(R, np.uint64), np.empty((R, self.history_bytes), np.uint8), np.empty(R, np.uint8)
        self.ctx._ck(lib.hzsdr_framesync_get_state(self._h, p.ctypes.data_as(_PU64), h.ctypes.data_as(_PU64), y.ctypes.data_as(_PU8),
                                                   d.ctypes.data_as(_PU8), R))
        return p, h, y, d

    def set_state(self, positions, holds, history, last):
        R = self.rows
        p, h = np.ascontiguousarray(positions, np.uint64), np.ascontiguousarray(holds, np.uint64)
        y, d = np.ascontiguousarray(history, np.uint8), np.ascontiguousarray(last, np.uint8)
        if p.shape != (R,) or h.shape != (R,) or y.shape != (R, self.history_bytes) or d.shape != (R,):
            raise ErrInvalidArgument("frame sync: the state is positions (rows,), holds (rows,), history (rows, ceil(K / 8)), last (rows,)")
        self.ctx._ck(lib.hzsdr_framesync_set_state(self._h, p.ctypes.data_as(_PU64), h.ctypes.data_as(_PU64), y.ctypes.data_as(_PU8),
                                                   d.ctypes.data_as(_PU8), R))


__all__ = ["FrameSync", "sync_hypotheses", "pack_bits", "unpack_bits", "FRAMESYNC_FORM_COMPLEX", "FRAMESYNC_FORM_DIBIT", "FRAMESYNC_FORM_DIFF",
           "FRAMESYNC_MAX_ROWS", "FRAMESYNC_MAX_WORD", "FRAMESYNC_MAX_PAYLOAD", "FRAMESYNC_MAX_HYPOTHESES"]

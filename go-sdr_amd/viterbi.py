"""The Viterbi decoder bank (include/hzsdr_viterbi.h): convolutionally coded frames -- the frame sync bank's packed
payload bits, or soft float32 values -- to data bits, a path metric and an optional CRC verdict per frame.

    K, gens, inv = hz.CCSDS_K7
    vd = ctx.viterbi(hz.VITERBI_BITS, K, gens, data_bits=78, inv=inv, crc=(16, 0x1021, 0xFFFF, 0), rows=100)
    frames, positions, sync, counts = fs.push(symbols, symbol_counts, cap=4)   # the frame sync bank, on the device
    data, info = vd.decode(frames, counts)        # data (rows, cap, DB) uint8; info = metric | crc_ok << 31

The code is rate 1/n (n = 2, 3, 4) with constraint length K = 3 ... 9, generators whose most significant bit multiplies
the newest input bit, an inversion mask and a puncture pattern; TAIL frames end in K - 1 zero bits, TRUNCATED ones do
not.  Soft values are quantised to -127 ... 127 by q = rint(clamp(x * scale)), a NaN is an erasure; hard bits are +-1,
so that the metric of a hard frame is the number of channel bit errors corrected.  Row r decodes min(counts[r], cap)
frames; the other slots of the destinations stay as they are.  Frames are independent and the bank keeps no state.

Not here: tail-biting, one continuous stream across frames, soft outputs of the decoder, bit unstuffing; descrambling and
the outer Reed-Solomon code are the next bank's (include/hzsdr_rs.h, Context.reed_solomon: it takes data and counts as
they are).  The VITERBI_SOFT_F32 frames are what the soft frame bank writes (include/hzsdr_softframe.h,
Context.soft_frames).
"""
import ctypes as C

import numpy as np

from . import ErrInvalidArgument
from ._frames import DecoderBank
from ._capi import (VITERBI_BITS, VITERBI_FORM_LDS, VITERBI_FORM_SCRATCH, VITERBI_MAX_BITS, VITERBI_MAX_FRAMES, VITERBI_MAX_K, VITERBI_MAX_PATTERN,
                    VITERBI_MAX_RATE, VITERBI_MAX_ROWS, VITERBI_MIN_K, VITERBI_SOFT_F32, VITERBI_TAIL, VITERBI_TRUNCATED)

CCSDS_K7 = (7, (0o171, 0o133), 0b10)  # (K, generators, inv): the second output inverted

_PATTERNS = {"1/2": "11", "2/3": "1101", "3/4": "110110", "5/6": "1101100110", "7/8": "11010101100110"}


def puncture_pattern(rate):
    """(pattern, pattern_bits) of the usual punctured rates of the K = 7 rate 1/2 code (DVB-S): "1/2", "2/3", "3/4",
    "5/6", "7/8"; the pattern's first bit is its most significant"""
    try:
        s = _PATTERNS[rate]
    except KeyError:
        raise ValueError('puncture_pattern: the rate is "1/2", "2/3", "3/4", "5/6" or "7/8"') from None
    return int(s, 2), len(s)


def _pattern(pattern, n):
    if pattern is None:
        return (1 << n) - 1, n
    if isinstance(pattern, str):
        return puncture_pattern(pattern)
    p, bits = pattern
    return int(p), int(bits)


def conv_encode(bits, K, gens, inv=0, pattern=None, termination=VITERBI_TAIL):
    """The encoder of the definition, in numpy: data bits (D,) of 0 / 1 -> the N transmitted code bits (uint8).
    `pattern` is None (no puncturing), a rate name of puncture_pattern, or (pattern, pattern_bits)."""
    u = np.asarray(bits, np.uint8).reshape(-1) & 1
    n = len(gens)
    pat, lp = _pattern(pattern, n)
    if termination == VITERBI_TAIL:
        u = np.concatenate([u, np.zeros(K - 1, np.uint8)])
    out, state = [], 0
    for t, b in enumerate(u):
        reg = (int(b) << (K - 1)) | state
        for j, g in enumerate(gens):
            if (pat >> (lp - 1 - (t * n + j) % lp)) & 1:
                out.append((bin(reg & int(g)).count("1") & 1) ^ ((inv >> j) & 1))
        state = reg >> 1
    return np.array(out, np.uint8)


def crc_register(bits, C, poly, init=0, xorout=0):
    """The CRC register of the definition over `bits` in stream order: no reflection, the first bit first"""
    reg, mask = int(init), (1 << C) - 1
    for b in np.asarray(bits, np.uint8).reshape(-1):
        top = ((reg >> (C - 1)) & 1) ^ (int(b) & 1)
        reg = (reg << 1) & mask
        if top:
            reg ^= int(poly)
    return reg ^ int(xorout)


class ViterbiDecoder(DecoderBank):
    """hzsdr_viterbi: decode(frames, counts) -> (data, info).  `kind` is VITERBI_BITS (uint8 frames of FB = ceil(N / 8)
    bytes, most significant bit first: FrameSync.push's frames) or VITERBI_SOFT_F32 (float32 frames of N values, positive
    meaning 1).  frames is (rows, cap, FB or N) -- (cap, ...) will do for one row -- with contiguous rows and any row
    pitch.  `crc` is None or (bits, poly, init, xorout).  numpy in a HOST context; torch tensors on the context's device,
    written on the context's stream, in a DEVICE context (info and counts are int32 there: the same bits)."""
    _c = _noun = "viterbi"
    _bits = VITERBI_BITS

    def __init__(self, ctx, kind, K, gens, data_bits, inv=0, pattern=None, termination=VITERBI_TAIL, scale=1.0, crc=None, rows=1):
        self.kind = int(kind)
        self._open(ctx, rows)
        gens = [int(g) for g in gens]
        self.K, self.gens, self.n, self.inv, self.D = int(K), gens, len(gens), int(inv), int(data_bits)
        self.pattern, self.pattern_bits = _pattern(pattern, self.n)
        self.termination, self.scale = int(termination), float(scale)
        self.crc = (0, 0, 0, 0) if crc is None else tuple(int(v) for v in crc)
        values = gens + [self.K, self.inv, self.D, self.pattern, self.pattern_bits, *self.crc]
        if not 1 <= self.n <= 8 or len(self.crc) != 4 or min(values) < 0 or max(gens + [self.K, self.inv, self.pattern_bits, *self.crc]) >= 1 << 32 or \
                self.pattern >= 1 << 64 or self.D >= 1 << 62:
            raise ErrInvalidArgument("viterbi: generators, sizes, the pattern and the CRC are unsigned values of their widths")
        g = (C.c_uint * self.n)(*gens)
        self._create(self.kind, self.K, self.n, g, self.inv, self.pattern, self.pattern_bits, self.termination, self.D, self.scale, *self.crc)
        self.N, self.frame_bytes, self.T, self.data_bytes = self.sizes()

    def sizes(self):
        """(N received positions, FB = ceil(N / 8), T trellis steps, DB = ceil(D / 8)) of a frame"""
        return self._sizes("sizes", 4)

    def plan(self):
        """(frames per wave, states per lane, bytes of a frame's decisions, VITERBI_FORM_LDS or VITERBI_FORM_SCRATCH)"""
        return self._plan()

    def decode(self, frames, counts=None, cap=None, out=None):
        """Decode min(counts[r], cap) frames of every row -> (data uint8 (rows, cap, DB), info (rows, cap) =
        metric | crc_ok << 31).  `counts`, when given, is what FrameSync.push returned beside the frames (values above
        cap are clamped); without it every row decodes cap frames.  `cap` defaults to the frames' second-last extent.
        Slots from a row's count up hold what the destination held (a new one is zero).  `out`, when given, is such a
        pair (data, info); data may be a view with a row pitch above cap * DB."""
        return self._decode(frames, counts, cap, out)

    def ragged(self, data, info, counts=None):
        """A call's results -> a list of `rows` host triples (data (k, DB), metric (k,) uint32, crc_ok (k,) bool),
        k = min(counts[r], cap) (this waits for the device in a DEVICE context)."""
        return self._ragged(data, info, counts)

    @staticmethod
    def _fields(w):
        return w & np.uint32(0x7FFFFFFF), (w >> np.uint32(31)).astype(bool)


__all__ = ["ViterbiDecoder", "conv_encode", "puncture_pattern", "crc_register", "CCSDS_K7", "VITERBI_BITS", "VITERBI_SOFT_F32", "VITERBI_TAIL",
           "VITERBI_TRUNCATED", "VITERBI_FORM_LDS", "VITERBI_FORM_SCRATCH", "VITERBI_MAX_ROWS", "VITERBI_MIN_K", "VITERBI_MAX_K", "VITERBI_MAX_RATE",
           "VITERBI_MAX_PATTERN", "VITERBI_MAX_BITS", "VITERBI_MAX_FRAMES"]

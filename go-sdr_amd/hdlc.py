"""The HDLC deframer bank (include/hzsdr_hdlc.h): hard decisions, flags, bit unstuffing and the FCS check, out of one row
of soft symbols or out of many rows, real or complex (Re only) -- AIS, AX.25 / APRS and every other HDLC-framed link.

    hd = ctx.hdlc(hz.SYMSYNC_REAL_F32, diff=2, fcs=16, min_bytes=3, max_bytes=64, rows=25)     # 25 AIS channels, NRZI
    frames, positions, info, counts = hd.push(*ts.push(rows))    # the symbol-timing bank's (symbols, counts) as they are
    for packets, starts, good in hd.ragged(frames, positions, info, counts): ...   # host lists, one triple per row

A float decides 1 when its sign bit is clear; `diff` is the frame sync bank's (2: NRZI).  A flag is 01111110, an abort
0 and seven 1s; between two consecutive flags the 0 behind five 1s is deleted, and what is left is a frame when it is a
whole number of bytes within [min_bytes, max_bytes].  The FCS (0: none, 16: CRC-16/X.25, 32: CRC-32) runs over the frame
including its FCS bytes, which stay in the frame; keep_bad = True also emits the frames that fail it, marked.  Bytes are
packed least significant bit first, HDLC's own order, unless msb_first.  Positions, the previous event and the last
Lmax + 8 bits carry from push to push, per row, so frames, positions, info, counts and state do not depend on how the
stream is cut, on the memory space, on the number of rows, on either pitch or on the other rows.  counts[r] above `cap`
says that row r lost frames in this push.

hdlc_encode makes such streams; hdlc_fcs16 / hdlc_fcs32 are the two checks over bytes.
"""
import ctypes as C

import numpy as np

from . import ErrInvalidArgument, _is_torch, lib
from ._frames import BitRingBank
from ._capi import (HDLC_EVENT_ABORT, HDLC_EVENT_FLAG, HDLC_FORM_COMPLEX, HDLC_FORM_DIFF, HDLC_FORM_FCS16, HDLC_FORM_FCS32, HDLC_FORM_KEEP_BAD,
                    HDLC_FORM_MSB_FIRST, HDLC_MAX_BYTES, HDLC_MAX_ROWS)

_PU64, _PU8 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
_FLAG = np.array([0, 1, 1, 1, 1, 1, 1, 0], np.uint8)


def _crc(data, poly, init):
    c = init
    for byte in bytes(data):
        c ^= byte
        for _ in range(8):
            c = (c >> 1) ^ (poly if c & 1 else 0)
    return c


def hdlc_fcs16(data):
    """CRC-16/X.25 of the bytes, as HDLC sends it behind them least significant byte first: hdlc_fcs16(b"123456789") == 0x906E"""
    return _crc(data, 0x8408, 0xFFFF) ^ 0xFFFF


def hdlc_fcs32(data):
    """CRC-32 of the bytes, sent least significant byte first: hdlc_fcs32(b"123456789") == 0xCBF43926"""
    return _crc(data, 0xEDB88320, 0xFFFFFFFF) ^ 0xFFFFFFFF


def _stuff(bits):
    out, ones = [], 0
    for b in bits:
        out.append(int(b))
        ones = ones + 1 if b else 0
        if ones == 5:
            out.append(0)
            ones = 0
    return out


def hdlc_encode(frames, fcs=16, flags=1, shared_zero=False, diff=0, msb_first=False):
    """frames (a list of bytes objects, the FCS NOT included) -> the raw decisions d (uint8 of 0 / 1) of a stream that
    holds them: `flags` flags, then per frame its bits with the FCS behind them (fcs 16 or 32; 0: none), stuffed, and
    `flags` flags again.  With shared_zero consecutive flags share their 0 (0111111 0111111 0).  A byte's bits go out
    least significant first, or most significant first with msb_first; the FCS runs over the bits in the order sent and
    goes out as HDLC sends it (the register's complement, its bit 0 first), so with msb_first the bank's FCS bytes are
    those of hdlc_fcs16 / hdlc_fcs32 over the bit-reversed bytes, bit-reversed.  `diff` is the bank's: 0: d is the bits;
    1: d[i] = b[i] ^ d[i-1];  2: NRZI, d[i] = 1 ^ b[i] ^ d[i-1];  d[-1] = 0.  A soft symbol of d is 2 d - 1."""
    fcs, flags, diff = int(fcs), int(flags), int(diff)
    if fcs not in (0, 16, 32) or flags < 1 or diff not in (0, 1, 2):
        raise ValueError("hdlc_encode: fcs is 0, 16 or 32, flags at least 1, diff 0, 1 or 2")

    def idle():
        if not shared_zero:
            return list(_FLAG) * flags
        return [0, 1, 1, 1, 1, 1, 1] * flags + [0]
    line = idle()
    for frame in frames:
        bits = np.unpackbits(np.frombuffer(bytes(frame), np.uint8), bitorder="big" if msb_first else "little").tolist()
        if fcs:
            c = (1 << fcs) - 1
            poly = 0x8408 if fcs == 16 else 0xEDB88320
            for b in bits:
                c = (c >> 1) ^ (poly if (c ^ b) & 1 else 0)
            c ^= (1 << fcs) - 1
            bits = bits + [(c >> k) & 1 for k in range(fcs)]
        line += _stuff(bits) + idle()
    return hdlc_line(np.array(line, np.uint8), diff)


def hdlc_line(bits, diff=0):
    """the bits b of a stream -> the raw decisions d that a bank with `diff` turns back into b (d[-1] = 0)"""
    b = np.asarray(bits, np.uint8) & 1
    if diff == 0:
        return b.copy()
    return (np.cumsum(b ^ 1 if diff == 2 else b) & 1).astype(np.uint8)


class Hdlc(BitRingBank):
    """hzsdr_hdlc: push(symbols, counts) -> (frames, positions, info, counts).  `kind` is SYMSYNC_REAL_F32 (float32 rows)
    or FMT_C64 (complex64 rows, Re only).  One row takes (n,) symbols; `rows` = R > 1 takes (R, n) with unit stride along
    a row and any row pitch.  numpy in a HOST context; torch tensors on the context's device, written on the context's
    stream, in a DEVICE context (positions are int64, info and counts int32 there: the same bits as the ABI's unsigned
    types)."""
    _c, _noun, _extent = "hdlc", "hdlc", "max_bytes"

    def __init__(self, ctx, kind, diff=0, fcs=16, min_bytes=None, max_bytes=256, msb_first=False, keep_bad=False, rows=1):
        self._open(ctx, kind, rows)
        self.diff, self.fcs, self.max_bytes = int(diff), int(fcs), int(max_bytes)
        self.min_bytes = self.fcs // 8 + 1 if min_bytes is None else int(min_bytes)
        self.msb_first, self.keep_bad = int(bool(msb_first)), int(bool(keep_bad))
        if min(self.diff, self.fcs, self.min_bytes, self.max_bytes) < 0 or max(self.fcs, self.min_bytes, self.max_bytes) >= 1 << 32:
            raise ErrInvalidArgument("hdlc: diff, fcs and the bounds are not negative")
        self.span_max = 8 * self.max_bytes + 8 * self.max_bytes // 5
        self.frame_bytes, self.history_bytes = self.max_bytes, (self.span_max + 8 + 7) // 8
        ctx._ck(lib.hzsdr_hdlc_create(ctx._h, self.kind, self.diff, self.fcs, self.min_bytes, self.max_bytes, self.msb_first, self.keep_bad, self.rows,
                                      C.byref(self._h)))

    def plan(self):
        """(rows per wave, bits per tile, words of the history ring, form): the form is a sum of HDLC_FORM_*."""
        return self._plan()

    def push(self, symbols, counts=None, cap=4, out=None):
        """Run the symbols of every row through the bank -> (frames, positions, info, counts).  `counts`, when given, is
        what SymbolSync.push returned beside the symbols: row r consumes min(counts[r], n) of its n symbols; without it
        every row consumes n.  frames is uint8 (rows, cap, max_bytes), positions (rows, cap) the frames' first bits, info
        (rows, cap) bytes | good << 31, counts (rows,) the frames emitted in this push: above cap where a row lost some.
        Slots from a row's count up, and a slot's bytes behind its frame, hold what the destination held (a new one is
        zero).  `out`, when given, is such a tuple (frames, positions, info, counts) to write into; frames may be a view
        with a row pitch above cap * max_bytes."""
        return self._push(symbols, counts, cap, out)

    def ragged(self, frames, positions, info, counts):
        """A push's results -> a list of `rows` host triples (packets: a list of k bytes objects, FCS included;
        positions (k,) uint64; good (k,) bool), k = min(counts[r], cap) (this waits for the device in a DEVICE context)."""
        if _is_torch(frames):
            frames, positions, info, counts = (t.cpu().numpy() for t in (frames, positions, info, counts))
        cap = frames.shape[1]
        out = []
        for r, c in enumerate(np.asarray(counts).reshape(-1).view(np.uint32)):
            k = min(int(c), cap)
            inf = info[r, :k].copy().view(np.uint32)
            packets = [bytes(frames[r, i, :int(inf[i] & 0x7FFFFFFF)]) for i in range(k)]
            out.append((packets, positions[r, :k].copy().view(np.uint64), (inf >> 31).astype(bool)))
        return out

    def state(self):
        """(positions uint64 (rows,), events uint64 (rows,), kinds uint8 (rows,), history uint8 (rows, ceil(K / 8)), last
        uint8 (rows,)): the symbols consumed, the previous events' positions plus one, their kinds (HDLC_EVENT_ABORT,
        HDLC_EVENT_FLAG), the last K = Lmax + 8 bits oldest first and most significant bit first, the last raw
        decisions; behind every push so far."""
        R = self.rows
        p, e, k = np.empty(R, np.uint64), np.empty(R, np.uint64), np.empty(R, np.uint8)
        y, d = np.empty((R, self.history_bytes), np.uint8), np.empty(R, np.uint8)
        self.ctx._ck(lib.hzsdr_hdlc_get_state(self._h, p.ctypes.data_as(_PU64), e.ctypes.data_as(_PU64), k.ctypes.data_as(_PU8), y.ctypes.data_as(_PU8),
                                              d.ctypes.data_as(_PU8), R))
        return p, e, k, y, d

    def set_state(self, positions, events, kinds, history, last):
        R = self.rows
        p, e, k = np.ascontiguousarray(positions, np.uint64), np.ascontiguousarray(events, np.uint64), np.ascontiguousarray(kinds, np.uint8)
        y, d = np.ascontiguousarray(history, np.uint8), np.ascontiguousarray(last, np.uint8)
        if p.shape != (R,) or e.shape != (R,) or k.shape != (R,) or y.shape != (R, self.history_bytes) or d.shape != (R,):
            raise ErrInvalidArgument("hdlc: the state is positions (rows,), events (rows,), kinds (rows,), history (rows, ceil(K / 8)), last (rows,)")
        self.ctx._ck(lib.hzsdr_hdlc_set_state(self._h, p.ctypes.data_as(_PU64), e.ctypes.data_as(_PU64), k.ctypes.data_as(_PU8), y.ctypes.data_as(_PU8),
                                              d.ctypes.data_as(_PU8), R))


__all__ = ["Hdlc", "hdlc_encode", "hdlc_line", "hdlc_fcs16", "hdlc_fcs32", "HDLC_EVENT_ABORT", "HDLC_EVENT_FLAG", "HDLC_FORM_COMPLEX", "HDLC_FORM_DIFF",
           "HDLC_FORM_FCS16", "HDLC_FORM_FCS32", "HDLC_FORM_MSB_FIRST", "HDLC_FORM_KEEP_BAD", "HDLC_MAX_ROWS", "HDLC_MAX_BYTES"]

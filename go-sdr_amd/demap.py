"""The demapper bank (include/hzsdr_demap.h): frames of received symbols -- the soft frame bank's float32 payloads -- to
per-bit soft values in the order and with the signs a decoder expects.

    pts = hz.qam_points(4)                                     # 16-QAM, Gray per axis, unit mean power
    perm = hz.block_interleaver(12, 16)                        # the transmitter wrote rows and sent columns
    dm = ctx.demapper(hz.DEMAP_C64, pts, symbols=48, perm=perm, flip=hz.pack_flip(prbs), gain=hz.demap_gain(0.1), rows=100)
    values, _ = soft.push(symbols, counts, positions, info, got, cap=4)   # the soft frame bank, on the device
    llrs = dm.run(values, got)                                 # (rows, cap, N) float32, what ViterbiDecoder / LdpcDecoder read
    data, info = ld.decode(llrs, got)

Per symbol and bit the value is (d0 - d1) * gain, d0 and d1 the least squared distances to the points whose bit is 0 and
1 (max-log), every step one float32 operation; positive says 1.  Point p carries the label p, bit j (0 first) of a symbol
is (p >> (m - 1 - j)) & 1.  out[k] = L[perm[k]], DEMAP_ERASED marks a hole; where flip's bit k is set the sign is flipped;
every NaN (an erased input, a hole) leaves as 0x7FC00000, the decoders' erasure.  Row r handles min(counts[r], cap) frames;
the other slots of the destination stay as they are.  Frames are independent and the bank keeps no state.

Not here: exact (log-sum) LLRs, soft combining of repeated positions, rotations that are not multiples of 90 degrees,
differential modes, a separable fast path for square QAM, changing the gain after create.
"""
import ctypes as C

import numpy as np

from . import ErrInvalidArgument, _is_torch, lib
from ._frames import _Bank, block_ptr, dense_ptr, new_like
from ._capi import (DEMAP_C64, DEMAP_ERASED, DEMAP_FORM_GROUPED, DEMAP_FORM_PERM, DEMAP_FORM_TREE, DEMAP_LLR_F32, DEMAP_MAX_BITS, DEMAP_MAX_FRAMES,
                    DEMAP_MAX_LLRS, DEMAP_MAX_OUT, DEMAP_MAX_ROWS, DEMAP_MAX_SYMBOLS, DEMAP_REAL_F32)


def _gray(n):
    """the Gray code of 0 ... n - 1"""
    k = np.arange(n)
    return k ^ (k >> 1)


def _by_label(labels, values):
    """values listed by position -> listed by label"""
    out = np.empty(len(values), np.asarray(values).dtype)
    out[np.asarray(labels)] = values
    return out


def pam_points(m):
    """2^m equally spaced real levels, unit mean power, Gray labels along the axis -> float32 (M,): the level at
    position i (ascending) carries the label i ^ (i >> 1)."""
    m = int(m)
    if not 1 <= m <= DEMAP_MAX_BITS:
        raise ValueError("pam_points: 1 <= m <= 8")
    M = 1 << m
    levels = 2.0 * np.arange(M) - (M - 1)
    levels /= np.sqrt(np.mean(levels ** 2))
    return _by_label(_gray(M), levels).astype(np.float32)


def psk_points(m):
    """2^m points on the unit circle, Gray labels around it -> complex64 (M,): the point at angle 2 pi (i + 1/2) / M for
    m = 2 (QPSK on the diagonals) and 2 pi i / M otherwise carries the label i ^ (i >> 1)."""
    m = int(m)
    if not 1 <= m <= DEMAP_MAX_BITS:
        raise ValueError("psk_points: 1 <= m <= 8")
    M = 1 << m
    ang = 2.0 * np.pi * (np.arange(M) + (0.5 if m == 2 else 0.0)) / M
    return _by_label(_gray(M), np.exp(1j * ang)).astype(np.complex64)


def qam_points(m):
    """Square 2^m-QAM for even m, Gray per axis, unit mean power -> complex64 (M,): the first m / 2 bits of a label are
    the Gray label of the real level, the last m / 2 that of the imaginary level."""
    m = int(m)
    if m % 2 or not 2 <= m <= DEMAP_MAX_BITS:
        raise ValueError("qam_points: m is 2, 4, 6 or 8")
    h = m // 2
    side = 1 << h
    axis = _by_label(_gray(side), 2.0 * np.arange(side) - (side - 1))  # by label, not yet scaled
    label = np.arange(1 << m)
    pts = axis[label >> h] + 1j * axis[label & (side - 1)]
    return (pts / np.sqrt(np.mean(np.abs(pts) ** 2))).astype(np.complex64)


def map_bits(points, bits):
    """The modulator: bits (..., S m), the first bit of a symbol the label's most significant -> symbols (..., S) of the
    points' dtype."""
    points = np.asarray(points)
    m = int(len(points)).bit_length() - 1
    if len(points) != 1 << m or m < 1:
        raise ValueError("map_bits: 2^m points")
    b = np.asarray(bits, np.int64) & 1
    if b.shape[-1] % m:
        raise ValueError("map_bits: the bits are a whole number of symbols")
    groups = b.reshape(*b.shape[:-1], -1, m)
    labels = (groups << np.arange(m - 1, -1, -1)).sum(axis=-1)
    return points[labels]


def block_interleaver(rows, cols):
    """The perm that undoes a block interleaver which wrote `rows` x `cols` bits row by row and sent them column by
    column: sent position c * rows + r holds bit r * cols + c, so out[k] = L[perm[k]] with perm[r * cols + c] =
    c * rows + r -> uint32 (rows * cols,)."""
    rows, cols = int(rows), int(cols)
    if rows < 1 or cols < 1:
        raise ValueError("block_interleaver: rows and cols are at least 1")
    r, c = np.divmod(np.arange(rows * cols), cols)
    return (c * rows + r).astype(np.uint32)


def demap_gain(sigma):
    """1 / (2 sigma^2): the gain that makes the values max-log LLRs under noise of deviation sigma per component"""
    return float(1.0 / (2.0 * float(sigma) ** 2))


def pack_flip(bits):
    """a 0 / 1 sequence (a randomiser's output) -> the packed `flip` bytes, most significant bit first"""
    return np.packbits(np.asarray(bits, np.uint8) & 1)


class Demapper(_Bank):
    """hzsdr_demap: run(frames, counts) -> soft values.  `kind` is DEMAP_C64 (frames of S complex symbols as 2 S float32
    re, im ...: SoftFrames.push's values of complex rows with two bits per symbol), DEMAP_REAL_F32 (S real symbols) or
    DEMAP_LLR_F32 (S per-bit values; `points` is None).  `points` are the 2^m constellation points by label (complex for
    C64, real for REAL_F32), `symbols` = S, `perm` a uint32 (N,) or None (N = S m), `flip` the packed bytes of N bits (pack_flip)
    or None, `gain` one positive value or one per row.  frames is (rows, cap,
    W) float32 -- (cap, W) will do for one row -- with contiguous rows and any row pitch.  numpy in a HOST context; torch
    tensors on the context's device, written on the context's stream, in a DEVICE context (counts are int32 there)."""
    _c = _noun = "demap"

    def __init__(self, ctx, kind, points, symbols, perm=None, flip=None, gain=1.0, rows=1):
        self.kind = int(kind)
        self._open(ctx, rows)
        fp, u32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
        pts, m = None, 1
        if points is not None:
            points = np.asarray(points)
            m = max(int(len(points)).bit_length() - 1, 0)
            if points.ndim != 1 or len(points) != 1 << m:
                raise ErrInvalidArgument("demap: 2^m points, listed by label")
            if self.kind == DEMAP_C64:
                pts = np.ascontiguousarray(points, np.complex64).view(np.float32)
            else:
                if np.iscomplexobj(points):
                    raise ErrInvalidArgument("demap: real symbols take real points")
                pts = np.ascontiguousarray(points, np.float32)
        self.points, self.m, self.S = points, m, int(symbols)
        if self.S < 0 or self.S >= 1 << 62:
            raise ErrInvalidArgument("demap: symbols is an unsigned value")
        prm = None if perm is None else np.ascontiguousarray(perm, np.uint32)
        if prm is not None and prm.ndim != 1:
            raise ErrInvalidArgument("demap: perm is a list of positions")
        N = len(prm) if prm is not None else self.S * m
        flp = None if flip is None else np.ascontiguousarray(flip, np.uint8)
        if flp is not None and (flp.ndim != 1 or len(flp) != (N + 7) // 8):
            raise ErrInvalidArgument("demap: flip is ceil(N / 8) packed bytes (pack_flip)")
        gains = np.ascontiguousarray(np.atleast_1d(gain), np.float32)
        if gains.ndim != 1:
            raise ErrInvalidArgument("demap: gain is one value, or one per row")
        self.perm, self.flip, self.gains = prm, flp, gains
        ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
        self.ctx._ck(lib.hzsdr_demap_create(self.ctx._h, self.kind, m, ptr(pts, fp), self.S, ptr(prm, u32p), N, ptr(flp, u8p), ptr(gains, fp), len(gains),
                                            self.rows, C.byref(self._h)))
        self.S, self.W, self.m, self.N = self.sizes()

    def sizes(self):
        """(S symbols, W input floats, m bits per symbol, N output floats) of a frame"""
        return self._sizes("sizes", 4)

    def plan(self):
        """(frames per workgroup, threads per frame, LDS bytes of a frame's values, a sum of DEMAP_FORM_*)"""
        return self._plan()

    def run(self, frames, counts=None, cap=None, out=None):
        """Demap min(counts[r], cap) frames of every row -> float32 (rows, cap, N).  `counts`, when given, is what
        FrameSync.push returned beside the frames (values above cap are clamped); without it every row handles cap
        frames.  `cap` defaults to the frames' second-last extent.  Slots from a row's count up hold what the destination
        held (a new one is zero).  `out`, when given, is such a block; it may be a view with a row pitch above cap * N."""
        noun, R = self._noun, self.rows
        if frames.ndim == 2 and R == 1:
            frames = frames[None]
        if frames.ndim != 3:
            raise ValueError(f"{noun}: frames are (rows, cap, W)")
        cap = int(frames.shape[1]) if cap is None else int(cap)
        fptr, fpitch = block_ptr(frames, (R, cap, self.W), np.float32, "frames", noun)
        if out is None:
            out = new_like((R, cap, self.N), np.float32, frames)
        optr, opitch = block_ptr(out, (R, cap, self.N), np.float32, "out", noun)
        cptr = None if counts is None else dense_ptr(counts, (R,), np.uint32, "the frames' counts", noun, "int32")
        self._call("run", fptr, fpitch, cptr, cap, optr, opitch)
        return out

    def ragged(self, values, counts=None):
        """A call's result -> a list of `rows` host arrays float32 (k, N), k = min(counts[r], cap) (this waits for the
        device in a DEVICE context)."""
        if _is_torch(values):
            values = values.cpu().numpy()
            counts = None if counts is None else counts.cpu().numpy()
        if values.ndim == 2:
            values = values[None]
        cap = values.shape[1]
        got = np.full(self.rows, cap, np.uint32) if counts is None else np.asarray(counts).reshape(-1).view(np.uint32)
        return [values[r, :min(int(c), cap)].copy() for r, c in enumerate(got)]


__all__ = ["Demapper", "psk_points", "qam_points", "pam_points", "map_bits", "block_interleaver", "demap_gain", "pack_flip", "DEMAP_C64", "DEMAP_REAL_F32",
           "DEMAP_LLR_F32", "DEMAP_ERASED", "DEMAP_FORM_GROUPED", "DEMAP_FORM_PERM", "DEMAP_FORM_TREE", "DEMAP_MAX_ROWS", "DEMAP_MAX_BITS",
           "DEMAP_MAX_SYMBOLS", "DEMAP_MAX_LLRS", "DEMAP_MAX_OUT", "DEMAP_MAX_FRAMES"]

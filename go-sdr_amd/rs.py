"""The Reed-Solomon decoder bank (include/hzsdr_rs.h): frames of symbol-interleaved Reed-Solomon codewords over GF(2^8)
-- the Viterbi bank's decoded frames, or the frame sync bank's for a link without an inner code -- to corrected data
bytes and a verdict per frame.

    rs = ctx.reed_solomon(hz.CCSDS_RS_255_223, interleave=2, scramble=hz.ccsds_randomizer(510), rows=100)
    data, verdict = vd.decode(frames, counts)       # the Viterbi bank, on the device
    clean, info = rs.decode(data, counts)           # clean (rows, cap, I k) uint8; info = E | nfail << 16 | ok << 31

A code is (gfpoly, fcr, prim, nroots, n): GF(2^8) by the primitive polynomial gfpoly, alpha = 2, codewords of n symbols,
the first the coefficient of x^(n-1), with the roots alpha^(prim (fcr + j)), j < nroots; systematic, k = n - nroots data
symbols first; n < 255 is a shortened code.  A frame is I n bytes, codeword i owning bytes i, i + I, ...  Every byte is
first xored with scramble[m mod len(scramble)] and then mapped through in_map; a codeword within t = nroots // 2 symbols
of the received word is the result (bounded distance), otherwise the codeword FAILS and passes through unchanged; the
first I k bytes go out through out_map.  Row r decodes min(counts[r], cap) frames; the other slots of the destinations,
and the bytes behind I k in a slot, stay as they are.  Frames are independent and the bank keeps no state.

Not here: erasures, soft decisions, encoding on the device (rs_encode is numpy), other symbol sizes, interleavers
across frames.
"""
import numpy as np

from . import ErrInvalidArgument
from ._frames import DecoderBank, pitched_block_ptr
from ._capi import RS_MAX_FRAMES, RS_MAX_INTERLEAVE, RS_MAX_N, RS_MAX_ROOTS, RS_MAX_ROWS, RS_MAX_SCRAMBLE, RS_MIN_ROOTS

CCSDS_RS_255_223 = (0x187, 112, 11, 32, 255)  # (gfpoly, fcr, prim, nroots, n)
CCSDS_RS_255_239 = (0x187, 120, 11, 16, 255)
DVB_RS_204_188 = (0x11D, 0, 1, 16, 204)


def _tables(gfpoly):
    """(exp (510,), log (256,)) of GF(2^8) by gfpoly, alpha = 2"""
    exp, log, x = np.zeros(510, np.int64), np.zeros(256, np.int64), 1
    for i in range(255):
        exp[i], log[x] = x, i
        x <<= 1
        if x & 0x100:
            x ^= gfpoly
    exp[255:] = exp[:255]
    return exp, log


def _mul(a, b, exp, log):
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    return np.where((a != 0) & (b != 0), exp[log[a] + log[b]], 0)


def rs_generator(code):
    """The generator polynomial of `code`, prod_j (x - alpha^(prim (fcr + j))): uint8 (nroots + 1,), the coefficient of
    x^nroots (1) first"""
    gfpoly, fcr, prim, nroots, _ = code
    exp, log = _tables(gfpoly)
    g = np.array([1], np.int64)
    for j in range(nroots):
        root = exp[(prim * (fcr + j)) % 255]
        g = np.concatenate([g, [0]]) ^ np.concatenate([[0], _mul(g, root, exp, log)])
    return g.astype(np.uint8)


def rs_encode(code, data):
    """data uint8 (..., k) -> codewords uint8 (..., n): the data symbols, then the nroots parity symbols"""
    gfpoly, _, _, nroots, n = code
    data = np.asarray(data, np.uint8)
    k = n - nroots
    if data.shape[-1] != k:
        raise ValueError(f"rs_encode: the last extent is k = {k}")
    exp, log = _tables(gfpoly)
    g = rs_generator(code).astype(np.int64)[1:]  # the coefficients of x^(nroots-1) ... x^0
    par = np.zeros(data.shape[:-1] + (nroots,), np.int64)
    for p in range(k):
        fb = data[..., p].astype(np.int64) ^ par[..., 0]
        par = np.concatenate([par[..., 1:], np.zeros_like(par[..., :1])], axis=-1) ^ _mul(fb[..., None], g, exp, log)
    return np.concatenate([data, par.astype(np.uint8)], axis=-1)


def interleave_codewords(words):
    """codewords uint8 (..., I, n) -> frames (..., I n): codeword i in the bytes i, i + I, ..."""
    words = np.asarray(words, np.uint8)
    return np.ascontiguousarray(np.swapaxes(words, -1, -2)).reshape(words.shape[:-2] + (-1,))


def ccsds_randomizer(length):
    """The CCSDS pseudo-randomiser as `length` bytes: bits b[0 ... 7] = 1, b[i + 8] = b[i] ^ b[i + 3] ^ b[i + 5] ^ b[i + 7],
    packed most significant bit first (FF 48 0E C0 ...; the period is 255 bits)"""
    b = np.ones(8 * int(length) + 8, np.uint8)
    for i in range(8 * int(length)):
        b[i + 8] = b[i] ^ b[i + 3] ^ b[i + 5] ^ b[i + 7]
    return np.packbits(b[:8 * int(length)])


def ccsds_dual_basis():
    """(to_dual, from_dual), uint8 (256,) each: bit j of to_dual[v], from the most significant, is Tr(v beta^j) with
    beta = alpha^117 in the field of 0x187 (Berlekamp's representation); from_dual is the inverse.  A CCSDS link that
    sends dual-basis symbols decodes with in_map=from_dual, out_map=to_dual."""
    exp, log = _tables(0x187)
    v = np.arange(256)

    def trace(x):
        acc, y = np.zeros(256, np.int64), x
        for _ in range(8):
            acc, y = acc ^ y, _mul(y, y, exp, log)
        return acc  # 0 or 1
    to_dual = np.zeros(256, np.int64)
    for j in range(8):
        to_dual |= trace(_mul(v, exp[(117 * j) % 255], exp, log)) << (7 - j)
    from_dual = np.zeros(256, np.int64)
    from_dual[to_dual] = v
    return to_dual.astype(np.uint8), from_dual.astype(np.uint8)


class ReedSolomon(DecoderBank):
    """hzsdr_rs: decode(frames, counts) -> (data, info).  frames is uint8 (rows, cap, width) -- (cap, width) will do for
    one row -- with width at least the frame bytes I n, unit stride along a frame, any frame pitch and any row pitch: the
    Viterbi bank's data block as it is.  numpy in a HOST context; torch tensors on the context's device, written on the
    context's stream, in a DEVICE context (info and counts are int32 there: the same bits)."""
    _c = _noun = "rs"

    def __init__(self, ctx, code, interleave=1, in_map=None, out_map=None, scramble=None, rows=1):
        self.interleave, self.code = int(interleave), tuple(int(v) for v in code)
        self._open(ctx, rows)
        if len(self.code) != 5 or min(self.code) < 0 or max(self.code) >= 1 << 32 or not 0 <= self.interleave < 1 << 32:
            raise ErrInvalidArgument("rs: a code is (gfpoly, fcr, prim, nroots, n), unsigned values")
        maps = []
        for m, what in ((in_map, "in_map"), (out_map, "out_map")):
            if m is not None:
                m = np.ascontiguousarray(m, np.uint8)
                if m.shape != (256,):
                    raise ErrInvalidArgument(f"rs: {what} is 256 bytes")
            maps.append(m)
        scr = None if scramble is None else np.ascontiguousarray(scramble, np.uint8).reshape(-1)
        if scr is not None and scr.size == 0:
            scr = None
        ptr = [None if m is None else m.ctypes.data for m in (*maps, scr)]
        self._create(*self.code, self.interleave, *ptr, 0 if scr is None else scr.size)
        self.k, self.t, self.frame_bytes, self.data_bytes = self.sizes()
        self.n, self.nroots = self.code[4], self.code[3]

    def sizes(self):
        """(k data symbols, t correctable symbols per codeword, frame bytes I n, data bytes I k)"""
        return self._sizes("sizes", 4)

    def plan(self):
        """(waves per workgroup, LDS bytes per workgroup, workgroups a compute unit holds, workgroups of a call at most)"""
        return self._sizes("plan", 4)

    def decode(self, frames, counts=None, cap=None, out=None):
        """Decode min(counts[r], cap) frames of every row -> (data uint8 (rows, cap, I k), info (rows, cap) =
        E | nfail << 16 | ok << 31).  `counts`, when given, is what the bank in front returned beside the frames (values
        above cap are clamped); without it every row decodes cap frames.  `cap` defaults to the frames' second-last
        extent.  Slots from a row's count up hold what the destination held (a new one is zero).  `out`, when given, is
        such a pair (data, info); data may be wider than I k, a view with pitches, or `frames` itself (in place)."""
        if frames.ndim == 2 and self.rows == 1:
            frames = frames[None]
        if frames.ndim != 3:
            raise ValueError("rs: frames are (rows, cap, width)")
        cap = int(frames.shape[1]) if cap is None else int(cap)
        fptr, fstride, fpitch = pitched_block_ptr(frames, self.rows, cap, self.frame_bytes, "frames", "rs")
        out = self._out(frames, cap, out)
        data, info = out
        if data.ndim == 2 and self.rows == 1:
            data = data[None]
        dptr, dstride, dpitch = pitched_block_ptr(data, self.rows, cap, self.data_bytes, "data", "rs")
        iptr, cptr = self._tail_ptrs(info, counts, cap)
        self._call("decode", fptr, fstride, fpitch, cptr, cap, dptr, dstride, dpitch, iptr)
        return out[0], info

    def ragged(self, data, info, counts=None):
        """A call's results -> a list of `rows` host tuples (data (k, I k), E (k,) uint32, nfail (k,) uint32, ok (k,)
        bool), k = min(counts[r], cap) (this waits for the device in a DEVICE context)."""
        return self._ragged(data, info, counts)

    @staticmethod
    def _fields(w):
        return w & np.uint32(0xFFFF), (w >> np.uint32(16)) & np.uint32(0x7FFF), (w >> np.uint32(31)).astype(bool)


__all__ = ["ReedSolomon", "rs_encode", "rs_generator", "interleave_codewords", "ccsds_randomizer", "ccsds_dual_basis", "CCSDS_RS_255_223",
           "CCSDS_RS_255_239", "DVB_RS_204_188", "RS_MAX_ROWS", "RS_MIN_ROOTS", "RS_MAX_ROOTS", "RS_MAX_N", "RS_MAX_INTERLEAVE", "RS_MAX_SCRAMBLE",
           "RS_MAX_FRAMES"]

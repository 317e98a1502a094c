"""The LDPC decoder bank (include/hzsdr_ldpc.h): frames of a binary low-density parity-check code -- the soft frame
bank's float32 payloads, or the frame sync bank's packed payload bits -- to data bits, the number of unsatisfied checks,
the iterations run and a verdict per frame.

    code, perm = hz.ldpc_systematic(hz.qc_code(shifts, Z))       # a standard's base table, brought by the user
    ld = ctx.ldpc(hz.LDPC_SOFT_F32, code, scale=16.0, max_iters=50, norm=12, rows=100)
    values, _ = soft.push(symbols, counts, positions, info, got, cap=4)   # the soft frame bank, on the device
    data, info = ld.decode(values, got)           # data (rows, cap, DB) uint8; info = u | iters << 16 | ok << 31

The decision is flooding min-sum in integers: q = rint(clamp(x * scale)) in -127 ... 127 (a NaN is an erasure), hard bits
are +-level; every iteration clamps P[v] - r_e to +-127, gives each edge of a check the smaller of the two smallest
magnitudes of the others, normalised by norm / 16 and lowered by offset, and sums exactly; a frame stops as soon as every
check is satisfied.  The received positions are the variables head ... head + N - 1, every other variable is punctured;
the data bits are the variables 0 ... D - 1.  Row r decodes min(counts[r], cap) frames; the other slots of the
destinations stay as they are.  Frames are independent and the bank keeps no state.

The code is its parity-check matrix in check-major compressed form (LdpcCode: row_ptr, col).  No standard's tables are
here; qc_code expands a quasi-cyclic base table, regular_code makes a reproducible random regular code,
ldpc_systematic and ldpc_encode bring a code into a form that can be encoded and encode under it.

Not here: layered schedules, non-binary codes, shortening by known bits, rate matching, the outer BCH code of DVB-S2,
soft outputs of the decoder.
"""
import ctypes as C

import numpy as np

from . import ErrInvalidArgument
from ._frames import DecoderBank
from ._capi import (LDPC_BITS, LDPC_FORM_TABLES_CACHE, LDPC_FORM_TABLES_LDS, LDPC_MAX_BITS, LDPC_MAX_CHECKS, LDPC_MAX_DEGREE, LDPC_MAX_EDGES,
                    LDPC_MAX_FRAMES, LDPC_MAX_ITERS, LDPC_MAX_ROWS, LDPC_MAX_VARIABLES, LDPC_SOFT_F32)


class LdpcCode:
    """A parity-check matrix of m checks over n variables in check-major compressed form: row_ptr uint32 (m + 1,), col
    uint32 (E,), the variables of check c at col[row_ptr[c]:row_ptr[c + 1]], ascending.  `k`, where known, says that
    the first k variables are free (ldpc_systematic)."""

    def __init__(self, n, row_ptr, col, k=None):
        self.n, self.k = int(n), k
        self.row_ptr, self.col = np.ascontiguousarray(row_ptr, np.uint32), np.ascontiguousarray(col, np.uint32)
        self.m, self.E = len(self.row_ptr) - 1, len(self.col)

    @classmethod
    def from_dense(cls, H, k=None):
        """a dense 0 / 1 matrix (m, n) -> the compressed form"""
        H = np.asarray(H) != 0
        rows, cols = np.nonzero(H)  # (row-major: ascending inside a row)
        row_ptr = np.concatenate([[0], np.cumsum(H.sum(axis=1))])
        return cls(H.shape[1], row_ptr, cols, k)

    def dense(self):
        """uint8 (m, n)"""
        H = np.zeros((self.m, self.n), np.uint8)
        H[np.repeat(np.arange(self.m), np.diff(self.row_ptr.astype(np.int64))), self.col] = 1
        return H

    def syndrome(self, x):
        """bits (..., n) -> uint8 (..., m): H x over GF(2), check by check"""
        x = np.asarray(x, np.uint8) & 1
        picked = x[..., self.col.astype(np.int64)]
        return np.bitwise_xor.reduceat(picked, self.row_ptr[:-1].astype(np.int64), axis=-1)


def qc_code(shifts, Z):
    """Expand a quasi-cyclic base table -> LdpcCode.  `shifts` is (mb, nb) of integers, -1 for "no block", s >= 0 for
    the Z x Z identity with its columns rotated by s: row i of the block has its 1 in column (i + s) mod Z.  Check
    bi * Z + i then holds the variables bj * Z + (i + shifts[bi][bj]) mod Z."""
    S = np.asarray(shifts, np.int64)
    Z = int(Z)
    if S.ndim != 2 or Z < 1 or S.min() < -1:
        raise ValueError("qc_code: shifts is a 2-D table of -1 or shifts >= 0, Z is at least 1")
    mb, nb = S.shape
    i = np.arange(Z)
    row_ptr, col = [0], []
    for bi in range(mb):
        used = np.nonzero(S[bi] >= 0)[0]
        block = np.stack([bj * Z + (i + S[bi, bj]) % Z for bj in used], axis=1) if len(used) else np.zeros((Z, 0), np.int64)
        col.append(block.reshape(-1))
        row_ptr.extend(row_ptr[-1] + len(used) * (i + 1))
    return LdpcCode(nb * Z, row_ptr, np.concatenate(col) if col else [])


def _splitmix(seed, count):
    x = (np.uint64(seed) + np.arange(1, count + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def regular_code(n, dv, dc, seed=0):
    """A reproducible random (dv, dc)-regular code of n variables and m = n dv / dc checks: every variable's dv sockets
    are dealt to the checks, dc each, in an order drawn from `seed`; a check that drew a variable twice exchanges the
    second socket with the next socket further on that leaves both checks without a repeat.  n dv is a multiple of dc,
    dc <= n."""
    n, dv, dc = int(n), int(dv), int(dc)
    if dc < 2 or dv < 1 or n < dc or (n * dv) % dc:
        raise ValueError("regular_code: dc >= 2, dv >= 1, dc <= n, n dv a multiple of dc")
    E, m = n * dv, n * dv // dc
    with np.errstate(over="ignore"):
        order = np.argsort(_splitmix(int(seed) * 1000003 + 1, E), kind="stable")
    rows = np.repeat(np.arange(n), dv)[order].reshape(m, dc)

    def clash(c, j, v):  # would v at socket j of check c repeat another socket of c?
        return any(rows[c, i] == v for i in range(dc) if i != j)
    for c in range(m):
        for j in range(1, dc):
            if rows[c, j] not in rows[c, :j]:
                continue
            for step in range(1, E):
                c2, j2 = divmod((c * dc + j + step) % E, dc)
                if c2 != c and not clash(c, j, rows[c2, j2]) and not clash(c2, j2, rows[c, j]):
                    rows[c, j], rows[c2, j2] = rows[c2, j2], rows[c, j]
                    break
            else:
                raise ValueError("regular_code: no code without a repeated edge for these sizes")
    return LdpcCode(n, np.arange(m + 1) * dc, np.sort(rows, axis=1).reshape(-1))


def _pack(H):
    return np.packbits(np.asarray(H, np.uint8), axis=1)


def _eliminate(H, order):
    """Gauss-Jordan over GF(2) on the columns in `order` -> (the reduced matrix (bit-packed rows), [(row, column)] of
    the pivots found)"""
    A = _pack(H)
    m = A.shape[0]
    pivots, at = [], 0
    for c in order:
        if at == m:
            break
        byte, bit = c >> 3, 0x80 >> (c & 7)
        hit = np.nonzero(A[at:, byte] & bit)[0]
        if not len(hit):
            continue
        p = at + int(hit[0])
        if p != at:
            A[[at, p]] = A[[p, at]]
        others = np.nonzero(A[:, byte] & bit)[0]
        others = others[others != at]
        A[others] ^= A[at]
        pivots.append((at, int(c)))
        at += 1
    return A, pivots


def ldpc_systematic(code):
    """GF(2) elimination with a column permutation -> (an equivalent LdpcCode whose first k = n - rank(H) variables are
    free, perm): variable j of the new code is variable perm[j] of the old one, the checks are the old ones, as sparse
    as before.  A rank-deficient H gives k > n - m."""
    H = code.dense()
    # pivots are looked for from the LAST column on: a code that is systematic already keeps its order
    _, pivots = _eliminate(H, range(code.n - 1, -1, -1))
    pivot_cols = sorted(c for _, c in pivots)
    is_pivot = np.zeros(code.n, bool)
    is_pivot[pivot_cols] = True
    perm = np.concatenate([np.nonzero(~is_pivot)[0], np.nonzero(is_pivot)[0]]).astype(np.int64)
    inv = np.empty(code.n, np.int64)
    inv[perm] = np.arange(code.n)
    col = inv[code.col.astype(np.int64)]
    rp = code.row_ptr.astype(np.int64)
    for c in range(code.m):
        col[rp[c]:rp[c + 1]].sort()
    return LdpcCode(code.n, code.row_ptr, col, k=code.n - len(pivots)), perm


def ldpc_encode(code, data):
    """Encode under a code whose first k variables are free (ldpc_systematic's): data bits (..., k) -> codewords
    (..., n) uint8 with H x = 0, the data in front."""
    if code.k is None:
        raise ValueError("ldpc_encode: the code comes from ldpc_systematic")
    k, n = code.k, code.n
    enc = getattr(code, "_enc", None)
    if enc is None:
        A, pivots = _eliminate(code.dense(), range(k, n))
        if len(pivots) != n - k:
            raise ValueError("ldpc_encode: the last n - k variables do not determine the checks")
        rows = np.array([r for r, _ in pivots], np.int64)
        cols = np.array([c for _, c in pivots], np.int64)
        enc = code._enc = (np.unpackbits(A[rows], axis=1)[:, :k].astype(np.uint8), cols)
    G, cols = enc
    d = np.asarray(data, np.uint8) & 1
    if d.shape[-1] != k:
        raise ValueError(f"ldpc_encode: data bits are (..., {k})")
    x = np.zeros(d.shape[:-1] + (n,), np.uint8)
    x[..., :k] = d
    x[..., cols] = (d.astype(np.int64) @ G.T.astype(np.int64)) & 1
    return x


class LdpcDecoder(DecoderBank):
    """hzsdr_ldpc: decode(frames, counts) -> (data, info).  `kind` is LDPC_SOFT_F32 (float32 frames of N values,
    positive meaning 1: SoftFrames.push's values) or LDPC_BITS (uint8 frames of FB = ceil(N / 8) bytes, most significant
    bit first: FrameSync.push's frames).  `code` is an LdpcCode; `received` defaults to every variable behind `head`,
    `data_bits` to the code's k (or n).  frames is (rows, cap, N or FB) -- (cap, ...) will do for one row -- with
    contiguous rows and any row pitch.  numpy in a HOST context; torch tensors on the context's device, written on the
    context's stream, in a DEVICE context (info and counts are int32 there: the same bits)."""
    _c = _noun = "ldpc"
    _bits = LDPC_BITS

    def __init__(self, ctx, kind, code, received=None, head=0, data_bits=None, scale=1.0, level=1, max_iters=50, norm=12, offset=0, rows=1):
        self.kind, self.code = int(kind), code
        self._open(ctx, rows)
        self.head = int(head)
        self.N = code.n - self.head if received is None else int(received)
        self.D = (code.n if code.k is None else code.k) if data_bits is None else int(data_bits)
        self.scale, self.level, self.max_iters, self.norm, self.offset = float(scale), int(level), int(max_iters), int(norm), int(offset)
        values = [self.head, self.N, self.D, self.level, self.max_iters, self.norm, self.offset]
        if min(values) < 0 or max(values[3:]) >= 1 << 32 or max(values[:3]) >= 1 << 62:
            raise ErrInvalidArgument("ldpc: sizes and parameters are unsigned values of their widths")
        rp, col = np.ascontiguousarray(code.row_ptr, np.uint32), np.ascontiguousarray(code.col, np.uint32)
        if len(rp) < 1:
            raise ErrInvalidArgument("ldpc: row_ptr has checks + 1 entries")
        self._create(self.kind, len(rp) - 1, int(code.n), rp.ctypes.data_as(C.POINTER(C.c_uint32)), col.ctypes.data_as(C.POINTER(C.c_uint32)), len(col),
                     self.head, self.N, self.D, self.scale, self.level, self.max_iters, self.norm, self.offset)
        _, self.frame_bytes, self.n, self.m, self.E, self.data_bytes = self.sizes()

    def sizes(self):
        """(N received positions, FB = ceil(N / 8), n, m, E, DB = ceil(D / 8))"""
        return self._sizes("sizes", 6)

    def plan(self):
        """(frames per workgroup, threads per frame, LDS bytes of a frame's state, LDPC_FORM_TABLES_LDS or _CACHE)"""
        return self._plan()

    def decode(self, frames, counts=None, cap=None, out=None):
        """Decode min(counts[r], cap) frames of every row -> (data uint8 (rows, cap, DB), info (rows, cap) =
        u | iters << 16 | ok << 31).  `counts`, when given, is what FrameSync.push returned beside the frames (values
        above cap are clamped); without it every row decodes cap frames.  `cap` defaults to the frames' second-last
        extent.  Slots from a row's count up hold what the destination held (a new one is zero).  `out`, when given, is
        such a pair (data, info); data may be a view with a row pitch above cap * DB."""
        return self._decode(frames, counts, cap, out)

    def ragged(self, data, info, counts=None):
        """A call's results -> a list of `rows` host tuples (data (k, DB), unsatisfied (k,) uint32, iters (k,) uint32,
        ok (k,) bool), k = min(counts[r], cap) (this waits for the device in a DEVICE context)."""
        return self._ragged(data, info, counts)

    @staticmethod
    def _fields(w):
        return w & np.uint32(0xFFFF), (w >> np.uint32(16)) & np.uint32(0xFF), (w >> np.uint32(31)).astype(bool)


__all__ = ["LdpcDecoder", "LdpcCode", "qc_code", "regular_code", "ldpc_systematic", "ldpc_encode", "LDPC_BITS", "LDPC_SOFT_F32",
           "LDPC_FORM_TABLES_LDS", "LDPC_FORM_TABLES_CACHE", "LDPC_MAX_ROWS", "LDPC_MAX_CHECKS", "LDPC_MAX_VARIABLES", "LDPC_MAX_EDGES",
           "LDPC_MAX_DEGREE", "LDPC_MAX_BITS", "LDPC_MAX_ITERS", "LDPC_MAX_FRAMES"]

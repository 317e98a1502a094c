"""The independent restatement of the LDPC decoder bank's definition (include/hzsdr_ldpc.h) in numpy, the frame makers of
its tests, and the runner of the host program tests/host/ldpc_ref.cpp (the bytes the device must produce).

The numpy restatement is written from the header's text and shaped unlike the C++: every step runs over the WHOLE edge
array at once (reduceat over the checks for the parity and the minima, the first edge of the smallest magnitude by a
masked minimum of edge numbers, one scatter-add for the sums) -- no loop over checks or edges."""
import os
import struct
import subprocess

import numpy as np

from util import splitmix64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS, SOFT_F32 = 1, 32
FORM_TABLES_LDS, FORM_TABLES_CACHE = 1, 2
MAX_ROWS, MAX_CHECKS, MAX_VARIABLES, MAX_EDGES, MAX_DEGREE, MAX_BITS, MAX_ITERS, MAX_FRAMES = 8192, 16384, 16384, 65536, 64, 8192, 255, 1 << 22

HAMMING74 = np.array([[1, 1, 0, 1, 1, 0, 0], [1, 0, 1, 1, 0, 1, 0], [0, 1, 1, 1, 0, 0, 1]], np.uint8)  # data bits 0 ... 3 in front


class Config:
    """a bank's configuration, as hzsdr_ldpc_create takes it; the code as (n, row_ptr, col)"""

    def __init__(self, n, row_ptr, col, N=None, head=0, D=None, kind=SOFT_F32, scale=1.0, level=1, max_iters=20, a=12, beta=0):
        self.n, self.row_ptr, self.col = int(n), np.asarray(row_ptr, np.int64), np.asarray(col, np.int64)
        self.m, self.E = len(self.row_ptr) - 1, len(self.col)
        self.head, self.kind, self.scale, self.level = int(head), int(kind), scale, int(level)
        self.N = self.n - self.head if N is None else int(N)
        self.D = self.n if D is None else int(D)
        self.max_iters, self.a, self.beta = int(max_iters), int(a), int(beta)
        self.FB, self.DB = (self.N + 7) // 8, (self.D + 7) // 8

    @classmethod
    def of(cls, code, **kw):
        """over a package LdpcCode (its n, row_ptr and col alone are taken)"""
        return cls(code.n, code.row_ptr, code.col, **kw)

    def dense(self):
        H = np.zeros((self.m, self.n), np.uint8)
        H[np.repeat(np.arange(self.m), np.diff(self.row_ptr)), self.col] = 1
        return H

    def create_args(self, code):
        """the arguments of Context.ldpc behind the context"""
        return (self.kind, code), dict(received=self.N, head=self.head, data_bits=self.D, scale=self.scale, level=self.level,
                                       max_iters=self.max_iters, norm=self.a, offset=self.beta)


def dense_code(H):
    """a dense 0 / 1 matrix -> (n, row_ptr, col)"""
    H = np.asarray(H) != 0
    return H.shape[1], np.concatenate([[0], np.cumsum(H.sum(axis=1))]), np.nonzero(H)[1]


def accepted(q):
    """the header's validation, restated (the arrays' lengths are the caller's: len(row_ptr) = m + 1, len(col) = E)"""
    if q.kind not in (BITS, SOFT_F32) or not 1 <= q.m <= 16384 or not 2 <= q.n <= 16384 or not 1 <= q.E <= 65536:
        return False
    if not 1 <= q.N <= 8192 or q.head < 0 or q.head + q.N > q.n or not 1 <= q.D <= q.n:
        return False
    if not 1 <= q.max_iters <= 255 or not 1 <= q.a <= 16 or not 0 <= q.beta <= 126:
        return False
    if q.kind == SOFT_F32 and not (np.isfinite(np.float32(q.scale)) and np.float32(q.scale) > 0):
        return False
    if q.kind == BITS and not 1 <= q.level <= 127:
        return False
    rp, col = q.row_ptr, q.col
    if rp[0] != 0 or rp[-1] != q.E or np.any(np.diff(rp) < 2) or np.any(np.diff(rp) > 64):
        return False
    if np.any(col < 0) or np.any(col >= q.n):
        return False
    inner = np.ones(q.E, bool)
    inner[rp[:-1]] = False  # an edge that is not its check's first
    if np.any((np.diff(col, prepend=-1) <= 0) & inner):
        return False
    deg = np.bincount(col, minlength=q.n)
    return bool(deg.min() >= 1 and deg.max() <= 64)


# ---- the definition, over whole arrays -------------------------------------------------------------------

def quantise(x, scale):
    """float32 values -> q in -127 ... 127, one float32 operation at a time; a NaN gives 0"""
    y = np.asarray(x, np.float32) * np.float32(scale)
    with np.errstate(invalid="ignore"):
        q = np.rint(np.minimum(np.maximum(y, np.float32(-127)), np.float32(127)))
    return np.where(np.isnan(y), 0, q).astype(np.int64)


def received(q, frame):
    """a frame as the bank takes it (FB packed bytes, or N float32) -> int64 (n,): q per variable, 0 where punctured"""
    if q.kind == BITS:
        v = (np.unpackbits(np.asarray(frame, np.uint8))[:q.N].astype(np.int64) * 2 - 1) * q.level
    else:
        v = quantise(np.asarray(frame, np.float32)[:q.N], q.scale)
    full = np.zeros(q.n, np.int64)
    full[q.head:q.head + q.N] = v
    return full


def unsatisfied(q, P):
    return int(np.bitwise_xor.reduceat((P[q.col] > 0).astype(np.int64), q.row_ptr[:-1]).sum())


def decode(q, frame):
    """one frame -> (data bytes (DB,), info, hard bits (n,)) by the three steps over the whole edge array"""
    q0 = received(q, frame)
    starts, E = q.row_ptr[:-1], q.E
    chk = np.repeat(np.arange(q.m), np.diff(q.row_ptr))  # the check of every edge
    edge = np.arange(E)
    r, P = np.zeros(E, np.int64), q0.copy()
    u, it = unsatisfied(q, P), 0
    while u and it < q.max_iters:
        it += 1
        t = np.clip(P[q.col] - r, -127, 127)
        pos = (t > 0).astype(np.int64)
        par = np.bitwise_xor.reduceat(pos, starts)
        mag = np.abs(t)
        m1 = np.minimum.reduceat(mag, starts)
        first = np.minimum.reduceat(np.where(mag == m1[chk], edge, E), starts)
        rest = mag.copy()
        rest[first] = 1 << 20
        m2 = np.minimum.reduceat(rest, starts)
        out = np.where(edge == first[chk], m2[chk], m1[chk])
        out = np.maximum(((out * q.a) >> 4) - q.beta, 0)
        r = np.where((par[chk] ^ pos) == 1, out, -out)
        P = q0.copy()
        np.add.at(P, q.col, r)
        assert np.abs(P).max() <= 127 * 65
        u = unsatisfied(q, P)
    hard = (P > 0).astype(np.uint8)
    return np.packbits(hard[:q.D]), u | (it << 16) | (int(u == 0) << 31), hard


def split(info):
    """info words -> (unsatisfied, iters, ok)"""
    info = np.asarray(info).view(np.uint32).astype(np.int64)
    return info & 0xFFFF, (info >> 16) & 0xFF, info >> 31


# ---- the frames ----------------------------------------------------------------------------------------

def random_bits(n, seed):
    return (splitmix64(seed, n) >> np.uint64(63)).astype(np.uint8)


def gaussian(seed, count):
    """reproducible standard normal values (Box-Muller over splitmix64)"""
    w = splitmix64(seed, 2 * count)
    u1 = ((w[:count] >> np.uint64(11)).astype(np.float64) + 1.0) / float(1 << 53)
    u2 = (w[count:] >> np.uint64(11)).astype(np.float64) / float(1 << 53)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def bpsk(bits, sigma, seed):
    """code bits (..., N) -> float32 +-1 (1 -> +1) with white noise of deviation sigma"""
    b = np.asarray(bits, np.float64) * 2 - 1
    return (b + sigma * gaussian(seed, b.size).reshape(b.shape)).astype(np.float32)


def hard_frames(values):
    """float frames (..., N) -> packed hard decisions (..., FB), sign bit clear meaning 1"""
    return np.packbits(~np.signbit(np.asarray(values, np.float32)), axis=-1)


# ---- the program ---------------------------------------------------------------------------------------

_EXE = {}


def build_exact(build_dir):
    """g++ -O2 of tests/host/ldpc_ref.cpp -> the program's path (built once per directory)"""
    if build_dir not in _EXE:
        os.makedirs(build_dir, exist_ok=True)
        exe = os.path.join(build_dir, "ldpc_ref")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"),
                               os.path.join(ROOT, "tests", "host", "ldpc_ref.cpp"), "-o", exe])
        _EXE[build_dir] = exe
    return _EXE[build_dir]


def _head(q, m=None, E=None):
    u32 = [q.kind, q.m if m is None else m, q.n, q.E if E is None else E, q.head, q.N, q.D, q.level, q.max_iters, q.a, q.beta]
    return struct.pack("<11I", *[int(v) & 0xFFFFFFFF for v in u32]) + struct.pack("<f", np.float32(q.scale))


def _u32(a):
    return (np.asarray(a, np.int64) & 0xFFFFFFFF).astype(np.uint32).tobytes()


def exact(build_dir, cases):
    """cases: [(config, frames (R, cap, FB or N), counts uint32 (R,) or None)] -> [(data (R, cap, DB), info (R, cap))]
    by the program; slots from a row's count up are zero"""
    exe = build_exact(build_dir)
    src, dst = os.path.join(build_dir, "ldpc_cases.bin"), os.path.join(build_dir, "ldpc_out.bin")
    shapes = []
    with open(src, "wb") as f:
        for q, frames, counts in cases:
            frames = np.ascontiguousarray(frames)
            R, cap, width = frames.shape
            assert frames.dtype == (np.uint8 if q.kind == BITS else np.float32) and width == (q.FB if q.kind == BITS else q.N)
            f.write(_head(q) + _u32(q.row_ptr) + _u32(q.col) + struct.pack("<qqi", R, cap, int(counts is not None)))
            if counts is not None:
                f.write(np.ascontiguousarray(counts, np.uint32).tobytes())
            f.write(frames.tobytes())
            shapes.append((q, R, cap))
    subprocess.check_call([exe, "run", src, dst])
    out, raw, off = [], open(dst, "rb").read(), 0
    for q, R, cap in shapes:
        data = np.frombuffer(raw, np.uint8, R * cap * q.DB, off).copy().reshape(R, cap, q.DB)
        off += data.nbytes
        info = np.frombuffer(raw, np.uint32, R * cap, off).copy().reshape(R, cap)
        off += info.nbytes
        out.append((data, info))
    assert off == len(raw)
    os.remove(src), os.remove(dst)
    return out


def check(build_dir, sets):
    """[(config, m or None, E or None)] -> [accepted] by csrc/hz_ldpc_plan.h; m and E, when given, are the scalars the
    program is told while the arrays keep their own lengths"""
    exe = build_exact(build_dir)
    src, dst = os.path.join(build_dir, "ldpc_sets.bin"), os.path.join(build_dir, "ldpc_checked.bin")
    with open(src, "wb") as f:
        for q, m, E in sets:
            f.write(_head(q, m, E) + struct.pack("<II", len(q.row_ptr), len(q.col)) + _u32(q.row_ptr) + _u32(q.col))
    subprocess.check_call([exe, "check", src, dst])
    got = np.fromfile(dst, np.int32)
    os.remove(src), os.remove(dst)
    assert len(got) == len(sets)
    return [bool(a) for a in got]

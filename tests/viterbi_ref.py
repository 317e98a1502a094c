"""The independent restatement of the Viterbi decoder bank's definition (include/hzsdr_viterbi.h) in numpy, the frame
makers of its tests, and the runner of the host program tests/host/viterbi_ref.cpp (the bytes the device must produce).

The numpy restatement is written from the header's text and shaped unlike the C++: the encoder's outputs of every state
and input are tabulated once, the add-compare-select runs over the WHOLE state array time step by time step, and an
exhaustive decoder for D <= 12 encodes all 2^D inputs and scores them by the metric definition alone -- no trellis."""
import os
import struct
import subprocess

import numpy as np

from util import splitmix64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS, SOFT_F32, TAIL, TRUNCATED = 1, 32, 0, 1
FORM_LDS, FORM_SCRATCH = 1, 2
MAX_ROWS, MIN_K, MAX_K, MAX_RATE, MAX_PATTERN, MAX_BITS, MAX_FRAMES = 8192, 3, 9, 4, 64, 8192, 1 << 22
INF = 1 << 30
K7 = (0o171, 0o133)
PATTERNS = {"1/2": (0b11, 2), "2/3": (0b1101, 4), "3/4": (0b110110, 6), "5/6": (0b1101100110, 10), "7/8": (0b11010101100110, 14)}
PATTERN64 = (0xB7DE_F6BD_EF7B_DEFF | 0xAAAA_AAAA_AAAA_AAAA, 64)  # 64 bits, n = 2: every pair has a 1, many pairs lose their second bit


class Config:
    """a bank's configuration, as hzsdr_viterbi_create takes it"""

    def __init__(self, K=7, gens=K7, D=78, inv=0, pattern=None, term=TAIL, kind=BITS, scale=1.0, crc=None):
        self.K, self.gens, self.D, self.inv, self.term, self.kind, self.scale = int(K), [int(g) for g in gens], int(D), int(inv), int(term), int(kind), scale
        self.n = len(self.gens)
        self.pattern, self.Lp = ((1 << self.n) - 1, self.n) if pattern is None else (int(pattern[0]), int(pattern[1]))
        self.crc = (0, 0, 0, 0) if crc is None else tuple(int(v) for v in crc)
        self.C = self.crc[0]
        self.T = self.D + (self.K - 1 if self.term == TAIL else 0)
        self.S = 1 << (self.K - 1)
        self.DB = (self.D + 7) // 8

    def sent(self):
        """bool (T * n,): is mother-code bit m transmitted?"""
        if not (0 < self.Lp <= 64):
            return np.zeros(0, bool)
        pat = np.array([(self.pattern >> (self.Lp - 1 - k)) & 1 for k in range(self.Lp)], bool)
        return np.resize(pat, self.T * self.n) if self.T * self.n else np.zeros(0, bool)

    @property
    def N(self):
        return int(self.sent().sum())

    @property
    def FB(self):
        return (self.N + 7) // 8

    def create_args(self):
        """the arguments of Context.viterbi behind the context"""
        return (self.kind, self.K, self.gens, self.D), dict(inv=self.inv, pattern=(self.pattern, self.Lp), termination=self.term, scale=self.scale,
                                                            crc=self.crc if self.C else None)


def accepted(q):
    """the header's validation, restated"""
    if q.kind not in (BITS, SOFT_F32) or not 3 <= q.K <= 9 or q.n not in (2, 3, 4):
        return False
    if any(not 0 < g < 1 << q.K for g in q.gens) or not 0 <= q.inv < 1 << q.n:
        return False
    if not (q.n <= q.Lp <= 64 and q.Lp % q.n == 0 and 0 <= q.pattern < 1 << q.Lp):
        return False
    pat = [(q.pattern >> (q.Lp - 1 - k)) & 1 for k in range(q.Lp)]
    if any(sum(pat[m:m + q.n]) == 0 for m in range(0, q.Lp, q.n)):
        return False
    if q.term not in (TAIL, TRUNCATED) or not 1 <= q.D <= 8192 or q.T > 8192 or q.N > 8192:
        return False
    if q.kind == SOFT_F32 and not (np.isfinite(np.float32(q.scale)) and np.float32(q.scale) > 0):
        return False
    C, poly, init, xorout = q.crc
    if C not in (0, 8, 16, 24, 32) or (C and C >= q.D):
        return False
    return all(0 <= v < max(1 << C, 1) for v in (poly, init, xorout)) if C else (poly, init, xorout) == (0, 0, 0)


# ---- the definition, over whole arrays -------------------------------------------------------------------

def quantise(x, scale):
    """float32 values -> q in -127 ... 127, one float32 operation at a time; a NaN gives 0"""
    y = np.asarray(x, np.float32) * np.float32(scale)
    with np.errstate(invalid="ignore"):
        q = np.rint(np.minimum(np.maximum(y, np.float32(-127)), np.float32(127)))
    return np.where(np.isnan(y), 0, q).astype(np.int64)


def received(q, frame):
    """a frame as the bank takes it (FB packed bytes, or N float32) -> int64 (T, n): q per mother-code bit, 0 where punctured"""
    if q.kind == BITS:
        v = np.unpackbits(np.asarray(frame, np.uint8))[:q.N].astype(np.int64) * 2 - 1
    else:
        v = quantise(np.asarray(frame, np.float32)[:q.N], q.scale)
    full = np.zeros(q.T * q.n, np.int64)
    full[q.sent()] = v
    return full.reshape(q.T, q.n)


def outputs(q):
    """int64 (2 S, n): the code bits of every register value reg = u << (K-1) | state"""
    reg = np.arange(2 * q.S)
    return np.stack([np.array([bin(int(r) & g).count("1") & 1 for r in reg]) ^ ((q.inv >> j) & 1) for j, g in enumerate(q.gens)], axis=1).astype(np.int64)


def costs(rx, code):
    """rx (..., n) values, code (..., n) bits -> the metric of the definition, summed over the positions"""
    wrong = (rx != 0) & ((rx > 0) != (code == 1))
    return np.where(wrong, np.abs(rx), 0).sum(axis=-1)


def crc_ok(q, u):
    C, poly, init, xorout = q.crc
    if not C:
        return 0
    reg = init
    for b in u[:q.D - C]:
        top = ((reg >> (C - 1)) & 1) ^ int(b)
        reg = (reg << 1) & ((1 << C) - 1)
        if top:
            reg ^= poly
    return int((reg ^ xorout) == int("".join(str(int(b)) for b in u[q.D - C:q.D]), 2))


def decode(q, frame):
    """one frame -> (data bytes (DB,), info) by add-compare-select over the whole state array, step by step"""
    rx, out = received(q, frame), outputs(q)
    s = np.arange(q.S)
    u = s >> (q.K - 2)
    p0 = (s & (q.S // 2 - 1)) << 1
    r0, r1 = (u << (q.K - 1)) | p0, (u << (q.K - 1)) | p0 | 1
    metric = np.full(q.S, INF, np.int64)
    metric[0] = 0
    dec = np.zeros((q.T, q.S), np.uint8)
    for t in range(q.T):
        a = metric[p0] + costs(rx[t], out[r0])
        b = metric[p0 | 1] + costs(rx[t], out[r1])
        dec[t] = b < a
        metric = np.where(b < a, b, a)
    end = 0 if q.term == TAIL else int(np.argmin(metric))  # (argmin: the first of equals)
    fin, st, bits = int(metric[end]), end, np.zeros(q.T, np.uint8)
    for t in range(q.T - 1, -1, -1):
        bits[t] = st >> (q.K - 2)
        st = ((st & (q.S // 2 - 1)) << 1) | int(dec[t, st])
    assert fin < 1 << 23
    return np.packbits(bits[:q.D]), fin | (crc_ok(q, bits) << 31)


def encode_all(q, inputs):
    """inputs (M, T) of 0 / 1 -> the mother code's bits (M, T, n)"""
    out = outputs(q)
    state = np.zeros(len(inputs), np.int64)
    code = np.zeros((len(inputs), q.T, q.n), np.int64)
    for t in range(q.T):
        reg = (inputs[:, t].astype(np.int64) << (q.K - 1)) | state
        code[:, t] = out[reg]
        state = reg >> 1
    return code


def exhaustive(q, frame):
    """D <= 12: every one of the 2^D data words encoded and scored by the metric's definition -> (the smallest metric,
    the data words that reach it (k, D)).  TAIL only: a TRUNCATED survivor is chosen by end state, not by data word."""
    assert q.D <= 12 and q.term == TAIL
    words = (np.arange(1 << q.D)[:, None] >> np.arange(q.D - 1, -1, -1)) & 1
    inputs = np.concatenate([words, np.zeros((len(words), q.T - q.D), np.int64)], axis=1)
    total = costs(received(q, frame)[None], encode_all(q, inputs)).sum(axis=1)
    best = int(total.min())
    return best, words[total == best].astype(np.uint8)


def encode(q, bits):
    """data bits (D,) -> the N transmitted code bits, by the tabulated outputs (the package's conv_encode is held to this)"""
    u = np.asarray(bits, np.int64).reshape(1, -1)
    inputs = np.concatenate([u, np.zeros((1, q.T - q.D), np.int64)], axis=1)
    return encode_all(q, inputs).reshape(-1)[q.sent()].astype(np.uint8)


# ---- the frames ----------------------------------------------------------------------------------------

def random_bits(n, seed):
    return (splitmix64(seed, n) >> np.uint64(63)).astype(np.uint8)


def with_crc(q, data):
    """data bits (D - C,) -> (D,) with the CRC behind them"""
    C, poly, init, xorout = q.crc
    if not C:
        return np.asarray(data, np.uint8)
    reg = init
    for b in data:
        top = ((reg >> (C - 1)) & 1) ^ int(b)
        reg = (reg << 1) & ((1 << C) - 1)
        if top:
            reg ^= poly
    reg ^= xorout
    return np.concatenate([np.asarray(data, np.uint8), np.array([(reg >> (C - 1 - k)) & 1 for k in range(C)], np.uint8)])


def frame_of(q, code, seed=0, flips=()):
    """code bits (N,) -> a frame as the bank takes it: packed bytes with `flips` positions inverted, or soft values of
    magnitude 0.5 ... 1.5 / scale"""
    c = np.asarray(code, np.uint8).copy()
    for k in flips:
        c[k] ^= 1
    if q.kind == BITS:
        return np.packbits(c)
    mag = ((splitmix64(seed ^ 0x50F7, len(c)) >> np.uint64(40)).astype(np.float64) / float(1 << 24) + 0.5) * 60.0 / float(q.scale)
    return ((c.astype(np.float64) * 2 - 1) * mag).astype(np.float32)


def clean_block(q, R, cap, seed):
    """(frames (R, cap, FB or N), data bits (R, cap, D)): a clean coded frame with random data (and its CRC) per slot"""
    width = q.FB if q.kind == BITS else q.N
    frames = np.zeros((R, cap, width), np.uint8 if q.kind == BITS else np.float32)
    data = np.zeros((R, cap, q.D), np.uint8)
    for r in range(R):
        for f in range(cap):
            s = seed * 100003 + r * cap + f
            data[r, f] = with_crc(q, random_bits(q.D - q.C, s))
            frames[r, f] = frame_of(q, encode(q, data[r, f]), s)
    return frames, data


# ---- the program ---------------------------------------------------------------------------------------

_EXE = {}


def build_exact(build_dir):
    """g++ -O2 of tests/host/viterbi_ref.cpp -> the program's path (built once per directory)"""
    if build_dir not in _EXE:
        os.makedirs(build_dir, exist_ok=True)
        exe = os.path.join(build_dir, "viterbi_ref")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"),
                               os.path.join(ROOT, "tests", "host", "viterbi_ref.cpp"), "-o", exe])
        _EXE[build_dir] = exe
    return _EXE[build_dir]


def _head(q):
    gens = ([g & 0xFFFFFFFF for g in q.gens] + [0] * 4)[:4]
    u32 = [q.kind, q.K, q.n, *gens, q.inv, q.Lp, q.term, q.D, *q.crc]
    return struct.pack("<15I", *[int(v) & 0xFFFFFFFF for v in u32]) + struct.pack("<Qf", q.pattern & (2 ** 64 - 1), np.float32(q.scale))


def exact(build_dir, cases):
    """cases: [(config, frames (R, cap, FB or N), counts uint32 (R,) or None)] -> [(data (R, cap, DB), info (R, cap))]
    by the program; slots from a row's count up are zero"""
    exe = build_exact(build_dir)
    src, dst = os.path.join(build_dir, "viterbi_cases.bin"), os.path.join(build_dir, "viterbi_out.bin")
    shapes = []
    with open(src, "wb") as f:
        for q, frames, counts in cases:
            frames = np.ascontiguousarray(frames)
            R, cap, width = frames.shape
            assert frames.dtype == (np.uint8 if q.kind == BITS else np.float32) and width == (q.FB if q.kind == BITS else q.N)
            f.write(_head(q) + struct.pack("<qqi", R, cap, int(counts is not None)))
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


def check(build_dir, configs):
    """[config] -> [(accepted, N, T)] by csrc/hz_viterbi_plan.h"""
    exe = build_exact(build_dir)
    src, dst = os.path.join(build_dir, "viterbi_sets.bin"), os.path.join(build_dir, "viterbi_checked.bin")
    with open(src, "wb") as f:
        for q in configs:
            f.write(_head(q))
    subprocess.check_call([exe, "check", src, dst])
    got = np.fromfile(dst, np.uint32).reshape(-1, 3)
    os.remove(src), os.remove(dst)
    assert len(got) == len(configs)
    return [(bool(a), int(n), int(t)) for a, n, t in got]

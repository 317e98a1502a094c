"""The independent restatement of the covariance bank and the beam scan (include/hzsdr_covar.h), the shapes of their
tests and their bounds.

    R_b[i][j] = sum_n a_i[n] conj(a_j[n])             n over block b of B snapshots (the last one as far as it goes)
    p[b][g]   = Re sum_i w_i sum_j Q_b[i][j] conj(w_j)

`covariance` and `scan` evaluate these in complex128 with numpy's own products: the Meaning of the header, NOT its
arithmetic -- no segments, no tree, no real rows.  Beside them the runner of the bit-exact restatement
tests/host/covar_ref.cpp (the program over csrc/hz_covar_math.h and csrc/hz_covar_plan.h whose outputs the device must
reproduce bit for bit) and a Python transcription of the tree's recursive definition.

The bound of the bank, per component of R_b[i][j], with u = 2^-24, nseg the block's segments, L = ceil(log2 nseg) and
A = sum_n |a_i[n]| |a_j[n]|:

  * A component is a sum of 2 n_present products of real rows: Re = sum (re_i re_j + im_i im_j), Im = sum (im_i re_j -
    re_i im_j).  By Cauchy-Schwarz |re_i re_j| + |im_i im_j| <= |a_i| |a_j| and |im_i re_j| + |re_i im_j| <= |a_i| |a_j|:
    the absolute values of the products of one component sum to at most A.  The padding contributes exact zeros.
  * Every product enters a chain of 256 fused steps (its own rounding is the step's): on its way out of the segment it
    passes through at most 256 roundings.                                                                       [256]
  * The tree has depth L -- T(lo, hi) splits at the largest power of two p strictly below n = hi - lo, the left part is
    balanced with depth log2 p, the right part has at most p segments and, by induction, depth at most log2 p, so the
    depth is 1 + log2 p = ceil(log2 n) -- one rounding per level.                                               [L]
  * The combine is one more rounding.                                                                          [1]
  * So every product carries a factor (1 + d)^k with k <= 257 + L and |d| <= u: the error is at most g_k A with
    g_k = k u / (1 - k u).  What is left is second order: g_k - k u <= (k u)^2 / (1 - k u) with k u <= 273 * 2^-24
    = 1.7e-5, under 0.005 u; this restatement's own float64 sums, about 2^-53 (log2 B + 2) A, under 1e-7 u.  One more
    u covers them all.                                                                                          [1]

      |R_float32 - R_float64| <= (256 + L + 2) u A     per component: c = 2

The bound of the scan, with S = sum_i sum_j (|w_i.re| + |w_i.im|) |Q[i][j]| |w_j|:

  * t_i.re and t_i.im are chains of 2N fused steps whose products' absolute values sum to at most T_i = sum_j |Q[i][j]|
    |w_j| (Cauchy-Schwarz again): each is off by at most g_2N T_i, and is itself at most (1 + g_2N) T_i.
  * p is a chain of 2N fused steps over w_i.re t_i.re and -w_i.im t_i.im: its own roundings give at most
    g_2N (1 + g_2N) S, the errors of the t_i come through as at most g_2N S.
  * Second order: (2N u)^2 terms, under 1e-5 u S; the float64 evaluation, under 1e-7 u S.  One more u covers them.

      |p_float32 - p_float64| <= (4N + 1) u S

No measured constant goes into either."""
import math
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
SEG = 256
FORMATS = ["c64", "u8", "i8", "i16"]
# (N, B): the issue's table
SHAPES = [(2, 1), (4, 256), (4, 257), (3, 1000), (8, 1280), (9, 768), (16, 4096), (16, 1539), (5, 65797), (4, 1 << 20)]
C_BANK = 2


def remainder(b):
    """the odd remainder behind the three blocks (none fits below B = 2)"""
    return (b // 2) | 1 if b > 1 else 0


def stream_length(b):
    return 3 * b + remainder(b)


def cuts(b):
    """push boundaries inside a group of four, inside a segment, around block edges and before the last snapshot"""
    n = stream_length(b)
    c = {3, 261, b + 130, 2 * b + 1, 3 * b - 2, 3 * b + 5, n - 1}
    return sorted(v for v in c if 0 < v < n)


# Carried state, for one tile and for three: (N, B) pushed as [0, 300), [300, B + 300) and the rest, 2 B + 512 snapshots in
# all.  The second push resumes the open block at one finished segment (level 0 of the stack comes in), closes it and
# leaves a new open block with one finished segment (level 0 goes out): the two blocks are walked side by side and use
# the same level.  The third does the same at two segments.  The flush then closes an open block of exactly two
# segments: it resumes, has nothing to compute and only collapses.
CARRY_SHAPES = [(16, 8192), (9, 768), (4, 1000)]


def carry_length(b):
    return 2 * b + 512


def carry_cuts(b):
    return [300, b + 300]


def blocks_after(n, b):
    return n // b


def segments(n_present):
    return -(-n_present // SEG)


def tree_shape(lo, hi):
    """the recursive definition, as nested tuples of segment indices"""
    if hi - lo == 1:
        return lo
    p = 1
    while p * 2 < hi - lo:
        p *= 2
    return (tree_shape(lo, lo + p), tree_shape(lo + p, hi))


def tree_sum(g):
    """the recursive definition over float32 values"""
    def t(lo, hi):
        if hi - lo == 1:
            return np.float32(g[lo])
        p = 1
        while p * 2 < hi - lo:
            p *= 2
        return np.float32(t(lo, lo + p) + t(lo + p, hi))
    return t(0, len(g))


def covariance(x, b):
    """x: (N, n) complex64, converted -> (ceil(n / B), N, N) complex128, the open block included"""
    x = np.asarray(x, np.complex64).astype(np.complex128)
    n = x.shape[1]
    return np.stack([x[:, s:s + b] @ x[:, s:s + b].conj().T for s in range(0, n, b)]) if n else np.zeros((0,) + (x.shape[0],) * 2, np.complex128)


def bank_bound(x, b):
    """(256 + L + c) u sum_n |a_i| |a_j| per block and entry: (blocks, N, N) float64, a bound on each component"""
    a = np.abs(np.asarray(x, np.complex64).astype(np.complex128))
    n = a.shape[1]
    out = []
    for s in range(0, n, b):
        blk = a[:, s:s + b]
        nseg = segments(blk.shape[1])
        lg = math.ceil(math.log2(nseg)) if nseg > 1 else 0
        out.append((SEG + lg + C_BANK) * U * (blk @ blk.T))
    return np.stack(out)


def scan(q, w):
    """q: (mats, N, N), w: (G, N) -> (mats, G) float64"""
    q = np.asarray(q, np.complex64).astype(np.complex128)
    w = np.asarray(w, np.complex64).astype(np.complex128)
    return np.einsum("gi,bij,gj->bg", w, q, w.conj()).real


def scan_bound(q, w):
    """(4N + 1) u sum_ij (|w_i.re| + |w_i.im|) |Q_ij| |w_j|: (mats, G)"""
    q = np.abs(np.asarray(q, np.complex64).astype(np.complex128))
    w = np.asarray(w, np.complex64).astype(np.complex128)
    n = w.shape[1]
    return (4 * n + 1) * U * np.einsum("gi,bij,gj->bg", np.abs(w.real) + np.abs(w.imag), q, np.abs(w))


def converted(fmt, raw):
    """hzsdr_convert's conversion of raw rows (N, n[, 2]) to complex64, by the CPU oracle"""
    if fmt == "c64":
        return np.ascontiguousarray(raw, np.complex64)
    import oracle as orc
    out = np.zeros(raw.shape[:2], np.complex64)
    for i in range(raw.shape[0]):
        orc.convert(out[i], np.ascontiguousarray(raw[i]))
    return out


_EXE = {}


def build_exact(build_dir):
    """g++ -O2 -ffp-contract=off of tests/host/covar_ref.cpp -> the program's path (built once per directory)"""
    if build_dir not in _EXE:
        os.makedirs(build_dir, exist_ok=True)
        exe = os.path.join(build_dir, "covar_ref")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"),
                               os.path.join(ROOT, "tests", "host", "covar_ref.cpp"), "-o", exe])
        _EXE[build_dir] = exe
    return _EXE[build_dir]


def _run(build_dir, records, sizes, jobs=8):
    """records: the packed cases; sizes: the bytes each answers with.  The cases are dealt to up to `jobs` runs of the
    program side by side, largest first -> the answers, in order"""
    exe = build_exact(build_dir)
    order = sorted(range(len(records)), key=lambda k: -len(records[k]))
    lanes = [[] for _ in range(max(1, min(jobs, len(records))))]
    load = [0] * len(lanes)
    for k in order:
        at = load.index(min(load))
        lanes[at].append(k)
        load[at] += len(records[k])
    procs = []
    for at, lane in enumerate(lanes):
        src, dst = os.path.join(build_dir, f"covar_cases_{at}.bin"), os.path.join(build_dir, f"covar_out_{at}.bin")
        with open(src, "wb") as f:
            for k in lane:
                f.write(records[k])
        procs.append((subprocess.Popen([exe, "run", src, dst]), src, dst, lane))
    out = [None] * len(records)
    for proc, src, dst, lane in procs:
        assert proc.wait() == 0, "covar_ref failed: its two evaluations differ, or a bad case"
        raw, off = open(dst, "rb").read(), 0
        for k in lane:
            out[k] = raw[off:off + sizes[k]]
            off += sizes[k]
        assert off == len(raw)
        os.remove(src), os.remove(dst)
    return out


def exact(build_dir, cases):
    """cases: [(B, x (N, n) complex64 converted, cuts)] -> [R (ceil(n / B), N, N) complex64, the flushed block
    included], by the program, which also checks its two evaluations against each other bit for bit"""
    records, sizes = [], []
    for b, x, cut in cases:
        x = np.ascontiguousarray(x, np.complex64)
        n_ch, n = x.shape
        records.append(struct.pack("<iiiiq", 0, n_ch, b, len(cut), n) + x.tobytes() + np.asarray(list(cut), np.int64).tobytes())
        sizes.append(8 + 8 * n_ch * n_ch * -(-n // b))
    out = []
    for (b, x, cut), raw in zip(cases, _run(build_dir, records, sizes)):
        n_ch, n = x.shape
        (blocks,) = struct.unpack_from("<q", raw, 0)
        assert blocks == -(-n // b)
        out.append(np.frombuffer(raw, np.complex64, blocks * n_ch * n_ch, 8).reshape(blocks, n_ch, n_ch).copy())
    return out


def exact_scan(build_dir, cases):
    """cases: [(q (mats, N, N) complex64, w (G, N) complex64)] -> [p (mats, G) float32] by the program"""
    records, sizes = [], []
    for q, w in cases:
        q, w = np.ascontiguousarray(q, np.complex64), np.ascontiguousarray(w, np.complex64)
        records.append(struct.pack("<iiiiq", 1, w.shape[1], w.shape[0], q.shape[0], 0) + w.tobytes() + q.tobytes())
        sizes.append(4 * q.shape[0] * w.shape[0])
    return [np.frombuffer(raw, np.float32).reshape(q.shape[0], w.shape[0]).copy() for (q, w), raw in zip(cases, _run(build_dir, records, sizes))]


# ---- exact float32 arithmetic for the cases that settle the order inside the matrix instruction ------------------------
def round_f32(v):
    """a Fraction -> the nearest float32 (ties to even), as a Fraction; the values used stay inside the normal range"""
    from fractions import Fraction
    if v == 0:
        return Fraction(0)
    s, a = (-1 if v < 0 else 1), abs(v)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    q = Fraction(2) ** (e - 23)  # the spacing of float32 in [2^e, 2^(e+1))
    k = a / q
    f = k.numerator // k.denominator
    r = k - f
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and f % 2 == 1):
        f += 1
    return s * f * q


def fused_chain(pairs):
    """acc = fmaf(a, b, acc) from +0 over the pairs, exactly rounded -> Fraction"""
    from fractions import Fraction
    acc = Fraction(0)
    for a, b in pairs:
        acc = round_f32(Fraction(a) * Fraction(b) + acc)
    return acc


def unfused_chain(pairs):
    """acc = acc + round(a b): two roundings per term"""
    from fractions import Fraction
    acc = Fraction(0)
    for a, b in pairs:
        acc = round_f32(acc + round_f32(Fraction(a) * Fraction(b)))
    return acc

"""The independent restatement of the tuner bank's definition (include/hzsdr_tuner.h), its counts and its bound.

    y_k[m] = sum_{q < Q} h[q] c(x[m D - q]) exp(-2 pi i ((w_k (m D - q)) mod 2^32) / 2^32)

in complex128 with exact integer phases -- the Meaning of the header, NOT its three steps: no modulated taps, no tables,
no rotator.  Beside it, the runner of the bit-exact restatement tests/host/tuner_ref.cpp (the program over
csrc/hz_tuner_math.h whose outputs the device must reproduce bit for bit).

The bound of the float32 contract against this restatement, per output, as a complex modulus, with u = 2^-24,
S = sum |h| and M = max (|a.re| + |a.im|) over the samples of the stream:

  * One rounding per component of G: G~ = G + d, |d| <= u |h[q]|; the sum moves by |sum d_q a_q| <= u S M.   [1]
  * Step 2 is, per component, a chain of n = 2 Qp fused steps: its result is sum t_j (1 + e_j), |e_j| <= g_n =
    n u / (1 - n u).  The error vector has |e.re| <= g_n sum_q (|g.re a.re| + |g.im a.im|) and |e.im| <= g_n sum_q
    (|g.im a.re| + |g.re a.im|); the vector v_q of the two bracketed sums has |v_q|^2 = |g|^2 |a|^2 + 4 |g.re g.im a.re
    a.im| <= |g|^2 (|a.re| + |a.im|)^2, so |e| <= g_n sum |g~_q| M <= g_n (1 + u) S M.                         [2 Qp]
  * Each table entry is a unit value rounded per component: relative error u, three of them.                 [3]
  * cmul(a, b): the inner product of each component is rounded (u |a.im| |b.x|) and the fused step rounds the component
    (u |component|): as a modulus 2 u |a| |b|, three cmuls -- two for r, one for y = s r, |s| <= S M.          [6]
  * What is left is second order: g_n - n u <= n u (n u) with n u <= 2048 * 2^-24 = 1.3e-4, under 0.25 u for
    n = 2048; the products of the first-order terms, about (2 Qp + 10) u * 10 u, under 0.002 u; the float64 evaluation of
    cos and sin behind G and the tables and this restatement's own complex128 sum, about 1e-16 Q, under 1e-5 u.  One
    more u covers them all.                                                                                  [1]

      |y_float32 - y_float64| <= (2 Qp + 11) u S M

No measured constant goes into it."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
BOUND_C = 11
N_T2, N_T1, N_T0 = 2048, 2048, 1024
# (K, Q, D) of the GPU tests (tests/test_gpu_tuner.py); tests/test_tuner_cpu.py checks the bound of the contract alone
# over the same list
SHAPES = [(1, 1, 1), (1, 2, 1), (3, 7, 3), (8, 64, 5), (9, 33, 2), (17, 129, 16), (5, 1024, 256), (256, 16, 1), (16, 1023, 255)]
SPECIAL_WORDS = [0, 1, 1 << 31, (1 << 32) - 1, 1 << 21, 1 << 10]


def outputs_after(n, down):
    """ceil(N / D): the outputs written once N samples have been pushed"""
    return -(-n // down)


def total_outputs(n, ntaps, down):
    """the whole stream's outputs, pushes and flush: ceil((N - 1 + Q) / D); none for N = 0"""
    return -(-(n - 1 + ntaps) // down) if n > 0 else 0


def words_for(k, seed=0):
    """k frequency words: the special ones first (as many as fit), then random ones"""
    rng = np.random.default_rng(77 + seed)
    w = SPECIAL_WORDS[:k] + [int(v) for v in rng.integers(0, 1 << 32, size=max(0, k - len(SPECIAL_WORDS)), dtype=np.uint64)]
    return np.array(w, np.uint32)


def taps_of(q, seed=0):
    """q float32 taps of both signs, sum |h| about 1"""
    h = np.random.default_rng(1000 * q + seed).standard_normal(q)
    return (h / np.abs(h).sum()).astype(np.float32) if q > 1 else np.ones(1, np.float32)


def unit(u):
    """exp(+2 pi i u / 2^32) of integer phases u (any integers) in complex128, exact on the axes: the phase is reduced
    to an octant in integers before the float64 cos and sin."""
    u = np.mod(np.asarray(u, np.int64), 1 << 32)
    quad, r = u >> 30, u & ((1 << 30) - 1)
    mirror = r > (1 << 29)
    t = np.where(mirror, (1 << 30) - r, r).astype(np.float64) * (2.0 * np.pi / 4294967296.0)
    a, b = np.where(r == 0, 1.0, np.cos(t)), np.where(r == 0, 0.0, np.sin(t))
    c, s = np.where(mirror, b, a), np.where(mirror, a, b)
    z = c + 1j * s
    return z * np.array([1, 1j, -1, -1j], np.complex128)[quad]


def tune(words, h, x, down):
    """the whole stream of complex64 samples x (already converted) -> (K, count) complex128"""
    h = np.asarray(h, np.float64)
    x = np.asarray(x, np.complex64).astype(np.complex128)
    n, q, d = x.shape[0], h.shape[0], int(down)
    count = total_outputs(n, q, d)
    xp = np.concatenate([np.zeros(q - 1, np.complex128), x, np.zeros(q + d, np.complex128)])
    at = np.arange(count, dtype=np.int64) * d  # m D
    y = np.zeros((len(words), count), np.complex128)
    for k, w in enumerate(int(v) for v in words):
        acc = np.zeros(count, np.complex128)
        for j in range(q):
            acc += h[j] * xp[at - j + (q - 1)] * np.conj(unit(w * (at - j)))
        y[k] = acc
    return y


def bound(h, x):
    """(2 Qp + 11) u sum|h| max(|a.re| + |a.im|): the docstring's derivation"""
    h = np.asarray(h, np.float64)
    x = np.asarray(x, np.complex64)
    qp = (h.shape[0] + 1) // 2 * 2
    m = float((np.abs(x.real.astype(np.float64)) + np.abs(x.imag.astype(np.float64))).max()) if x.shape[0] else 0.0
    return (2 * qp + BOUND_C) * U * float(np.abs(h).sum()) * m


def modulated_taps(w, h):
    """step 1 in float64, NOT rounded: h[q] exp(+2 pi i ((w q) mod 2^32) / 2^32), padded to Qp"""
    h = np.asarray(h, np.float64)
    g = h * unit(int(w) * np.arange(h.shape[0], dtype=np.int64))
    return np.concatenate([g, np.zeros(h.shape[0] % 2, np.complex128)])


def tables():
    """(T2, T1, T0) in complex128, not rounded"""
    return (np.conj(unit(np.arange(N_T2, dtype=np.int64) << 21)), np.conj(unit(np.arange(N_T1, dtype=np.int64) << 10)),
            np.conj(unit(np.arange(N_T0, dtype=np.int64))))


_EXE = {}


def build_exact(build_dir):
    """g++ -O2 -ffp-contract=off of tests/host/tuner_ref.cpp -> the program's path (built once per directory)"""
    if build_dir not in _EXE:
        os.makedirs(build_dir, exist_ok=True)
        exe = os.path.join(build_dir, "tuner_ref")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"),
                               os.path.join(ROOT, "tests", "host", "tuner_ref.cpp"), "-o", exe])
        _EXE[build_dir] = exe
    return _EXE[build_dir]


def exact(build_dir, cases):
    """cases: [(words, down, taps, x complex64, operands)] with operands None (the program makes the modulated taps and
    the tables itself) or (G (K, Qp) complex64, T2, T1, T0) as read out of the library
    -> [(y (K, count) complex64, G (K, Qp) complex64, tables (5120,) complex64)], by the program"""
    exe = build_exact(build_dir)
    src, dst = os.path.join(build_dir, "tuner_cases.bin"), os.path.join(build_dir, "tuner_out.bin")
    with open(src, "wb") as f:
        for words, down, taps, x, ops in cases:
            words, taps, x = np.ascontiguousarray(words, np.uint32), np.ascontiguousarray(taps, np.float32), np.ascontiguousarray(x, np.complex64)
            f.write(struct.pack("<iiiiq", words.shape[0], down, taps.shape[0], int(ops is not None), x.shape[0]))
            f.write(words.tobytes())
            f.write(taps.tobytes())
            if ops is not None:
                qp = (taps.shape[0] + 1) // 2 * 2
                g = np.ascontiguousarray(ops[0], np.complex64)
                assert g.shape == (words.shape[0], qp) and [len(t) for t in ops[1:]] == [N_T2, N_T1, N_T0]
                f.write(g.tobytes())
                for t in ops[1:]:
                    f.write(np.ascontiguousarray(t, np.complex64).tobytes())
            f.write(x.tobytes())
    subprocess.check_call([exe, "run", src, dst])
    out, raw, off = [], open(dst, "rb").read(), 0
    for words, down, taps, x, ops in cases:
        k, qp = len(words), (len(taps) + 1) // 2 * 2
        (count,) = struct.unpack_from("<q", raw, off)
        assert count == total_outputs(len(x), len(taps), down)
        off += 8
        y = np.frombuffer(raw, np.complex64, k * count, off).reshape(k, count).copy()
        off += 8 * k * count
        g = np.frombuffer(raw, np.complex64, k * qp, off).reshape(k, qp).copy()
        off += 8 * k * qp
        t = np.frombuffer(raw, np.complex64, N_T2 + N_T1 + N_T0, off).copy()
        off += 8 * (N_T2 + N_T1 + N_T0)
        out.append((y, g, t))
    assert off == len(raw)
    os.remove(src), os.remove(dst)
    return out

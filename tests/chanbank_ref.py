"""The independent restatement of the channel bank's definition (include/hzsdr_chanbank.h), its counts and its bound.

    y[j][k] = sum_{i < L} g[i] c(x[jD + i]) exp(-2 pi i ((k (jD + i)) mod M) / M)

`definition` evaluates this term by term in complex128, the phase reduced mod M in integers -- the Meaning of the
header, NOT its three steps: no fold, no table.  `fold_dft` is the float64 fold followed by the float64 DFT (the three
steps without their roundings), cheap enough for every shape; tests/test_chanbank_cpu.py holds it against `definition`
on the small shapes.  Beside them the runner of the bit-exact restatement tests/host/chanbank_ref.cpp (the program over
csrc/hz_chanbank_math.h and csrc/hz_chanbank_plan.h whose outputs the device must reproduce bit for bit).

The bound of the float32 contract against this restatement, per output, as a complex modulus, with u = 2^-24,
S = sum |g| and X = max (|re c(x)| + |im c(x)|) over the samples of the stream.  Write u_r for the fold's output r and
note sum_r sum_p |g[i_p]| = S, and |a| <= |a.re| + |a.im| <= X for every sample a:

  * The fold is, per component, a chain of P fused steps: its error is at most g_P sum_p |g[i_p]| |a_p.comp|,
    g_n = n u / (1 - n u); as a modulus (Minkowski) at most g_P sum_p |g[i_p]| |a_p|.  Through the table, whose
    entries have modulus at most 1 + u, and summed over r: g_P S X.                                             [P]
  * Each table entry is a unit value rounded per component: |dW| <= u.  The sum moves by at most
    u sum_r |u_r| <= u S X.                                                                                     [1]
  * The product is, per component, a chain of n = 2 Mp fused steps: its result is sum t_j (1 + e_j), |e_j| <= g_n.
    The error vector has |e.re| <= g_n sum_r (|w.re a.re| + |w.im a.im|) and |e.im| <= g_n sum_r (|w.im a.re| +
    |w.re a.im|), a = u_r; the vector v_r of the two bracketed sums has |v_r|^2 = |w|^2 |a|^2 + 4 |w.re w.im a.re a.im|
    <= |w|^2 (|a.re| + |a.im|)^2, and |u_r.re| + |u_r.im| <= sum_p |g[i_p]| (|a_p.re| + |a_p.im|) <= sum_p |g[i_p]| X,
    so |e| <= g_n S X.                                                                                          [2 Mp]
  * What is left is second order: g_n - n u <= (n u)^2 with n u <= 512 * 2^-24 = 3.1e-5, under 0.02 u; the products of
    the first-order terms, about (2 Mp + P) u * (P + 1) u, under 0.001 u; the float64 evaluation of cos and sin behind
    the table and this restatement's own complex128 sums, about 1e-16 L, under 1e-4 u.  One more u covers them all.  [1]

      |y_float32 - y_float64| <= (2 Mp + P + 2) u S X

The sum |u_r.re| + |u_r.im| is bounded through X directly, so the derivation needs no factor sqrt(2) in front: this is
the derived constant, smaller than (2 Mp + P + 2) sqrt(2).  No measured constant goes into it."""
import math
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
CHANNELS = [2, 3, 7, 8, 12, 16, 17, 100, 128, 255]
TAPS_PER_CHANNEL = [1, 3, 32]
FORMATS = ["c64", "u8", "i8", "i16"]


def coprime_hop(m):
    """a hop coprime to M strictly between 1 and M (the first at or above 0.6 M); None for M = 2, which has none"""
    for d in range(max(2, math.ceil(0.6 * m)), m):
        if math.gcd(d, m) == 1:
            return d
    return None


def hops(m):
    return [d for d in (1, coprime_hop(m), m) if d is not None]


# (M, P, D) of the CPU comparison and of the GPU tests
SHAPES = [(m, p, d) for m in CHANNELS for p in TAPS_PER_CHANNEL for d in hops(m)]


def tile_frames(m):
    """the frames of one workgroup's tile: 64 where 2 Mp 65 floats fit 66 KiB of LDS (M <= 128), 32 above; the GPU
    tests take it from plan()"""
    return 64 if m <= 128 else 32


def frames_after(n, ntaps, hop):
    """frames that exist once n samples have been pushed"""
    return (n - ntaps) // hop + 1 if n >= ntaps else 0


def taps_of(m, p, seed=0):
    """P M float32 taps of both signs, sum |g| about 1"""
    g = np.random.default_rng(1000 * m + p + seed).standard_normal(m * p)
    return (g / np.abs(g).sum()).astype(np.float32)


def pos(k, m, negative_first):
    """the output position of channel k"""
    return (k + m // 2) % m if negative_first else k


def positions(m, negative_first):
    return np.array([pos(k, m, negative_first) for k in range(m)])


def unit(n, m):
    """exp(-2 pi i n / M) of integer phases n (any integers) in complex128, the phase reduced mod M in integers"""
    n = np.mod(np.asarray(n, np.int64), m)
    return np.exp(-2j * np.pi * n.astype(np.float64) / m)


def table(m):
    """W[k][r] in complex128, not rounded: an evaluation of its own (numpy's exp behind the integer reduction mod M)"""
    k = np.arange(m, dtype=np.int64)
    return unit(np.outer(k, k), m)


def definition(g, x, m, hop):
    """the whole stream of complex64 samples x (already converted) -> (frames, M) complex128, term by term"""
    g = np.asarray(g, np.float64)
    x = np.asarray(x, np.complex64).astype(np.complex128)
    ntaps, frames = g.shape[0], frames_after(x.shape[0], g.shape[0], hop)
    y = np.zeros((frames, m), np.complex128)
    k = np.arange(m, dtype=np.int64)
    for j in range(frames):
        acc = np.zeros(m, np.complex128)
        for i in range(ntaps):
            acc += g[i] * x[j * hop + i] * unit(k * (j * hop + i), m)
        y[j] = acc
    return y


def fold_dft(g, x, m, hop):
    """the same frames as the float64 fold (indexed by absolute time mod M) and the float64 DFT"""
    g = np.asarray(g, np.float64)
    x = np.asarray(x, np.complex64).astype(np.complex128)
    ntaps, frames = g.shape[0], frames_after(x.shape[0], g.shape[0], hop)
    w = table(m)
    y = np.zeros((frames, m), np.complex128)
    i = np.arange(ntaps, dtype=np.int64)
    for j in range(frames):
        u = np.zeros(m, np.complex128)
        np.add.at(u, (j * hop + i) % m, g * x[j * hop:j * hop + ntaps])
        y[j] = w @ u
    return y


def bound(g, x, m):
    """(2 Mp + P + 2) u sum|g| max(|a.re| + |a.im|): the docstring's derivation"""
    g = np.asarray(g, np.float64)
    x = np.asarray(x, np.complex64)
    mp, p = (m + 1) // 2 * 2, g.shape[0] // m
    big = float((np.abs(x.real.astype(np.float64)) + np.abs(x.imag.astype(np.float64))).max()) if x.shape[0] else 0.0
    return (2 * mp + p + 2) * U * float(np.abs(g).sum()) * big


def converted(fmt, raw):
    """hzsdr_convert's conversion of a raw buffer to complex64, by the CPU oracle"""
    if fmt == "c64":
        return np.ascontiguousarray(raw, np.complex64)
    import oracle as orc
    out = np.zeros(raw.shape[0], np.complex64)
    orc.convert(out, raw)
    return out


_EXE = {}


def build_exact(build_dir):
    """g++ -O2 -ffp-contract=off of tests/host/chanbank_ref.cpp -> the program's path (built once per directory)"""
    if build_dir not in _EXE:
        os.makedirs(build_dir, exist_ok=True)
        exe = os.path.join(build_dir, "chanbank_ref")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"),
                               os.path.join(ROOT, "tests", "host", "chanbank_ref.cpp"), "-o", exe])
        _EXE[build_dir] = exe
    return _EXE[build_dir]


def exact(build_dir, cases):
    """cases: [(M, hop, taps, x complex64, cuts, table)] with cuts a list of ascending stream positions at which the
    host transcription of the kernel cuts the stream into pushes, and table None (the program makes it itself) or the
    (M, Mp) complex64 read out of the library -> [(y (frames, M) complex64, ZeroFirst; table (M, Mp) complex64)], by the
    program, which also checks its two evaluations against each other bit for bit"""
    exe = build_exact(build_dir)
    src, dst = os.path.join(build_dir, "chanbank_cases.bin"), os.path.join(build_dir, "chanbank_out.bin")
    with open(src, "wb") as f:
        for m, hop, taps, x, cuts, tab in cases:
            taps, x = np.ascontiguousarray(taps, np.float32), np.ascontiguousarray(x, np.complex64)
            assert taps.shape[0] % m == 0
            f.write(struct.pack("<iiiiiq", m, taps.shape[0] // m, hop, int(tab is not None), len(cuts), x.shape[0]))
            f.write(taps.tobytes())
            if tab is not None:
                tab = np.ascontiguousarray(tab, np.complex64)
                assert tab.shape == (m, (m + 1) // 2 * 2)
                f.write(tab.tobytes())
            f.write(x.tobytes())
            f.write(np.asarray(list(cuts), np.int64).tobytes())
    subprocess.check_call([exe, "run", src, dst])
    out, raw, off = [], open(dst, "rb").read(), 0
    for m, hop, taps, x, cuts, tab in cases:
        mp = (m + 1) // 2 * 2
        (frames,) = struct.unpack_from("<q", raw, off)
        assert frames == frames_after(len(x), len(taps), hop)
        off += 8
        y = np.frombuffer(raw, np.complex64, frames * m, off).reshape(frames, m).copy()
        off += 8 * frames * m
        t = np.frombuffer(raw, np.complex64, m * mp, off).reshape(m, mp).copy()
        off += 8 * m * mp
        out.append((y, t))
    assert off == len(raw)
    os.remove(src), os.remove(dst)
    return out

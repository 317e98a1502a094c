"""The independent restatement of the symbol-timing recovery bank's definition (include/hzsdr_symsync.h) in float64, the
signal maker of its tests, and the runner of the bit-exact restatement tests/host/symsync_ref.cpp (the program over
csrc/hz_symsync_math.h whose symbols, counts and state the device must reproduce bit for bit).

The float64 restatement is written from the header's text, not from the C++: a branching loop, the interpolator in its
Lagrange-basis form (the contract evaluates the power form by Horner's rule: another arrangement, the same cubic)."""
import math
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL_F32 = 32
FORM_PER_ROW, FORM_COMPLEX = 1, 2
MAX_ROWS = 8192


def loop_constants(params):
    """(sps, limit, g_mu, g_omega) float32 -> (h0, hmin, hmax) float32, each computed in float64 and rounded"""
    sps, limit = float(np.float32(params[0])), float(np.float32(params[1]))
    h0 = sps / 2.0
    return np.float32(h0), np.float32(h0 * (1.0 - limit)), np.float32(h0 * (1.0 + limit))


def accepted(params):
    """the header's validation, restated"""
    q = np.asarray(params, np.float32)
    if not np.isfinite(q).all():
        return False
    sps, limit, g_mu, g_omega = (float(v) for v in q)
    if not (2.0 < sps <= 256.0 and 0.0 <= limit <= 0.25 and g_mu >= 0.0 and g_omega >= 0.0):
        return False
    _, hmin, _ = loop_constants(q)
    return bool(np.float32(hmin - q[2]) >= np.float32(1.0))  # one float32 subtraction, as the kernel's fmaf(g_mu, -1, hmin)


def max_symbols(n, params):
    """the header's output bound: floor(n / (2 amin)) + 2, amin the smallest hmin - g_mu in float64 less 2^-20 relative"""
    if n == 0:
        return 0
    q = np.asarray(params, np.float32).reshape(-1, 4)
    amin = min(float(loop_constants(p)[1]) - float(p[2]) for p in q)
    return int(math.floor(n / (2.0 * amin * (1.0 - 2.0 ** -20)))) + 2


def lagrange(x3, x2, x1, x0, mu):
    """the cubic through (-1, x3), (0, x2), (1, x1), (2, x0) at mu, by its Lagrange basis"""
    return (-mu * (mu - 1.0) * (mu - 2.0) / 6.0 * x3 + (mu + 1.0) * (mu - 1.0) * (mu - 2.0) / 2.0 * x2
            - (mu + 1.0) * mu * (mu - 2.0) / 2.0 * x1 + (mu + 1.0) * mu * (mu - 1.0) / 6.0 * x0)


def float64(params, x):
    """One row x (real or complex) through the loop in float64 -> (symbols, h at every symbol)."""
    q = np.asarray(params, np.float32)
    g_mu, g_omega = float(q[2]), float(q[3])
    h0, hmin, hmax = (float(v) for v in loop_constants(q))
    cplx = np.iscomplexobj(x)
    v = np.asarray(x).astype(np.complex128 if cplx else np.float64)
    c, h, flag = 0.0, h0, 0
    yp = ym = x1 = x2 = x3 = 0.0
    out, hs = [], []
    for x0 in v:
        if c < 1.0:
            y = lagrange(x3, x2, x1, x0, c)
            if flag == 0:
                ym, adv = y, h
            else:
                d = yp - y
                e = d.real * ym.real + d.imag * ym.imag if cplx else d * ym
                e = min(1.0, max(-1.0, e))
                h = min(hmax, max(hmin, h + g_omega * e))
                adv = h + g_mu * e
                out.append(y)
                hs.append(h)
                yp = y
            flag ^= 1
            c += adv
        c -= 1.0
        x3, x2, x1 = x2, x1, x0
    return np.array(out, np.complex128 if cplx else np.float64), np.array(hs)


# ---- the signal ------------------------------------------------------------------------------------

def rc(t, beta=0.5):
    """the raised cosine of roll-off beta at t symbols"""
    t = np.asarray(t, np.float64)
    den = 1.0 - (2.0 * beta * t) ** 2
    safe = np.where(np.abs(den) < 1e-9, 1.0, den)
    v = np.sinc(t) * np.cos(np.pi * beta * t) / safe
    return np.where(np.abs(den) < 1e-9, np.pi / 4.0 * np.sinc(1.0 / (2.0 * beta)), v)


def symbols(count, seed, cplx=False):
    """a_k: +-1, or (+-1 +- i) / sqrt 2, from a seeded generator"""
    rng = np.random.default_rng(seed)
    a = 2.0 * rng.integers(0, 2, count) - 1.0
    if cplx:
        return (a + 1j * (2.0 * rng.integers(0, 2, count) - 1.0)) / math.sqrt(2.0)
    return a


def signal(a, sps_true, off, noise_db=None, seed=0):
    """x[n] = sum_k a_k rc((n + off) / sps_true - k) over +-8 symbols, for every n whose symbols all exist; float32 or
    complex64.  noise_db: white Gaussian noise that far below the unit symbol power (per component for complex rows)."""
    a = np.asarray(a)
    n = np.arange(int((len(a) - 1) * sps_true - off))
    t = (n + off) / sps_true
    k0 = np.floor(t).astype(np.int64)
    x = np.zeros(n.shape, a.dtype)
    for d in range(-8, 10):
        k = k0 + d
        ok = (k >= 0) & (k < len(a))
        x[ok] += a[k[ok]] * rc(t[ok] - k[ok])
    if noise_db is not None:
        rng = np.random.default_rng(seed)
        s = 10.0 ** (noise_db / 20.0)
        w = rng.standard_normal(n.shape) * s
        x = x + (w + 1j * rng.standard_normal(n.shape) * s if np.iscomplexobj(a) else w)
    return x.astype(np.complex64 if np.iscomplexobj(a) else np.float32)


def best_lag(y, a, skip, lags=range(-2, 6)):
    """the lag at which sign(y[k]) (of re and of im for complex rows) matches a[k - lag] most often over k >= skip
    -> (lag, mismatches, symbols compared)"""
    best = None
    for lag in lags:
        k = np.arange(skip, len(y))
        k = k[(k - lag >= 0) & (k - lag < len(a))]
        ref, got = a[k - lag], y[k]
        bad = int((np.sign(got.real) != np.sign(ref.real)).sum())
        if np.iscomplexobj(a):
            bad += int((np.sign(got.imag) != np.sign(ref.imag)).sum())
        if best is None or bad < best[1]:
            best = (lag, bad, len(k))
    return best


# ---- the program -----------------------------------------------------------------------------------

_EXE = {}


def build_exact(build_dir):
    """g++ -O2 -ffp-contract=off of tests/host/symsync_ref.cpp -> the program's path (built once per directory)"""
    if build_dir not in _EXE:
        os.makedirs(build_dir, exist_ok=True)
        exe = os.path.join(build_dir, "symsync_ref")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"),
                               os.path.join(ROOT, "tests", "host", "symsync_ref.cpp"), "-o", exe])
        _EXE[build_dir] = exe
    return _EXE[build_dir]


def state_floats(cplx):
    return 13 if cplx else 8


def exact(build_dir, cases):
    """cases: [(params, x)] or [(params, x, state)] -> [(symbols, counts, state, negative)] by the program.  x: float32
    or complex64, (N,) or (R, N); params: float32 (4,) shared or (R, 4) per row -- or a list [(start, params), ...], the
    parameters in force from sample `start` on (the first start is 0); state: what to start from (get_state's layout,
    (R, 8) or (R, 13)), the initial state without it.  symbols is (R, N // 2 + 2) of x's type, +0 behind a row's
    count; counts uint32 (R,); state float32 (R, 8 or 13); negative: steps that left the counter below 0."""
    exe = build_exact(build_dir)
    src, dst = os.path.join(build_dir, "symsync_cases.bin"), os.path.join(build_dir, "symsync_out.bin")
    shapes = []
    with open(src, "wb") as f:
        for case in cases:
            params, x = case[0], np.asarray(case[1])
            state = case[2] if len(case) > 2 else None
            segs = params if isinstance(params, list) else [(0, params)]
            cplx = np.iscomplexobj(x)
            rows = 1 if x.ndim == 1 else x.shape[0]
            x2 = np.ascontiguousarray(x.reshape(rows, x.shape[-1]), np.complex64 if cplx else np.float32)
            first = np.ascontiguousarray(segs[0][1], np.float32)
            per_row = first.ndim == 2
            assert segs[0][0] == 0 and first.shape[-1] == 4 and (not per_row or first.shape[0] == x2.shape[0])
            f.write(struct.pack("<iiiiqq", 2 if cplx else 1, len(segs), int(per_row), int(state is not None), x2.shape[0], x2.shape[1]))
            for start, p in segs:
                p = np.ascontiguousarray(p, np.float32)
                assert p.shape == first.shape
                f.write(struct.pack("<q", start))
                f.write(p.tobytes())
            if state is not None:
                z = np.ascontiguousarray(state, np.float32)
                assert z.shape == (x2.shape[0], state_floats(cplx))
                f.write(z.tobytes())
            f.write(x2.tobytes())
            shapes.append((x2.shape, cplx))
    subprocess.check_call([exe, "run", src, dst])
    out, raw, off = [], open(dst, "rb").read(), 0
    for (r, n), cplx in shapes:
        pl, cap, zf = (2 if cplx else 1), n // 2 + 2, state_floats(cplx)
        counts = np.frombuffer(raw, np.uint32, r, off).copy()
        off += 4 * r
        y = np.frombuffer(raw, np.float32, r * cap * pl, off).copy()
        off += 4 * r * cap * pl
        z = np.frombuffer(raw, np.float32, r * zf, off).copy().reshape(r, zf)
        off += 4 * r * zf
        (neg,) = struct.unpack_from("<I", raw, off)
        off += 4
        out.append(((y.view(np.complex64) if cplx else y).reshape(r, cap), counts, z, neg))
    assert off == len(raw)
    os.remove(src), os.remove(dst)
    return out


def derive(build_dir, sets):
    """sets (K, 4) float32 -> [(accepted, h0, hmin, hmax, hmin - g_mu in float64)] by csrc/hz_symsync_plan.h"""
    exe = build_exact(build_dir)
    src, dst = os.path.join(build_dir, "symsync_sets.bin"), os.path.join(build_dir, "symsync_derived.bin")
    q = np.ascontiguousarray(sets, np.float32).reshape(-1, 4)
    q.tofile(src)
    subprocess.check_call([exe, "derive", src, dst])
    raw = open(dst, "rb").read()
    os.remove(src), os.remove(dst)
    assert len(raw) == 24 * q.shape[0]
    out = []
    for k in range(q.shape[0]):
        ok, h0, hmin, hmax, least = struct.unpack_from("<ifffd", raw, 24 * k)
        out.append((bool(ok), np.float32(h0), np.float32(hmin), np.float32(hmax), least))
    return out


def bound(build_dir, n, amin):
    """max_symbols(n, amin) of csrc/hz_symsync_plan.h"""
    return int(subprocess.check_output([build_exact(build_dir), "bound", str(int(n)), repr(float(amin))], text=True))

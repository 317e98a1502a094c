"""The independent restatement of the equalizer bank's definition (include/hzsdr_equalizer.h) in numpy float32, the
signal makers of its tests, and the runner of the bit-exact restatement tests/host/equalizer_ref.cpp (the program over
csrc/hz_equalizer_math.h whose outputs, track and state the device must reproduce bit for bit).

The numpy restatement is written from the header's text, not from the C++: the taps of a row are one array, every
product and sum is a float32 operation of numpy, and fmaf is emulated through float64 (fmaf below, with the argument
why it rounds once)."""
import math
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL_F32, C64 = 32, 1
CMA, DD_BPSK, DD_QPSK = 0, 1, 2
FORM_PER_ROW, FORM_COMPLEX = 1, 2
MAX_ROWS, MAX_TAPS = 8192, 64
LOW, HIGH = 2.0 ** -64, 2.0 ** 64
TILE = 256

f32 = np.float32


def fmaf(a, b, c):
    """fmaf(a, b, c) of float32 arrays, rounded ONCE.  In float64 the product a b is exact (48 bits of 53, and the
    exponents of two float32 stay far inside float64's).  s = p + c is rounded to 53 bits, and err, the two-sum's
    remainder, is exactly p + c - s.  Rounding s to float32 is the single rounding of the exact sum unless s lies
    exactly on the midpoint of two neighbouring float32 while the exact sum does not (every such midpoint is a float64,
    so the exact sum and s lie on the same side of every OTHER midpoint): there err's sign says on which side of the
    midpoint the exact sum lies, and the neighbour on that side is taken instead of the tie's even one."""
    a, b, c = (np.asarray(v, f32).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        r = s.astype(f32)
        d = s - r.astype(np.float64)
        other = np.nextafter(r, np.where(d > 0, np.inf, -np.inf).astype(f32))
        tie = (d != 0) & (np.abs(other.astype(np.float64) - s) == np.abs(d)) & (err != 0)
        # the exact sum lies on `other`'s side of the midpoint when err has d's sign
        return np.where(tie & ((err > 0) == (d > 0)), other, r).astype(f32)


def pow2_up(n):
    p = 1
    while p < n:
        p *= 2
    return p


def accepted(params):
    """the header's validation of a parameter set, restated"""
    q = np.asarray(params, f32)
    if q.shape != (2,) or not np.isfinite(q).all():
        return False
    return 0.0 <= float(q[0]) <= 1.0 and LOW <= float(q[1]) <= HIGH


def geometry_accepted(taps, centre, mode, complex_rows):
    return 1 <= taps <= MAX_TAPS and 0 <= centre < taps and mode in (CMA, DD_BPSK, DD_QPSK) and (mode != DD_QPSK or complex_rows)


def initial_state(rows, taps, centre, complex_rows):
    pl = 2 if complex_rows else 1
    z = np.zeros((rows, (2 * taps - 1) * pl), f32)
    z[:, centre * pl] = 1.0
    return z


def clip(v):
    return np.where(v < f32(-1), f32(-1), np.where(v > f32(1), f32(1), v)).astype(f32)


def restated(mode, taps, centre, params, x, state=None, count=None):
    """One row x (float32 or complex64) through the header's steps in numpy float32 -> (y of x's type, track float32,
    state float32 ((2 taps - 1) * planes,)); `count` symbols are consumed (all without it)."""
    x = np.asarray(x)
    cplx = np.iscomplexobj(x)
    n = len(x) if count is None else min(int(count), len(x))
    mu, level = f32(params[0]), f32(params[1])
    z = initial_state(1, taps, centre, cplx)[0] if state is None else np.array(state, f32)
    np_ = pow2_up(taps)
    with np.errstate(all="ignore"):
        if cplx:
            wr, wi = z[0:2 * taps:2].copy(), z[1:2 * taps:2].copy()
            hr, hi = z[2 * taps::2].copy(), z[2 * taps + 1::2].copy()
            xr, xi = x.real.astype(f32), x.imag.astype(f32)
            y, tr = np.zeros(len(x), np.complex64), np.zeros(len(x), f32)
            for k in range(n):
                Xr, Xi = np.concatenate([[xr[k]], hr]).astype(f32), np.concatenate([[xi[k]], hi]).astype(f32)
                pr, pi = np.zeros(np_, f32), np.zeros(np_, f32)
                pr[:taps] = fmaf(-wi, Xi, wr * Xr)
                pi[:taps] = fmaf(wi, Xr, wr * Xi)
                s = 1
                idx = np.arange(np_)
                while s < np_:
                    pr, pi = pr + pr[idx ^ s], pi + pi[idx ^ s]
                    s *= 2
                yr, yi = pr[0], pi[0]
                if mode == CMA:
                    c = level - fmaf(yi, yi, yr * yr)
                    er, ei = c * yr, c * yi
                else:
                    er = np.copysign(level, yr) - yr
                    ei = np.copysign(level, yi) - yi if mode == DD_QPSK else -yi
                er, ei = clip(f32(er)), clip(f32(ei))
                gr, gi = f32(mu * er), f32(mu * ei)
                wr, wi = fmaf(gi, Xi, fmaf(gr, Xr, wr)), fmaf(-gr, Xi, fmaf(gi, Xr, wi))
                y[k] = complex(yr, yi)
                tr[k] = fmaf(ei, ei, er * er)
                hr, hi = Xr[:taps - 1], Xi[:taps - 1]
            out = np.empty((2 * taps - 1) * 2, f32)
            out[0:2 * taps:2], out[1:2 * taps:2], out[2 * taps::2], out[2 * taps + 1::2] = wr, wi, hr, hi
            return y, tr, out
        w, h = z[:taps].copy(), z[taps:].copy()
        xs = x.astype(f32)
        y, tr = np.zeros(len(x), f32), np.zeros(len(x), f32)
        for k in range(n):
            X = np.concatenate([[xs[k]], h]).astype(f32)
            p = np.zeros(np_, f32)
            p[:taps] = w * X
            s = 1
            idx = np.arange(np_)
            while s < np_:
                p = p + p[idx ^ s]
                s *= 2
            yy = p[0]
            e = (level - yy * yy) * yy if mode == CMA else np.copysign(level, yy) - yy
            e = clip(f32(e))
            g = f32(mu * e)
            w = fmaf(g, X, w)
            y[k], tr[k] = yy, e * e
            h = X[:taps - 1]
        return y, tr, np.concatenate([w, h]).astype(f32)


# ---- the signals -----------------------------------------------------------------------------------

CHANNEL = np.array([0.2 - 0.1j, 1.0, 0.45 + 0.3j, -0.2 + 0.15j])


def white(shape, seed, complex_rows=True, scale=0.5):
    """white samples, components uniform in [-scale, scale): complex64, or float32 where not complex_rows"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape)) * (2 if complex_rows else 1)
    f = (rng.uniform(-scale, scale, n)).astype(f32)
    return (f.view(np.complex64) if complex_rows else f).reshape(shape)


def qpsk_through_channel(n, seed, h=CHANNEL, sigma=0.02):
    """-> (received complex64 (n,), the symbols sent complex128 (n,)): n QPSK symbols (+-1 +-i) / sqrt 2 from
    default_rng(seed) through h (received[k] = sum_j h[j] sent[k - j]) plus complex Gaussian noise of deviation sigma per
    component"""
    rng = np.random.default_rng(seed)
    a = ((2.0 * rng.integers(0, 2, n) - 1.0) + 1j * (2.0 * rng.integers(0, 2, n) - 1.0)) / math.sqrt(2.0)
    r = np.convolve(a, h)[:n] + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return r.astype(np.complex64), a


def sign_errors(y, sent, delays=range(4, 9), rotations=True):
    """the fewest wrong sign decisions (a symbol is wrong where either component's sign differs) of y against `sent`
    over the delays and, with `rotations`, the four rotations by a quarter turn -> (errors, delay, rotation)"""
    best = None
    y = np.asarray(y).astype(np.complex128)
    for d in delays:
        a = sent[:len(sent) - d] if d else sent
        for q in (range(4) if rotations else (0,)):
            v = y[d:] * (1j ** q)
            bad = int(((np.sign(v.real) != np.sign(a.real)) | (np.sign(v.imag) != np.sign(a.imag))).sum())
            if best is None or bad < best[0]:
                best = (bad, d, q)
    return best


def converge(run, r, a):
    """run(mode, taps, centre, params, x[, state]) -> (y (1, n), track, state (1, 42)) -> (wrong decisions unequalized,
    behind CMA, behind DD; the largest |w| of the CMA taps)"""
    y, _, z = run(CMA, 11, 5, np.array([0.01, 1.0], np.float32), r)
    raw = sign_errors(r[4000:], a[4000:], delays=range(0, 4), rotations=False)[0]
    cma = sign_errors(y[0][4000:], a[4000:])[0]
    state = np.zeros((1, 42), np.float32)
    state[0, :22] = z[0][:22]
    y2, _, _ = run(DD_QPSK, 11, 5, np.array([0.01, math.sqrt(0.5)], np.float32), r[3000:], state)
    dd = sign_errors(y2[0][1000:], a[4000:])[0]
    return raw, cma, dd, float(np.abs(z[0][:22].view(np.complex64)).max())


# ---- the program -----------------------------------------------------------------------------------

_EXE = {}


def build_exact(build_dir):
    """g++ -O2 -ffp-contract=off of tests/host/equalizer_ref.cpp -> the program's path (built once per directory)"""
    if build_dir not in _EXE:
        os.makedirs(build_dir, exist_ok=True)
        exe = os.path.join(build_dir, "equalizer_ref")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"),
                               os.path.join(ROOT, "tests", "host", "equalizer_ref.cpp"), "-o", exe])
        _EXE[build_dir] = exe
    return _EXE[build_dir]


def state_width(taps, complex_rows):
    return (2 * taps - 1) * (2 if complex_rows else 1)


def exact(build_dir, cases):
    """cases: [(mode, taps, centre, params, x)], [(..., x, state)] or [(..., x, state, counts)] -> [(y, track, state)] by
    the program.  x: float32 or complex64, (W,) or (R, W); params: float32 (2,) shared or (R, 2) per row; state: the state
    to start from (float32 (R, (2 taps - 1) * planes)) or None for the initial one; counts: uint32 (R,) or None.  y is of
    x's type (R, W) and track float32 (R, W), zero behind a row's count; state float32 (R, (2 taps - 1) * planes)."""
    exe = build_exact(build_dir)
    tag = f"{os.getpid()}"
    src, dst = os.path.join(build_dir, f"equalizer_cases_{tag}.bin"), os.path.join(build_dir, f"equalizer_out_{tag}.bin")
    shapes = []
    with open(src, "wb") as f:
        for case in cases:
            mode, taps, centre, params, x = case[:5]
            x = np.asarray(x)
            state = case[5] if len(case) > 5 else None
            counts = case[6] if len(case) > 6 else None
            rows = 1 if x.ndim == 1 else x.shape[0]
            cplx = np.iscomplexobj(x)
            assert x.dtype in (np.float32, np.complex64)
            x2 = np.ascontiguousarray(x.reshape(rows, x.shape[-1]))
            p = np.ascontiguousarray(params, np.float32)
            per_row = p.ndim == 2
            assert p.shape[-1] == 2 and (not per_row or p.shape[0] == rows)
            f.write(struct.pack("<iiiiiiqqqq", int(cplx), mode, int(per_row), int(state is not None), int(counts is not None), 0,
                                rows, x2.shape[1], taps, centre))
            f.write(p.tobytes())
            if state is not None:
                z = np.ascontiguousarray(state, np.float32).reshape(rows, -1)
                assert z.shape == (rows, state_width(taps, cplx))
                f.write(z.tobytes())
            if counts is not None:
                c = np.ascontiguousarray(counts).astype(np.uint32)
                assert c.shape == (rows,)
                f.write(c.tobytes())
            f.write(x2.tobytes())
            shapes.append((rows, x2.shape[1], x2.dtype, state_width(taps, cplx)))
    subprocess.check_call([exe, "run", src, dst])
    out, raw, off = [], open(dst, "rb").read(), 0
    for r, n, dt, zw in shapes:
        y = np.frombuffer(raw, dt, r * n, off).copy().reshape(r, n)
        off += dt.itemsize * r * n
        tr = np.frombuffer(raw, np.float32, r * n, off).copy().reshape(r, n)
        off += 4 * r * n
        z = np.frombuffer(raw, np.float32, r * zw, off).copy().reshape(r, zw)
        off += 4 * r * zw
        out.append((y, tr, z))
    assert off == len(raw)
    os.remove(src), os.remove(dst)
    return out


def check(build_dir, records):
    """records: [(mu, level, taps, centre, mode, complex)] -> [(parameters accepted, geometry accepted)] by
    csrc/hz_equalizer_plan.h"""
    exe = build_exact(build_dir)
    src, dst = os.path.join(build_dir, f"equalizer_sets_{os.getpid()}.bin"), os.path.join(build_dir, f"equalizer_checked_{os.getpid()}.bin")
    with open(src, "wb") as f:
        for mu, level, taps, centre, mode, cplx in records:
            f.write(struct.pack("<ffiiii", mu, level, taps, centre, mode, int(cplx)))
    subprocess.check_call([exe, "check", src, dst])
    raw = open(dst, "rb").read()
    os.remove(src), os.remove(dst)
    assert len(raw) == 8 * len(records)
    return [(bool(a), bool(b)) for a, b in struct.iter_unpack("<ii", raw)]

"""The independent restatement of the AGC bank's definition (include/hzsdr_agc.h) in float64, the signal makers of its
tests, and the runner of the bit-exact restatement tests/host/agc_ref.cpp (the program over csrc/hz_agc_math.h whose
outputs, track and state the device must reproduce bit for bit).

The float64 restatement is written from the header's text, not from the C++: the level is abs() of a Python number, the
step is float64 expressions with the gate as a condition of its own."""
import math
import os
import struct
import subprocess

import numpy as np

from util import splitmix64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL_F32, C64 = 32, 1
FORM_PER_ROW, FORM_COMPLEX = 1, 2
MAX_ROWS = 8192
LOW, HIGH = 2.0 ** -64, 2.0 ** 64
BRANCHES = ("attack", "decay", "clip", "gate", "gmin", "gmax")

# the two sets that together reach every branch of the step on white rows: ref, attack, decay, floor, g0, gmin, gmax
LOUD = np.array([0.25, 0.5, 0.25, 0.2, 1.0, 0.5, 2.0], np.float32)
QUIET = np.array([4.0, 0.5, 0.5, 0.2, 1.0, 0.5, 2.0], np.float32)


def accepted(params):
    """the header's validation, restated"""
    q = np.asarray(params, np.float32)
    if q.shape != (7,) or not np.isfinite(q).all():
        return False
    ref, attack, decay, floor, g0, gmin, gmax = (float(v) for v in q)
    return LOW <= ref <= HIGH and 0.0 <= attack <= 0.5 and 0.0 <= decay <= 0.5 and 0.0 <= floor and LOW <= gmin <= g0 <= gmax <= HIGH


def iref_of(params):
    return np.float32(1.0 / float(np.float32(params[0])))


def rates(attack_samples, decay_samples):
    """1 - exp(-1 / tau) (agc.agc_rates, restated)"""
    return 1.0 - math.exp(-1.0 / attack_samples), 1.0 - math.exp(-1.0 / decay_samples)


def float64(params, x, state=None):
    """One row x (real or complex) through the loop in float64 -> (y, track float64, g)."""
    ref, attack, decay, floor, g0, gmin, gmax = (float(np.float32(v)) for v in params)
    iref = 1.0 / ref
    g = g0 if state is None else float(state)
    v = np.asarray(x)
    v = v.astype(np.complex128 if np.iscomplexobj(v) else np.float64)
    y, track = np.empty_like(v), np.empty(len(v), np.float64)
    for n, xn in enumerate(v):
        a = abs(xn)
        y[n], track[n] = xn * g, g
        e = 1.0 - a * iref * g
        e = -1.0 if e < -1.0 else e
        s = (attack if e < 0.0 else decay) * e
        if s != s or a < floor:
            s = 0.0
        g = g + g * s
        g = gmin if g < gmin else (gmax if g > gmax else g)
    return y, track, g


def settle_bound(level, ref, attack, decay):
    """The samples after which |y| is within 5 % of ref, from g0 = 1 at the constant level `level`: a quiet row's gain
    grows by (1 + decay) per sample until the error is below 1, ln A / ln(1 + decay) samples for A = ref / level, and
    closes the last 5 % at the rate decay, ln 20 / decay; a loud row's falls by (1 - attack) per sample under the clipped
    error, ln A / ln(1 / (1 - attack)) for A = level / ref, then ln 20 / attack.  Times 1.1."""
    if level < ref:
        return 1.1 * (math.log(ref / level) / math.log(1.0 + decay) + math.log(20.0) / decay)
    return 1.1 * (math.log(level / ref) / math.log(1.0 / (1.0 - attack)) + math.log(20.0) / attack)


# ---- the signals -----------------------------------------------------------------------------------

def white(shape, seed, complex_rows=True):
    """white samples, components in [-1, 1): complex64, or float32 where not complex_rows"""
    n = int(np.prod(shape)) * (2 if complex_rows else 1)
    z = splitmix64(seed, n)
    f = ((z >> np.uint64(40)).astype(np.float64) / float(1 << 23) - 1.0).astype(np.float32)
    return (f.view(np.complex64) if complex_rows else f).reshape(shape)


def constant_modulus(n, level, seed, complex_rows=True):
    """n samples of modulus `level`: a complex tone at a seeded frequency and phase, or real +-level at seeded signs"""
    z = splitmix64(seed, n + 2)
    if complex_rows:
        f, p = float(z[0] >> np.uint64(11)) / float(1 << 53) - 0.5, float(z[1] >> np.uint64(11)) / float(1 << 53)
        return (level * np.exp(2j * math.pi * (f * np.arange(n) + p))).astype(np.complex64)
    return (((z[2:] >> np.uint64(63)).astype(np.float64) * 2.0 - 1.0) * level).astype(np.float32)


def noisy_qpsk(n, level, seed, sps=4, noise=0.1):
    """QPSK symbols of modulus `level` held for sps samples, with white uniform noise of deviation noise * level per
    component"""
    z = splitmix64(seed, 2 * (n // sps + 1) + 2 * n)
    bits = (z[:2 * (n // sps + 1)] >> np.uint64(63)).astype(np.float64) * 2.0 - 1.0
    k = np.arange(n)
    a = (bits[0::2][k // sps] + 1j * bits[1::2][k // sps]) / math.sqrt(2.0)
    u = (z[2 * (n // sps + 1):] >> np.uint64(11)).astype(np.float64) / float(1 << 53) * 2.0 - 1.0
    return (level * (a + noise * math.sqrt(3.0) * (u[0::2] + 1j * u[1::2]))).astype(np.complex64)


# ---- the program -----------------------------------------------------------------------------------

_EXE = {}


def build_exact(build_dir):
    """g++ -O2 -ffp-contract=off of tests/host/agc_ref.cpp -> the program's path (built once per directory)"""
    if build_dir not in _EXE:
        os.makedirs(build_dir, exist_ok=True)
        exe = os.path.join(build_dir, "agc_ref")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"),
                               os.path.join(ROOT, "tests", "host", "agc_ref.cpp"), "-o", exe])
        _EXE[build_dir] = exe
    return _EXE[build_dir]


def exact(build_dir, cases, branches=False):
    """cases: [(params, x)] or [(params, x, state)] -> [(y, track, state)] by the program ([(y, track, state, counts)]
    with `branches`: counts is a dict over BRANCHES).  x: float32 or complex64, (N,) or (R, N); params: float32 (7,)
    shared or (R, 7) per row -- or a list [(start, params), ...], the parameters in force from sample `start` on (the
    first start is 0); state: the gains to start from (float32 (R,)), the initial state without it.  y is of x's type
    (R, N), track float32 (R, N), state float32 (R,)."""
    exe = build_exact(build_dir)
    src, dst = os.path.join(build_dir, "agc_cases.bin"), os.path.join(build_dir, "agc_out.bin")
    shapes = []
    with open(src, "wb") as f:
        for case in cases:
            params, x = case[0], np.asarray(case[1])
            state = case[2] if len(case) > 2 else None
            segs = params if isinstance(params, list) else [(0, params)]
            rows = 1 if x.ndim == 1 else x.shape[0]
            cplx = np.iscomplexobj(x)
            assert x.dtype in (np.float32, np.complex64)
            x2 = np.ascontiguousarray(x.reshape(rows, x.shape[-1]))
            first = np.ascontiguousarray(segs[0][1], np.float32)
            per_row = first.ndim == 2
            assert segs[0][0] == 0 and first.shape[-1] == 7 and (not per_row or first.shape[0] == rows)
            f.write(struct.pack("<iiiiqq", int(cplx), len(segs), int(per_row), int(state is not None), rows, x2.shape[1]))
            for start, p in segs:
                p = np.ascontiguousarray(p, np.float32)
                assert p.shape == first.shape
                f.write(struct.pack("<q", start))
                f.write(p.tobytes())
            if state is not None:
                z = np.ascontiguousarray(state, np.float32)
                assert z.shape == (rows,)
                f.write(z.tobytes())
            f.write(x2.tobytes())
            shapes.append((rows, x2.shape[1], x2.dtype))
    subprocess.check_call([exe, "run", src, dst])
    out, raw, off = [], open(dst, "rb").read(), 0
    for r, n, dt in shapes:
        y = np.frombuffer(raw, dt, r * n, off).copy().reshape(r, n)
        off += dt.itemsize * r * n
        tr = np.frombuffer(raw, np.float32, r * n, off).copy().reshape(r, n)
        off += 4 * r * n
        z = np.frombuffer(raw, np.float32, r, off).copy()
        off += 4 * r
        counts = dict(zip(BRANCHES, (int(v) for v in np.frombuffer(raw, np.int64, 6, off))))
        off += 48
        out.append((y, tr, z, counts) if branches else (y, tr, z))
    assert off == len(raw)
    os.remove(src), os.remove(dst)
    return out


def derive(build_dir, sets):
    """sets (K, 7) float32 -> [(accepted, iref)] by csrc/hz_agc_plan.h"""
    exe = build_exact(build_dir)
    src, dst = os.path.join(build_dir, "agc_sets.bin"), os.path.join(build_dir, "agc_derived.bin")
    q = np.ascontiguousarray(sets, np.float32).reshape(-1, 7)
    q.tofile(src)
    subprocess.check_call([exe, "derive", src, dst])
    raw = open(dst, "rb").read()
    os.remove(src), os.remove(dst)
    assert len(raw) == 8 * q.shape[0]
    return [(bool(ok), np.float32(iref)) for ok, iref in struct.iter_unpack("<if", raw)]


def two_channels(nsym, offsets, amplitudes, seed, sps=5, down=4, centres=(0.2, -0.15)):
    """carrier_ref.two_channels with an amplitude per channel: a wide stream that holds one QPSK channel per entry of
    `offsets`, raised-cosine symbols of amplitude `amplitudes[k]` -> (x complex64, the tuners' frequency words uint32,
    the decimation low-pass float32 of unit DC gain, the symbols (K, nsym))."""
    import symsync_ref
    wide = sps * down
    a = np.stack([symsync_ref.symbols(nsym, seed + k, True) for k in range(len(offsets))])
    rows = [symsync_ref.signal(a[k], float(wide), 0.25 * k).astype(np.complex128) for k in range(len(offsets))]
    n = min(len(r) for r in rows)
    t = np.arange(n)
    x = sum(amp * r[:n] * np.exp(2j * math.pi * ((c + off / down) * t + 0.1 + 0.2 * k))
            for k, (r, c, off, amp) in enumerate(zip(rows, centres, offsets, amplitudes)))
    words = np.array([int(round(c * 4294967296.0)) % (1 << 32) for c in centres[:len(offsets)]], np.uint32)
    m = np.arange(65) - 32
    h = np.sinc(m * 2.0 * 0.09) * np.hamming(65)
    return x.astype(np.complex64), words, (h / h.sum()).astype(np.float32), a

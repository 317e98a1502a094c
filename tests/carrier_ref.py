"""The independent restatement of the carrier recovery bank's definition (include/hzsdr_carrier.h) in float64 and Python
integers, the signal maker of its tests, and the runner of the bit-exact restatement tests/host/carrier_ref.cpp (the
program over csrc/hz_carrier_math.h whose outputs, track and state the device must reproduce bit for bit).

The float64 restatement is written from the header's text, not from the C++: the oscillator's unit vector is libm's cos
and sin of the phase word, the product and the detectors are float64 expressions, the phase and the frequency Python
integers."""
import math
import os
import struct
import subprocess

import numpy as np

from util import splitmix64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TONE, BPSK, QPSK = 0, 1, 2
FORM_PER_ROW, FORM_MODE = 1, 2
MAX_ROWS = 8192
TWO32 = 4294967296.0


def loop_constants(params):
    """(alpha, beta, f0, fmin, fmax) float32 -> (alpha_w, beta_w float32; F0, Fmin, Fmax integers), computed in float64"""
    q = [float(np.float32(v)) for v in params]
    rint = lambda v: int(np.rint(v))  # (to nearest, ties to even: llrint in the default rounding mode)
    return np.float32(q[0] * TWO32), np.float32(q[1] * TWO32), rint(q[2] * TWO32), rint(q[3] * TWO32), rint(q[4] * TWO32)


def accepted(params):
    """the header's validation, restated"""
    q = np.asarray(params, np.float32)
    if q.shape != (5,) or not np.isfinite(q).all():
        return False
    alpha, beta, f0, fmin, fmax = (float(v) for v in q)
    return 0.0 <= alpha <= 0.125 and 0.0 <= beta <= 0.125 and -0.25 <= fmin <= f0 <= fmax <= 0.25


def gains(bandwidth, damping=0.7071):
    """the usual second-order formulas (carrier.carrier_gains, restated)"""
    tn = bandwidth / (damping + 1.0 / (4.0 * damping))
    d = 1.0 + 2.0 * damping * tn + tn * tn
    return 4.0 * damping * tn / d / (2.0 * math.pi), 4.0 * tn * tn / d / (2.0 * math.pi)


def _trunc(v):
    return 0 if v != v else int(v)  # (int() truncates toward zero)


def float64(mode, params, x, state=None):
    """One row x (complex) through the loop in float64 -> (y complex128, track float64, (theta, F))."""
    aw, bw, f0, fmin, fmax = loop_constants(params)
    aw, bw = float(aw), float(bw)
    theta, f = (0, f0) if state is None else (int(state[0]), int(state[1]))
    v = np.asarray(x).astype(np.complex128)
    y, track = np.empty(len(v), np.complex128), np.empty(len(v), np.float64)
    for n, xn in enumerate(v):
        ang = 2.0 * math.pi * theta / TWO32
        yn = xn * complex(math.cos(ang), -math.sin(ang))
        yr, yi = yn.real, yn.imag
        if mode == TONE:
            e = yi
        elif mode == BPSK:
            e = yr * yi
        else:
            e = (-yi if yr < 0.0 else yi) - (-yr if yi < 0.0 else yr)
        e = -1.0 if e < -1.0 else (1.0 if e > 1.0 else e)
        f = min(fmax, max(fmin, f + _trunc(bw * e)))
        theta = (theta + f + _trunc(aw * e)) % (1 << 32)
        y[n], track[n] = yn, f / TWO32
    return y, track, (theta, f)


# ---- the signal ------------------------------------------------------------------------------------

def white(shape, seed):
    """white complex64 samples, components in [-1, 1)"""
    n = int(np.prod(shape))
    z = splitmix64(seed, 2 * n)
    f = ((z >> np.uint64(40)).astype(np.float64) / float(1 << 23) - 1.0).astype(np.float32)
    return f.view(np.complex64).reshape(shape)


def signal(mode, n, offset, phase, seed, sps=4, noise=0.0):
    """n complex64 samples of a unit-amplitude tone (TONE), or of BPSK (+-1) / QPSK ((+-1 +- i) / sqrt 2) symbols held
    for `sps` samples each, at a carrier offset of `offset` cycles per sample and a start phase of `phase` radians;
    `noise`: the deviation of white uniform noise per component.  Seeded by splitmix64."""
    k = np.arange(n)
    z = splitmix64(seed, 2 * (n // sps + 1) + 2 * n)
    bits = (z[:2 * (n // sps + 1)] >> np.uint64(63)).astype(np.float64) * 2.0 - 1.0
    if mode == TONE:
        a = np.ones(n, np.complex128)
    elif mode == BPSK:
        a = bits[0::2][k // sps].astype(np.complex128)
    else:
        a = (bits[0::2][k // sps] + 1j * bits[1::2][k // sps]) / math.sqrt(2.0)
    x = a * np.exp(1j * (2.0 * math.pi * offset * k + phase))
    if noise:
        u = (z[2 * (n // sps + 1):] >> np.uint64(11)).astype(np.float64) / float(1 << 53) * 2.0 - 1.0
        x = x + noise * math.sqrt(3.0) * (u[0::2] + 1j * u[1::2])
    return x.astype(np.complex64)


def power_of(mode):
    """the power that removes the detector's ambiguity: y^1, y^2, y^4"""
    return {TONE: 1, BPSK: 2, QPSK: 4}[mode]


def phase_spread(mode, y):
    """the largest distance on the circle, in radians, of the phases of y^m from their mean direction"""
    w = np.asarray(y, np.complex128) ** power_of(mode)
    mean = w.sum()
    return float(np.abs(np.angle(w * np.conj(mean))).max())


# ---- the program -----------------------------------------------------------------------------------

_EXE = {}


def build_exact(build_dir):
    """g++ -O2 -ffp-contract=off of tests/host/carrier_ref.cpp -> the program's path (built once per directory)"""
    if build_dir not in _EXE:
        os.makedirs(build_dir, exist_ok=True)
        exe = os.path.join(build_dir, "carrier_ref")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"),
                               os.path.join(ROOT, "tests", "host", "carrier_ref.cpp"), "-o", exe])
        _EXE[build_dir] = exe
    return _EXE[build_dir]


def exact(build_dir, cases):
    """cases: [(mode, params, x)] or [(mode, params, x, state)] -> [(y, track, state)] by the program.  x: complex64, (N,)
    or (R, N); params: float32 (5,) shared or (R, 5) per row -- or a list [(start, params), ...], the parameters in
    force from sample `start` on (the first start is 0); state: what to start from (uint32 (R, 2)), the initial state
    without it.  y is complex64 (R, N), track float32 (R, N), state uint32 (R, 2)."""
    exe = build_exact(build_dir)
    src, dst = os.path.join(build_dir, "carrier_cases.bin"), os.path.join(build_dir, "carrier_out.bin")
    shapes = []
    with open(src, "wb") as f:
        for case in cases:
            mode, params, x = case[0], case[1], np.asarray(case[2])
            state = case[3] if len(case) > 3 else None
            segs = params if isinstance(params, list) else [(0, params)]
            rows = 1 if x.ndim == 1 else x.shape[0]
            x2 = np.ascontiguousarray(x.reshape(rows, x.shape[-1]), np.complex64)
            first = np.ascontiguousarray(segs[0][1], np.float32)
            per_row = first.ndim == 2
            assert segs[0][0] == 0 and first.shape[-1] == 5 and (not per_row or first.shape[0] == rows)
            f.write(struct.pack("<iiiiqq", int(mode), len(segs), int(per_row), int(state is not None), rows, x2.shape[1]))
            for start, p in segs:
                p = np.ascontiguousarray(p, np.float32)
                assert p.shape == first.shape
                f.write(struct.pack("<q", start))
                f.write(p.tobytes())
            if state is not None:
                z = np.ascontiguousarray(state, np.uint32)
                assert z.shape == (rows, 2)
                f.write(z.tobytes())
            f.write(x2.tobytes())
            shapes.append(x2.shape)
    subprocess.check_call([exe, "run", src, dst])
    out, raw, off = [], open(dst, "rb").read(), 0
    for r, n in shapes:
        y = np.frombuffer(raw, np.complex64, r * n, off).copy().reshape(r, n)
        off += 8 * r * n
        tr = np.frombuffer(raw, np.float32, r * n, off).copy().reshape(r, n)
        off += 4 * r * n
        z = np.frombuffer(raw, np.uint32, r * 2, off).copy().reshape(r, 2)
        off += 8 * r
        out.append((y, tr, z))
    assert off == len(raw)
    os.remove(src), os.remove(dst)
    return out


def derive(build_dir, sets):
    """sets (K, 5) float32 -> [(accepted, alpha_w, beta_w, F0, Fmin, Fmax)] by csrc/hz_carrier_plan.h"""
    exe = build_exact(build_dir)
    src, dst = os.path.join(build_dir, "carrier_sets.bin"), os.path.join(build_dir, "carrier_derived.bin")
    q = np.ascontiguousarray(sets, np.float32).reshape(-1, 5)
    q.tofile(src)
    subprocess.check_call([exe, "derive", src, dst])
    raw = open(dst, "rb").read()
    os.remove(src), os.remove(dst)
    assert len(raw) == 24 * q.shape[0]
    out = []
    for k in range(q.shape[0]):
        ok, aw, bw, f0, fmin, fmax = struct.unpack_from("<iffiii", raw, 24 * k)
        out.append((bool(ok), np.float32(aw), np.float32(bw), f0, fmin, fmax))
    return out


def unit(build_dir, stride, threads=8):
    """the program's `unit` mode over every stride-th phase word and the axes, the diagonals and their neighbours ->
    (words, car_unit's largest error, where, the tuner rotator's largest error, where, axis words that are not exact)"""
    v = subprocess.check_output([build_exact(build_dir), "unit", str(int(stride)), str(int(threads))], text=True).split()
    return int(v[0]), float(v[1]), int(v[2]), float(v[3]), int(v[4]), int(v[5])


def two_channels(nsym, offsets, seed, sps=5, down=4, centres=(0.2, -0.15)):
    """A wide stream that holds one QPSK channel per entry of `offsets`: raised-cosine symbols (roll-off 0.5, unit
    amplitude) at sps * down wide samples per symbol, channel k centred `centres[k]` cycles per WIDE sample plus
    `offsets[k]` cycles per NARROW sample (what a tuner at the centre leaves to the carrier loop) -> (x complex64,
    the tuners' frequency words uint32, the decimation low-pass float32 of unit DC gain, the symbols (K, nsym))."""
    import symsync_ref
    wide = sps * down
    a = np.stack([symsync_ref.symbols(nsym, seed + k, True) for k in range(len(offsets))])
    rows = [symsync_ref.signal(a[k], float(wide), 0.25 * k).astype(np.complex128) for k in range(len(offsets))]
    n = min(len(r) for r in rows)
    t = np.arange(n)
    x = sum(r[:n] * np.exp(2j * math.pi * ((c + off / down) * t + 0.1 + 0.2 * k)) for k, (r, c, off) in enumerate(zip(rows, centres, offsets)))
    words = np.array([int(round(c * TWO32)) % (1 << 32) for c in centres[:len(offsets)]], np.uint32)
    m = np.arange(65) - 32
    h = np.sinc(m * 2.0 * 0.09) * np.hamming(65)
    return x.astype(np.complex64), words, (h / h.sum()).astype(np.float32), a

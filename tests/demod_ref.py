"""The independent restatement of the demodulator bank's definition (include/hzsdr_demod.h), its counts and its bound.

    d[n] = angle(a conj(b)) | angle(a) | |a| | |a|^2,   a = c(x[n]), b = c(x[n - 1])
    y[m] = sum_{q < Q} h[q] d[m D - q]                  scipy.signal.upfirdn(h, d, 1, D)

The separately rounded float32 product and squares are numpy float32 operations; from there on everything is float64:
arctan2 / sqrt, then the FIR.  Beside it, the runner of the bit-exact restatement tests/host/demod_ref.cpp (the program
over csrc/hz_demod_math.h whose outputs the device must reproduce bit for bit)."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FM, PHASE, ENVELOPE, POWER = 1, 2, 3, 4
MODES = {"fm": FM, "phase": PHASE, "envelope": ENVELOPE, "power": POWER}
# The bound on demod_angle's error against float64 atan2 that tests/test_demod_cpu.py asserts of the measured E (and
# every bound below is derived from): 2^-21 rad, two ulps of the largest result.
E_BOUND = 2.0 ** -21
# E as tests/host/demod_ref.cpp's sweep measures it (tests/test_demod_cpu.py runs the sweep and asserts that it finds
# no more than this): the bounds below are derived from it.
E = 2.673684e-07


def outputs_after(n, down):
    """ceil(N / D): the outputs written once N samples have been pushed"""
    return -(-n // down)


def total_outputs(n, ntaps, down):
    """the whole stream's outputs, pushes and flush: upfirdn(h, d, 1, D)'s length, ceil((N - 1 + Q) / D); none for N = 0"""
    return -(-(n - 1 + ntaps) // down) if n > 0 else 0


def detector(mode, x):
    """d[n] of complex64 samples (already converted) -> float64.  The product and the squares are float32 operations,
    each rounded by itself; the arctangent and the square root are float64 (of the float32 sum)."""
    x = np.ascontiguousarray(x, np.complex64)
    re, im = x.real.astype(np.float32), x.imag.astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        if mode == FM:
            bre, bim = np.concatenate([np.zeros(1, np.float32), re[:-1]]), np.concatenate([np.zeros(1, np.float32), im[:-1]])
            pre = (re * bre).astype(np.float32) + (im * bim).astype(np.float32)
            pim = (im * bre).astype(np.float32) - (re * bim).astype(np.float32)
            assert pre.dtype == pim.dtype == np.float32
            d = np.arctan2(pim.astype(np.float64), pre.astype(np.float64))
            return np.where((pre == 0) & (pim == 0), 0.0, d)  # angle(+-0, +-0) = +0
        if mode == PHASE:
            d = np.arctan2(im.astype(np.float64), re.astype(np.float64))
            return np.where((re == 0) & (im == 0), 0.0, d)
        p = (re * re).astype(np.float32) + (im * im).astype(np.float32)
        assert p.dtype == np.float32
        return np.sqrt(p.astype(np.float64)) if mode == ENVELOPE else p.astype(np.float64)


def fir(h, d, down):
    """y[m] = sum_q h[q] d[m D - q] in float64 over the whole stream -> (y, sum_q |h[q] d[m D - q]|)"""
    h = np.asarray(h, np.float64)
    d = np.asarray(d, np.float64)
    n, q = d.shape[0], h.shape[0]
    count = total_outputs(n, q, down)
    dp = np.concatenate([np.zeros(q - 1), d, np.zeros(q + down)])
    m = np.arange(count, dtype=np.int64) * down + (q - 1)
    y, mag = np.zeros(count), np.zeros(count)
    for k in range(q):
        t = h[k] * dp[m - k]
        y += t
        mag += np.abs(t)
    return y, mag


def demodulate(mode, h, x, down):
    """the whole stream of complex64 samples x -> (y, mag) in float64"""
    return fir(h, detector(mode, x), down)


def bound(mode, h, mag):
    """|y_float32 - y_float64| per output.  The detector: an angle within E of atan2, a float32 square root
    within half an ulp, the power exact (it IS the float32 sum); each scaled by |h| and summed: E sum|h| for the angles,
    2^-24 mag for the envelope.  The FIR: Q fused steps, each rounding a partial sum no larger than mag to half an
    ulp, (Q + 2) 2^-24 mag with the two to spare for the detector's own last rounding."""
    h = np.asarray(h, np.float64)
    q = h.shape[0]
    e = E * np.abs(h).sum() if mode in (FM, PHASE) else 0.0
    return e + (q + 2) * 2.0 ** -24 * mag


_EXE = {}


def build_exact(build_dir):
    """g++ -O2 -ffp-contract=off of tests/host/demod_ref.cpp -> the program's path (built once per directory)"""
    if build_dir not in _EXE:
        os.makedirs(build_dir, exist_ok=True)
        exe = os.path.join(build_dir, "demod_ref")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"),
                               os.path.join(ROOT, "tests", "host", "demod_ref.cpp"), "-o", exe])
        _EXE[build_dir] = exe
    return _EXE[build_dir]


def exact(build_dir, cases):
    """cases: [(mode, down, taps, x complex64)] -> the float32 outputs of each whole stream, by the program"""
    exe = build_exact(build_dir)
    src, dst = os.path.join(build_dir, "demod_cases.bin"), os.path.join(build_dir, "demod_out.bin")
    with open(src, "wb") as f:
        for mode, down, taps, x in cases:
            taps, x = np.ascontiguousarray(taps, np.float32), np.ascontiguousarray(x, np.complex64)
            f.write(struct.pack("<iiiq", mode, down, taps.shape[0], x.shape[0]))
            f.write(taps.tobytes())
            f.write(x.tobytes())
    subprocess.check_call([exe, "run", src, dst])
    out, raw, off = [], open(dst, "rb").read(), 0
    for mode, down, taps, x in cases:
        (count,) = struct.unpack_from("<q", raw, off)
        assert count == total_outputs(len(x), len(taps), down)
        out.append(np.frombuffer(raw, np.float32, count, off + 8).copy())
        off += 8 + 4 * count
    assert off == len(raw)
    os.remove(src), os.remove(dst)
    return out


def measure_angle_error(build_dir):
    """the program's sweep -> E, the largest |demod_angle - atan2| it found"""
    out = subprocess.run([build_exact(build_dir), "sweep"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1800)
    assert out.returncode == 0, out.stdout[-2000:]
    line = [s for s in out.stdout.splitlines() if s.startswith("E ")]
    assert len(line) == 1, out.stdout[-2000:]
    return float(line[0].split()[1]), out.stdout

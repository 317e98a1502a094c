"""The independent restatement of the IIR bank's definition (include/hzsdr_iir.h) and its bound.

    per section (b0, b1, b2, a1, a2):   y[n] = b0 x[n] + b1 x[n-1] + b2 x[n-2] - a1 y[n-1] - a2 y[n-2]

in float64 and in DIRECT form I (the contract steps the transposed form II in float32: another structure, the same
transfer function), section after section.  Beside it, the runner of the bit-exact restatement tests/host/iir_ref.cpp
(the program over csrc/hz_iir_math.h whose outputs the device must reproduce bit for bit), the impulse-response l1
gains the bound is made of, and the decay row that runs through the denormals."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL_F32 = 32
FORM_PER_ROW, FORM_COMPLEX = 1, 2
U = 2.0 ** -24       # half an ulp of a float32 result, relative
TINY = 2.0 ** -150   # half the spacing of the float32 denormals, absolute


def float64(sections, x):
    """One row x (float32 or complex64 values, taken exactly) through the cascade (S, 5) in float64, direct form I.
    -> y, float64 or complex128."""
    s = np.asarray(sections, np.float64).reshape(-1, 5)
    v = np.asarray(x).astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    for b0, b1, b2, a1, a2 in s:
        y = np.zeros_like(v)
        x1 = x2 = y1 = y2 = 0.0
        for n in range(v.shape[0]):
            xn = v[n]
            yn = b0 * xn + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
            x2, x1, y2, y1 = x1, xn, y1, yn
            y[n] = yn
        v = y
    return v


def impulse_l1(b, a, cap=1 << 22):
    """sum |h[n]| of H = B / A in float64, B = (b0, b1, b2), A = (1, a1, a2): summed until the response has decayed
    below 2^-60 of the sum over a whole block (or `cap` samples: an unstable section has no bound)."""
    b0, b1, b2 = (float(v) for v in b)
    a1, a2 = (float(v) for v in a)
    total, x1, x2, y1, y2, n = 0.0, 0.0, 0.0, 0.0, 0.0, 0
    while n < cap:
        block = 0.0
        for _ in range(256):
            xn = 1.0 if n == 0 else 0.0
            yn = b0 * xn + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
            x2, x1, y2, y1 = x1, xn, y1, yn
            block += abs(yn)
            n += 1
        total += block
        if block <= total * 2.0 ** -60:
            return total
    raise ValueError("the section does not decay")


def nodes(sections, x):
    """max |node| per section over the row, the nodes being the five rounded values of the step (y, t, z1, u, z2), from
    a float64 run of the transposed form.  x real or complex (the larger of re and im)."""
    s = np.asarray(sections, np.float64).reshape(-1, 5)
    parts = [np.asarray(x).real.astype(np.float64), np.asarray(x).imag.astype(np.float64)] if np.iscomplexobj(x) else [np.asarray(x, np.float64)]
    peak = np.zeros(s.shape[0])
    for v in parts:
        for k, (b0, b1, b2, a1, a2) in enumerate(s):
            y = np.zeros_like(v)
            z1 = z2 = 0.0
            m = 0.0
            for n in range(v.shape[0]):
                xn = v[n]
                yn = b0 * xn + z1
                t = b1 * xn + z2
                z1 = t - a1 * yn
                u = b2 * xn
                z2 = u - a2 * yn
                m = max(m, abs(yn), abs(t), abs(z1), abs(u), abs(z2))
                y[n] = yn
            peak[k] = max(peak[k], m)
            v = y
    return peak


def bound(sections, x):
    """|y_float32 - y_float64| per output of one row.  The step rounds five values, each by at most 2^-24 of itself
    (2^-150 absolute among the denormals); an error made inside section s reaches the section's output through 1 / A_s
    and the cascade's output through the sections behind it:
        sum_s 5 (2^-24 max|node_s| + 2^-150) ||1 / A_s||_1 prod_{t > s} ||H_t||_1
    with the l1 gains computed numerically from the row's own coefficients."""
    s = np.asarray(sections, np.float64).reshape(-1, 5)
    peak = nodes(s, x)
    inv = [impulse_l1((1.0, 0.0, 0.0), c[3:]) for c in s]
    gain = [impulse_l1(c[:3], c[3:]) for c in s]
    total = 0.0
    for k in range(s.shape[0]):
        behind = float(np.prod(gain[k + 1:])) if k + 1 < s.shape[0] else 1.0
        total += 5.0 * (U * peak[k] + TINY) * inv[k] * behind
    return total


def decay_section():
    """a pole at 0.5: the impulse response 2^-n is exact in float32 down to the smallest denormal 2^-149, and +0 from
    n = 150 on (2^-150 is a tie between 0 and 2^-149 and goes to the even one)"""
    return np.array([[1.0, 0.0, 0.0, -0.5, 0.0]], np.float32)


def decay_row(n, amplitude=1.0):
    x = np.zeros(n, np.float32)
    x[0] = amplitude
    return x


_EXE = {}


def build_exact(build_dir):
    """g++ -O2 -ffp-contract=off of tests/host/iir_ref.cpp -> the program's path (built once per directory)"""
    if build_dir not in _EXE:
        os.makedirs(build_dir, exist_ok=True)
        exe = os.path.join(build_dir, "iir_ref")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"),
                               os.path.join(ROOT, "tests", "host", "iir_ref.cpp"), "-o", exe])
        _EXE[build_dir] = exe
    return _EXE[build_dir]


def exact(build_dir, cases):
    """cases: [(sections, x)] -> [(y, state)] by the program.  x: float32 or complex64 (already converted), (N,) or
    (R, N); sections: float32 (S, 5) shared or (R, S, 5) per row -- or a list [(start, sections), ...], the cascade in
    force from sample `start` on (the first start is 0).  y has x's shape and type; state is float32 (R, S, 2) for real
    rows and (R, S, 2, 2) for complex ones (hzsdr_iir_get_state's layout)."""
    exe = build_exact(build_dir)
    src, dst = os.path.join(build_dir, "iir_cases.bin"), os.path.join(build_dir, "iir_out.bin")
    shapes = []
    with open(src, "wb") as f:
        for sections, x in cases:
            segs = sections if isinstance(sections, list) else [(0, sections)]
            x = np.asarray(x)
            cplx = np.iscomplexobj(x)
            x2 = np.ascontiguousarray(x.reshape(-1, x.shape[-1]), np.complex64 if cplx else np.float32)
            first = np.ascontiguousarray(segs[0][1], np.float32)
            per_row, s = first.ndim == 3, first.shape[-2]
            assert segs[0][0] == 0 and (not per_row or first.shape[0] == x2.shape[0])
            f.write(struct.pack("<iiiiqq", s, 2 if cplx else 1, len(segs), int(per_row), x2.shape[0], x2.shape[1]))
            for start, c in segs:
                c = np.ascontiguousarray(c, np.float32)
                assert c.shape == first.shape
                f.write(struct.pack("<q", start))
                f.write(c.tobytes())
            f.write(x2.tobytes())
            shapes.append((x.shape, x2.shape, s, cplx))
    subprocess.check_call([exe, "run", src, dst])
    out, raw, off = [], open(dst, "rb").read(), 0
    for shape, (r, n), s, cplx in shapes:
        pl = 2 if cplx else 1
        y = np.frombuffer(raw, np.float32, r * n * pl, off).copy()
        off += 4 * r * n * pl
        z = np.frombuffer(raw, np.float32, r * s * 2 * pl, off).copy()
        off += 4 * r * s * 2 * pl
        y = (y.view(np.complex64) if cplx else y).reshape(shape)
        out.append((y, z.reshape((r, s, 2) + ((2,) if cplx else ()))))
    assert off == len(raw)
    os.remove(src), os.remove(dst)
    return out

"""The IIR bank (include/hzsdr_iir.h): a cascade of biquads over one row, or over many rows, real or complex.

    de = ctx.iir_bank(hz.IIR_REAL_F32, hz.deemphasis(75e-6, 48e3), rows=100)
    audio = de.push(fm.push(rows))          # the demodulator's float32 block as it is, any row pitch
    dc = ctx.iir_bank(hz.FMT_U8, hz.dc_block(0.999))   # a complex row: re and im through the same real cascade

Each section is (b0, b1, b2, a1, a2) with a0 = 1, stepped in transposed direct form II, every operation one float32
operation rounded by itself:

    y = fma(b0, x, z1);  z1 = fma(-a1, y, fma(b1, x, z2));  z2 = fma(-a2, y, b2 * x)

One output per input, nothing to flush.  The bits do not depend on how the stream is cut into pushes, on the memory
space, on the number of rows, on either pitch or on the other rows.  A NaN poisons its row until reset() or
set_state().  One row runs at one lane's rate: the parallelism is across the rows.

The designers return float32 (S, 5) arrays, computed in float64 and divided by a0.
"""
import ctypes as C
import math

import numpy as np

from . import ErrInvalidArgument, FMT_C64, FMT_I8, FMT_I16, FMT_U8, lib  # noqa: F401
from ._rows import RowWaveBank, cut, rows_input, rows_output
from ._capi import IIR_FORM_COMPLEX, IIR_FORM_PER_ROW, IIR_MAX_ROWS, IIR_MAX_SECTIONS, IIR_REAL_F32

_PF = C.POINTER(C.c_float)


def _sections(rows):
    """float64 rows of (b0, b1, b2, a0, a1, a2) -> float32 (S, 5), divided by a0"""
    out = []
    for b0, b1, b2, a0, a1, a2 in rows:
        if not (math.isfinite(a0) and a0 != 0.0):
            raise ValueError("iir: a0 is zero or not finite")
        out.append([b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0])
    s = np.asarray(out, np.float64)
    if not np.isfinite(s).all():
        raise ValueError("iir: a coefficient is not finite")
    return s.astype(np.float32)


def one_pole(alpha):
    """y[n] = alpha x[n] + (1 - alpha) y[n - 1], 0 < alpha <= 1: the smoother that turns the power detector into a
    squelch level (unit gain at DC, time constant about 1 / alpha samples)."""
    a = float(alpha)
    if not 0.0 < a <= 1.0:
        raise ValueError("one_pole: 0 < alpha <= 1")
    return _sections([(a, 0.0, 0.0, 1.0, -(1.0 - a), 0.0)])


def dc_block(r):
    """H(z) = (1 - z^-1) / (1 - r z^-1), 0 <= r < 1: a zero at DC, the pole at r setting how narrow the notch is."""
    r = float(r)
    if not 0.0 <= r < 1.0:
        raise ValueError("dc_block: 0 <= r < 1")
    return _sections([(1.0, -1.0, 0.0, 1.0, -r, 0.0)])


def deemphasis(tau, fs):
    """FM de-emphasis: the bilinear transform of H(s) = 1 / (1 + s tau) at the sample rate fs (tau = 75e-6 or 50e-6)."""
    tau, fs = float(tau), float(fs)
    if not (tau > 0.0 and fs > 0.0):
        raise ValueError("deemphasis: tau and fs are positive")
    k = 2.0 * fs * tau
    return _sections([(1.0, 1.0, 0.0, 1.0 + k, 1.0 - k, 0.0)])


def _rbj(f, q, fs, who):
    f, q, fs = float(f), float(q), float(fs)
    if not (fs > 0.0 and 0.0 < f < fs / 2.0 and q > 0.0):
        raise ValueError(f"{who}: 0 < f < fs / 2 and q > 0")
    w0 = 2.0 * math.pi * f / fs
    return math.cos(w0), math.sin(w0) / (2.0 * q)


def notch(f0, q, fs):
    """The RBJ cookbook notch: zeros on the unit circle at f0, bandwidth f0 / q."""
    c, al = _rbj(f0, q, fs, "notch")
    return _sections([(1.0, -2.0 * c, 1.0, 1.0 + al, -2.0 * c, 1.0 - al)])


def lowpass(fc, q, fs):
    """The RBJ cookbook low-pass (q = 1 / sqrt 2: Butterworth)."""
    c, al = _rbj(fc, q, fs, "lowpass")
    return _sections([((1.0 - c) / 2.0, 1.0 - c, (1.0 - c) / 2.0, 1.0 + al, -2.0 * c, 1.0 - al)])


def highpass(fc, q, fs):
    """The RBJ cookbook high-pass (a CTCSS high-pass at 300 Hz, say)."""
    c, al = _rbj(fc, q, fs, "highpass")
    return _sections([((1.0 + c) / 2.0, -(1.0 + c), (1.0 + c) / 2.0, 1.0 + al, -2.0 * c, 1.0 - al)])


def butterworth(order, fc, fs, highpass=False):
    """A Butterworth low-pass (or high-pass) of `order` 1 ... 16 with its -3.01 dB point at fc, as ceil(order / 2)
    second-order sections: the bilinear transform, prewarped at fc, of the analogue prototype's pole pairs (the
    cookbook forms with q_k = 1 / (2 sin(pi (2 k + 1) / (2 order)))) and, for an odd order, of its real pole."""
    n = int(order)
    if not 1 <= n <= 2 * IIR_MAX_SECTIONS:
        raise ValueError("butterworth: order is 1 ... 16")
    c, _ = _rbj(fc, 1.0, fs, "butterworth")
    s = math.sqrt(1.0 - c * c)  # sin w0
    rows = []
    for k in range(n // 2):
        al = s * math.sin(math.pi * (2 * k + 1) / (2.0 * n))  # sin w0 / (2 q_k)
        if highpass:
            rows.append(((1.0 + c) / 2.0, -(1.0 + c), (1.0 + c) / 2.0, 1.0 + al, -2.0 * c, 1.0 - al))
        else:
            rows.append(((1.0 - c) / 2.0, 1.0 - c, (1.0 - c) / 2.0, 1.0 + al, -2.0 * c, 1.0 - al))
    if n % 2:
        kk = math.tan(math.pi * float(fc) / float(fs))
        rows.append((1.0, -1.0, 0.0, 1.0 + kk, kk - 1.0, 0.0) if highpass else (kk, kk, 0.0, 1.0 + kk, kk - 1.0, 0.0))
    return _sections(rows)


def response(sections, f, fs):
    """H(exp(2 pi i f / fs)) of a cascade (S, 5), in float64 (f a scalar or an array)."""
    s = np.asarray(sections, np.float64).reshape(-1, 5)
    z1 = np.exp(-2j * np.pi * np.asarray(f, np.float64) / float(fs))
    h = np.ones_like(z1)
    for b0, b1, b2, a1, a2 in s:
        h = h * (b0 + b1 * z1 + b2 * z1 * z1) / (1.0 + a1 * z1 + a2 * z1 * z1)
    return h


class IirBank(RowWaveBank):
    """hzsdr_iir: push(samples) -> the filtered rows.  `kind` is IIR_REAL_F32 (float32 in and out) or a source format
    (u8 / i8 / i16 / c64 in, complex64 out).  One row takes (n,) samples ((n, 2) for the byte and int16 formats);
    `rows` = R > 1 takes (R, n) with unit stride along a row and any row pitch and returns (R, n).  `sections` is
    (S, 5) shared by all rows, or (R, S, 5), one cascade per row.  numpy in a HOST context; torch tensors on the
    context's device, written on the context's stream, in a DEVICE context."""

    _c, _noun = "iir", "iir bank"
    _state_msg = "the state is (rows, S, 2), with a last axis (re, im) for complex rows"

    def __init__(self, ctx, kind, sections, rows=1):
        self.kind = int(kind)
        self._open(ctx, rows)
        self.sections = self._check(sections, None)
        self.per_row = self.sections.ndim == 3
        self.n_sections = int(self.sections.shape[-2])
        self.complex = self.kind != IIR_REAL_F32
        ctx._ck(lib.hzsdr_iir_create(ctx._h, self.kind, self.sections.ctypes.data_as(_PF), self.n_sections, int(self.per_row), self.rows,
                                     C.byref(self._h)))

    def _check(self, sections, like):
        s = np.ascontiguousarray(sections, np.float32)
        if s.ndim not in (2, 3) or s.shape[-1] != 5 or s.shape[-2] == 0 or (s.ndim == 3 and s.shape[0] != self.rows):
            raise ErrInvalidArgument("iir bank: sections are (S, 5), or (rows, S, 5)")
        if like is not None and s.shape != like.shape:
            raise ErrInvalidArgument("iir bank: the section count and form cannot change")
        return s

    def plan(self):
        """(rows per wave, samples per tile, form): the form is a sum of IIR_FORM_PER_ROW and IIR_FORM_COMPLEX."""
        return self._plan()

    def push(self, samples, out=None):
        """Filter every sample of every row of `samples`.  `out`, when given, is a float32 (real rows) or complex64
        buffer ((cap,), or (rows, cap) with any row pitch; columns past the samples are left as they are); for
        float32 and complex64 rows it may be `samples` itself: the rows are filtered in place."""
        ptr, n, pitch = rows_input(samples, self.kind, self.rows, "iir bank")
        out, optr, cap, opitch = rows_output(out, n, samples, self.rows, np.complex64 if self.complex else np.float32, "iir bank", unit="row")
        got = C.c_size_t(0)
        self._call("push", ptr, n, pitch, optr if cap else None, cap, opitch, C.byref(got))
        return cut(out, self.rows, got.value)

    def set_sections(self, sections):
        """Exchange the coefficients (same shape) between two pushes; the state and the position stay."""
        s = self._check(sections, self.sections)
        self._call("set_sections", s.ctypes.data_as(_PF), self.n_sections)
        self.sections = s

    def _state_shape(self):
        return (self.rows, self.n_sections, 2) + ((2,) if self.complex else ())

    def state(self):
        """(z, position): z is float32 (rows, S, 2) for real rows -- z1, z2 -- and (rows, S, 2, 2) for complex rows,
        the last axis re, im; behind every push so far."""
        return self._state()


__all__ = ["IirBank", "one_pole", "dc_block", "deemphasis", "notch", "lowpass", "highpass", "butterworth", "response", "IIR_REAL_F32",
           "IIR_FORM_PER_ROW", "IIR_FORM_COMPLEX", "IIR_MAX_SECTIONS", "IIR_MAX_ROWS"]

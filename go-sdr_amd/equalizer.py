"""The adaptive equalizer bank (include/hzsdr_equalizer.h): an N-tap linear equalizer at the symbol rate over one real
float32 or complex64 row of soft symbols, or over many rows, one output per symbol consumed.

    eq = ctx.equalizer(hz.FMT_C64, hz.EQUALIZER_CMA, taps=11, centre=5, params=(0.01, 1.0), rows=100)   # mu, level
    soft, counts = ts.push(block)                        # the symbol-timing bank's ragged block
    frames = fs.push(eq.push(soft, counts), counts)      # equalized where it lies in the chain; the counts go on as they are
    y, err = eq.push(soft, counts, track=True)           # err: the squared clipped error of every symbol
    w = eq.taps()                                        # the inverse-channel estimate, (rows, taps)

Blind (EQUALIZER_CMA: e = (level - |y|^2) y) or decision-directed (EQUALIZER_DD_BPSK, EQUALIZER_DD_QPSK:
e = decision - y with decisions of amplitude `level` per component); w += mu e conj(X), the error clipped to [-1, 1]
per component (the header has the step).  The taps and the last N - 1 inputs carry from push to push, so outputs, track
and state do not depend on how the stream is cut, on the memory space, on the number of rows, on any pitch or on the
other rows.  set_state with mu = 0 makes the bank a fixed FIR over many rows.  A NaN or a diverged row garbles its own
row alone, until reset or set_state.  The taps of a row are dealt to the lanes of a wave, so a symbol costs about the
same whatever the number of taps.

Not here: fractionally spaced input, trained adaptation, decision feedback, tap leakage.
"""
import ctypes as C

import numpy as np

from . import _is_torch, ErrInvalidArgument, FMT_C64, lib
from ._rows import RowWaveBank, cut, rows_input, rows_output
from ._capi import (EQUALIZER_CMA, EQUALIZER_DD_BPSK, EQUALIZER_DD_QPSK, EQUALIZER_FORM_COMPLEX, EQUALIZER_FORM_PER_ROW, EQUALIZER_MAX_ROWS,
                    EQUALIZER_MAX_TAPS, EQUALIZER_REAL_F32)

_PF = C.POINTER(C.c_float)


class Equalizer(RowWaveBank):
    """hzsdr_equalizer: push(rows[, counts]) -> the equalized rows.  `kind` is EQUALIZER_REAL_F32 (float32 rows, real
    taps) or FMT_C64 (complex64 rows, complex taps); `mode` EQUALIZER_CMA, EQUALIZER_DD_BPSK or EQUALIZER_DD_QPSK (complex
    rows only).  One row takes (n,) symbols; `rows` = R > 1 takes (R, n) with unit stride along a row and any row pitch
    and returns (R, n).  `params` is float32 (2,) -- mu, level -- shared by all rows, or (R, 2), one set per row.  numpy in
    a HOST context; torch tensors on the context's device, written on the context's stream, in a DEVICE context."""

    _c = _noun = "equalizer"
    _state_msg = "the state is float32 (rows, 2 * taps - 1), or (rows, 2 * (2 * taps - 1)) for complex rows"

    def __init__(self, ctx, kind, mode, taps, centre, params, rows=1, per_row=False):
        self.kind, self.mode, self.taps_count, self.centre = int(kind), int(mode), int(taps), int(centre)
        self._open(ctx, rows)
        self.per_row = bool(per_row)
        self.params = self._check(params)
        self.complex = self.kind == FMT_C64
        self._dtype = np.complex64 if self.complex else np.float32
        if self.taps_count < 0 or self.centre < 0:
            raise ErrInvalidArgument("equalizer: 1 ... 64 taps, 0 <= centre < taps")
        ctx._ck(lib.hzsdr_equalizer_create(ctx._h, self.kind, self.mode, self.taps_count, self.centre, self.params.ctypes.data_as(_PF),
                                           int(self.per_row), self.rows, C.byref(self._h)))

    def _check(self, params):
        p = np.ascontiguousarray(params, np.float32)
        if p.shape != ((self.rows, 2) if self.per_row else (2,)):
            raise ErrInvalidArgument("equalizer: params are (2,) -- mu, level -- or (rows, 2) with per_row")
        return p

    def plan(self):
        """(rows per wave, symbols per tile, form): the form is EQUALIZER_FORM_PER_ROW | EQUALIZER_FORM_COMPLEX."""
        return self._plan()

    def push(self, symbols, counts=None, out=None, track=None):
        """Run the symbols of every row of `symbols` through the equalizer -> the equalized rows, or (rows, track) where
        a track is asked for.  `counts`, when given, is the symbol-timing bank's: (rows,) contiguous uint32 (numpy) or
        int32 (torch) values; row r consumes min(counts[r], n) symbols, and what lies behind them in the destination is
        what it held (a new one is not initialised).  `out`, when given, is a buffer of the symbols' type ((cap,), or
        (rows, cap) with any row pitch); it may be `symbols` itself: the rows are equalized in place.  `track` is True (a
        new float32 array) or a float32 buffer of that form: the squared clipped error of every symbol."""
        noun = self._noun
        ptr, n, pitch = rows_input(symbols, self.kind, self.rows, noun)
        cptr = None
        if counts is not None:
            if _is_torch(counts):
                import torch
                ok, cptr = counts.dtype == torch.int32 and counts.is_contiguous() and tuple(counts.shape) == (self.rows,), counts.data_ptr()
            else:
                ok, cptr = counts.dtype == np.uint32 and counts.flags.c_contiguous and counts.shape == (self.rows,), counts.ctypes.data
            if not ok or _is_torch(counts) != _is_torch(symbols):
                raise ValueError("equalizer: counts are (rows,) contiguous uint32 (numpy) or int32 (torch) values, where the symbols live")
        out, optr, cap, opitch = rows_output(out, n, symbols, self.rows, self._dtype, noun, unit="row")
        if cap < n:
            raise ValueError("equalizer: the destination is shorter than the rows")
        if track is None or track is False:
            self._call("push", ptr, n, pitch, cptr, optr if cap else None, opitch, None, 0)
            return cut(out, self.rows, n)
        track, tptr, tcap, tpitch = rows_output(None if track is True else track, n, symbols, self.rows, np.float32, f"{noun} track", unit="row")
        if tcap < n:
            raise ValueError("equalizer: the track is shorter than the rows")
        self._call("push", ptr, n, pitch, cptr, optr if cap else None, opitch, tptr if tcap else None, tpitch)
        return cut(out, self.rows, n), cut(track, self.rows, n)

    def set_params(self, params):
        """Exchange the parameters (same shape) between two pushes; the state stays."""
        p = self._check(params)
        self._call("set_params", p.ctypes.data_as(_PF))
        self.params = p

    def _state_shape(self):
        return (self.rows, (2 * self.taps_count - 1) * (2 if self.complex else 1))

    def state(self):
        """z, float32 (rows, 2 * taps - 1) -- the taps, then the taps - 1 latest inputs, newest first -- and twice as wide
        for complex rows, whose entries are (re, im) pairs; behind every push so far."""
        z = np.empty(self._state_shape(), np.float32)
        self._call("get_state", z.ctypes.data_as(_PF), z.size)
        return z

    def set_state(self, z):
        """Replace the state (the shape of state()); the values are taken as they are."""
        z = np.ascontiguousarray(z, np.float32)
        if z.shape != self._state_shape():
            raise ErrInvalidArgument(f"equalizer: {self._state_msg}")
        self._call("set_state", z.ctypes.data_as(_PF), z.size)

    def position(self):
        raise AttributeError("equalizer: nothing depends on a position, so none is offered")

    def taps(self):
        """The taps of every row, (rows, taps) float32 or complex64: the inverse-channel estimate."""
        z = self.state()
        w = z[:, :self.taps_count * (2 if self.complex else 1)]
        return np.ascontiguousarray(w).view(self._dtype) if self.complex else w.copy()


__all__ = ["Equalizer", "EQUALIZER_REAL_F32", "EQUALIZER_CMA", "EQUALIZER_DD_BPSK", "EQUALIZER_DD_QPSK", "EQUALIZER_FORM_PER_ROW",
           "EQUALIZER_FORM_COMPLEX", "EQUALIZER_MAX_ROWS", "EQUALIZER_MAX_TAPS"]

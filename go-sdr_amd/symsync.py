"""The symbol-timing recovery bank (include/hzsdr_symsync.h): soft symbols at the symbol rate out of one row, or out of
many rows, real or complex.

    sps = 48e3 / 9600                                   # AIS: 9600 Bd GMSK at 5 samples per symbol
    ts = ctx.symbol_sync(hz.SYMSYNC_REAL_F32, (sps, 0.01, *hz.loop_gains(sps)), rows=100)
    soft, counts = ts.push(de.push(fm.push(rows)))      # the IIR bank's float32 block as it is, any row pitch
    per_row = ts.ragged(soft, counts)                   # host arrays, one per row, each of its own length

A Gardner timing-error detector around a 4-point cubic Lagrange interpolator, advanced once per input sample, every
operation one float32 operation rounded by itself (the header has the step).  Per row it keeps a counter, the
half-period estimate h (2 h samples is the measured symbol period), a flag, two interpolants and three samples; the
state carries from push to push, so symbols, counts and state do not depend on how the stream is cut, on the memory
space, on the number of rows, on either pitch or on the other rows.  The output is RAGGED: row r of a push holds
counts[r] symbols, at most max_symbols(n) of them; the columns behind a row's count are left as they were.  A NaN or an
infinity may silence or garble its own row until reset() or set_state().  The latency is two samples and there is
nothing to flush.  One row runs at one lane's rate: the parallelism is across the rows.

Not here: the matched filter (the resampler's taps or the demodulator's post-filter in front of this stage) and the
carrier.  The decisions, the sync-word search and the frames are the frame sync bank's (include/hzsdr_framesync.h,
Context.frame_sync): it takes (symbols, counts) as push returns them.
"""
import ctypes as C

import numpy as np

from . import ErrInvalidArgument, _is_torch, lib
from ._rows import RowWaveBank, cut, rows_input, rows_output
from ._capi import SYMSYNC_FORM_COMPLEX, SYMSYNC_FORM_PER_ROW, SYMSYNC_MAX_ROWS, SYMSYNC_REAL_F32

_PF = C.POINTER(C.c_float)


def loop_gains(sps, alpha=0.06, ted_gain=2.7):
    """(g_mu, g_omega) = (alpha sps / ted_gain, g_mu alpha / 4) for a loop of `sps` samples per symbol: a proportional
    step of alpha symbols' worth per unit of detector output, and an integral one a quarter of alpha below it.
    `ted_gain` is a NOMINAL slope of the Gardner detector for unit-amplitude binary symbols; it has not been measured,
    and another pulse shape or amplitude has another slope: scale the rows to unit symbol amplitude, or the gains by
    the square of the amplitude.  With the defaults the loop acquired raised-cosine (roll-off 0.5) streams of 2.5 to 10
    samples per symbol with clock offsets up to 1000 ppm inside 1000 symbols."""
    sps, alpha, ted_gain = float(sps), float(alpha), float(ted_gain)
    if not (sps > 0.0 and alpha > 0.0 and ted_gain > 0.0):
        raise ValueError("loop_gains: sps, alpha and ted_gain are positive")
    g_mu = alpha * sps / ted_gain
    return g_mu, g_mu * alpha / 4.0


class SymbolSync(RowWaveBank):
    """hzsdr_symsync: push(rows) -> (symbols, counts).  `kind` is SYMSYNC_REAL_F32 (float32 in and out) or FMT_C64
    (complex64 in and out).  One row takes (n,) samples; `rows` = R > 1 takes (R, n) with unit stride along a row and
    any row pitch.  `params` is float32 (4,) -- sps, limit, g_mu, g_omega -- shared by all rows, or (R, 4), one set per
    row.  numpy in a HOST context; torch tensors on the context's device, written on the context's stream, in a DEVICE
    context (counts are int32 there: the same bits as the ABI's uint32)."""

    _c, _noun = "symsync", "symbol sync"
    _state_msg = "the state is (rows, 8), or (rows, 13) for complex rows"

    def __init__(self, ctx, kind, params, rows=1):
        self.kind = int(kind)
        self._open(ctx, rows)
        self.params = self._check(params, None)
        self.per_row = self.params.ndim == 2
        self.complex = self.kind != SYMSYNC_REAL_F32
        ctx._ck(lib.hzsdr_symsync_create(ctx._h, self.kind, self.params.ctypes.data_as(_PF), int(self.per_row), self.rows, C.byref(self._h)))

    def _check(self, params, like):
        p = np.ascontiguousarray(params, np.float32)
        if p.ndim not in (1, 2) or p.shape[-1] != 4 or (p.ndim == 2 and p.shape[0] != self.rows):
            raise ErrInvalidArgument("symbol sync: params are (4,) -- sps, limit, g_mu, g_omega -- or (rows, 4)")
        if like is not None and p.shape != like.shape:
            raise ErrInvalidArgument("symbol sync: the form of the parameters cannot change")
        return p

    def plan(self):
        """(rows per wave, samples per tile, form): the form is a sum of SYMSYNC_FORM_PER_ROW and SYMSYNC_FORM_COMPLEX."""
        return self._plan()

    def max_symbols(self, n):
        """The most symbols a push of n samples writes into one row."""
        b = C.c_size_t(0)
        self._call("max_symbols", int(n), C.byref(b))
        return b.value

    def push(self, samples, out=None, counts=None):
        """Run every sample of every row of `samples` through the loop -> (symbols, counts).  `symbols` is float32
        (real rows) or complex64, (max_symbols(n),) or (rows, max_symbols(n)): cut to the BOUND, not to the counts, so
        that nothing waits for the device; row r holds counts[r] symbols, and what lies behind them is what the
        destination held (a new one is not initialised).  `out`, when given, is a buffer of that type with a capacity of
        at least the bound ((cap,), or (rows, cap) with any row pitch); `counts` one of `rows` uint32 (numpy) or int32
        (torch) values."""
        ptr, n, pitch = rows_input(samples, self.kind, self.rows, "symbol sync")
        bound = self.max_symbols(n)
        out, optr, cap, opitch = rows_output(out, bound, samples, self.rows, np.complex64 if self.complex else np.float32, "symbol sync", unit="row")
        if counts is None:
            if _is_torch(samples):
                import torch
                counts = torch.zeros(self.rows, dtype=torch.int32, device=samples.device)
            else:
                counts = np.zeros(self.rows, np.uint32)
        if _is_torch(counts):
            import torch
            ok, cptr = counts.dtype == torch.int32 and counts.is_contiguous() and tuple(counts.shape) == (self.rows,), counts.data_ptr()
        else:
            ok, cptr = counts.dtype == np.uint32 and counts.flags.c_contiguous and counts.shape == (self.rows,), counts.ctypes.data
        if not ok:
            raise ValueError("symbol sync: counts are (rows,) contiguous uint32 (numpy) or int32 (torch) values")
        self._call("push", ptr, n, pitch, optr if cap else None, cap, opitch, cptr, None)
        return cut(out, self.rows, bound), counts

    def ragged(self, symbols, counts):
        """A push's (symbols, counts) -> a list of `rows` host arrays, row r of counts[r] symbols (this waits for the
        device in a DEVICE context)."""
        if _is_torch(symbols):
            symbols, counts = symbols.cpu().numpy(), counts.cpu().numpy()
        s = np.asarray(symbols).reshape(self.rows, -1)
        return [s[r, :int(c)].copy() for r, c in enumerate(np.asarray(counts).reshape(-1))]

    def set_params(self, params):
        """Exchange the parameters (same shape) between two pushes; the state and the position stay."""
        p = self._check(params, self.params)
        self._call("set_params", p.ctypes.data_as(_PF))
        self.params = p

    def _state_shape(self):
        return (self.rows, 13 if self.complex else 8)

    def state(self):
        """(z, position): z is float32 (rows, 8) for real rows -- c, h, flag, y_prev, y_mid, x1, x2, x3 -- and
        (rows, 13) for complex rows, the five sample-valued entries as (re, im) pairs; behind every push so far.
        2 * z[:, 1] is the measured symbol period in samples."""
        return self._state()


__all__ = ["SymbolSync", "loop_gains", "SYMSYNC_REAL_F32", "SYMSYNC_FORM_PER_ROW", "SYMSYNC_FORM_COMPLEX", "SYMSYNC_MAX_ROWS"]

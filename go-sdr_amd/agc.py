"""The AGC bank (include/hzsdr_agc.h): a level-independent gain loop over one real float32 or complex64 row, or over many
rows, one output per input of the input's type.

    attack, decay = hz.agc_rates(10, 100)                # time constants in samples: down fast, up slowly
    agc = ctx.agc(hz.FMT_C64, (1.0, attack, decay, 1e-4, 1.0, 1e-3, 1e3), rows=100)   # ref, attack, decay, floor, g0, gmin, gmax
    soft, counts = ts.push(cr.push(agc.push(tuned)))     # the tuner's complex64 block as it is, any row pitch
    y, g = agc.push(tuned, track=True)                   # g: the gain applied to every sample
    rssi = hz.agc.level(g, 1.0)                         # ref / g: the row's level as the loop sees it

A multiplicative loop: e = 1 - |y| / ref clipped at -1, g *= 1 + (e < 0 ? attack : decay) e, held to [gmin, gmax] (the
header has the step).  Multiplicative, so that the settling time in samples does not depend on the input's level.  A
level under `floor` holds the gain (the hang gate: a silent row does not wind up to gmax).  The gain carries from push to
push, so outputs, track and state do not depend on how the stream is cut, on the memory space, on the number of rows, on
any pitch or on the other rows.  A NaN stays in its sample.  One row runs at one lane's rate: the parallelism is across
the rows.

Not here: look-ahead, a level filter apart from the loop, a squelch output.
"""
import ctypes as C
import math

import numpy as np

from . import ErrInvalidArgument, FMT_C64, lib
from ._rows import RowWaveBank
from ._capi import AGC_FORM_COMPLEX, AGC_FORM_PER_ROW, AGC_MAX_ROWS, AGC_REAL_F32

_PF = C.POINTER(C.c_float)


def agc_rates(attack_samples, decay_samples):
    """(attack, decay): the rates 1 - exp(-1 / tau) of the time constants `attack_samples` (towards a lower gain) and
    `decay_samples` (towards a higher gain), in samples.  A rate above 0.5 (a time constant under 1.4427 samples) is
    refused, as the bank refuses it."""
    rates = []
    for tau in (attack_samples, decay_samples):
        tau = float(tau)
        if not tau > 0.0:
            raise ValueError("agc_rates: time constants are positive")
        r = -math.expm1(-1.0 / tau)
        if r > 0.5:
            raise ValueError("agc_rates: a rate above 0.5 per sample (a time constant below 1 / ln 2 samples)")
        rates.append(r)
    return tuple(rates)


def level(track, ref):
    """ref / g: the level of a row as the loop sees it (its RSSI, in the samples' units), from a gain track or a state."""
    if hasattr(track, "reciprocal") and not isinstance(track, np.ndarray):
        return track.reciprocal() * float(ref)
    return np.float32(ref) / np.asarray(track, np.float32)


class Agc(RowWaveBank):
    """hzsdr_agc: push(rows) -> the levelled rows.  `kind` is AGC_REAL_F32 (float32 rows) or FMT_C64 (complex64 rows).
    One row takes (n,) samples; `rows` = R > 1 takes (R, n) with unit stride along a row and any row pitch and returns
    (R, n).  `params` is float32 (7,) -- ref, attack, decay, floor, g0, gmin, gmax -- shared by all rows, or (R, 7), one
    set per row.  numpy in a HOST context; torch tensors on the context's device, written on the context's stream, in
    a DEVICE context."""

    _c = _noun = "agc"
    _state_msg = "the state is float32 (rows,)"

    def __init__(self, ctx, kind, params, rows=1, per_row=False):
        self.kind = int(kind)
        self._open(ctx, rows)
        self.per_row = bool(per_row)
        self.params = self._check(params)
        self._dtype = np.complex64 if self.kind == FMT_C64 else np.float32
        ctx._ck(lib.hzsdr_agc_create(ctx._h, self.kind, self.params.ctypes.data_as(_PF), int(self.per_row), self.rows, C.byref(self._h)))

    def _check(self, params):
        p = np.ascontiguousarray(params, np.float32)
        if p.shape != ((self.rows, 7) if self.per_row else (7,)):
            raise ErrInvalidArgument("agc: params are (7,) -- ref, attack, decay, floor, g0, gmin, gmax -- or (rows, 7) with per_row")
        return p

    def plan(self):
        """(rows per wave, samples per tile, form): the form is AGC_FORM_PER_ROW | AGC_FORM_COMPLEX."""
        return self._plan()

    def push(self, samples, out=None, track=None):
        """Run every sample of every row of `samples` through the loop -> the levelled rows, or (rows, track) where a
        track is asked for.  `out`, when given, is a buffer of the samples' type ((cap,), or (rows, cap) with any row
        pitch; columns past the samples are left as they are); it may be `samples` itself: the rows are levelled in
        place.  `track` is True (a new float32 array) or a float32 buffer of that form: the gain applied to every
        sample (level turns it into the row's level)."""
        return self._push_tracked(samples, self.kind, self._dtype, out, track)

    def set_params(self, params):
        """Exchange the parameters (same shape) between two pushes; the gains and the position stay."""
        p = self._check(params)
        self._call("set_params", p.ctypes.data_as(_PF))
        self.params = p

    def state(self):
        """(g, position): g is float32 (rows,), the gain of every row behind every push so far."""
        return self._state()

    def _state_shape(self):
        return (self.rows,)

    def set_state(self, g, position=0):
        super().set_state(g, position)


__all__ = ["Agc", "agc_rates", "level", "AGC_REAL_F32", "AGC_FORM_PER_ROW", "AGC_FORM_COMPLEX", "AGC_MAX_ROWS"]

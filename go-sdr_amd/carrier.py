"""The carrier recovery bank (include/hzsdr_carrier.h): a Costas loop or a PLL over one complex64 row, or over many rows,
one derotated output per input.

    alpha, beta = hz.carrier_gains(0.01)                 # a loop of 0.01 cycles per sample of noise bandwidth
    cr = ctx.carrier_loop(hz.CARRIER_QPSK, (alpha, beta, 0.0, -0.02, 0.02), rows=100)
    soft, counts = ts.push(cr.push(tuned))               # the tuner's complex64 block as it is, any row pitch
    y, f = cr.push(tuned, track=True)                    # f: the frequency estimate behind every sample, cycles / sample

A second-order loop around a numerically controlled oscillator: a 32-bit phase and a 32-bit frequency per row, a unit
vector made without a table, a phase detector -- CARRIER_TONE (e = im y: a pilot, a residual carrier, FM by PLL),
CARRIER_BPSK (e = re y im y) or CARRIER_QPSK (e = sign(re y) im y - sign(im y) re y) -- clipped to [-1, 1], and two
integer updates (the header has the step).  The state carries from push to push, so outputs, track and state do not
depend on how the stream is cut, on the memory space, on the number of rows, on any pitch or on the other rows.  A NaN
stays in its sample.  One row runs at one lane's rate: the parallelism is across the rows.

The detectors are amplitude-dependent: put the AGC bank (include/hzsdr_agc.h, Context.agc) in front to bring the rows
to unit symbol amplitude, or scale the gains by the amplitude.

Not here: decision-directed detectors for 8PSK or QAM, a lock indicator.
"""
import ctypes as C
import math

import numpy as np

from . import ErrInvalidArgument, FMT_C64, lib
from ._rows import RowWaveBank
from ._capi import CARRIER_BPSK, CARRIER_FORM_MODE, CARRIER_FORM_PER_ROW, CARRIER_MAX_ROWS, CARRIER_QPSK, CARRIER_TONE

_PF = C.POINTER(C.c_float)


def carrier_gains(bandwidth, damping=0.7071):
    """(alpha, beta) of a second-order loop of noise bandwidth `bandwidth` (cycles per sample) and damping zeta, for a
    detector of unit slope, in turns per unit error:  theta_n = bw / (zeta + 1 / (4 zeta)),
    d = 1 + 2 zeta theta_n + theta_n^2,  alpha = 4 zeta theta_n / d / (2 pi),  beta = 4 theta_n^2 / d / (2 pi)."""
    bw, zeta = float(bandwidth), float(damping)
    if not (bw > 0.0 and zeta > 0.0):
        raise ValueError("carrier_gains: bandwidth and damping are positive")
    tn = bw / (zeta + 1.0 / (4.0 * zeta))
    d = 1.0 + 2.0 * zeta * tn + tn * tn
    return 4.0 * zeta * tn / d / (2.0 * math.pi), 4.0 * tn * tn / d / (2.0 * math.pi)


class CarrierLoop(RowWaveBank):
    """hzsdr_carrier: push(rows) -> the derotated rows.  `mode` is CARRIER_TONE, CARRIER_BPSK or CARRIER_QPSK.  One row
    takes (n,) complex64 samples; `rows` = R > 1 takes (R, n) with unit stride along a row and any row pitch and returns
    (R, n).  `params` is float32 (5,) -- alpha, beta, f0, fmin, fmax -- shared by all rows, or (R, 5), one set per row.
    numpy in a HOST context; torch tensors on the context's device, written on the context's stream, in a DEVICE
    context."""

    _c, _noun = "carrier", "carrier loop"
    _state_c, _state_msg = C.c_uint32, "the state is uint32 (rows, 2)"

    def __init__(self, ctx, mode, params, rows=1, per_row=False):
        self.mode = int(mode)
        self._open(ctx, rows)
        self.per_row = bool(per_row)
        self.params = self._check(params)
        ctx._ck(lib.hzsdr_carrier_create(ctx._h, self.mode, self.params.ctypes.data_as(_PF), int(self.per_row), self.rows, C.byref(self._h)))

    def _check(self, params):
        p = np.ascontiguousarray(params, np.float32)
        if p.shape != ((self.rows, 5) if self.per_row else (5,)):
            raise ErrInvalidArgument("carrier loop: params are (5,) -- alpha, beta, f0, fmin, fmax -- or (rows, 5) with per_row")
        return p

    def plan(self):
        """(rows per wave, samples per tile, form): the form is CARRIER_FORM_PER_ROW (or 0) plus mode * CARRIER_FORM_MODE."""
        return self._plan()

    def push(self, samples, out=None, track=None):
        """Run every sample of every row of `samples` through the loop -> the derotated rows, or (rows, track) where a
        track is asked for.  `out`, when given, is a complex64 buffer ((cap,), or (rows, cap) with any row pitch;
        columns past the samples are left as they are); it may be `samples` itself: the rows are derotated in place.
        `track` is True (a new float32 array) or a float32 buffer of that form: the frequency estimate behind every
        sample, in cycles per sample."""
        return self._push_tracked(samples, FMT_C64, np.complex64, out, track)

    def set_params(self, params):
        """Exchange the parameters (same shape) between two pushes; theta, F and the position stay."""
        p = self._check(params)
        self._call("set_params", p.ctypes.data_as(_PF))
        self.params = p

    def state(self):
        """(z, position): z is uint32 (rows, 2) -- theta (2^32 to the turn) and F (an int32's bits, phase units per
        sample: z[:, 1].view(int32) * 2^-32 is the measured offset in cycles per sample); behind every push so far."""
        return self._state()

    def _state_shape(self):
        return (self.rows, 2)


__all__ = ["CarrierLoop", "carrier_gains", "CARRIER_TONE", "CARRIER_BPSK", "CARRIER_QPSK", "CARRIER_FORM_PER_ROW", "CARRIER_FORM_MODE",
           "CARRIER_MAX_ROWS"]

"""The polyphase rational resampler (include/hzsdr_resampler.h): the rate of one stream, or of many rows, times U/D.

    rs = ctx.resampler(hz.FMT_C64, 4, 1, streams=256)       # 12.5 kHz channelizer rows -> 50 kHz
    y = rs.push(channels)            # channels: (256, frames) complex64 with any row pitch; y: (256, frames * 4)
    tail = rs.flush()                # the outputs that still depend on samples pushed

With phi_m = (m D) mod U and i_m = floor(m D / U),

    y[m] = sum_q taps[phi_m + q U] * c(x[i_m - q])

i.e. scipy.signal.upfirdn(taps, x, U, D): zero-stuff by U, filter, keep every D-th.  U and D are not reduced.  The bits
do not depend on how the stream is cut into pushes, on the memory space, on the number of streams or on the pitch.
"""
import ctypes as C

import numpy as np

from . import ErrDstTooSmall, ErrInvalidArgument, FMT_C64, FMT_I8, FMT_I16, FMT_U8, lib  # noqa: F401
from ._rows import cut, device_like, rows_input, rows_output
from ._capi import RESAMPLER_FORM_DIRECT, RESAMPLER_FORM_TAPS_GLOBAL, RESAMPLER_FORM_TAPS_UNIFORM, RESAMPLER_FORM_WINDOW_PADDED



def resampler_taps(up, down, taps_per_phase=16, beta=8.0):
    """A filter for the ratio up/down: the Kaiser-windowed (beta) sinc with its cutoff at 1 / max(up, down) of the
    zero-stuffed stream's Nyquist frequency, taps_per_phase * up values formed in float64, scaled to sum `up` (every
    phase then sums to about 1), rounded once to float32."""
    u, d, p = int(up), int(down), int(taps_per_phase)
    if u <= 0 or d <= 0 or p <= 0:
        raise ValueError("resampler_taps: up, down and taps_per_phase are at least 1")
    n = u * p
    t = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
    h = np.sinc(t / max(u, d)) * np.kaiser(n, float(beta))
    return (h * (u / h.sum())).astype(np.float32)


class Resampler:
    """hzsdr_resampler: push(samples) -> the outputs they complete, complex64; flush() -> the rest of the stream.
    One stream takes (n,) samples ((n, 2) for the byte and int16 formats) and returns (count,); `streams` = R > 1
    takes (R, n) rows with unit stride along a row and any row pitch (a view of a wider buffer, as the channelizer's
    channel-major output is) and returns (R, count).  numpy in a HOST context; torch tensors on the context's
    device, written on the context's stream, in a DEVICE context."""

    def __init__(self, ctx, src_fmt, up, down, taps=None, streams=1):
        self.ctx, self.src_fmt, self.up, self.down, self.streams = ctx, src_fmt, int(up), int(down), int(streams)
        if self.up <= 0 or self.down <= 0 or self.streams <= 0:
            raise ErrInvalidArgument("resampler: up, down and streams are at least 1")
        if taps is None:
            taps = resampler_taps(self.up, self.down)
        self.taps = np.ascontiguousarray(taps, np.float32).reshape(-1)
        self._h = C.c_void_p()
        ctx._ck(lib.hzsdr_resampler_create(ctx._h, src_fmt, self.up, self.down, self.taps.ctypes.data_as(C.POINTER(C.c_float)),
                                           self.taps.shape[0], self.streams, C.byref(self._h)))

    def outputs_for(self, n_in):
        """The outputs per stream a push of n_in samples would write now."""
        c = C.c_size_t(0)
        self.ctx._ck(lib.hzsdr_resampler_outputs_for(self._h, int(n_in), C.byref(c)))
        return c.value

    def pending(self):
        """(samples consumed, index of the next output, outputs a flush would write now), per stream."""
        n, m, f = C.c_uint64(0), C.c_uint64(0), C.c_size_t(0)
        self.ctx._ck(lib.hzsdr_resampler_pending(self._h, C.byref(n), C.byref(m), C.byref(f)))
        return n.value, m.value, f.value

    def plan(self):
        """(outputs per workgroup, kernel form): the form is a sum of RESAMPLER_FORM_DIRECT (no input window in LDS),
        RESAMPLER_FORM_TAPS_GLOBAL (the polyphase table is read from memory, not LDS), RESAMPLER_FORM_TAPS_UNIFORM
        (U divides D: the one row in use is read as scalars common to a wave) and RESAMPLER_FORM_WINDOW_PADDED (the
        window in LDS has one empty slot behind every 32 samples)."""
        t, f = C.c_size_t(0), C.c_int32(0)
        self.ctx._ck(lib.hzsdr_resampler_plan(self._h, C.byref(t), C.byref(f)))
        return t.value, f.value

    def push(self, samples, out=None):
        """Consume every sample of every row of `samples`; return the outputs they complete.  `out`, when given, is a
        complex64 buffer ((cap,), or (streams, cap) with any row pitch; columns past the outputs written are left as
        they are); the result is its written part."""
        ptr, n, pitch = rows_input(samples, self.src_fmt, self.streams, "resampler")
        out, optr, cap, opitch = rows_output(out, self.outputs_for(n), samples, self.streams, np.complex64, "resampler")
        got = C.c_size_t(0)
        self.ctx._ck(lib.hzsdr_resampler_push(self._h, ptr, n, pitch, optr if cap else None, cap, opitch, C.byref(got)))
        return cut(out, self.streams, got.value)

    def flush(self, out=None):
        """The outputs that still depend on samples pushed, the samples behind the last one taken as zero; the
        resampler starts over.  Pushes and flush together have scipy.signal.upfirdn's length."""
        out, optr, cap, opitch = rows_output(out, self.pending()[2], device_like(self.ctx), self.streams, np.complex64, "resampler")
        got = C.c_size_t(0)
        self.ctx._ck(lib.hzsdr_resampler_flush(self._h, optr if cap else None, cap, opitch, C.byref(got)))
        return cut(out, self.streams, got.value)

    def reset(self):
        self.ctx._ck(lib.hzsdr_resampler_reset(self._h))

    def sample_rate(self, input_rate):
        """The sample rate of the output: input_rate * up / down."""
        return float(input_rate) * self.up / self.down

    def close(self):
        if self._h:
            lib.hzsdr_resampler_free(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


__all__ = ["Resampler", "resampler_taps", "RESAMPLER_FORM_DIRECT", "RESAMPLER_FORM_TAPS_GLOBAL",
           "RESAMPLER_FORM_TAPS_UNIFORM", "RESAMPLER_FORM_WINDOW_PADDED"]

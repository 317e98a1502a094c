"""The demodulator bank (include/hzsdr_demod.h): FM, phase, envelope or power of one stream, or of many rows.

    fm = ctx.demodulator(hz.FMT_C64, hz.DEMOD_FM, hz.fm_gain(50e3, 5e3) * lowpass, down=5, streams=256)
    audio = fm.push(rows)            # rows: (256, n) complex64 with any row pitch; audio: (256, ceil(n / 5)) float32
    tail = fm.flush()                # the outputs that still depend on samples pushed

With a = c(x[n]) and b = c(x[n - 1]), d[n] = angle(a conj(b)) (FM), angle(a) (PHASE), |a| (ENVELOPE) or |a|^2 (POWER)
in float32, and

    y[m] = sum_q taps[q] * d[m D - q]

i.e. scipy.signal.upfirdn(taps, d, 1, D).  The default taps [1.0] with D = 1 are the bare detector.  The bits do not
depend on how the stream is cut into pushes, on the memory space, on the number of streams or on either pitch.
"""
import ctypes as C
import math

import numpy as np

from . import ErrDstTooSmall, ErrInvalidArgument, FMT_C64, FMT_I8, FMT_I16, FMT_U8, lib  # noqa: F401
from ._rows import cut, device_like, rows_input, rows_output
from ._capi import DEMOD_ENVELOPE, DEMOD_FM, DEMOD_FORM_HALF_TILE, DEMOD_FORM_TRANSPOSED, DEMOD_PHASE, DEMOD_POWER



def fm_gain(sample_rate, deviation):
    """The factor that turns the FM detector's radians per sample into units of the deviation: a tone `deviation` Hz
    off the carrier reads 1.0 after it.  sample_rate / (2 pi deviation), to be folded into the taps."""
    fs, dev = float(sample_rate), float(deviation)
    if not (fs > 0.0 and dev > 0.0):
        raise ValueError("fm_gain: sample_rate and deviation are positive")
    return fs / (2.0 * math.pi * dev)


class Demodulator:
    """hzsdr_demod: push(samples) -> the outputs they complete, float32; flush() -> the rest of the stream.  One
    stream takes (n,) samples ((n, 2) for the byte and int16 formats) and returns (count,); `streams` = R > 1 takes
    (R, n) rows with unit stride along a row and any row pitch (a view of a wider buffer, as the channelizer's
    channel-major output is) and returns (R, count).  numpy in a HOST context; torch tensors on the context's device,
    written on the context's stream, in a DEVICE context."""

    def __init__(self, ctx, src_fmt, mode, taps=None, down=1, streams=1):
        self.ctx, self.src_fmt, self.mode, self.down, self.streams = ctx, src_fmt, int(mode), int(down), int(streams)
        if self.down <= 0 or self.streams <= 0:
            raise ErrInvalidArgument("demodulator: down and streams are at least 1")
        if taps is None:
            taps = np.ones(1, np.float32)
        self.taps = np.ascontiguousarray(taps, np.float32).reshape(-1)
        self._h = C.c_void_p()
        ctx._ck(lib.hzsdr_demod_create(ctx._h, src_fmt, self.mode, self.down, self.taps.ctypes.data_as(C.POINTER(C.c_float)),
                                       self.taps.shape[0], self.streams, C.byref(self._h)))

    def outputs_for(self, n_in):
        """The outputs per stream a push of n_in samples would write now."""
        c = C.c_size_t(0)
        self.ctx._ck(lib.hzsdr_demod_outputs_for(self._h, int(n_in), C.byref(c)))
        return c.value

    def pending(self):
        """(samples consumed, index of the next output, outputs a flush would write now), per stream."""
        n, m, f = C.c_uint64(0), C.c_uint64(0), C.c_size_t(0)
        self.ctx._ck(lib.hzsdr_demod_pending(self._h, C.byref(n), C.byref(m), C.byref(f)))
        return n.value, m.value, f.value

    def plan(self):
        """(outputs per workgroup, kernel form): the form is a sum of DEMOD_FORM_HALF_TILE (128 outputs per workgroup:
        the window of 256 is past the LDS budget) and DEMOD_FORM_TRANSPOSED (the window in LDS is stored as `down`
        rows; whenever down > 1)."""
        t, f = C.c_size_t(0), C.c_int32(0)
        self.ctx._ck(lib.hzsdr_demod_plan(self._h, C.byref(t), C.byref(f)))
        return t.value, f.value

    def push(self, samples, out=None):
        """Consume every sample of every row of `samples`; return the outputs they complete.  `out`, when given, is a
        float32 buffer ((cap,), or (streams, cap) with any row pitch; columns past the outputs written are left as
        they are); the result is its written part."""
        ptr, n, pitch = rows_input(samples, self.src_fmt, self.streams, "demodulator")
        out, optr, cap, opitch = rows_output(out, self.outputs_for(n), samples, self.streams, np.float32, "demodulator")
        got = C.c_size_t(0)
        self.ctx._ck(lib.hzsdr_demod_push(self._h, ptr, n, pitch, optr if cap else None, cap, opitch, C.byref(got)))
        return cut(out, self.streams, got.value)

    def flush(self, out=None):
        """The outputs that still depend on samples pushed, the detector values behind the last sample taken as zero;
        the demodulator starts over.  Pushes and flush together have scipy.signal.upfirdn(taps, d, 1, down)'s length."""
        out, optr, cap, opitch = rows_output(out, self.pending()[2], device_like(self.ctx), self.streams, np.float32, "demodulator")
        got = C.c_size_t(0)
        self.ctx._ck(lib.hzsdr_demod_flush(self._h, optr if cap else None, cap, opitch, C.byref(got)))
        return cut(out, self.streams, got.value)

    def reset(self):
        self.ctx._ck(lib.hzsdr_demod_reset(self._h))

    def sample_rate(self, input_rate):
        """The sample rate of the output: input_rate / down."""
        return float(input_rate) / self.down

    def close(self):
        if self._h:
            lib.hzsdr_demod_free(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


__all__ = ["Demodulator", "fm_gain", "DEMOD_FM", "DEMOD_PHASE", "DEMOD_ENVELOPE", "DEMOD_POWER", "DEMOD_FORM_HALF_TILE",
           "DEMOD_FORM_TRANSPOSED"]

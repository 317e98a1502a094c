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

from . import _is_torch, ErrDstTooSmall, ErrInvalidArgument, FMT_C64, FMT_I8, FMT_I16, FMT_U8, lib, MEM_HOST  # noqa: F401
from ._capi import RESAMPLER_FORM_DIRECT, RESAMPLER_FORM_TAPS_GLOBAL, RESAMPLER_FORM_TAPS_UNIFORM, RESAMPLER_FORM_WINDOW_PADDED

_NP_IN = {FMT_C64: (np.complex64, 8), FMT_U8: (np.uint8, 2), FMT_I8: (np.int8, 2), FMT_I16: (np.int16, 4)}


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

    def _input(self, x):
        """-> (pointer, samples per row, row pitch in samples) of a block of the source format."""
        dt, size = _NP_IN[self.src_fmt]
        torch_in = _is_torch(x)
        if torch_in:
            import torch
            tdt = {np.complex64: torch.complex64, np.uint8: torch.uint8, np.int8: torch.int8, np.int16: torch.int16}[dt]
            if x.dtype != tdt:
                raise ValueError("resampler: samples are not of the source format")
            strides, ptr, item = tuple(x.stride()), x.data_ptr(), x.element_size()
        else:
            if x.dtype != dt:
                raise ValueError("resampler: samples are not of the source format")
            item = x.dtype.itemsize
            strides, ptr = tuple(s // item for s in x.strides), x.ctypes.data
        shape = tuple(x.shape)
        per = size // item  # elements per sample: 1 for complex64, 2 (I, Q) otherwise
        if per == 2:
            if not shape or shape[-1] != 2 or (strides[-1] != 1 and shape[-1] > 1):
                raise ValueError("resampler: samples of this format are (..., n, 2)")
            shape, strides = shape[:-1], strides[:-1]
        if self.streams == 1 and len(shape) == 1:
            shape, strides = (1,) + shape, (0,) + strides
        if len(shape) != 2 or shape[0] != self.streams:
            raise ValueError("resampler: input is (n,) for one stream, (streams, n) otherwise")
        n = int(shape[1])
        if n == 0:
            return None, 0, 0
        if (n > 1 and strides[1] != per) or (self.streams > 1 and (strides[0] % per or strides[0] // per < n)):
            raise ValueError("resampler: rows are contiguous, their pitch at least the samples of a row")
        return ptr, n, int(strides[0] // per) if self.streams > 1 else n

    def _empty(self, count, like):
        shape = (count,) if self.streams == 1 else (self.streams, count)
        if _is_torch(like):
            import torch
            return torch.empty(shape, dtype=torch.complex64, device=like.device)
        return np.empty(shape, np.complex64)

    def _output(self, out, count, like):
        """-> (out, pointer, capacity, pitch) of a complex64 destination: (cap,) for one stream, (streams, cap) rows
        with unit stride along a row and any pitch otherwise."""
        if out is None:
            out = self._empty(count, like)
        torch_out = _is_torch(out)
        if torch_out:
            import torch
            ok = out.dtype == torch.complex64
            strides, ptr = tuple(out.stride()), out.data_ptr()
        else:
            ok = out.dtype == np.complex64
            strides, ptr = tuple(s // 8 for s in out.strides), out.ctypes.data
        if not ok:
            raise ValueError("resampler: the destination is complex64")
        if self.streams == 1:
            if out.ndim != 1 or (out.shape[0] > 1 and strides[0] != 1):
                raise ValueError("resampler: the destination of one stream is a contiguous (cap,)")
            return out, ptr, int(out.shape[0]), int(out.shape[0])
        if out.ndim != 2 or out.shape[0] != self.streams or (out.shape[1] > 1 and strides[1] != 1) or strides[0] < out.shape[1]:
            raise ValueError("resampler: the destination is (streams, cap) with contiguous rows")
        return out, ptr, int(out.shape[1]), int(strides[0])

    def _like(self):
        if self.ctx.memspace == MEM_HOST:
            return None
        import torch
        return torch.empty(0, device=f"cuda:{self.ctx.device}")

    def _cut(self, out, got):
        return out[:got] if self.streams == 1 else out[:, :got]

    def push(self, samples, out=None):
        """Consume every sample of every row of `samples`; return the outputs they complete.  `out`, when given, is a
        complex64 buffer ((cap,), or (streams, cap) with any row pitch; columns past the outputs written are left as
        they are); the result is its written part."""
        ptr, n, pitch = self._input(samples)
        out, optr, cap, opitch = self._output(out, self.outputs_for(n), samples)
        got = C.c_size_t(0)
        self.ctx._ck(lib.hzsdr_resampler_push(self._h, ptr, n, pitch, optr if cap else None, cap, opitch, C.byref(got)))
        return self._cut(out, got.value)

    def flush(self, out=None):
        """The outputs that still depend on samples pushed, the samples behind the last one taken as zero; the
        resampler starts over.  Pushes and flush together have scipy.signal.upfirdn's length."""
        out, optr, cap, opitch = self._output(out, self.pending()[2], self._like())
        got = C.c_size_t(0)
        self.ctx._ck(lib.hzsdr_resampler_flush(self._h, optr if cap else None, cap, opitch, C.byref(got)))
        return self._cut(out, got.value)

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

"""The channel bank (include/hzsdr_chanbank.h): the polyphase channelizer for the small channel counts, any M from 2
to 255, powers of two or not.

    taps = channelizer_taps(100, 8)
    bank = ctx.channel_bank(hz.FMT_U8, 100, taps, layout="channels")   # 100 FM channels of 200 kHz out of 20 MHz
    y = bank.push(samples)           # (100, frames) complex64: row pos(k) is channel k at the rate fs / hop

Frame j covers stream samples [jD, jD + L), L = len(taps) = P * M, and

    y[j][k] = sum_i taps[i] * c(x[jD + i]) * exp(-2 pi i k (jD + i) / M)

exactly the channelizer's meaning; channelizer.Channelizer takes over at M = 256.  The rows of layout "channels" are
what ctx.resampler(..., streams=M) and ctx.demodulator(..., streams=M) take as they are.  The bits of a frame do not
depend on how the stream is cut into pushes, on the memory space, on the layout, the order or the pitch.
"""
import ctypes as C

import numpy as np

from . import _is_torch, _ptr, ErrDstTooSmall, ErrInvalidArgument, length, lib  # noqa: F401  (ErrDstTooSmall: re-export)
from ._capi import (CHANBANK_FORM_A_LDS, CHANBANK_READ_DFT, CHANBANK_READ_TAPS, CHANNELIZER_CHANNEL_MAJOR,
                    CHANNELIZER_FRAME_MAJOR)
from .channelizer import _LAYOUTS, channelizer_taps
from .spectrum import NegativeFirst, ZeroFirst, _order


class ChannelBank:
    """hzsdr_chanbank: push(samples) -> the frames that complete, complex64, (frames, M) for layout "frames" or
    (M, frames) for layout "channels" (numpy for a HOST context, a torch tensor on the samples' device, written on the
    context's stream, for a DEVICE context).  channelizer.Channelizer's interface, and plan() and readout()."""

    def __init__(self, ctx, src_fmt, channels, taps, hop=None, order=NegativeFirst, layout="frames"):
        self.ctx, self.src_fmt, self.channels = ctx, src_fmt, int(channels)
        self.hop = self.channels if hop is None else int(hop)
        self.order = _order(order)
        if layout not in _LAYOUTS:
            raise ValueError(f"channel bank: unknown layout {layout!r}")
        self.layout = _LAYOUTS[layout]
        self.taps = np.ascontiguousarray(taps, np.float32).reshape(-1)
        if self.channels <= 0 or self.hop <= 0:
            raise ErrInvalidArgument("channel bank: channels and hop are at least 1")
        self._h = C.c_void_p()
        ctx._ck(lib.hzsdr_chanbank_create(ctx._h, src_fmt, self.channels, self.taps.ctypes.data_as(C.POINTER(C.c_float)),
                                          self.taps.shape[0], self.hop, self.order, self.layout, C.byref(self._h)))

    @property
    def channel_major(self):
        return self.layout == CHANNELIZER_CHANNEL_MAJOR

    def frames_for(self, n_in):
        """The frames a push of n_in samples would write now."""
        f = C.c_size_t(0)
        self.ctx._ck(lib.hzsdr_chanbank_frames_for(self._h, int(n_in), C.byref(f)))
        return f.value

    def push(self, samples, out=None):
        """Consume every sample of `samples`; return the frames that complete.  `out`, when given, is a complex64
        buffer: (cap, M) contiguous rows for layout "frames"; (M, cap) rows with unit stride along a row and any pitch
        for layout "channels" (columns past the frames written are left as they are); the result is its written part."""
        n_in = length(samples)
        frames = self.frames_for(n_in)
        m = self.channels
        if out is None:
            shape = (m, frames) if self.channel_major else (frames, m)
            if _is_torch(samples):
                import torch
                out = torch.empty(shape, dtype=torch.complex64, device=samples.device)
            else:
                out = np.empty(shape, np.complex64)
        if self.channel_major:
            if out.ndim != 2 or out.shape[0] != m:
                raise ValueError("channel bank: a channel-major destination is (channels, cap)")
            strides = tuple(out.stride()) if _is_torch(out) else tuple(s // 8 for s in out.strides)
            if (out.shape[1] > 1 and strides[1] != 1) or strides[0] < out.shape[1]:
                raise ValueError("channel bank: a channel-major destination has contiguous rows")
            cap, stride = int(out.shape[1]), int(strides[0])
            optr = out.data_ptr() if _is_torch(out) else out.ctypes.data  # (rows with a pitch are not contiguous)
        else:
            cap, stride, optr = int(np.prod(out.shape)) // m, 0, _ptr(out)
        got = C.c_size_t(0)
        self.ctx._ck(lib.hzsdr_chanbank_push(self._h, _ptr(samples) if n_in else None, n_in, optr if cap else None, cap, stride,
                                             C.byref(got)))
        if self.channel_major:
            return out[:, :got.value]
        return out[:got.value] if out.ndim == 2 else out[:got.value * m]

    def pending(self):
        """(samples held for the next frame, index of the next frame)."""
        h, j = C.c_size_t(0), C.c_uint64(0)
        self.ctx._ck(lib.hzsdr_chanbank_pending(self._h, C.byref(h), C.byref(j)))
        return h.value, j.value

    def reset(self):
        self.ctx._ck(lib.hzsdr_chanbank_reset(self._h))

    def channel_rate(self, sample_rate):
        """The sample rate of every channel: sample_rate / hop."""
        return float(sample_rate) / self.hop

    def close(self):
        if self._h:
            lib.hzsdr_chanbank_free(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def plan(self):
        """(frames per workgroup, rows of the real matrix per workgroup -- two per channel and the padding rows --,
        kernel form): tile i of a push holds its frames [i * tile_frames, (i + 1) * tile_frames); the form is
        CHANBANK_FORM_A_LDS where the matrix is staged in LDS beside the folded frames."""
        t, r, f = C.c_size_t(0), C.c_size_t(0), C.c_int32(0)
        self.ctx._ck(lib.hzsdr_chanbank_plan(self._h, C.byref(t), C.byref(r), C.byref(f)))
        return t.value, r.value, f.value

    def readout(self, what, index=0):
        """The host-made operands as the kernel uses them: CHANBANK_READ_DFT -> row `index` of the DFT table (the
        channels rounded up to an even count of complex64 values); CHANBANK_READ_TAPS -> the prototype, float32."""
        if what == CHANBANK_READ_TAPS:
            out = np.empty(self.taps.shape[0], np.float32)
        else:
            out = np.empty((self.channels + 1) // 2 * 2, np.complex64)
        self.ctx._ck(lib.hzsdr_chanbank_readout(self._h, int(what), int(index), out.ctypes.data, out.shape[0]))
        return out

    def channel_center(self, k, sample_rate):
        """The signed center frequency of output position k (row k of layout "channels", column k of "frames"):
        ZeroFirst 0, fs/M, ... floor((M - 1) / 2) fs/M, then the negative ones ascending to -fs/M; NegativeFirst
        ascending from -floor(M / 2) fs/M (numpy's fftshift, for odd M too)."""
        m = self.channels
        if k < 0 or k >= m:
            raise IndexError("channel bank: channel position out of range")
        idx = (k - m if k > (m - 1) // 2 else k) if self.order == ZeroFirst else k - m // 2
        return float(sample_rate) * idx / m


__all__ = ["ChannelBank", "channelizer_taps", "ZeroFirst", "NegativeFirst", "CHANNELIZER_FRAME_MAJOR", "CHANNELIZER_CHANNEL_MAJOR",
           "CHANBANK_FORM_A_LDS", "CHANBANK_READ_DFT", "CHANBANK_READ_TAPS"]

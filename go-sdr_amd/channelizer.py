"""The polyphase channelizer (include/hzsdr_channelizer.h): one wide IQ stream split into M channels per push.

    taps = channelizer_taps(1024, 8)
    ch = ctx.channelizer(hz.FMT_U8, 1024, taps, hop=512, layout="channels")
    y = ch.push(samples)             # (1024, frames) complex64: row pos(k) is channel k at the rate fs / hop

Frame j covers stream samples [jD, jD + L), L = len(taps) = P * M, and

    y[j][k] = sum_i taps[i] * c(x[jD + i]) * exp(-2 pi i k (jD + i) / M)

i.e. channel k is Shift(-k fs / M) with phase zero at stream position 0, the FIR whose impulse response is the taps
reversed, and every D-th output.  The bits do not depend on how the stream is cut into pushes, on the memory space or
on the layout.
"""
import ctypes as C

import numpy as np

from . import _is_torch, _ptr, ErrDstTooSmall, ErrInvalidArgument, length, lib  # noqa: F401  (ErrDstTooSmall: re-export)
from ._capi import CHANNELIZER_CHANNEL_MAJOR, CHANNELIZER_FRAME_MAJOR
from .spectrum import NegativeFirst, ZeroFirst, _order

_LAYOUTS = {"frames": CHANNELIZER_FRAME_MAJOR, "channels": CHANNELIZER_CHANNEL_MAJOR,
            CHANNELIZER_FRAME_MAJOR: CHANNELIZER_FRAME_MAJOR, CHANNELIZER_CHANNEL_MAJOR: CHANNELIZER_CHANNEL_MAJOR}


def channelizer_taps(channels, taps_per_channel, beta=8.0):
    """A prototype for `channels` channels: the Kaiser-windowed (beta) sinc with its cutoff at fs / (2 channels),
    channels * taps_per_channel values formed in float64, scaled to a DC gain of 1, rounded once to float32."""
    m, p = int(channels), int(taps_per_channel)
    if m <= 0 or p <= 0:
        raise ValueError("channelizer_taps: channels and taps_per_channel are at least 1")
    n = m * p
    t = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
    h = np.sinc(t / m) * np.kaiser(n, float(beta))
    return (h / h.sum()).astype(np.float32)


class Channelizer:
    """hzsdr_channelizer: push(samples) -> the frames that complete, complex64, (frames, M) for layout "frames" or
    (M, frames) for layout "channels" (numpy for a HOST context, a torch tensor on the samples' device, written on the
    context's stream, for a DEVICE context)."""

    def __init__(self, ctx, src_fmt, channels, taps, hop=None, order=NegativeFirst, layout="frames"):
        self.ctx, self.src_fmt, self.channels = ctx, src_fmt, int(channels)
        self.hop = self.channels if hop is None else int(hop)
        self.order = _order(order)
        if layout not in _LAYOUTS:
            raise ValueError(f"channelizer: unknown layout {layout!r}")
        self.layout = _LAYOUTS[layout]
        self.taps = np.ascontiguousarray(taps, np.float32).reshape(-1)
        if self.channels <= 0 or self.hop <= 0:
            raise ErrInvalidArgument("channelizer: channels and hop are at least 1")
        self._h = C.c_void_p()
        ctx._ck(lib.hzsdr_channelizer_create(ctx._h, src_fmt, self.channels, self.taps.ctypes.data_as(C.POINTER(C.c_float)),
                                             self.taps.shape[0], self.hop, self.order, self.layout, C.byref(self._h)))

    @property
    def channel_major(self):
        return self.layout == CHANNELIZER_CHANNEL_MAJOR

    def frames_for(self, n_in):
        f = C.c_size_t(0)
        self.ctx._ck(lib.hzsdr_channelizer_frames_for(self._h, int(n_in), C.byref(f)))
        return f.value

    def push(self, samples, out=None):
        """Consume every sample of `samples`; return the frames that complete.  `out`, when given, is a complex64
        buffer: (cap, M) rows for layout "frames", (M, stride) for layout "channels" (columns past the frames written
        are left as they are); the result is its written part."""
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
                raise ValueError("channelizer: a channel-major destination is (channels, stride)")
            cap = stride = int(out.shape[1])
        else:
            cap, stride = int(np.prod(out.shape)) // m, 0
        got = C.c_size_t(0)
        self.ctx._ck(lib.hzsdr_channelizer_push(self._h, _ptr(samples) if n_in else None, n_in,
                                                _ptr(out) if cap else None, cap, stride, C.byref(got)))
        if self.channel_major:
            return out[:, :got.value]
        return out[:got.value] if out.ndim == 2 else out[:got.value * m]

    def pending(self):
        """(samples held for the next frame, index of the next frame)."""
        h, j = C.c_size_t(0), C.c_uint64(0)
        self.ctx._ck(lib.hzsdr_channelizer_pending(self._h, C.byref(h), C.byref(j)))
        return h.value, j.value

    def reset(self):
        self.ctx._ck(lib.hzsdr_channelizer_reset(self._h))

    def channel_rate(self, sample_rate):
        """The sample rate of every channel: sample_rate / hop."""
        return float(sample_rate) / self.hop

    def channel_center(self, k, sample_rate):
        """The signed center frequency of output position k (row k of layout "channels", column k of "frames") in
        the channelizer's order: ZeroFirst 0, fs/M, ... then -fs/2 ... -fs/M; NegativeFirst -fs/2 ... fs/2 - fs/M."""
        m = self.channels
        if k < 0 or k >= m:
            raise IndexError("channelizer: channel position out of range")
        idx = (k - m if k >= m // 2 else k) if self.order == ZeroFirst else k - m // 2
        return float(sample_rate) * idx / m

    def close(self):
        if self._h:
            lib.hzsdr_channelizer_free(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


__all__ = ["Channelizer", "channelizer_taps", "ZeroFirst", "NegativeFirst", "CHANNELIZER_FRAME_MAJOR",
           "CHANNELIZER_CHANNEL_MAJOR"]

"""The polyphase synthesis bank (include/hzsdr_synthesizer.h): M channels put back into one wide IQ stream per push.

    g = channelizer_taps(1024, 8)
    sy = ctx.synthesizer(hz.FMT_C64, 1024, g, hop=512, layout="channels")
    x = sy.push(y)                   # y: (1024, frames) complex64, row pos(k) is channel k; x: frames * 512 samples
    tail = sy.flush()                # the len(g) - 512 samples behind them

Input frame j lands at output positions [jD, jD + L), L = len(taps) = P * M, and

    x^[t] = sum_j taps[t - jD] * sum_k Y[j][k] exp(+2 pi i k t / M)

i.e. channel k is zero-stuffed by D, filtered by the taps and Shift(+k fs / M) with phase zero at position 0, and the
channels are summed: the adjoint of channelizer.Channelizer with the same taps, channels and hop.  The bits do not
depend on how the frames are cut into pushes, on the memory space or on the layout.
"""
import ctypes as C

import numpy as np

from . import _is_torch, _ptr, ErrDstTooSmall, ErrInvalidArgument, FMT_C64, FMT_I8, FMT_I16, FMT_U8, MEM_HOST  # noqa: F401
from ._capi import CHANNELIZER_CHANNEL_MAJOR, CHANNELIZER_FRAME_MAJOR
from ._polyphase import _PolyphaseBank
from ._rows import device_like, torch_dtype
from .spectrum import NegativeFirst, ZeroFirst

_NP_OUT = {FMT_C64: (np.complex64, ()), FMT_U8: (np.uint8, (2,)), FMT_I8: (np.int8, (2,)), FMT_I16: (np.int16, (2,))}


def wola_taps(channels):
    """The periodic square-root Hann of `channels` = M values, sqrt((1 - cos(2 pi i / M)) / 2) = sin(pi i / M), formed
    in float64 and rounded once to float32.  As the prototype of both banks at hop M / 2 the product window's shifted
    copies sum to 1 (sum_j g^2[t - j M / 2] = 1) and, L being M, no aliasing term exists: channelizer followed by
    synthesizer returns M times the input (weighted overlap-add)."""
    m = int(channels)
    if m <= 0:
        raise ValueError("wola_taps: channels is at least 1")
    return np.sin(np.pi * np.arange(m, dtype=np.float64) / m).astype(np.float32)


class Synthesizer(_PolyphaseBank):
    """hzsdr_synthesizer: push(frames) -> the frames * hop samples they complete, in the destination format (numpy for
    a HOST context, a torch tensor on the frames' device, written on the context's stream, for a DEVICE context);
    flush() -> the stream's tail.  The object's life, channel_major, reset and close are _polyphase._PolyphaseBank's."""
    _c, _noun = "synthesizer", "synthesizer"

    def __init__(self, ctx, dst_fmt, channels, taps, hop=None, order=NegativeFirst, layout="frames"):
        self.dst_fmt = dst_fmt
        self._open(ctx, dst_fmt, channels, taps, hop, order, layout)

    @property
    def group_frames(self):
        """Frames per internal launch group: a longer push is processed in groups of this many."""
        f = C.c_size_t(0)
        self._call("group_frames", C.byref(f))
        return f.value

    def _empty(self, n, like):
        """n samples of the destination format, where `like` lives"""
        dt, tail = _NP_OUT[self.dst_fmt]
        if _is_torch(like):
            import torch
            return torch.empty((n,) + tail, dtype=torch_dtype(dt), device=like.device)
        return np.empty((n,) + tail, dt)

    def _input(self, frames):
        """-> (pointer, frames, pitch) of a complex64 block in the synthesizer's layout: (frames, M) rows, or (M, frames)
        with unit stride along the frames and any row pitch (a view of a wider buffer, as the channelizer leaves it)."""
        m = self.channels
        torch_in = _is_torch(frames)
        if torch_in:
            import torch
            if frames.dtype != torch.complex64:
                raise ValueError("synthesizer: frames are complex64")
        elif frames.dtype != np.complex64:
            raise ValueError("synthesizer: frames are complex64")
        if not self.channel_major:
            n = int(np.prod(frames.shape))
            if n % m or (frames.ndim == 2 and frames.shape[1] != m) or frames.ndim > 2:
                raise ValueError("synthesizer: frame-major input is (frames, channels)")
            return (_ptr(frames) if n else None), n // m, 0
        if frames.ndim != 2 or frames.shape[0] != m:
            raise ValueError("synthesizer: channel-major input is (channels, frames)")
        f = int(frames.shape[1])
        if f == 0:
            return None, 0, 0
        if torch_in:
            s0, s1, ptr = frames.stride(0), frames.stride(1), frames.data_ptr()
        else:
            s0, s1, ptr = frames.strides[0] // 8, frames.strides[1] // 8, frames.ctypes.data
        if (f > 1 and s1 != 1) or s0 < f:
            raise ValueError("synthesizer: channel-major rows are contiguous, their pitch at least the frames")
        return ptr, f, int(s0)

    def push(self, frames, out=None):
        """Consume every frame of `frames`; return the frames * hop samples they complete.  `out`, when given, is a
        buffer of the destination format; the result is its written part."""
        ptr, f, pitch = self._input(frames)
        if out is None:
            out = self._empty(f * self.hop, frames)
        cap = int(out.shape[0])
        got = C.c_size_t(0)
        self._call("push", ptr, f, pitch, _ptr(out) if cap else None, cap, C.byref(got))
        return out[:got.value]

    def flush(self, out=None):
        """The held partial sums, i.e. the stream's last len(taps) - hop samples; the synthesizer starts over.  Without
        `out` the result is a numpy array in a HOST context and a torch tensor on the context's device otherwise."""
        held = self.pending()[0]
        if out is None:
            out = self._empty(held, device_like(self.ctx))
        cap = int(out.shape[0])
        got = C.c_size_t(0)
        self._call("flush", _ptr(out) if cap else None, cap, C.byref(got))
        return out[:got.value]

    def pending(self):
        """(partial sums held behind the samples written, index of the next frame)."""
        return self._pending()

    def sample_rate(self, channel_rate):
        """The sample rate of the output stream: channel_rate * hop."""
        return float(channel_rate) * self.hop


__all__ = ["Synthesizer", "wola_taps", "ZeroFirst", "NegativeFirst", "CHANNELIZER_FRAME_MAJOR", "CHANNELIZER_CHANNEL_MAJOR"]

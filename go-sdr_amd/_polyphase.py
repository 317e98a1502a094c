"""What the classes of the three polyphase banks (channelizer.Channelizer, chanbank.ChannelBank, synthesizer.Synthesizer)
are built on: the object's life and the calls around its pushes (csrc/hz_polyphase.h is the same layer in C).

_PolyphaseBank holds the create over a C prefix and a noun, the layout, pending, reset and close; _AnalysisBank adds what
the two analysis banks do alike: frames_for, push, channel_rate and channel_center.  The errors carry the calling class's
noun.
"""
import ctypes as C

import numpy as np

from . import _is_torch, _ptr, ErrInvalidArgument, length, lib
from ._capi import CHANNELIZER_CHANNEL_MAJOR, CHANNELIZER_FRAME_MAJOR
from .spectrum import NegativeFirst, ZeroFirst, _order

_LAYOUTS = {"frames": CHANNELIZER_FRAME_MAJOR, "channels": CHANNELIZER_CHANNEL_MAJOR,
            CHANNELIZER_FRAME_MAJOR: CHANNELIZER_FRAME_MAJOR, CHANNELIZER_CHANNEL_MAJOR: CHANNELIZER_CHANNEL_MAJOR}


class _PolyphaseBank:
    """The context, the configuration, the handle, and the calls hzsdr_<_c>_create, _pending, _reset and _free over them.
    A subclass names its C prefix `_c` and the noun of its errors `_noun`, and keeps pending() for its doc string."""
    _c = _noun = None

    def _open(self, ctx, fmt, channels, taps, hop, order, layout):
        self.ctx, self.channels = ctx, int(channels)
        self.hop = self.channels if hop is None else int(hop)
        self.order = _order(order)
        if layout not in _LAYOUTS:
            raise ValueError(f"{self._noun}: unknown layout {layout!r}")
        self.layout = _LAYOUTS[layout]
        self.taps = np.ascontiguousarray(taps, np.float32).reshape(-1)
        if self.channels <= 0 or self.hop <= 0:
            raise ErrInvalidArgument(f"{self._noun}: channels and hop are at least 1")
        self._h = C.c_void_p()
        ctx._ck(getattr(lib, f"hzsdr_{self._c}_create")(ctx._h, fmt, self.channels, self.taps.ctypes.data_as(C.POINTER(C.c_float)),
                                                        self.taps.shape[0], self.hop, self.order, self.layout, C.byref(self._h)))

    def _call(self, name, *args):
        self.ctx._ck(getattr(lib, f"hzsdr_{self._c}_{name}")(self._h, *args))

    @property
    def channel_major(self):
        return self.layout == CHANNELIZER_CHANNEL_MAJOR

    def _pending(self):
        h, j = C.c_size_t(0), C.c_uint64(0)
        self._call("pending", C.byref(h), C.byref(j))
        return h.value, j.value

    def reset(self):
        self._call("reset")

    def close(self):
        if self._h:
            getattr(lib, f"hzsdr_{self._c}_free")(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class _AnalysisBank(_PolyphaseBank):
    """push(samples) -> the frames that complete, complex64, (frames, M) for layout "frames" or (M, frames) for layout
    "channels" (numpy for a HOST context, a torch tensor on the samples' device, written on the context's stream, for
    a DEVICE context)."""

    def frames_for(self, n_in):
        """The frames a push of n_in samples would write now."""
        f = C.c_size_t(0)
        self._call("frames_for", int(n_in), C.byref(f))
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
                raise ValueError(f"{self._noun}: a channel-major destination is (channels, cap)")
            strides = tuple(out.stride()) if _is_torch(out) else tuple(s // 8 for s in out.strides)
            if (out.shape[1] > 1 and strides[1] != 1) or strides[0] < out.shape[1]:
                raise ValueError(f"{self._noun}: a channel-major destination has contiguous rows")
            cap = int(out.shape[1])
            stride = int(strides[0]) if cap else 0  # (dense rows: the pitch is the capacity)
            optr = out.data_ptr() if _is_torch(out) else out.ctypes.data  # (rows with a pitch are not contiguous)
        else:
            cap, stride, optr = int(np.prod(out.shape)) // m, 0, _ptr(out)
        got = C.c_size_t(0)
        self._call("push", _ptr(samples) if n_in else None, n_in, optr if cap else None, cap, stride, C.byref(got))
        if self.channel_major:
            return out[:, :got.value]
        return out[:got.value] if out.ndim == 2 else out[:got.value * m]

    def pending(self):
        """(samples held for the next frame, index of the next frame)."""
        return self._pending()

    def channel_rate(self, sample_rate):
        """The sample rate of every channel: sample_rate / hop."""
        return float(sample_rate) / self.hop

    def channel_center(self, k, sample_rate):
        """The signed center frequency of output position k (row k of layout "channels", column k of "frames"):
        ZeroFirst 0, fs/M, ... floor((M - 1) / 2) fs/M, then the negative ones ascending to -fs/M; NegativeFirst
        ascending from -floor(M / 2) fs/M (numpy's fftshift, for odd M too)."""
        m = self.channels
        if k < 0 or k >= m:
            raise IndexError(f"{self._noun}: channel position out of range")
        idx = (k - m if k > (m - 1) // 2 else k) if self.order == ZeroFirst else k - m // 2
        return float(sample_rate) * idx / m


__all__ = ["_PolyphaseBank", "_AnalysisBank", "_LAYOUTS", "NegativeFirst", "ZeroFirst"]

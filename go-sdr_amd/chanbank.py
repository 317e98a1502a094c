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

from . import ErrDstTooSmall, ErrInvalidArgument  # noqa: F401  (re-exports)
from ._capi import (CHANBANK_FORM_A_LDS, CHANBANK_READ_DFT, CHANBANK_READ_TAPS, CHANNELIZER_CHANNEL_MAJOR,
                    CHANNELIZER_FRAME_MAJOR)
from ._polyphase import _AnalysisBank
from .channelizer import channelizer_taps
from .spectrum import NegativeFirst, ZeroFirst


class ChannelBank(_AnalysisBank):
    """hzsdr_chanbank: push(samples) -> the frames that complete, complex64, (frames, M) for layout "frames" or
    (M, frames) for layout "channels" (numpy for a HOST context, a torch tensor on the samples' device, written on the
    context's stream, for a DEVICE context).  channelizer.Channelizer's interface (_polyphase._AnalysisBank), and plan()
    and readout()."""
    _c, _noun = "chanbank", "channel bank"

    def __init__(self, ctx, src_fmt, channels, taps, hop=None, order=NegativeFirst, layout="frames"):
        self.src_fmt = src_fmt
        self._open(ctx, src_fmt, channels, taps, hop, order, layout)

    def plan(self):
        """(frames per workgroup, rows of the real matrix per workgroup -- two per channel and the padding rows --,
        kernel form): tile i of a push holds its frames [i * tile_frames, (i + 1) * tile_frames); the form is
        CHANBANK_FORM_A_LDS where the matrix is staged in LDS beside the folded frames."""
        t, r, f = C.c_size_t(0), C.c_size_t(0), C.c_int32(0)
        self._call("plan", C.byref(t), C.byref(r), C.byref(f))
        return t.value, r.value, f.value

    def readout(self, what, index=0):
        """The host-made operands as the kernel uses them: CHANBANK_READ_DFT -> row `index` of the DFT table (the
        channels rounded up to an even count of complex64 values); CHANBANK_READ_TAPS -> the prototype, float32."""
        if what == CHANBANK_READ_TAPS:
            out = np.empty(self.taps.shape[0], np.float32)
        else:
            out = np.empty((self.channels + 1) // 2 * 2, np.complex64)
        self._call("readout", int(what), int(index), out.ctypes.data, out.shape[0])
        return out


__all__ = ["ChannelBank", "channelizer_taps", "ZeroFirst", "NegativeFirst", "CHANNELIZER_FRAME_MAJOR", "CHANNELIZER_CHANNEL_MAJOR",
           "CHANBANK_FORM_A_LDS", "CHANBANK_READ_DFT", "CHANBANK_READ_TAPS"]

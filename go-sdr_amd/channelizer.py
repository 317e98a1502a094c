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
import numpy as np

from . import ErrDstTooSmall, ErrInvalidArgument  # noqa: F401  (re-exports)
from ._capi import CHANNELIZER_CHANNEL_MAJOR, CHANNELIZER_FRAME_MAJOR
from ._polyphase import _AnalysisBank, _LAYOUTS  # noqa: F401  (_LAYOUTS: where it used to live)
from .spectrum import NegativeFirst, ZeroFirst


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


class Channelizer(_AnalysisBank):
    """hzsdr_channelizer: push(samples) -> the frames that complete, complex64, (frames, M) for layout "frames" or
    (M, frames) for layout "channels" (numpy for a HOST context, a torch tensor on the samples' device, written on the
    context's stream, for a DEVICE context).  A channel-major destination given to push may be a view of a wider
    buffer: rows with unit stride along a row and any pitch (it had to be contiguous before the polyphase classes
    shared their push).  frames_for, push, pending, reset, channel_rate and channel_center are _polyphase._AnalysisBank's."""
    _c, _noun = "channelizer", "channelizer"

    def __init__(self, ctx, src_fmt, channels, taps, hop=None, order=NegativeFirst, layout="frames"):
        self.src_fmt = src_fmt
        self._open(ctx, src_fmt, channels, taps, hop, order, layout)


__all__ = ["Channelizer", "channelizer_taps", "ZeroFirst", "NegativeFirst", "CHANNELIZER_FRAME_MAJOR",
           "CHANNELIZER_CHANNEL_MAJOR"]

"""The fused power spectrum (include/hzsdr_spectrum.h) and the reference's fft.FrequencySlice helpers.

    sp = ctx.spectrum(hz.FMT_U8, 1024, hop=512, avg=16, window=hann(1024), scale="power")
    rows = sp.push(samples)          # rows x 1024 float32, NegativeFirst by default

FrequencySlice helpers restate fft/result.go:120-236 over (bins, sample_rate, order): BinBandwidth in float32 as
the reference computes it, its error cases and its asymmetric BinByFreq edges.
"""
import ctypes as C

import numpy as np

from . import _capi, _is_torch, _ptr, ErrDstTooSmall, fmt_of, length, lib  # noqa: F401  (ErrDstTooSmall: re-export)
from ._capi import (ORDER_NEGATIVE_FIRST, ORDER_ZERO_FIRST, SPECTRUM_DB, SPECTRUM_FORM_AUTO,
                    SPECTRUM_FORM_FRAME_PARALLEL, SPECTRUM_FORM_ROW_WALK, SPECTRUM_POWER)

# fft.ZeroFirst / fft.NegativeFirst (fft/result.go:34-47)
ZeroFirst, NegativeFirst = ORDER_ZERO_FIRST, ORDER_NEGATIVE_FIRST


class ErrFrequencyOutOfSamplingRange(ValueError):
    """fft.ErrFrequencyOutOfSamplingRange (fft/result.go:28-32)."""

    def __init__(self, msg="fft: target frequency is out of sampling rate"):
        super().__init__(msg)


def _order(order):
    if order is True or order is False:
        return int(order)
    if order in (ZeroFirst, NegativeFirst):
        return int(order)
    raise ValueError("fft: Unknown fft layout")


# ---- fft.FrequencySlice helpers (fft/result.go:120-236) ---------------------------------------

def bin_bandwidth(bins, sample_rate):
    """BinBandwidth: float32(sampleRate) / float32(frequencyLen), widened (fft/result.go:120-123)."""
    return float(np.float32(sample_rate) / np.float32(bins))


def nyquist(sample_rate):
    """Nyquest: rf.Hz(sampleRate) / 2 (fft/result.go:125-129)."""
    return float(sample_rate) / 2


def freq_by_bin(bins, sample_rate, order, b):
    """FreqByBin: the center frequency of bin `b` (fft/result.go:180-204)."""
    order = _order(order)
    if b < 0 or b > bins:
        raise ErrFrequencyOutOfSamplingRange()
    midpoint = bins // 2
    bw = bin_bandwidth(bins, sample_rate)
    if order == ZeroFirst:
        if b > midpoint:
            b = b - bins
        return bw * float(b)
    return bw * float(b - midpoint)


def _go_int(x):
    """Go's int(float64): truncation toward zero."""
    return int(np.trunc(x))


def bin_by_freq(bins, sample_rate, order, freq):
    """BinByFreq (fft/result.go:206-228): freq in (-nyquist, nyquist]; the bin index truncates toward zero."""
    order = _order(order)
    nyq = nyquist(sample_rate)
    if freq > nyq or freq <= -nyq:
        raise ErrFrequencyOutOfSamplingRange()
    bin_idx = float(freq) / bin_bandwidth(bins, sample_rate)
    if order == ZeroFirst:
        if bin_idx < 0:
            return bins + _go_int(bin_idx)
        return _go_int(bin_idx)
    return bins // 2 + _go_int(bin_idx)


def bins_by_range(bins, sample_rate, order, rng):
    """BinsByRange: the bins of the range (lo, hi), in walk order (fft/result.go:131-178)."""
    order = _order(order)
    nyq = nyquist(sample_rate)
    lo, hi = rng
    if hi > nyq or hi < -nyq:
        raise ErrFrequencyOutOfSamplingRange()
    low_bin = bin_by_freq(bins, sample_rate, order, lo)
    high_bin = bin_by_freq(bins, sample_rate, order, hi)
    if lo >= 0 or hi < 0:
        return list(range(low_bin, high_bin + 1))
    if order == ZeroFirst:
        return list(range(low_bin, bins)) + list(range(0, high_bin + 1))
    return list(range(low_bin, high_bin + 1))


def shift(frequency):
    """Shift: swap the halves of a ZeroFirst / NegativeFirst buffer in place (fft/result.go:82-97, 230-236);
    numpy arrays and torch tensors along the last axis.  Returns the buffer."""
    zero = frequency.shape[-1] // 2
    lo = frequency[..., :zero].clone() if _is_torch(frequency) else frequency[..., :zero].copy()
    frequency[..., :zero] = frequency[..., zero:2 * zero]
    frequency[..., zero:2 * zero] = lo
    return frequency


# ---- windows and scales ----------------------------------------------------------------------

def hann(n):
    """The periodic Hann window 0.5 - 0.5 cos(2 pi i / n), float64 rounded to float32 (scipy.signal.get_window's)."""
    i = np.arange(n, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2 * np.pi * i / n)).astype(np.float32)


def spectrum_scale(kind, n, avg, window=None, sample_rate=None):
    """The float32 scale of a spectrum's rows, computed in float64: "power" 1 / (K (sum w)^2) (a tone of amplitude A
    in a bin reads A^2), "density" 1 / (K fs sum w^2) (scipy.signal.welch's scaling="density"); a number as it is."""
    if not isinstance(kind, str):
        return float(np.float32(kind))
    w = np.ones(n, np.float64) if window is None else np.asarray(window, np.float32).astype(np.float64)
    if kind == "power":
        return float(np.float32(1.0 / (avg * float(w.sum()) ** 2)))
    if kind == "density":
        if not sample_rate:
            raise ValueError("spectrum: scale=\"density\" needs the sample rate")
        return float(np.float32(1.0 / (avg * float(sample_rate) * float((w * w).sum()))))
    raise ValueError(f"spectrum: unknown scale {kind!r}")


# ---- the operator ----------------------------------------------------------------------------

class Spectrum:
    """hzsdr_spectrum: push(samples) -> the rows that complete, rows x n float32 (numpy for a HOST context, a torch
    CUDA tensor for a DEVICE context)."""

    def __init__(self, ctx, src_fmt, n, hop=None, avg=1, window=None, scale=1.0, order=NegativeFirst, db=False,
                 sample_rate=None):
        self.ctx, self.src_fmt, self.n = ctx, src_fmt, int(n)
        self.hop = self.n if hop is None else int(hop)
        self.avg, self.order, self.db, self.sample_rate = int(avg), _order(order), bool(db), sample_rate
        if self.n <= 0 or self.avg <= 0 or self.hop <= 0:
            from . import ErrInvalidArgument
            raise ErrInvalidArgument("spectrum: n, hop and avg are at least 1")
        self.window = None if window is None else np.ascontiguousarray(window, np.float32)
        if self.window is not None and self.window.shape != (self.n,):
            raise ValueError("spectrum: the window has n values")
        self.scale = spectrum_scale(scale, self.n, self.avg, self.window, sample_rate)
        wp = None if self.window is None else self.window.ctypes.data_as(C.POINTER(C.c_float))
        self._h = C.c_void_p()
        ctx._ck(lib.hzsdr_spectrum_create(ctx._h, src_fmt, self.n, self.hop, self.avg, wp, self.scale, self.order,
                                          SPECTRUM_DB if self.db else SPECTRUM_POWER, C.byref(self._h)))

    def rows_for(self, n_in):
        r = C.c_size_t(0)
        self.ctx._ck(lib.hzsdr_spectrum_rows_for(self._h, int(n_in), C.byref(r)))
        return r.value

    def push(self, samples, out=None):
        """Consume every sample of `samples`; return the rows that complete (into `out` when given: a float32 buffer
        of at least rows x n values, the rows at its start)."""
        n_in = length(samples)
        rows = self.rows_for(n_in)
        if out is None:
            if _is_torch(samples):
                import torch
                out = torch.empty((rows, self.n), dtype=torch.float32, device=samples.device)
            else:
                out = np.empty((rows, self.n), np.float32)
        cap = int(np.prod(out.shape)) // self.n
        got = C.c_size_t(0)
        self.ctx._ck(lib.hzsdr_spectrum_push(self._h, _ptr(samples) if n_in else None, n_in,
                                             _ptr(out) if cap else None, cap, C.byref(got)))
        return out[:got.value] if out.ndim == 2 else out[:got.value * self.n]

    def pending(self):
        """(frames summed into the unfinished row, samples held for the next frame)."""
        f, h = C.c_size_t(0), C.c_size_t(0)
        self.ctx._ck(lib.hzsdr_spectrum_pending(self._h, C.byref(f), C.byref(h)))
        return f.value, h.value

    def options(self, form=SPECTRUM_FORM_AUTO):
        """SPECTRUM_FORM_AUTO / _ROW_WALK / _FRAME_PARALLEL for later pushes (the same bits either way)."""
        self.ctx._ck(lib.hzsdr_spectrum_options(self._h, int(form)))
        return self

    def last_form(self):
        f = C.c_int(0)
        self.ctx._ck(lib.hzsdr_spectrum_last_form(self._h, C.byref(f)))
        return f.value

    def reset(self):
        self.ctx._ck(lib.hzsdr_spectrum_reset(self._h))

    def frequency_slice(self):
        """(bins, sample_rate, order): the arguments of the FrequencySlice helpers for this spectrum's rows."""
        return self.n, self.sample_rate, self.order

    def close(self):
        if self._h:
            lib.hzsdr_spectrum_free(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


__all__ = ["ZeroFirst", "NegativeFirst", "ErrFrequencyOutOfSamplingRange", "bin_bandwidth", "nyquist",
           "freq_by_bin", "bin_by_freq", "bins_by_range", "shift", "hann", "spectrum_scale", "Spectrum",
           "SPECTRUM_FORM_AUTO", "SPECTRUM_FORM_ROW_WALK", "SPECTRUM_FORM_FRAME_PARALLEL"]

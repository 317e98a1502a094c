"""The tuner bank (include/hzsdr_tuner.h): K tuners at arbitrary centre frequencies over one pass of one IQ stream.

    words = [hz.tuner_word(f, fs) for f in (851.0125e6 - fc, 851.5125e6 - fc, 852.0375e6 - fc)]
    bank = ctx.tuner_bank(hz.FMT_U8, words, lowpass, down=40)
    rows = bank.push(block)          # block: (n, 2) uint8; rows: (3, ceil(n / 40)) complex64
    tail = bank.flush()              # the outputs that still depend on samples pushed
    bank.retune(1, [hz.tuner_word(852.5e6 - fc, fs)])

With z_k[n] = c(x[n]) exp(-2 pi i w_k n / 2^32),

    y_k[m] = sum_q taps[q] * z_k[m D - q]

i.e. Shift(-f_k), the FIR and every D-th output, f_k = w_k fs / 2^32.  The rows are what ctx.resampler(..., streams=K) and
ctx.demodulator(..., streams=K) take as they are.  The bits of a row do not depend on how the stream is cut into pushes,
on the memory space, on the output pitch or on the other tuners.
"""
import ctypes as C

import numpy as np

from . import ErrDstTooSmall, ErrInvalidArgument, FMT_C64, FMT_I8, FMT_I16, FMT_U8, lib  # noqa: F401
from ._rows import cut, device_like, rows_input, rows_output
from ._capi import TUNER_FORM_CHUNKED, TUNER_FORM_TRANSPOSED, TUNER_READ_T0, TUNER_READ_T1, TUNER_READ_T2, TUNER_READ_TAPS

_READ_LEN = {TUNER_READ_T2: 2048, TUNER_READ_T1: 2048, TUNER_READ_T0: 1024}


def tuner_word(freq_hz, sample_rate):
    """The frequency word of a tuner centred on freq_hz at sample_rate: round(f / fs * 2^32) mod 2^32.  Negative
    frequencies are the words at or above 2^31; frequencies fs apart share a word."""
    fs = float(sample_rate)
    if not fs > 0.0:
        raise ValueError("tuner_word: sample_rate is positive")
    return int(round(float(freq_hz) / fs * 4294967296.0)) % (1 << 32)


class TunerBank:
    """hzsdr_tuner: push(samples) -> the (K, count) outputs they complete, complex64; flush() -> the rest of the stream.
    Samples are (n,) complex64 or (n, 2) for the byte and int16 formats; a bank of ONE tuner returns (count,).  numpy in
    a HOST context; torch tensors on the context's device, written on the context's stream, in a DEVICE context."""

    def __init__(self, ctx, src_fmt, words, taps, down=1):
        self.ctx, self.src_fmt, self.down = ctx, src_fmt, int(down)
        self.words = self._words(words)
        self.tuners = int(self.words.shape[0])
        if self.down <= 0 or self.tuners <= 0:
            raise ErrInvalidArgument("tuner bank: down and the number of tuners are at least 1")
        self.taps = np.ascontiguousarray(taps, np.float32).reshape(-1)
        self._h = C.c_void_p()
        ctx._ck(lib.hzsdr_tuner_create(ctx._h, src_fmt, self.words.ctypes.data_as(C.POINTER(C.c_uint32)), self.tuners, self.down,
                                       self.taps.ctypes.data_as(C.POINTER(C.c_float)), self.taps.shape[0], C.byref(self._h)))

    @staticmethod
    def _words(words):
        w = [int(v) for v in np.asarray(words).reshape(-1)]
        if any(v < 0 or v >= 1 << 32 for v in w):
            raise ErrInvalidArgument("tuner bank: a frequency word is a uint32 (tuner_word)")
        return np.array(w, np.uint32)

    def outputs_for(self, n_in):
        """The outputs per tuner a push of n_in samples would write now."""
        c = C.c_size_t(0)
        self.ctx._ck(lib.hzsdr_tuner_outputs_for(self._h, int(n_in), C.byref(c)))
        return c.value

    def pending(self):
        """(samples consumed, index of the next output, outputs per tuner a flush would write now)."""
        n, m, f = C.c_uint64(0), C.c_uint64(0), C.c_size_t(0)
        self.ctx._ck(lib.hzsdr_tuner_pending(self._h, C.byref(n), C.byref(m), C.byref(f)))
        return n.value, m.value, f.value

    def plan(self):
        """(outputs per workgroup, rows of the real matrix per workgroup -- two per tuner --, kernel form): the form is
        a sum of TUNER_FORM_CHUNKED (the filter is staged in chunks: the window of a tile under the whole filter is past
        the LDS budget) and TUNER_FORM_TRANSPOSED (the window in LDS is stored as `down` rows; whenever down > 1)."""
        t, r, f = C.c_size_t(0), C.c_size_t(0), C.c_int32(0)
        self.ctx._ck(lib.hzsdr_tuner_plan(self._h, C.byref(t), C.byref(r), C.byref(f)))
        return t.value, r.value, f.value

    def retune(self, first, words):
        """Replace the words of tuners [first, first + len(words)), in effect from the next push on; the stream
        position and the phase reference (stream position 0) stay."""
        w = self._words(words)
        self.ctx._ck(lib.hzsdr_tuner_set_words(self._h, int(first), int(w.shape[0]), w.ctypes.data_as(C.POINTER(C.c_uint32))))
        self.words[int(first):int(first) + w.shape[0]] = w

    def readout(self, what, index=0):
        """The host-made operands as the kernel uses them, complex64: TUNER_READ_TAPS -> the modulated taps of tuner
        `index` (the taps rounded up to an even count); TUNER_READ_T2 / _T1 / _T0 -> the rotator's tables."""
        n = _READ_LEN.get(what, (self.taps.shape[0] + 1) // 2 * 2)
        out = np.empty(n, np.complex64)
        self.ctx._ck(lib.hzsdr_tuner_readout(self._h, int(what), int(index), out.ctypes.data, n))
        return out

    def push(self, samples, out=None):
        """Consume every sample; return the outputs they complete.  `out`, when given, is a complex64 buffer ((cap,), or
        (tuners, cap) with any row pitch; columns past the outputs written are left as they are); the result is its
        written part."""
        ptr, n, _ = rows_input(samples, self.src_fmt, None, "tuner bank")
        out, optr, cap, opitch = rows_output(out, self.outputs_for(n), samples, self.tuners, np.complex64, "tuner bank", "tuner")
        got = C.c_size_t(0)
        self.ctx._ck(lib.hzsdr_tuner_push(self._h, ptr, n, optr if cap else None, cap, opitch, C.byref(got)))
        return cut(out, self.tuners, got.value)

    def flush(self, out=None):
        """The outputs that still depend on samples pushed, the samples behind the last one taken as zero; the bank
        starts over.  Pushes and flush together have scipy.signal.upfirdn(taps, z, 1, down)'s length."""
        out, optr, cap, opitch = rows_output(out, self.pending()[2], device_like(self.ctx), self.tuners, np.complex64, "tuner bank", "tuner")
        got = C.c_size_t(0)
        self.ctx._ck(lib.hzsdr_tuner_flush(self._h, optr if cap else None, cap, opitch, C.byref(got)))
        return cut(out, self.tuners, got.value)

    def reset(self):
        self.ctx._ck(lib.hzsdr_tuner_reset(self._h))

    def sample_rate(self, input_rate):
        """The sample rate of the output: input_rate / down."""
        return float(input_rate) / self.down

    def close(self):
        if self._h:
            lib.hzsdr_tuner_free(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


__all__ = ["TunerBank", "tuner_word", "TUNER_FORM_CHUNKED", "TUNER_FORM_TRANSPOSED", "TUNER_READ_TAPS", "TUNER_READ_T2", "TUNER_READ_T1",
           "TUNER_READ_T0"]

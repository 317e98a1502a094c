"""What the bank classes share around a call: the source formats, rows of samples in, rows of results out.

A bank of R streams takes (R, n) rows with unit stride along a row and any row pitch (a view of a wider buffer) and
writes (R, count) rows likewise; one stream takes (n,) and writes (count,).  numpy in a HOST context, torch tensors on
the context's device in a DEVICE context.  The errors carry the calling class's noun.

RowWaveBank is what the classes of the four row-wave banks (iir.IirBank, symsync.SymbolSync, carrier.CarrierLoop, agc.Agc)
are built on: the object's life and the calls around its pushes (csrc/hz_loopbank.h is the same layer in C).  The
equalizer bank's class (equalizer.Equalizer) takes the object's life, plan and reset from it and has no position.
"""
import ctypes as C

import numpy as np

from . import _is_torch, ErrInvalidArgument, FMT_C64, FMT_I8, FMT_I16, FMT_U8, MEM_HOST, lib
from ._capi import IIR_REAL_F32

# format -> (numpy dtype of an element, bytes of a sample); beside the four source formats, the IIR bank's real float32 rows
_NP_IN = {FMT_C64: (np.complex64, 8), FMT_U8: (np.uint8, 2), FMT_I8: (np.int8, 2), FMT_I16: (np.int16, 4), IIR_REAL_F32: (np.float32, 4)}


def torch_dtype(dt):
    import torch
    return {np.complex64: torch.complex64, np.float32: torch.float32, np.uint8: torch.uint8, np.int8: torch.int8, np.int16: torch.int16}[dt]


def device_like(ctx):
    """What a result made without an input lives like: None (numpy) in a HOST context, else a tensor on its device."""
    if ctx.memspace == MEM_HOST:
        return None
    import torch
    return torch.empty(0, device=f"cuda:{ctx.device}")


def rows_input(x, fmt, rows, noun):
    """-> (pointer, samples per row, row pitch in samples) of a block of format `fmt`: (rows, n), or (n,) for one row;
    a trailing (I, Q) axis of 2 for the byte and int16 formats.  rows = None: one row, given as (n,) only."""
    dt, size = _NP_IN[fmt]
    if x.dtype != (torch_dtype(dt) if _is_torch(x) else dt):
        raise ValueError(f"{noun}: samples are not of the source format")
    if _is_torch(x):
        strides, ptr, item = tuple(x.stride()), x.data_ptr(), x.element_size()
    else:
        item = x.dtype.itemsize
        strides, ptr = tuple(s // item for s in x.strides), x.ctypes.data
    shape = tuple(x.shape)
    per = size // item  # elements per sample: 1 for complex64, 2 (I, Q) otherwise
    if per == 2:
        if not shape or shape[-1] != 2 or (strides[-1] != 1 and shape[-1] > 1):
            raise ValueError(f"{noun}: samples of this format are (..., n, 2)")
        shape, strides = shape[:-1], strides[:-1]
    if len(shape) == 1 and rows in (None, 1):
        shape, strides = (1,) + shape, (0,) + strides
    elif rows is None:
        shape = ()
    rows = rows or 1
    if len(shape) != 2 or shape[0] != rows:
        raise ValueError(f"{noun}: input is (n,) for one stream, (streams, n) otherwise")
    n = int(shape[1])
    if n == 0:
        return None, 0, 0
    if (n > 1 and strides[1] != per) or (rows > 1 and (strides[0] % per or strides[0] // per < n)):
        raise ValueError(f"{noun}: rows are contiguous, their pitch at least the samples of a row")
    return ptr, n, int(strides[0] // per) if rows > 1 else n


def rows_output(out, count, like, rows, dtype, noun, unit="stream"):
    """-> (out, pointer, capacity, pitch) of a destination of numpy type `dtype`: (cap,) for one row, (rows, cap) with
    unit stride along a row and any pitch otherwise.  out = None: a new one of `count` per row, where `like` lives."""
    if out is None:
        shape = (count,) if rows == 1 else (rows, count)
        if _is_torch(like):
            import torch
            out = torch.empty(shape, dtype=torch_dtype(dtype), device=like.device)
        else:
            out = np.empty(shape, dtype)
    if _is_torch(out):
        ok, strides, ptr = out.dtype == torch_dtype(dtype), tuple(out.stride()), out.data_ptr()
    else:
        ok, strides, ptr = out.dtype == dtype, tuple(s // np.dtype(dtype).itemsize for s in out.strides), out.ctypes.data
    if not ok:
        raise ValueError(f"{noun}: the destination is {np.dtype(dtype).name}")
    if rows == 1:
        if out.ndim != 1 or (out.shape[0] > 1 and strides[0] != 1):
            raise ValueError(f"{noun}: the destination of one {unit} is a contiguous (cap,)")
        return out, ptr, int(out.shape[0]), int(out.shape[0])
    if out.ndim != 2 or out.shape[0] != rows or (out.shape[1] > 1 and strides[1] != 1) or strides[0] < out.shape[1]:
        raise ValueError(f"{noun}: the destination is ({unit}s, cap) with contiguous rows")
    return out, ptr, int(out.shape[1]), int(strides[0])


def cut(out, rows, got):
    """The written part of a destination of rows_output."""
    return out[:got] if rows == 1 else out[:, :got]


class RowWaveBank:
    """The context, the rows, the handle, and the calls hzsdr_<_c>_plan, _position, _get_state, _set_state, _reset and
    _free over them.  A subclass names its C prefix `_c`, the noun of its errors `_noun`, the C type of a state word
    `_state_c` and what a state of another shape is told, `_state_msg`; it gives _state_shape(), creates `_h` behind
    _open(), and keeps plan() and state() for their doc strings."""
    _c = _noun = _state_msg = None
    _state_c = C.c_float

    def _open(self, ctx, rows):
        self.ctx, self.rows, self._h = ctx, int(rows), C.c_void_p()
        if self.rows <= 0:
            raise ErrInvalidArgument(f"{self._noun}: rows is at least 1")

    def _call(self, name, *args):
        self.ctx._ck(getattr(lib, f"hzsdr_{self._c}_{name}")(self._h, *args))

    def _plan(self):
        g, t, f = C.c_size_t(0), C.c_size_t(0), C.c_int32(0)
        self._call("plan", C.byref(g), C.byref(t), C.byref(f))
        return g.value, t.value, f.value

    def position(self):
        """Samples consumed per row."""
        p = C.c_uint64(0)
        self._call("position", C.byref(p))
        return p.value

    def _state(self):
        z = np.empty(self._state_shape(), self._state_c)
        self._call("get_state", z.ctypes.data_as(C.POINTER(self._state_c)), z.size)
        return z, self.position()

    def set_state(self, z, position=0):
        z = np.ascontiguousarray(z, self._state_c)
        if z.shape != self._state_shape():
            raise ErrInvalidArgument(f"{self._noun}: {self._state_msg}")
        self._call("set_state", z.ctypes.data_as(C.POINTER(self._state_c)), z.size, int(position))

    def _push_tracked(self, samples, fmt, dtype, out, track):
        """The push of a bank with one output per input and an optional float32 track -> the rows, or (rows, track)."""
        noun = self._noun
        ptr, n, pitch = rows_input(samples, fmt, self.rows, noun)
        out, optr, cap, opitch = rows_output(out, n, samples, self.rows, dtype, noun, unit="row")
        if cap < n:
            raise ValueError(f"{noun}: the destination is shorter than the rows")
        if track is None or track is False:
            self._call("push", ptr, n, pitch, optr if cap else None, opitch, None, 0)
            return cut(out, self.rows, n)
        track, tptr, tcap, tpitch = rows_output(None if track is True else track, n, samples, self.rows, np.float32, f"{noun} track", unit="row")
        if tcap < n:
            raise ValueError(f"{noun}: the track is shorter than the rows")
        self._call("push", ptr, n, pitch, optr if cap else None, opitch, tptr if tcap else None, tpitch)
        return cut(out, self.rows, n), cut(track, self.rows, n)

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

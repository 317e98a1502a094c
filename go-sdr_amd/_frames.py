"""What the classes of the frame banks (framesync.FrameSync, hdlc.Hdlc, softframe.SoftFrames, viterbi.ViterbiDecoder,
ldpc.LdpcDecoder, rs.ReedSolomon) share around a call: new blocks of slots where the input lives, the pointers of blocks and of dense
arrays behind their checks.  numpy in a HOST context; torch tensors on the context's device in a DEVICE context, where
the ABI's unsigned 32- and 64-bit types are the signed types of the same width.  The errors carry the calling class's noun.

BitRingBank is what the classes of the two bit-ring banks (FrameSync, Hdlc) are built on: the object's life and its
push (csrc/hz_framebank.h is the same layer in C).  DecoderBank is what the classes of the three decoder banks
(ViterbiDecoder, LdpcDecoder, ReedSolomon) are built on: the create, sizes, plan, the dense decode and ragged
(csrc/hz_decodebank.h).  Both stand on _Bank: the handle, its calls and its end.
"""
import ctypes as C

import numpy as np

from . import _is_torch, ErrInvalidArgument, lib
from ._rows import rows_input


def _torch_dtype(dtype):
    import torch
    return {np.uint8: torch.uint8, np.uint64: torch.int64, np.uint32: torch.int32, np.float32: torch.float32}[dtype]


def new_like(shape, dtype, like):
    """zeros of `shape`: numpy of `dtype`, or where `like` is a tensor, torch of the same width on its device"""
    if _is_torch(like):
        import torch
        return torch.zeros(shape, dtype=_torch_dtype(dtype), device=like.device)
    return np.zeros(shape, dtype)


def dense_ptr(a, shape, dtype, what, noun, torch_type="the signed type of that width"):
    """pointer of a contiguous array of `shape`: numpy of `dtype`, or torch of the same width"""
    if _is_torch(a):
        ok, ptr = a.dtype == _torch_dtype(dtype) and a.is_contiguous(), a.data_ptr()
    else:
        ok, ptr = a.dtype == dtype and a.flags.c_contiguous, a.ctypes.data
    if not ok or tuple(a.shape) != tuple(shape):
        raise ValueError(f"{noun}: {what} is a contiguous {np.dtype(dtype).name} {tuple(shape)} (torch: {torch_type})")
    return ptr


def _strides(a, dtype):
    """(the dtype is right, strides in elements, pointer)"""
    if _is_torch(a):
        return a.dtype == _torch_dtype(dtype), tuple(a.stride()), a.data_ptr()
    return a.dtype == dtype, tuple(s // a.itemsize for s in a.strides), a.ctypes.data


def block_ptr(a, shape, dtype, what, noun):
    """(pointer, row pitch in elements) of a (rows, cap, width) block with contiguous rows"""
    ok, strides, ptr = _strides(a, dtype)
    R, cap, w = shape
    if not ok or tuple(a.shape) != shape or (w > 1 and strides[2] != 1) or (cap > 1 and strides[1] != w) or (R > 1 and strides[0] < cap * w):
        raise ValueError(f"{noun}: {what} is {np.dtype(dtype).name} {shape} with contiguous rows")
    return ptr, int(strides[0]) if R > 1 else cap * w


def pitched_block_ptr(a, rows, cap, least, what, noun):
    """(pointer, row pitch, slot pitch) in bytes of a (rows, cap, width >= least) uint8 block with any pitches"""
    ok, strides, ptr = _strides(a, np.uint8)
    shape = tuple(a.shape)
    if not ok or len(shape) != 3 or shape[:2] != (rows, cap) or shape[2] < least or (shape[2] > 1 and strides[2] != 1):
        raise ValueError(f"{noun}: {what} is uint8 ({rows}, {cap}, at least {least}) with unit stride along a frame")
    pitch = int(strides[1]) if cap > 1 else shape[2]
    return ptr, int(strides[0]) if rows > 1 else cap * pitch, pitch


class _Bank:
    """The context, the rows and the handle `_h` of a bank whose C functions are hzsdr_<_c>_*, the calls over them and
    the object's end.  A subclass names `_c` and the noun of its errors, `_noun`."""
    _c = _noun = None

    def _open(self, ctx, rows):
        self.ctx, self.rows, self._h = ctx, int(rows), C.c_void_p()
        if self.rows <= 0:
            raise ErrInvalidArgument(f"{self._noun}: rows is at least 1")

    def _call(self, name, *args):
        self.ctx._ck(getattr(lib, f"hzsdr_{self._c}_{name}")(self._h, *args))

    def _sizes(self, name, n):
        """the `n` size_t results of hzsdr_<_c>_<name>"""
        v = [C.c_size_t(0) for _ in range(n)]
        self._call(name, *[C.byref(x) for x in v])
        return tuple(x.value for x in v)

    def _plan(self):
        g, t, r, f = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_int32(0)
        self._call("plan", C.byref(g), C.byref(t), C.byref(r), C.byref(f))
        return g.value, t.value, r.value, f.value

    def close(self):
        if self._h:
            getattr(lib, f"hzsdr_{self._c}_free")(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class DecoderBank(_Bank):
    """What the classes of the three decoder banks (ViterbiDecoder, LdpcDecoder, ReedSolomon) are built on
    (csrc/hz_decodebank.h is the same layer in C): hzsdr_<_c>_create behind _open(), the dense decode of the banks that
    take hard bits (`kind` is `_bits`: uint8 frames of `frame_bytes`) or soft float32 values (frames of `N`), and ragged()
    over _fields(info words) -> what a frame's tuple holds behind its data.  A subclass keeps decode(), ragged(), plan()
    and sizes() for their doc strings."""
    _bits = None

    def _create(self, *args):
        self.ctx._ck(getattr(lib, f"hzsdr_{self._c}_create")(self.ctx._h, *args, self.rows, C.byref(self._h)))

    def _out(self, frames, cap, out):
        """a call's (data, info): new ones where `frames` lives when `out` is None"""
        if out is None:
            out = (new_like((self.rows, cap, self.data_bytes), np.uint8, frames), new_like((self.rows, cap), np.uint32, frames))
        return out

    def _tail_ptrs(self, info, counts, cap):
        """the pointers of a call's info and counts"""
        noun, R = self._noun, self.rows
        iptr = dense_ptr(info, (R, cap), np.uint32, "info", noun, "int32")
        return iptr, None if counts is None else dense_ptr(counts, (R,), np.uint32, "the frames' counts", noun, "int32")

    def _decode(self, frames, counts, cap, out):
        noun, R = self._noun, self.rows
        width, dtype = (self.frame_bytes, np.uint8) if self.kind == self._bits else (self.N, np.float32)
        if frames.ndim == 2 and R == 1:
            frames = frames[None]
        if frames.ndim != 3:
            raise ValueError(f"{noun}: frames are (rows, cap, FB or N)")
        cap = int(frames.shape[1]) if cap is None else int(cap)
        fptr, fpitch = block_ptr(frames, (R, cap, width), dtype, "frames", noun)
        data, info = self._out(frames, cap, out)
        dptr, dpitch = block_ptr(data, (R, cap, self.data_bytes), np.uint8, "data", noun)
        iptr, cptr = self._tail_ptrs(info, counts, cap)
        self._call("decode", fptr, fpitch, cptr, cap, dptr, dpitch, iptr)
        return data, info

    def _ragged(self, data, info, counts):
        if _is_torch(data):
            data, info = data.cpu().numpy(), info.cpu().numpy()
            counts = None if counts is None else counts.cpu().numpy()
        if data.ndim == 2:
            data, info = data[None], np.asarray(info).reshape(1, -1)
        cap = data.shape[1]
        info = np.asarray(info).view(np.uint32)
        got = np.full(self.rows, cap, np.uint32) if counts is None else np.asarray(counts).reshape(-1).view(np.uint32)
        out = []
        for r, c in enumerate(got):
            k = min(int(c), cap)
            out.append((data[r, :k, :self.data_bytes].copy(), *self._fields(info[r, :k])))
        return out


class BitRingBank(_Bank):
    """The context, the rows, the handle, and the calls hzsdr_<_c>_push, _plan, _positions, _reset and _free over them.
    A subclass names its C prefix `_c`, the noun of its errors `_noun` and what its errors call a slot's extent,
    `_extent`; it sets `kind` and `frame_bytes`, a slot's bytes, creates `_h` behind _open(), and keeps push() and plan()
    for their doc strings."""
    _extent = None

    def _open(self, ctx, kind, rows):
        self.kind = int(kind)
        super()._open(ctx, rows)

    def positions(self):
        """Symbols consumed per row: uint64 (rows,), behind every push so far."""
        p = np.empty(self.rows, np.uint64)
        self._call("positions", p.ctypes.data_as(C.POINTER(C.c_uint64)), p.size)
        return p

    def _push(self, symbols, counts, cap, out):
        noun = self._noun
        ptr, n, pitch = rows_input(symbols, self.kind, self.rows, noun)
        cap, R, FB = int(cap), self.rows, self.frame_bytes
        if cap < 0:
            raise ValueError(f"{noun}: cap is not negative")
        if out is None:
            out = (new_like((R, cap, FB), np.uint8, symbols), new_like((R, cap), np.uint64, symbols), new_like((R, cap), np.uint32, symbols),
                   new_like((R,), np.uint32, symbols))
        frames, positions, info, got = out
        ok, strides, fptr = _strides(frames, np.uint8)
        if not ok or tuple(frames.shape) != (R, cap, FB) or (cap and (strides[2] != 1 or (cap > 1 and strides[1] != FB) or (R > 1 and strides[0] < cap * FB))):
            raise ValueError(f"{noun}: frames are uint8 (rows, cap, {self._extent}) with contiguous rows")
        pptr, iptr = dense_ptr(positions, (R, cap), np.uint64, "positions", noun), dense_ptr(info, (R, cap), np.uint32, "info", noun)
        gptr = dense_ptr(got, (R,), np.uint32, "counts", noun)
        cptr = None
        if counts is not None:
            cptr = dense_ptr(counts, (R,), np.uint32, "the symbols' counts", noun)
        self._call("push", ptr, n, pitch, cptr, fptr if cap else None, cap, int(strides[0]) if cap else 0, pptr if cap else None, iptr if cap else None,
                   gptr, None)
        return frames, positions, info, got

    def reset(self):
        self._call("reset")

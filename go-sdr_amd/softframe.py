"""The soft frame bank (include/hzsdr_softframe.h): the payload FLOATS of the frames a frame sync bank found, in the
layout the Viterbi bank's soft input reads.

    fs = ctx.frame_sync(hz.SYMSYNC_REAL_F32, 32, [0x1ACFFC1D], [0], payload_bits=168, rows=100)
    sf = ctx.soft_frames(fs)                                  # the same kind, B, P, maps and rows
    vd = ctx.viterbi(hz.VITERBI_SOFT_F32, K, gens, data_bits=78, scale=32.0, rows=100)
    frames, positions, info, got = fs.push(symbols, counts, cap=4)          # the frame sync bank, on the device
    soft, status = sf.push(symbols, counts, positions, info, got, cap=4)    # the SAME symbols and counts
    data, verdict = vd.decode(soft, got, 4)                   # soft (rows, cap, P) float32, nothing read in between

Float k of a frame is decision float s * B + k of the row's stream (the floats of a real row, the Re parts of a complex
row at B = 1, re, im, re, im ... at B = 2) through the frame's hypothesis map, which flips sign BITS and exchanges the
floats of a pair and does no arithmetic: NaN payloads, -0 and infinities pass.  The sign of float k decides the bit the
frame sync bank packed at place k.  The bank keeps the last P / B - 1 symbols of every row, so floats, status and state
do not depend on how the stream is cut into pushes.  A frame whose payload does not end in the push, or began before
what the bank holds, or whose hypothesis the bank does not have, is all quiet NaN (erasures to the decoder) and says so
in `status` (SOFTFRAME_OUTSIDE, SOFTFRAME_NO_HYPOTHESIS); every frame the frame sync bank emits in the same push is
SOFTFRAME_SERVED.

Not here: a soft form of the frame sync bank's differential decodings (Context.soft_frames refuses a bank with
diff != 0); level normalisation (the AGC bank in front, the decoder's `scale` behind); int8 soft values.
"""
import ctypes as C

import numpy as np

from . import ErrInvalidArgument, _is_torch, lib
from ._frames import dense_ptr, new_like
from ._rows import rows_input
from ._capi import (SOFTFRAME_FORM_COMPLEX, SOFTFRAME_FORM_DIBIT, SOFTFRAME_MAX_HYPOTHESES, SOFTFRAME_MAX_PAYLOAD, SOFTFRAME_MAX_ROWS,
                    SOFTFRAME_MAX_SLOTS, SOFTFRAME_NO_HYPOTHESIS, SOFTFRAME_OUTSIDE, SOFTFRAME_SERVED)

_PU64, _PF32 = C.POINTER(C.c_uint64), C.POINTER(C.c_float)


class SoftFrames:
    """hzsdr_softframe: push(symbols, counts, positions, info, got, cap) -> (soft, status).  `kind`, `bits_per_symbol`,
    `payload_bits`, `maps` and `rows` are the frame sync bank's (Context.soft_frames takes them from it).  numpy in a
    HOST context; torch tensors on the context's device, written on the context's stream, in a DEVICE context
    (positions are int64, info, counts and status int32 there: the same bits as the ABI's unsigned types)."""

    def __init__(self, ctx, kind, payload_bits, maps, bits_per_symbol=1, rows=1):
        self.ctx, self.kind, self.rows = ctx, int(kind), int(rows)
        if self.rows <= 0:
            raise ErrInvalidArgument("soft frames: rows is at least 1")
        self.P, self.B = int(payload_bits), int(bits_per_symbol)
        maps = [int(m) for m in np.atleast_1d(maps)]
        if not 1 <= len(maps) <= SOFTFRAME_MAX_HYPOTHESES or min(maps + [self.P, self.B]) < 0 or max(maps + [self.P, self.B]) >= 1 << 32:
            raise ErrInvalidArgument("soft frames: 1 ... 4 maps; maps and sizes are unsigned values")
        self.maps = maps
        m = (C.c_uint * len(maps))(*maps)
        self._h = C.c_void_p()
        ctx._ck(lib.hzsdr_softframe_create(ctx._h, self.kind, self.B, self.P, len(maps), m, self.rows, C.byref(self._h)))
        self.history_floats = self.plan()[1]

    def plan(self):
        """(floats a workgroup moves per step, history floats per row, form): the form is a sum of SOFTFRAME_FORM_COMPLEX
        and SOFTFRAME_FORM_DIBIT."""
        s, h, f = C.c_size_t(0), C.c_size_t(0), C.c_int32(0)
        self.ctx._ck(lib.hzsdr_softframe_plan(self._h, C.byref(s), C.byref(h), C.byref(f)))
        return s.value, h.value, f.value

    def positions(self):
        """Symbols consumed per row: uint64 (rows,), behind every push so far."""
        p = np.empty(self.rows, np.uint64)
        self.ctx._ck(lib.hzsdr_softframe_positions(self._h, p.ctypes.data_as(_PU64), p.size))
        return p

    def push(self, symbols, counts, positions, info, got, cap, out=None):
        """Serve the frames of FrameSync.push(symbols, counts, cap) -> (frames, positions, info, got) and run the symbols
        into the history -> (soft float32 (rows, cap, P), status (rows, cap)).  `symbols` and `counts` (or None) are
        what that push got.  Slots from a row's min(got, cap) up hold what the destination held (a new one is zero).
        `out`, when given, is such a pair (soft, status); soft may be a view with a row pitch above cap * P."""
        ptr, n, pitch = rows_input(symbols, self.kind, self.rows, "soft frames")
        cap, R, P = int(cap), self.rows, self.P
        if cap < 0:
            raise ValueError("soft frames: cap is not negative")
        if out is None:
            out = (new_like((R, cap, P), np.float32, symbols), new_like((R, cap), np.uint32, symbols))
        soft, status = out
        if _is_torch(soft):
            import torch
            ok, strides, optr = soft.dtype == torch.float32, tuple(soft.stride()), soft.data_ptr()
        else:
            ok, strides, optr = soft.dtype == np.float32, tuple(s // 4 for s in soft.strides), soft.ctypes.data
        if not ok or tuple(soft.shape) != (R, cap, P) or (cap and ((P > 1 and strides[2] != 1) or (cap > 1 and strides[1] != P) or (R > 1 and strides[0] < cap * P))):
            raise ValueError("soft frames: soft is float32 (rows, cap, P) with contiguous rows")
        noun = "soft frames"
        sptr = dense_ptr(status, (R, cap), np.uint32, "status", noun)
        pptr, iptr = dense_ptr(positions, (R, cap), np.uint64, "positions", noun), dense_ptr(info, (R, cap), np.uint32, "info", noun)
        gptr = dense_ptr(got, (R,), np.uint32, "the frames' counts", noun)
        cptr = None if counts is None else dense_ptr(counts, (R,), np.uint32, "the symbols' counts", noun)
        self.ctx._ck(lib.hzsdr_softframe_push(self._h, ptr, n, pitch, cptr, pptr if cap else None, iptr if cap else None, gptr if cap else None, cap,
                                              optr if cap else None, int(strides[0]) if cap and R > 1 else cap * P, sptr if cap else None))
        return soft, status

    def ragged(self, soft, status, got):
        """A push's results -> a list of `rows` host pairs (soft (k, P) float32, status (k,) uint32), k = min(got[r], cap)
        (this waits for the device in a DEVICE context)."""
        if _is_torch(soft):
            soft, status, got = (t.cpu().numpy() for t in (soft, status, got))
        cap = soft.shape[1]
        out = []
        for r, c in enumerate(np.asarray(got).reshape(-1).view(np.uint32)):
            k = min(int(c), cap)
            out.append((soft[r, :k].copy(), status[r, :k].copy().view(np.uint32)))
        return out

    def state(self):
        """(positions uint64 (rows,), history float32 (rows, history_floats)): the symbols consumed and the decision
        floats of the last P / B - 1 symbols, oldest first, bit for bit; behind every push so far."""
        p, y = np.empty(self.rows, np.uint64), np.empty((self.rows, self.history_floats), np.float32)
        self.ctx._ck(lib.hzsdr_softframe_get_state(self._h, p.ctypes.data_as(_PU64), y.ctypes.data_as(_PF32) if y.size else None, self.rows))
        return p, y

    def set_state(self, positions, history):
        p = np.ascontiguousarray(positions, np.uint64)
        y = np.ascontiguousarray(history, np.float32)
        if p.shape != (self.rows,) or y.shape != (self.rows, self.history_floats):
            raise ErrInvalidArgument("soft frames: the state is positions (rows,), history (rows, history_floats)")
        self.ctx._ck(lib.hzsdr_softframe_set_state(self._h, p.ctypes.data_as(_PU64), y.ctypes.data_as(_PF32) if y.size else None, self.rows))

    def reset(self):
        self.ctx._ck(lib.hzsdr_softframe_reset(self._h))

    def close(self):
        if self._h:
            lib.hzsdr_softframe_free(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


__all__ = ["SoftFrames", "SOFTFRAME_SERVED", "SOFTFRAME_OUTSIDE", "SOFTFRAME_NO_HYPOTHESIS", "SOFTFRAME_FORM_COMPLEX", "SOFTFRAME_FORM_DIBIT",
           "SOFTFRAME_MAX_ROWS", "SOFTFRAME_MAX_PAYLOAD", "SOFTFRAME_MAX_HYPOTHESES", "SOFTFRAME_MAX_SLOTS"]

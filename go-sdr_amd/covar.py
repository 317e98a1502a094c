"""The covariance bank and the beam scan (include/hzsdr_covar.h): where a signal comes from.

    w = steering_weights(433.9e6, np.arange(-90, 91), distances)      # (181, 4): one beamform_angles row per angle
    cov = ctx.covariance(hz.FMT_U8, 4, 4096)
    scan = ctx.beam_scan(w)
    for r in cov.push(rows):                 # rows: (4, n, 2) uint8, or a list of 4 buffers as Context.beamform takes
        p = music(scan, r, sources=2)        # (181,) float32: peaks(p, 2) are the two bearings' grid indices

Block b of B snapshots gives R_b[i][j] = sum_n c(x_i[n]) conj(c(x_j[n])), N x N complex64, unnormalised
(Covariance.normalise divides).  Scan.run maps any N x N matrices Q to p[g] = Re w_g Q w_g^H: with Q = R the power of the
beam Context.beamform forms with w_g (bartlett), with Q = R^-1 the reciprocal of Capon's spectrum, with Q the projector
on the noise subspace the reciprocal of MUSIC's.  The bits of R_b do not depend on how the stream is cut into pushes, on
the memory space, on the entry or the pitches, or on the other channels.
"""
import ctypes as C

import numpy as np

from . import MEM_DEVICE, ErrInvalidArgument, _is_torch, _ptr, beamform_angles, lib
from ._capi import COVAR_FORM_ONE_TILE, COVAR_FORM_THREE_TILES


def _rows(samples):
    """a pitched block -> (rows, n, pitch in samples, pointer); a list of buffers -> None"""
    if isinstance(samples, (list, tuple)):
        return None
    per = 1 if str(samples.dtype).endswith("complex64") else 2
    if samples.ndim != (2 if per == 1 else 3):
        raise ValueError("covariance: a block is (channels, n) complex64 or (channels, n, 2) integers")
    strides = tuple(samples.stride()) if _is_torch(samples) else tuple(s // samples.itemsize for s in samples.strides)
    n = int(samples.shape[1])
    inner_ok = strides[1] == per if per == 1 else (strides[1] == 2 and strides[2] == 1)
    if n > 1 and not inner_ok:
        raise ValueError("covariance: the rows of a block are contiguous")
    if strides[0] % per or strides[0] // per < n:
        raise ValueError("covariance: the row pitch is a whole number of samples, at least n")
    ptr = samples.data_ptr() if _is_torch(samples) else samples.ctypes.data  # (rows with a pitch are not contiguous)
    return int(samples.shape[0]), n, strides[0] // per, ptr


class Covariance:
    """hzsdr_covar: push(rows) -> the matrices of the blocks that complete, (blocks, N, N) complex64 (numpy for a HOST
    context, a torch tensor on the rows' device, written on the context's stream, for a DEVICE context)."""

    def __init__(self, ctx, src_fmt, channels, block):
        self.ctx, self.src_fmt, self.channels, self.block = ctx, src_fmt, int(channels), int(block)
        if self.channels <= 0 or self.block <= 0:
            raise ErrInvalidArgument("covariance: channels and block are at least 1")
        self._h = C.c_void_p()
        ctx._ck(lib.hzsdr_covar_create(ctx._h, src_fmt, self.channels, self.block, C.byref(self._h)))

    def blocks_for(self, n_in):
        """The blocks a push of n_in snapshots would write now."""
        b = C.c_size_t(0)
        self.ctx._ck(lib.hzsdr_covar_blocks_for(self._h, int(n_in), C.byref(b)))
        return b.value

    def _out(self, like, blocks, out):
        n = self.channels
        if out is None:
            if _is_torch(like):
                import torch
                out = torch.empty((blocks, n, n), dtype=torch.complex64, device=like.device)
            else:
                out = np.empty((blocks, n, n), np.complex64)
        if out.ndim == 3:
            if tuple(out.shape[1:]) != (n, n):
                raise ValueError("covariance: a destination is (cap, channels, channels) or (cap, pitch)")
            return out, int(out.shape[0]), n * n, _ptr(out)
        strides = tuple(out.stride()) if _is_torch(out) else tuple(s // 8 for s in out.strides)
        if out.ndim != 2 or out.shape[1] < n * n or (out.shape[1] > 1 and strides[1] != 1) or strides[0] < out.shape[1]:
            raise ValueError("covariance: a pitched destination is (cap, pitch >= channels^2) with contiguous rows")
        return out, int(out.shape[0]), int(strides[0]), (out.data_ptr() if _is_torch(out) else out.ctypes.data)

    def push(self, samples, out=None):
        """Consume every snapshot of `samples` -- one block (channels, n[, 2]) whose rows may have a pitch, taken through
        hzsdr_covar_push, or a list of `channels` buffers, through hzsdr_covar_push_channels: the same bits -- and return
        the matrices that complete.  `out`, when given, is complex64, (cap, N, N) or (cap, pitch) with pitch >= N^2
        (the values behind N^2 are left as they are); the result is its written part."""
        rows = _rows(samples)
        if rows is None:
            if len(samples) != self.channels:
                raise ErrInvalidArgument("covariance: one buffer per channel")
            n_in, like = int(samples[0].shape[0]), samples[0]
            if any(int(s.shape[0]) != n_in for s in samples):
                raise ErrInvalidArgument("covariance: the channels' buffers have one length")
        else:
            if rows[0] != self.channels:
                raise ErrInvalidArgument("covariance: one row per channel")
            n_in, like = rows[1], samples
        out, cap, stride, optr = self._out(like, self.blocks_for(n_in), out)
        got = C.c_size_t(0)
        if rows is None:
            arr = (C.c_void_p * self.channels)(*[_ptr(s) for s in samples])
            self.ctx._ck(lib.hzsdr_covar_push_channels(self._h, arr, n_in, optr if cap else None, cap, stride, C.byref(got)))
        else:
            self.ctx._ck(lib.hzsdr_covar_push(self._h, rows[3] if n_in else None, n_in, rows[2], optr if cap else None, cap, stride,
                                              C.byref(got)))
        return out[:got.value]

    def flush(self, device=None):
        """The open block with the snapshots it holds, (1, N, N), or (0, N, N) when nothing is open; back to stream
        position 0.  `device`: the torch device of a DEVICE context's result (default: the current one)."""
        n = self.channels
        if self.ctx.memspace == MEM_DEVICE:
            import torch
            out = torch.empty((1, n, n), dtype=torch.complex64, device="cuda" if device is None else device)
        else:
            out = np.empty((1, n, n), np.complex64)
        got = C.c_size_t(0)
        self.ctx._ck(lib.hzsdr_covar_flush(self._h, _ptr(out), 1, C.byref(got)))
        return out[:got.value]

    def pending(self):
        """(snapshots consumed per row, index of the open block, snapshots it holds)."""
        c, b, o = C.c_uint64(0), C.c_uint64(0), C.c_size_t(0)
        self.ctx._ck(lib.hzsdr_covar_pending(self._h, C.byref(c), C.byref(b), C.byref(o)))
        return c.value, b.value, o.value

    def plan(self):
        """(segment length, segments one workgroup sums where an aligned group lies inside the push, kernel form):
        COVAR_FORM_ONE_TILE up to 8 channels, COVAR_FORM_THREE_TILES above."""
        s, g, f = C.c_size_t(0), C.c_size_t(0), C.c_int32(0)
        self.ctx._ck(lib.hzsdr_covar_plan(self._h, C.byref(s), C.byref(g), C.byref(f)))
        return s.value, g.value, f.value

    def normalise(self, r, snapshots=None):
        """r / snapshots (default: the block length): the sample covariance."""
        return r / float(self.block if snapshots is None else snapshots)

    def reset(self):
        self.ctx._ck(lib.hzsdr_covar_reset(self._h))

    def close(self):
        if self._h:
            lib.hzsdr_covar_free(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Scan:
    """hzsdr_scan over the rows of `weights`, (G, N) complex64: run(Q) -> p[b][g] = Re w_g Q_b w_g^H, float32."""

    def __init__(self, ctx, weights):
        self.ctx = ctx
        self.weights = np.ascontiguousarray(weights, np.complex64)
        if self.weights.ndim != 2:
            raise ErrInvalidArgument("beam scan: the weights are (vectors, channels)")
        self.count, self.channels = (int(v) for v in self.weights.shape)
        self._h = C.c_void_p()
        ctx._ck(lib.hzsdr_scan_create(ctx._h, self.channels, self.weights.ctypes.data, self.count, C.byref(self._h)))

    def upload(self, mats):
        """host matrices as complex64 in the context's memory space"""
        mats = np.ascontiguousarray(mats, np.complex64)
        if self.ctx.memspace == MEM_DEVICE:
            import torch
            return torch.from_numpy(mats).cuda()
        return mats

    def run(self, mats, out=None):
        """mats: (N, N) or (count, N, N) complex64 in the context's memory space, contiguous -> (G,) or (count, G)
        float32 beside it."""
        n = self.channels
        one = mats.ndim == 2
        if tuple(mats.shape[-2:]) != (n, n) or mats.ndim not in (2, 3):
            raise ErrInvalidArgument("beam scan: matrices are (channels, channels)")
        count = 1 if one else int(mats.shape[0])
        if out is None:
            if _is_torch(mats):
                import torch
                out = torch.empty((count, self.count), dtype=torch.float32, device=mats.device)
            else:
                out = np.empty((count, self.count), np.float32)
        if count:
            self.ctx._ck(lib.hzsdr_scan_run(self._h, _ptr(mats), count, n * n, _ptr(out), count * self.count, self.count))
        return out[0] if one else out

    def close(self):
        if self._h:
            lib.hzsdr_scan_free(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def steering_weights(freq_hz, angles_deg, distances):
    """One beamform_angles(freq_hz, angle, distances) row per angle: (G, N) complex64, the weights Context.beamform
    steers a line array with."""
    return np.stack([beamform_angles(float(freq_hz), float(a), distances) for a in np.atleast_1d(angles_deg)])


def _host64(r):
    """matrices -> complex128 numpy, (count, N, N), and whether one matrix came in"""
    if _is_torch(r):
        r = r.cpu().numpy()
    r = np.asarray(r).astype(np.complex128)
    return (r[None], True) if r.ndim == 2 else (r, False)


def _spectrum(scan, mats, one, reciprocal):
    p = scan.run(scan.upload(mats))
    if _is_torch(p):
        scan.ctx.synchronize()
        p = p.cpu().numpy()
    if reciprocal:
        with np.errstate(divide="ignore"):
            p = np.float32(1.0) / np.maximum(p, np.finfo(np.float32).tiny)
    return p[0] if one else p


def bartlett(scan, r):
    """The conventional beam's power w R w^H over the scan's grid: (G,) or (count, G) float32, numpy."""
    r64, one = _host64(r)
    return _spectrum(scan, r64, one, False)


def capon(scan, r, loading=0.0):
    """Capon's spectrum 1 / (w R^-1 w^H): the inverse in float64 (numpy.linalg.inv) of R + loading * trace(R) / N * I,
    uploaded as complex64, scanned, reciprocal."""
    r64, one = _host64(r)
    n = r64.shape[-1]
    inv = np.stack([np.linalg.inv(m + (loading * np.trace(m).real / n) * np.eye(n)) for m in r64])
    return _spectrum(scan, inv, one, True)


def music(scan, r, sources):
    """MUSIC's pseudo-spectrum 1 / (w P w^H), P the projector on the span of the N - sources eigenvectors of R with the
    smallest eigenvalues (float64 numpy.linalg.eigh), uploaded as complex64, scanned, reciprocal."""
    r64, one = _host64(r)
    n = r64.shape[-1]
    if not 0 < sources < n:
        raise ErrInvalidArgument("music: 0 < sources < channels")
    proj = []
    for m in r64:
        _, vec = np.linalg.eigh((m + m.conj().T) / 2)  # (ascending eigenvalues)
        noise = vec[:, :n - sources]
        proj.append(noise @ noise.conj().T)
    return _spectrum(scan, np.stack(proj), one, True)


def peaks(p, k):
    """Grid indices of the k largest local maxima of a spectrum p (an end point counts where it exceeds its one
    neighbour), the largest first."""
    p = np.asarray(p, np.float64).reshape(-1)
    left = np.concatenate(([-np.inf], p[:-1]))
    right = np.concatenate((p[1:], [-np.inf]))
    idx = np.flatnonzero((p > left) & (p >= right))
    return idx[np.argsort(-p[idx], kind="stable")][:k]


__all__ = ["Covariance", "Scan", "steering_weights", "bartlett", "capon", "music", "peaks", "COVAR_FORM_ONE_TILE", "COVAR_FORM_THREE_TILES"]

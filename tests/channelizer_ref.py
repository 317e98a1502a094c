"""float64 restatements of the polyphase channelizer's definition (include/hzsdr_channelizer.h), for the tests.

Two statements of the same thing over a stream `c` of converted samples (complex), a prototype `g` of L = P*M values
and a hop D:

  channels_direct:  y[j][k] = sum_i g[i] c[jD + i] exp(-2 pi i k (jD + i) / M)      -- the definition
  channels_fold:    u_j[r] = sum_p g[i_p] c[jD + i_p], i_p = ((r - jD) mod M) + pM;  y[j] = FFT_M(u_j)

and the error bound B(M, P) every comparison of the kernel against them uses.
"""
import numpy as np


def frames_of(n, L, D):
    """frames a stream of n samples completes"""
    return (n - L) // D + 1 if n >= L else 0


def bound(M, P):
    """B(M, P): the project's FFT bar (3e-7 log2 M) plus the float32 unit roundoff per fold term."""
    return 3e-7 * np.log2(M) + 6e-8 * (P + 2)


def channels_direct(c, g, M, D, ks=None, frames=None):
    """The definition, term by term: (frames, len(ks)) complex128.  The phase's argument k (jD + i) is reduced mod M
    in integer arithmetic before it is scaled."""
    c = np.asarray(c).astype(np.complex128)
    g = np.asarray(g).astype(np.float64)
    L = g.shape[0]
    F = frames_of(c.shape[0], L, D) if frames is None else frames
    ks = np.arange(M, dtype=np.int64) if ks is None else np.asarray(ks, np.int64)
    out = np.zeros((F, ks.shape[0]), np.complex128)
    i = np.arange(L, dtype=np.int64)
    for j in range(F):
        t = j * D + i
        ph = (ks[:, None] * (t % M)[None, :]) % M
        e = np.exp(-2j * np.pi * ph.astype(np.float64) / M)
        out[j] = e @ (g * c[t])
    return out


def channels_fold(c, g, M, D, frames=None):
    """The fold indexed by absolute time modulo M, then one forward transform per frame: (frames, M) complex128,
    ZeroFirst."""
    c = np.asarray(c).astype(np.complex128)
    g = np.asarray(g).astype(np.float64)
    L = g.shape[0]
    P = L // M
    F = frames_of(c.shape[0], L, D) if frames is None else frames
    if F == 0:
        return np.zeros((0, M), np.complex128)
    j = np.arange(F, dtype=np.int64)
    idx = j[:, None] * D + np.arange(L, dtype=np.int64)[None, :]
    v = (c[idx] * g).reshape(F, P, M).sum(axis=1)            # v_j[i0] = sum_p g[i0 + pM] c[jD + i0 + pM]
    src = (np.arange(M, dtype=np.int64)[None, :] - (j * D)[:, None]) % M
    u = np.take_along_axis(v, src, axis=1)                   # u_j[r] = v_j[(r - jD) mod M]
    return np.fft.fft(u, axis=1)


def pos(k, M, negative_first):
    """output position of channel k"""
    return (np.asarray(k) + M // 2) % M if negative_first else np.asarray(k)

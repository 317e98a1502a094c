"""float64 restatements of the polyphase synthesis bank's definition (include/hzsdr_synthesizer.h), for the tests.

Two statements of the same thing over frames Y (F x M complex, ZeroFirst), a prototype `g` of L = P*M values and a
hop D; the output has (F - 1) D + L positions:

  synth_direct:  x^[t] = sum_{j : 0 <= t - jD < L} g[t - jD] sum_k Y[j][k] exp(+2 pi i k t / M)    -- the definition
  synth_ola:     w_j = M * IFFT_M(Y[j]);  x^[jD + i] += g[i] w_j[(jD + i) mod M],  i = 0 .. L-1

and the error bound B(M, Q), Q = ceil(L / D), every comparison of the kernels against them uses.
"""
import numpy as np


def samples_of(F, L, D):
    """samples a whole stream of F frames yields: push plus flush"""
    return (F - 1) * D + L if F else 0


def terms(L, D):
    """Q: the most frames that cover one output position"""
    return -(-L // D)


def bound(M, Q):
    """B(M, Q): the project's FFT bar (3e-7 log2 M) plus the float32 unit roundoff per overlap-add term, the
    construction of channelizer_ref.bound."""
    return 3e-7 * np.log2(M) + 6e-8 * (Q + 2)


def synth_direct(Y, g, M, D, ts):
    """The definition, term by term, at the output positions `ts`: complex128.  The phase's argument k t is reduced
    mod M in integer arithmetic before it is scaled."""
    Y = np.asarray(Y).astype(np.complex128)
    g = np.asarray(g).astype(np.float64)
    F, L = Y.shape[0], g.shape[0]
    k = np.arange(M, dtype=np.int64)
    out = np.zeros(len(ts), np.complex128)
    for n, t in enumerate(int(t) for t in ts):
        e = np.exp(2j * np.pi * ((k * (t % M)) % M).astype(np.float64) / M)
        for j in range(max(0, (t - L) // D + 1), min(F - 1, t // D) + 1):
            out[n] += g[t - j * D] * (Y[j] @ e)
    return out


def synth_ola(Y, g, M, D):
    """One unnormalised backward transform per frame, repeated with period M, weighted by g and overlap-added:
    (F - 1) D + L complex128 values."""
    Y = np.asarray(Y).astype(np.complex128)
    g = np.asarray(g).astype(np.float64)
    F, L = Y.shape[0], g.shape[0]
    out = np.zeros(samples_of(F, L, D), np.complex128)
    w = np.fft.ifft(Y, axis=1) * M
    i = np.arange(L, dtype=np.int64)
    for j in range(F):
        out[j * D:j * D + L] += g * w[j][(j * D + i) % M]
    return out


def overlap_gain(g, D, n):
    """c[t] = sum_j g^2[t - jD] over every frame j >= 0, t = 0 .. n-1, in float64 from the taps as given"""
    g2 = np.asarray(g).astype(np.float64) ** 2
    L = g2.shape[0]
    c = np.zeros(n + L, np.float64)
    for s in range(0, n, D):
        c[s:s + L] += g2
    return c[:n]

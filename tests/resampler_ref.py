"""Float64 restatements of the polyphase resampler's definition (include/hzsdr_resampler.h), its counts and its bound.

    phi_m = (m D) mod U,  i_m = floor(m D / U),  y[m] = sum_{q < Q} h[phi_m + q U] x[i_m - q]

with Q = ceil(L / U), h zero past L and x zero outside [0, N): scipy.signal.upfirdn(h, x, U, D)."""
import numpy as np


def outputs_after(n, up, down):
    """M(N) = ceil(N U / D): the outputs written once N samples have been pushed"""
    return -((-n * up) // down)


def total_outputs(n, ntaps, up, down):
    """the whole stream's outputs, pushes and flush: upfirdn's length, ceil(((N - 1) U + L) / D); none for N = 0"""
    return -((-((n - 1) * up + ntaps)) // down) if n > 0 else 0


def stream_outputs(n, ntaps, up, down):
    """the outputs of pushes and flush together: upfirdn's length, except that with L < U the pushes alone may already
    have written more, M(N) of them, the last ones sums of padding taps only (+0)"""
    return max(outputs_after(n, up, down), total_outputs(n, ntaps, up, down))


def bound(q):
    """relative L2 of a block of float32 outputs against float64: the fold term of the banks' bounds, Q terms each
    rounded once plus the conversion and the final rounding"""
    return 6e-8 * (q + 2)


def upfirdn_direct(h, x, up, down):
    """the literal restatement: zero-stuff by U, convolve with h, keep every D-th"""
    h = np.asarray(h, np.float64)
    x = np.asarray(x).astype(np.complex128)
    if x.shape[0] == 0:
        return np.zeros(0, np.complex128)
    z = np.zeros((x.shape[0] - 1) * up + 1, np.complex128)
    z[::up] = x
    return np.convolve(z, h)[::down]


def upfirdn_poly(h, x, up, down):
    """the polyphase sum of the definition, vectorised over m"""
    h = np.asarray(h, np.float64)
    x = np.asarray(x).astype(np.complex128)
    n, L = x.shape[0], h.shape[0]
    q = -(-L // up)
    count = total_outputs(n, L, up, down)
    hp = np.zeros(q * up, np.float64)
    hp[:L] = h
    xp = np.concatenate([np.zeros(q - 1, np.complex128), x, np.zeros(q + 1 + (count * down) // up - n if count else 0, np.complex128)])
    m = np.arange(count, dtype=np.int64)
    phi, i = (m * down) % up, (m * down) // up
    y = np.zeros(count, np.complex128)
    for k in range(q):
        y += hp[phi + k * up] * xp[i - k + (q - 1)]
    return y

"""Structured inputs that read the polyphase kernels' tables out one entry at a time, and what they must give.

White input under a relative-L2 bound does not see every wrong tap: one entry at a filter's edge is 1e-4 of the
largest, and a block's error moves by less than the bound leaves room for (tests/test_readout_cpu.py keeps that
experiment).  An input with ONE non-zero term per output makes every output a single product h * amp:

  resampler    impulses every Q samples, amp a power of two times (1 - 0.5j) or a unit: the product is exact in
               float32 and every other term is fma(h, +-0, acc), so the output EQUALS the float64 reference rounded;
  channelizer  one impulse every L samples: every frame is the transform of a one-hot vector g[l] * amp;
  synthesizer  one non-zero frame value: the output is g[t - j0 D] * amp * exp(+2 pi i k0 t / M) over L positions.

No GPU and no library here: numpy alone, shared by the CPU and the GPU tests."""
import numpy as np

import resampler_ref as rref
from util import DT, FFT_FLOOR, FFT_K, fft_bin_errors, fft_yardstick, impulse, impulse_want64

# ---- amplitudes ------------------------------------------------------------------------------------
# c64: 2^-(k mod 8) (1 - 0.5j).  i8 converts as b / 128: (64 >> k, -(32 >> k)), k mod 6, is 2^-(1 + k) (1 - 0.5j).
# i16 converts as v / 32767, whose only exact non-zero values are +-1: units with differing components.
_I16_UNITS = [(32767, 0), (0, -32767), (-32767, 32767), (32767, -32767)]


def train_amp(fmt, k):
    """-> (the raw (I, Q) pair or complex64 value of impulse k, its converted value as a Python complex)"""
    if fmt == "c64":
        a = 2.0 ** -(k % 8) * (1 - 0.5j)
        return np.complex64(a), a
    if fmt == "i8":
        s = k % 6
        return (64 >> s, -(32 >> s)), complex((64 >> s) / 128.0, -(32 >> s) / 128.0)
    if fmt == "i16":
        i, q = _I16_UNITS[k % 4]
        return (i, q), complex(i / 32767.0, q / 32767.0)
    raise ValueError("no zero in this format's conversion: " + fmt)


def train(fmt, n, spacing, first=0):
    """n samples, zero except impulse k at first + k * spacing -> (raw samples of the format, converted complex64)"""
    raw = np.zeros(n, np.complex64) if fmt == "c64" else np.zeros((n, 2), DT[fmt])
    conv = np.zeros(n, np.complex64)
    at = np.arange(first, n, spacing)
    period = [train_amp(fmt, k) for k in range(24)]  # (a multiple of every format's period)
    k = np.arange(at.shape[0]) % 24
    raw[at] = np.array([r for r, _ in period], raw.dtype)[k]
    conv[at] = np.array([a for _, a in period], np.complex64)[k]
    return raw, conv


def train_rows(fmt, n, q):
    """Q rows of n samples, row r the train of spacing Q shifted by r: across the rows every sample position carries
    an impulse once, so every output position meets every q.  -> the raw rows; row r's converted values are
    train(fmt, n, q, first=r)[1] (not kept: Q rows of complex64 are half a gigabyte at the largest shape)"""
    first = train(fmt, n, q, first=0)[0]
    rows = np.zeros((q,) + first.shape, first.dtype)
    for r in range(q):
        rows[r] = train(fmt, n, q, first=r)[0]
    return rows


# ---- the resampler ---------------------------------------------------------------------------------

def resampler_indices(n, ntaps, up, down, count=None):
    """(phi_m, i_m) of the outputs m < count (the whole stream's, pushes and flush, by default)"""
    count = rref.total_outputs(n, ntaps, up, down) if count is None else count
    m = np.arange(count, dtype=np.int64)
    return (m * down) % up, (m * down) // up


def resampler_terms(x, ntaps, up, down):
    """the number of non-zero terms h[phi_m + q U] x[i_m - q] of every output (padding taps count: the kernel
    evaluates them)"""
    n = x.shape[0]
    q = -(-ntaps // up)
    phi, i = resampler_indices(n, ntaps, up, down)
    xp = np.concatenate([np.zeros(q - 1, bool), np.asarray(x) != 0, np.zeros(int(i.max()) + 1, bool)])
    return sum(xp[i - k + (q - 1)].astype(np.int64) for k in range(q))


def resampler_coverage(n, ntaps, up, down, count=None):
    """Over the Q rows of train_rows(fmt, n, Q): -> (table entries (phi, q) read by a non-zero sample, entries there
    are).  An entry is hp[phi][q] = h[phi + q U] with phi + q U < L and phi a multiple of gcd(U, D), the phases a
    stream can have (U and D are not reduced).  From the definition's indices alone."""
    q = -(-ntaps // up)
    phi, i = resampler_indices(n, ntaps, up, down, count)
    read = np.zeros((up, q), bool)
    for k in range(q):
        j = i - k  # the sample term k of an output reads: some row has its impulse there whenever it is in the stream
        ok = (j >= 0) & (j < n)
        read[phi[ok], k] = True
    exists = (np.arange(up)[:, None] + up * np.arange(q)[None, :] < ntaps) & (np.arange(up) % np.gcd(up, down) == 0)[:, None]
    return int((read & exists).sum()), int(exists.sum())


def polyphase_table(h, up):
    """hp[phi][q] = h[phi + q U] as float32, +0 past L: the table a create builds"""
    h = np.asarray(h, np.float32)
    q = -(-h.shape[0] // up)
    hp = np.zeros(q * up, np.float32)
    hp[:h.shape[0]] = h
    return np.ascontiguousarray(hp.reshape(q, up).T)


def resampler_f32(hp, x, ntaps, up, down):
    """A float32 emulation of the kernel's sum over a table hp[phi][q]: q ascending from +0, every term one
    multiply-add rounded to float32 once per component (the product of two float32 values is exact in float64, and
    the sum is rounded to float32 from there)."""
    x = np.asarray(x, np.complex64)
    n, q = x.shape[0], hp.shape[1]
    phi, i = resampler_indices(n, ntaps, up, down)
    xp = np.concatenate([np.zeros(q - 1, np.complex64), x, np.zeros(int(i.max()) + 1, np.complex64)])
    re, im = np.zeros(phi.shape[0], np.float32), np.zeros(phi.shape[0], np.float32)
    for k in range(q):
        h = hp[phi, k].astype(np.float64)
        s = xp[i - k + (q - 1)]
        re = (h * s.real.astype(np.float64) + re.astype(np.float64)).astype(np.float32)
        im = (h * s.imag.astype(np.float64) + im.astype(np.float64)).astype(np.float32)
    return (re + 1j * im.astype(np.complex64)).astype(np.complex64)


def readout_equal(got, want64):
    """the read-out's assertion: value equality with the float64 reference rounded to complex64 (+0 equals -0), no NaN"""
    got = np.asarray(got)
    return got.shape == want64.shape and not np.isnan(got.view(np.float32)).any() and np.array_equal(got, want64.astype(np.complex64))


# ---- the channelizer -------------------------------------------------------------------------------

def channelizer_train(fmt, n, L, first):
    """one impulse every L samples from `first` (< L): every window of L samples holds exactly one"""
    assert 0 <= first < L
    return train(fmt, n, L, first=first)


def channelizer_onehots(conv, g, m, d, frames):
    """For the converted train `conv`: -> (taps' indices l_j, one-hot fold vectors u (frames, M) complex64 with
    u_j[t mod M] = g[l_j] * amp, their float64 transforms).  The product is formed in float64 and must be exact in
    float32."""
    g = np.asarray(g, np.float32)
    L = g.shape[0]
    at = np.flatnonzero(conv)
    ls = np.zeros(frames, np.int64)
    u = np.zeros((frames, m), np.complex64)
    want = np.zeros((frames, m), np.complex128)
    for j in range(frames):
        inside = at[(at >= j * d) & (at < j * d + L)]
        assert inside.shape[0] == 1, "a window of L samples without exactly one impulse"
        t = int(inside[0])
        ls[j] = t - j * d
        v = float(g[ls[j]]) * complex(conv[t])
        assert complex(np.complex64(v)) == v, "the fold's one product is not exact in float32"
        u[j, t % m] = v
        want[j] = impulse_want64(m, t % m, a=v)
    return ls, u, want


# ---- the synthesizer -------------------------------------------------------------------------------

def synthesizer_want(g, m, d, frames, j0, k0, amp):
    """The stream of `frames` frames that are zero but for Y[j0][k0] = amp (k0 a ZeroFirst channel): -> (want as
    complex128 over (frames - 1) D + L positions, |g[t - j0 D]| |amp| per position, 0 outside the frame's span)"""
    g = np.asarray(g, np.float32).astype(np.float64)
    L = g.shape[0]
    want = np.zeros((frames - 1) * d + L, np.complex128)
    scale = np.zeros(want.shape[0], np.float64)
    t = j0 * d + np.arange(L, dtype=np.int64)
    ang = 2.0 * np.pi * ((k0 * (t % m)) % m).astype(np.float64) / float(m)
    want[t] = g * complex(amp) * (np.cos(ang) + 1j * np.sin(ang))
    scale[t] = np.abs(g) * abs(complex(amp))
    return want, scale


def synthesizer_yardstick(m, k0, amp):
    """max_bin of the single-precision backward transform of the one-hot frame: measured on scipy's transform, not on
    the code under test"""
    x = impulse(m, k0, a=amp)
    return fft_bin_errors(fft_yardstick(x, forward=False), impulse_want64(m, k0, a=amp, forward=False))[0]


def synthesizer_bound(m, k0, amp):
    """per output, relative to |g[t - j0 D]| |amp|: the transform's K = FFT_K over the yardstick with its floor, plus
    2^-24 for the one rounding of the product with the tap"""
    return FFT_K * max(synthesizer_yardstick(m, k0, amp), FFT_FLOOR) + 2.0 ** -24


# ---- shapes and filters shared by the CPU and the GPU tests ----------------------------------------
# (U, D, L, T) of the resampler's accuracy list: T is the planner's tile, which the GPU tests confirm with plan()
RESAMPLER_SHAPES = [(3, 2, 24, 1024), (2, 3, 50, 1024), (160, 147, 1920, 1024), (1, 8, 128, 256), (8, 1, 64, 1024), (7, 5, 3, 1024),
                    (5, 5, 20, 1024), (1, 1024, 256, 256), (1024, 1, 2048, 1024), (147, 160, 18816, 1024),
                    # the forms the list lacked: T1024 pad uniform (twice), lds, global; T256 pad lds, global
                    (1, 2, 31, 1024), (1, 4, 64, 1024), (2, 5, 50, 1024), (64, 135, 7000, 1024), (3, 20, 90, 256), (40, 300, 8000, 256),
                    # the largest LDS request of all shapes (tests/host/resampler_plan.cpp searches for it): 66 776 bytes,
                    # T256 pad lds; and the largest of the four-chain kernel, 66 688 bytes
                    (26, 498, 6110, 256), (170, 845, 5440, 1024),
                    # direct with the table in memory
                    (32, 1024, 8192, 256)]
LARGEST_LDS = (26, 498, 235, 5120, 66776)  # U, D, Q, window, bytes
# the one shape whose Q rows of 2 T + 3 outputs would be a gigabyte: i8 rows and T + 3 outputs
READOUT_SMALL = (1, 1024, 256, 256)


def readout_outputs(shape):
    return (shape[3] + 3) if shape == READOUT_SMALL else 2 * shape[3] + 3


def samples_for(count, up, down):
    """the fewest samples after which `count` outputs have been written"""
    return -(-count * down // up)


def kaiser_taps(up, down, ntaps):
    """a Kaiser-windowed sinc of any length, cutoff 1 / max(U, D), scaled to sum U, float32"""
    t = np.arange(ntaps, dtype=np.float64) - (ntaps - 1) / 2.0
    h = np.sinc(t / max(up, down)) * np.kaiser(ntaps, 8.0)
    return (h * (up / h.sum())).astype(np.float32)


def bank_taps(m, p, beta=8.0):
    """channelizer_taps restated: the Kaiser-windowed sinc with its cutoff at fs / (2 M), DC gain 1, float32"""
    n = m * p
    t = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
    h = np.sinc(t / m) * np.kaiser(n, float(beta))
    return (h / h.sum()).astype(np.float32)


def block_errors(got, want, block=256):
    """relative L2 of every block of outputs against the float64 reference (a block of an all-zero reference: 0 if the
    outputs are zero, inf otherwise)"""
    d = np.asarray(got).astype(np.complex128) - want
    out = []
    for a in range(0, want.shape[0], block):
        nw = np.linalg.norm(want[a:a + block])
        nd = np.linalg.norm(d[a:a + block])
        out.append(nd / nw if nw else (0.0 if nd == 0 else np.inf))
    return np.array(out)

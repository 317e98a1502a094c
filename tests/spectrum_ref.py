"""The fused power spectrum restated in numpy, and the per-bin bar its kernels are held to.

    want_rows      float64 restatement of the definition (the older row-L1 tests use it)
    spectrum_bar   (want, bound) per bin: the frames as the kernel forms them (complex64 sample times float32 window, one
                   rounding per component, so the input's own rounding is not charged), numpy's float64 transform, and a
                   bound built from the amplitude bar the FFT core already meets (util.FFT_K over scipy's complex64
                   transform with util.FFT_FLOOR) -- no constant of its own:
                       e_frame   = FFT_K * max(max_bin(Y, X), FFT_FLOOR) * max_k |X_k|
                       bin       : 2 sqrt(P) e + e^2 + 3 * 2^-24 P          (P = |X_k|^2; the three roundings of bin_power)
                       row       : the sum over its frames + (avg + 1) * 2^-24 * sum(P)   (float32 sums, the scale's product)
                   all times `scale`
    input classes  white, comb, tones, tone_off_bin: raw samples of a format and their converted complex64
    exact streams  zero except one sample per frame, amplitudes of readout.train_amp chosen so that every prefix of a
                   row's float64 sum is a float32 value: the row is then the same bits in any summation order

No GPU and no library here: numpy (and scipy for the yardstick), shared by the CPU and the GPU tests."""
import numpy as np

from readout import train_amp
from util import DT, FFT_FLOOR, FFT_K, splitmix64

CLASSES = ("white", "comb", "tones", "tone_off_bin")
U24 = 2.0 ** -24


def want_rows(c, n, hop, avg, w, scale):
    """float64 restatement: the complete rows of one stream of converted samples c, ZeroFirst."""
    L = c.shape[0]
    F = (L - n) // hop + 1 if L >= n else 0
    rows = F // avg
    if rows == 0:
        return np.zeros((0, n))
    idx = np.arange(rows * avg)[:, None] * hop + np.arange(n)[None, :]
    w64 = np.ones(n) if w is None else w.astype(np.float64)
    X = np.fft.fft(c.astype(np.complex128)[idx] * w64, axis=1)
    p = (X.real ** 2 + X.imag ** 2).reshape(rows, avg, n).sum(axis=1)
    return float(scale) * p


def row_l1_bound(n, avg):
    """the older tests' bound on a row's relative L1 error (tests/test_gpu_spectrum.py)"""
    return 2 * (3e-7 * np.log2(n) + 1e-7) + 6e-8 * (avg + 4)


def row_l1(got, want):
    return np.abs(np.asarray(got, np.float64) - want).sum(axis=1) / want.sum(axis=1)


# ---- the frames and the bar ------------------------------------------------------------------------------------------

def counts(L, n, hop, avg):
    """-> (frames, complete rows) of a stream of L samples"""
    F = (L - n) // hop + 1 if L >= n else 0
    return F, F // avg


def frames32(c, n, hop, w, count, first=0):
    """frames first .. first + count - 1 as the kernel forms them: complex64 samples times the float32 window, each
    component one float32 product"""
    c = np.asarray(c, np.complex64)
    idx = (first + np.arange(count))[:, None] * hop + np.arange(n)[None, :]
    f = c[idx]
    if w is None:
        return f
    w32 = np.asarray(w, np.float32)[None, :]
    out = np.empty(f.shape, np.complex64)
    out.real = f.real * w32
    out.imag = f.imag * w32
    return out


def _yardstick(f):
    import scipy.fft
    y = scipy.fft.fft(f, axis=1)
    assert y.dtype == np.complex64, "the yardstick left single precision: %s" % y.dtype
    return y


def frame_bar(f):
    """-> (P, bound) per frame and bin for complex64 frames f (frames, n), both float64, unscaled"""
    X = np.fft.fft(f.astype(np.complex128), axis=1)
    Y = _yardstick(np.ascontiguousarray(f)).astype(np.complex128)
    peak = np.abs(X).max(axis=1)
    max_bin = np.abs(Y - X).max(axis=1) / np.maximum(peak, 1e-300)
    e = (FFT_K * np.maximum(max_bin, FFT_FLOOR) * peak)[:, None]
    P = X.real ** 2 + X.imag ** 2
    return P, 2.0 * np.sqrt(P) * e + e * e + 3.0 * U24 * P


def spectrum_bar(c, n, hop, avg, w, scale, slab=256):
    """-> (want, bound), both (rows, n) float64, ZeroFirst: the complete rows of the converted stream c and how far a
    bin of a float32 spectrum may lie from them (module docstring).  Rows are walked `slab` at a time."""
    _, rows = counts(c.shape[0], n, hop, avg)
    want, bound = np.zeros((rows, n)), np.zeros((rows, n))
    for r0 in range(0, rows, slab):
        r1 = min(rows, r0 + slab)
        P, b = frame_bar(frames32(c, n, hop, w, (r1 - r0) * avg, first=r0 * avg))
        P, b = P.reshape(r1 - r0, avg, n).sum(axis=1), b.reshape(r1 - r0, avg, n).sum(axis=1)
        want[r0:r1] = P
        bound[r0:r1] = b + (avg + 1) * U24 * P
    return float(scale) * want, float(scale) * bound


def negative_first(a):
    """ZeroFirst rows -> NegativeFirst rows"""
    return np.fft.fftshift(a, axes=-1)


def bar_ratio(got, want, bound):
    """|got - want| / bound per bin; where the bound is zero (an all-zero row) 0 for an exact zero, inf otherwise; NaN
    stays NaN"""
    d = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = d / bound
    return np.where(bound > 0, r, np.where(d == 0, 0.0, np.where(np.isnan(d), np.nan, np.inf)))


def check_bar(got, want, bound, what=""):
    """|got - want| <= bound for every bin of every row; a failure names the row and the bin, a NaN fails.
    -> the worst ratio"""
    got = np.asarray(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.size == 0:
        return 0.0
    d = np.abs(got.astype(np.float64) - want)
    bad = ~(d <= bound)
    if bad.any():
        r, k = np.argwhere(bad)[0]
        raise AssertionError("%s: %d of %d bins over the bar, the first at row %d bin %d: got %.9g want %.9g, off by %.3e > %.3e"
                             % (what, int(bad.sum()), bad.size, r, k, got[r, k], want[r, k], d[r, k], bound[r, k]))
    return float(bar_ratio(got, want, bound).max())


# ---- input classes ---------------------------------------------------------------------------------------------------

def converted(orc, x):
    """hzsdr_convert's arithmetic, by the oracle's converters."""
    if x.dtype == np.complex64:
        return x.copy()
    out = np.zeros(x.shape[0], np.complex64)
    assert orc.convert(out, x) == x.shape[0]
    return out


def quantize(fmt, z):
    """complex128 values with components in [-1, 1] -> raw samples of the format at 0.9 of its full range"""
    z = 0.9 * np.asarray(z, np.complex128)
    if fmt == "c64":
        return z.astype(np.complex64)
    v = np.stack([z.real, z.imag], axis=1)
    if fmt == "u8":
        return np.clip(np.round(127.5 + 127.0 * v), 0, 255).astype(np.uint8)
    full = 127.0 if fmt == "i8" else 32767.0
    return np.round(full * v).astype(DT[fmt])


def _unit(z):
    return z / max(np.abs(z.real).max(), np.abs(z.imag).max())


def white_raw(fmt, L, seed):
    """full-range bytes / i16, c64 components in [-1, 1)"""
    z = splitmix64(seed, 2 * L)
    if fmt == "u8":
        return (z >> np.uint64(56)).astype(np.uint8).reshape(L, 2)
    if fmt == "i8":
        return (z >> np.uint64(56)).astype(np.uint8).view(np.int8).reshape(L, 2)
    if fmt == "i16":
        return (z >> np.uint64(48)).astype(np.uint16).view(np.int16).reshape(L, 2)
    f = ((z >> np.uint64(40)).astype(np.float64) / float(1 << 23) - 1.0).astype(np.float32)
    return f.view(np.complex64).reshape(L)


def comb_period(n, seed):
    """one period (n samples, float64) of the signal whose bin k has amplitude 1 + k / n and a random phase"""
    ph = 2.0 * np.pi * (splitmix64(seed, n) >> np.uint64(11)).astype(np.float64) / float(1 << 53)
    return _unit(np.fft.ifft((1.0 + np.arange(n) / float(n)) * np.exp(1j * ph)))


def tone_bins(n):
    t = n // 16
    return [0, 1, t - 1, t, n // 2 - 1, n // 2, n // 2 + 1, n - 1]


def class_raw(cls, fmt, n, L, seed):
    """L raw samples of input class `cls` for transforms of n"""
    if cls == "white":
        return white_raw(fmt, L, seed)
    t = np.arange(L, dtype=np.int64)
    if cls == "comb":
        return quantize(fmt, comb_period(n, seed)[t % n])
    if cls == "tones":  # block j of n samples: the tone on bin tone_bins[j mod 8] (one per frame with hop = n)
        k = np.array(tone_bins(n), np.int64)[(t // n) % 8]
        ang = 2.0 * np.pi * ((k * (t % n)) % n).astype(np.float64) / float(n)
        return quantize(fmt, np.cos(ang) + 1j * np.sin(ang))
    if cls == "tone_off_bin":
        ang = 2.0 * np.pi * (((n // 3) * t) % n + 0.37 * t) / float(n)
        return quantize(fmt, np.cos(ang) + 1j * np.sin(ang))
    raise ValueError(cls)


def class_input(orc, cls, fmt, n, L, seed):
    """-> (raw samples of the format, their converted complex64)"""
    x = class_raw(cls, fmt, n, L, seed)
    return x, converted(orc, x)


def asym_window(n):
    """0.25 + 0.75 p / n: no two entries equal, the first one non-zero"""
    return (0.25 + 0.75 * np.arange(n, dtype=np.float64) / n).astype(np.float32)


# ---- exact impulse streams -------------------------------------------------------------------------------------------
# Frame j is zero except amplitude a_j at position p_j of the frame.  train_amp's amplitudes are 2^-s (1 - 0.5j) (c64:
# s < 8; i8: s = 1 ... 6), so |a|^2 = 5 * 4^-(s+1): a row's sum is 5 * 4^-(m) * M with an integer M, and it is a float32
# value at every prefix as long as 5 M < 2^24.  With the first m amplitudes in turn, M <= ceil(avg / m) (4^m - 1) / 3.
# u8 has no exact zero and i16 only units: i8 and c64.

EXACT_FORMATS = ("i8", "c64")


def exact_period(fmt, avg):
    """how many of train_amp's amplitudes a row of `avg` frames may cycle through and stay exact in float32"""
    best = 1
    for m in range(1, (8 if fmt == "c64" else 6) + 1):
        if 5 * (-(-avg // m)) * ((4 ** m - 1) // 3) < (1 << 24):
            best = m
    return best


def impulse_stream(fmt, n, hop, positions, period, tail=0):
    """frames j < len(positions), frame j zero except train_amp(fmt, j mod period) at j * hop + positions[j]; `tail`
    zero samples behind the last frame -> (raw, |a_j|^2 per frame as float64, exact)"""
    positions = np.asarray(positions, np.int64)
    F = positions.shape[0]
    L = (F - 1) * hop + n + tail if F else tail
    raw = np.zeros(L, np.complex64) if fmt == "c64" else np.zeros((L, 2), DT[fmt])
    amps = [train_amp(fmt, k) for k in range(period)]
    k = np.arange(F) % period
    if F:
        raw[np.arange(F, dtype=np.int64) * hop + positions] = np.array([r for r, _ in amps], raw.dtype)[k]
    p = np.array([a.real * a.real + a.imag * a.imag for _, a in amps], np.float64)[k]
    return raw, p


def exact_rows(p, avg, w2, scale):
    """rows of scale * sum_t w2 * p[r avg + t], float64 -> (rows,) (w2: the squared window value, a float or per frame)"""
    rows = p.shape[0] // avg
    return float(scale) * (np.asarray(w2, np.float64) * p)[:rows * avg].reshape(rows, avg).sum(axis=1)


def prefix_sums_exact(p, avg):
    """every prefix of every row's float64 sum of p is a float32 value (and so is every float32 partial sum, in any
    order of the same terms up to that prefix)"""
    rows = p.shape[0] // avg
    c = np.cumsum(p[:rows * avg].reshape(rows, avg), axis=1)
    return bool((c.astype(np.float32).astype(np.float64) == c).all()) and bool((c < 3e38).all())


def pending_after(total, n, hop, avg):
    """(frames in the open row, samples held) after `total` samples of a stream"""
    F = (total - n) // hop + 1 if total >= n else 0
    nxt = F * hop
    return F % avg, (total - nxt if total > nxt else 0)


def slot_positions(n):
    """positions of a frame that include the first and last 64 and, for each of a lane's sixteen register slots (the
    sixteen runs of n / 16 consecutive positions), every lane residue modulo 64 from both ends of the run: all n
    positions up to 2048, 2048 of them beyond"""
    if n <= 2048:
        return np.arange(n)
    t = n // 16
    lanes = np.concatenate([np.arange(64), np.arange(t - 64, t)])
    return (np.arange(16)[:, None] * t + lanes[None, :]).reshape(-1)

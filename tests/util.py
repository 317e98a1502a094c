"""Shared helpers for the parity tests: formats, seeded synthetic inputs
(splitmix64), ULP distance, guarded device slices and the
per-bin FFT checker with its single-precision yardstick."""
import numpy as np

FMT = {"c64": 1, "u8": 2, "i16": 3, "i8": 4}
DT = {"c64": np.complex64, "u8": np.uint8, "i16": np.int16, "i8": np.int8}


def samples(fmt, data):
    """Build a sample buffer of format `fmt` from [[I, Q], ...] pairs."""
    if fmt == "c64":
        a = np.asarray(data, np.float32).reshape(-1, 2)
        return np.ascontiguousarray(a).view(np.complex64).reshape(-1)
    return np.ascontiguousarray(np.asarray(data).reshape(-1, 2).astype(DT[fmt]))


def filled(fmt, n, pair):
    if fmt == "c64":
        return np.full(n, np.complex64(complex(pair[0], pair[1])), np.complex64)
    a = np.empty((n, 2), DT[fmt])
    a[:, 0], a[:, 1] = pair[0], pair[1]
    return a


def zeros(fmt, n):
    return np.zeros(n, np.complex64) if fmt == "c64" else np.zeros((n, 2), DT[fmt])


def splitmix64(seed, n):
    """n uint64 values of the splitmix64 sequence (vectorised)."""
    idx = np.arange(1, n + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + idx * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z


def rand_u8(seed, n):
    return (splitmix64(seed, 2 * n) >> np.uint64(56)).astype(np.uint8).reshape(n, 2)


def rand_i8(seed, n):
    return rand_u8(seed, n).view(np.int8)


def rand_i16(seed, n):
    return (splitmix64(seed, 2 * n) >> np.uint64(48)).astype(np.uint16).view(np.int16).reshape(n, 2)


def rand_c64(seed, n):
    """re/im uniform in [-1, 1) as float32."""
    u = (splitmix64(seed, 2 * n) >> np.uint64(40)).astype(np.float64) / float(1 << 24)
    f = (u * 2.0 - 1.0).astype(np.float32)
    return f.view(np.complex64).reshape(n)


def ulp_diff(a, b):
    """Per-component ULP distance between two float32/complex64 arrays."""
    a = np.ascontiguousarray(a).view(np.float32).ravel()
    b = np.ascontiguousarray(b).view(np.float32).ravel()
    ai = a.view(np.int32).astype(np.int64)
    bi = b.view(np.int32).astype(np.int64)
    ai = np.where(ai < 0, -(ai & 0x7FFFFFFF), ai)
    bi = np.where(bi < 0, -(bi & 0x7FFFFFFF), bi)
    return np.abs(ai - bi)


def bits_equal(a, b):
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def in_epsilon(expected, actual, eps):
    """testify assert.InEpsilon: |e - a| / |e| <= eps."""
    e = np.asarray(expected, np.float64)
    a = np.asarray(actual, np.float64)
    return bool(np.all(np.abs(e - a) <= eps * np.abs(e)))


# ---- the FIR-decimate bound (one definition for every test, smoke() and bench.py repeat it) ----
# float32 FFT overlap-save against a float64 direct form: max-abs error per output
# <= FIR_ABS * sum|h| * max|x| AND relative L2 error <= FIR_REL_L2.  Round 1 used 4e-6 for the
# max-abs term, 50-100x what the kernels achieve; these are ~3x the worst case observed.
FIR_ABS = 6e-7
FIR_REL_L2 = 3e-7
# The two mixer orders against EACH OTHER.  Each is a float32 FFT pipeline of ~45 sequential
# roundings (1.6e-7 .. 2.0e-7 relative L2 from the oracle, tests/accuracy_probe.py) whose
# rounding errors are independent of the other's, so their distance measures sqrt(2) times
# that: 2.1e-7 .. 2.5e-7 on the cases here.  A late-mixer defect (a wrong modulated-tap
# spectrum, a phase slip of 1e-6 rad) shows up as 1e-6 or more.
CROSS_REL_L2 = 3e-7


def fir_errors(got, want, taps, xmax):
    """-> (max abs error, its bound, relative L2 error) of a FIR-decimate output."""
    g = np.asarray(got).astype(np.complex128)
    w = np.asarray(want).astype(np.complex128)
    err = float(np.abs(g - w).max()) if len(w) else 0.0
    bound = FIR_ABS * float(np.abs(np.asarray(taps)).sum()) * max(float(xmax), 1e-30)
    den = float(np.linalg.norm(w))
    rel = float(np.linalg.norm(g - w)) / den if den > 0 else 0.0
    return err, bound, rel


def assert_fir_close(got, want, taps, xmax, what=""):
    err, bound, rel = fir_errors(got, want, taps, xmax)
    assert err <= bound, (what, "max abs", err, bound)
    # very short / very quiet outputs: the L2 ratio is dominated by the float32 rounding of a
    # handful of outputs, the max-abs bound is the meaningful one there
    if len(np.asarray(want)) >= 64:
        assert rel <= FIR_REL_L2, (what, "rel L2", rel, FIR_REL_L2)
    return err, bound, rel


# ---- guarded device slices (tests/test_gpu_subslices.py, tests/test_gpu_fft_plans.py) ---------------------------------

SENT = 0xA5
GUARD = 64  # bytes of sentinel either side of a slice (a multiple of 32: the slice's residue is its offset's)
ES = {"c64": 8, "i16": 4, "u8": 2, "i8": 2}


def dtype_of(fmt):
    return zeros(fmt, 0).dtype


def typed(torch, raw, fmt):
    if fmt == "c64":
        return raw.view(torch.complex64)
    if fmt == "i16":
        return raw.view(torch.int16).view(-1, 2)
    if fmt == "i8":
        return raw.view(torch.int8).view(-1, 2)
    return raw.view(-1, 2)


class Guarded:
    """`n` samples of `fmt`, `off` samples (plus GUARD bytes) into a sentinel-filled device allocation (or into `raw`,
    another Guarded's allocation: a second view of the same bytes)."""

    def __init__(self, torch, fmt, n, off, fill=None, raw=None):
        es = ES[fmt]
        self.fmt, self.n = fmt, n
        self.lo = GUARD + off * es
        self.hi = self.lo + n * es
        if raw is None:
            total = self.hi + GUARD + (-(self.hi + GUARD) % 8)
            raw = torch.full((total,), SENT, dtype=torch.uint8, device="cuda")
        self.raw = raw
        assert raw.data_ptr() % 256 == 0, "the allocator's alignment changed: %#x" % raw.data_ptr()
        self.t = typed(torch, raw, fmt)[self.lo // es:self.hi // es]
        if n:  # (an empty slice has no address: data_ptr() is 0)
            assert self.t.data_ptr() % 32 == (off * es) % 32, (fmt, off, self.t.data_ptr() % 32)
        if fill is not None and n:
            self.t.copy_(torch.from_numpy(np.array(fill)))

    def bytes(self):
        return self.raw.cpu().numpy()

    def values(self):
        return self.bytes()[self.lo:self.hi].view(dtype_of(self.fmt)).reshape(zeros(self.fmt, self.n).shape)

    def check(self, want, what):
        """The guards intact and the slice equal to `want` byte for byte (want None: the guards only)."""
        b = self.bytes()
        assert (b[:self.lo] == SENT).all(), (what, "guard in front written", int((b[:self.lo] != SENT).sum()))
        assert (b[self.hi:] == SENT).all(), (what, "guard behind written", int((b[self.hi:] != SENT).sum()))
        if want is not None:
            w = np.ascontiguousarray(want).view(np.uint8).ravel()
            g = b[self.lo:self.hi]
            assert w.size == g.size, (what, w.size, g.size)
            if not np.array_equal(g, w):
                bad = np.flatnonzero((g != w).reshape(self.n, -1).any(1))
                raise AssertionError("%s: %d of %d samples differ, the first at %d of the slice"
                                     % (what, bad.size, self.n, bad[0]))
        return b


# ---- the per-bin FFT check and its single-precision yardstick --------------------------------------------------------
# A kernel's transform is scored against `want64`, the float64 transform of the float32 input AS STORED (the input's
# own rounding is not charged to the kernel), by two numbers: the worst single bin relative to the largest bin, and
# the relative L2 error.  The same two numbers of a single-precision transform of the same input (scipy's pocketfft,
# which stays in complex64) are the yardstick, and the assertion is
#     m(kernel) <= K * max(m(yardstick), 2**-23)        for m in (max_bin, rel_l2),  K = FFT_K = 4.
# K: a textbook float32 radix-2 transform whose twiddles are products of two rounded table entries (the kernels' own
# split form) measures 0.4 ... 2.4 x the yardstick on random, impulse and tone inputs at N = 2^12 ... 2^20, and one
# table entry off by 1e-5 measures 21 ... 57 x in max_bin (tests/test_fft_checker_cpu.py pins both); the floor is one
# float32 ulp for inputs the yardstick transforms almost exactly (an on-bin tone: 2.3e-8).
FFT_K = 4.0
FFT_FLOOR = 2.0 ** -23


def fft_bin_errors(got, want64):
    """-> (max_bin, rel_l2): max_k |got_k - want_k| / max_k |want_k| and ||got - want|| / ||want||."""
    g = np.asarray(got).astype(np.complex128).ravel()
    w = np.asarray(want64, np.complex128).ravel()
    d = np.abs(g - w)
    return float(d.max() / max(np.abs(w).max(), 1e-300)), float(np.linalg.norm(d) / max(np.linalg.norm(w), 1e-300))


def fft_worst_bin(got, want64):
    d = np.abs(np.asarray(got).astype(np.complex128).ravel() - np.asarray(want64, np.complex128).ravel())
    return int(np.argmax(np.where(np.isnan(d), np.inf, d)))


def fft_want64(x, forward=True):
    """numpy's float64 transform of the stored input; backward is unnormalised, like the plans."""
    x = np.asarray(x).astype(np.complex128)
    return np.fft.fft(x) if forward else np.fft.ifft(x) * len(x)


def impulse(n, p, a=1 + 1j):
    x = np.zeros(n, np.complex64)
    x[p % n] = a
    return x


def impulse_want64(n, p, a=1 + 1j, forward=True):
    """The transform of an impulse `a` at sample p: a * exp(-+2 pi i ((p k) mod N) / N), the product reduced in exact
    integer arithmetic (p k < 2^48)."""
    r = (np.arange(n, dtype=np.int64) * np.int64(p % n)) % np.int64(n)
    ang = (-2.0 if forward else 2.0) * np.pi * r.astype(np.float64) / float(n)
    return complex(np.complex64(a)) * (np.cos(ang) + 1j * np.sin(ang))


_CHIRP = {}  # (n, forward) -> (chirp as complex64, chirp filter's spectrum as complex64); the last length only


def _chirp(n, forward):
    if (n, forward) not in _CHIRP:
        if len(_CHIRP) >= 2:
            _CHIRP.clear()
        m = 1
        while m < 2 * n - 1:
            m <<= 1
        k = np.arange(n, dtype=np.int64)
        ang = (-np.pi if forward else np.pi) * ((k * k) % (2 * n)).astype(np.float64) / float(n)
        c64 = np.cos(ang) + 1j * np.sin(ang)
        b = np.zeros(m, np.complex128)
        b[:n] = np.conj(c64)
        b[m - n + 1:] = np.conj(c64[1:][::-1])
        _CHIRP[(n, forward)] = (c64.astype(np.complex64), np.fft.fft(b).astype(np.complex64))
    return _CHIRP[(n, forward)]


def bluestein_f32(x, forward, fft32, ifft32):
    """Bluestein's chirp transform in single precision over the M-point complex64 transforms `fft32` / `ifft32`
    (ifft32 normalised), the algorithm of csrc/hz_fft.hip: the chirp from n^2 mod 2N in float64 rounded once, the chirp
    filter's spectrum in float64 rounded once, two M-point single transforms and three complex64 products."""
    x = np.asarray(x, np.complex64)
    n = len(x)
    c, B = _chirp(n, bool(forward))
    m = len(B)
    a = np.zeros(m, np.complex64)
    a[:n] = x * c
    y = ifft32(fft32(a) * B)
    return (y[:n] * c).astype(np.complex64)


def _scipy_fft32(a):
    import scipy.fft
    y = scipy.fft.fft(np.asarray(a, np.complex64))
    assert y.dtype == np.complex64, "the yardstick left single precision: %s" % y.dtype
    return y


def _scipy_ifft32(a):
    import scipy.fft
    y = scipy.fft.ifft(np.asarray(a, np.complex64))
    assert y.dtype == np.complex64, "the yardstick left single precision: %s" % y.dtype
    return y


def fft_yardstick(x, forward=True):
    """A single-precision transform of the complex64 input: scipy's for a power of two, for any other length a float32
    Bluestein over scipy's power-of-two transforms (the algorithm the kernels implement, not pocketfft's mixed radix).
    Backward is unnormalised."""
    x = np.ascontiguousarray(x, np.complex64)
    n = len(x)
    if n & (n - 1):
        return bluestein_f32(x, forward, _scipy_fft32, _scipy_ifft32)
    if forward:
        return _scipy_fft32(x)
    import scipy.fft
    y = scipy.fft.ifft(x, norm="forward")
    assert y.dtype == np.complex64, "the yardstick left single precision: %s" % y.dtype
    return y


def fft_ratios(got, x, want64, forward=True):
    """-> ((max_bin, rel_l2) of `got`, the same of the yardstick, the two ratios got / max(yardstick, floor))."""
    mine = fft_bin_errors(got, want64)
    yard = fft_bin_errors(fft_yardstick(x, forward), want64)
    return mine, yard, tuple(m / max(y, FFT_FLOOR) for m, y in zip(mine, yard))


def assert_fft_close(got, x, want64, forward=True, what="", k=FFT_K):
    """The assertion above on both metrics; a failure names `what` and the worst bin.  -> the two ratios."""
    mine, yard, ratio = fft_ratios(got, x, want64, forward)
    for name, m, y, r in zip(("max_bin", "rel_l2"), mine, yard, ratio):
        # (not (m <= bound): a NaN fails)
        assert m <= k * max(y, FFT_FLOOR), "%s: %s %.3e > %g * max(yardstick %.3e, 2^-23), ratio %.1f, worst bin %d" % (
            what, name, m, k, y, r, fft_worst_bin(got, want64))
    return ratio


def assert_fft_rows_close(got, x, forward=True, what="", k=FFT_K, want64=None):
    """assert_fft_close on every row of a (rows, N) pair, the float64 transforms and the yardstick taken along the rows
    in one call each (numpy's float64 transform of x unless `want64` is given).  -> the worst two ratios."""
    got = np.asarray(got)
    x = np.ascontiguousarray(x, np.complex64)
    rows, n = x.shape
    if want64 is None:
        x64 = x.astype(np.complex128)
        want64 = np.fft.fft(x64, axis=1) if forward else np.fft.ifft(x64, axis=1) * n
    if n & (n - 1):
        yard = np.stack([fft_yardstick(r, forward) for r in x])
    else:
        import scipy.fft
        yard = scipy.fft.fft(x, axis=1) if forward else scipy.fft.ifft(x, axis=1, norm="forward")
        assert yard.dtype == np.complex64, "the yardstick left single precision: %s" % yard.dtype
    peak = np.maximum(np.abs(want64).max(axis=1), 1e-300)
    norm = np.maximum(np.linalg.norm(want64, axis=1), 1e-300)
    worst = [0.0, 0.0]
    dg, dy = np.abs(got.astype(np.complex128) - want64), np.abs(yard.astype(np.complex128) - want64)
    for i, (name, mg, my) in enumerate((("max_bin", dg.max(axis=1) / peak, dy.max(axis=1) / peak),
                                        ("rel_l2", np.linalg.norm(dg, axis=1) / norm, np.linalg.norm(dy, axis=1) / norm))):
        bound = k * np.maximum(my, FFT_FLOOR)
        bad = np.flatnonzero(~(mg <= bound))
        if bad.size:
            r = int(bad[0])
            raise AssertionError("%s: row %d (%d of %d rows fail): %s %.3e > %g * max(yardstick %.3e, 2^-23), worst bin %d"
                                 % (what, r, bad.size, rows, name, mg[r], k, my[r], fft_worst_bin(got[r], want64[r])))
        worst[i] = float((mg / np.maximum(my, FFT_FLOOR)).max())
    return tuple(worst)


def fft_inputs(n, few=False):
    """The structured inputs of one length -> [(name, x as complex64, want64 forward or None, want64 backward or None)]
    (None: numpy's float64 transform of x).  `few`: random, the impulses at 1 and near N/3 and one tone (the longest lengths)."""
    t = np.arange(n, dtype=np.float64)
    third = (n // 3) | 1
    out = [("random", rand_c64(n, n), None, None)]
    ps = [("impulse@1", 1), ("impulse@N-1", n - 1), ("impulse@N/2+1", n // 2 + 1), ("impulse@~N/3", third)]
    # (few: p = 1 puts exp(-2 pi i k / N) itself into the bins, p ~ N/3 a product of every table's entries)
    for name, p in (ps[0::3] if few else ps):
        out.append((name, impulse(n, p), impulse_want64(n, p, forward=True), impulse_want64(n, p, forward=False)))

    def tone(f):
        ang = 2.0 * np.pi * ((t * f) % n) / n
        return (np.cos(ang) + 1j * np.sin(ang)).astype(np.complex64)

    if not few:
        out.append(("dc", np.full(n, np.complex64(0.75 - 0.5j)), None, None))
        out.append(("alternating", (1.0 - 2.0 * (np.arange(n) & 1)).astype(np.complex64), None, None))
        out.append(("tone_on_bin", tone(float(n // 3)), None, None))
    out.append(("tone_off_bin", tone(n // 3 + 0.37), None, None))
    return out

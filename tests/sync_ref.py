"""Independent restatements, in numpy, of the coherent-sync path in front of Beamform (rtl/kerberos/internal/align.go,
fft/convolution.go) and the checks that tests/test_gpu_sync.py makes with them.  tests/test_sync_ref_cpu.py holds the
restatements to the oracle and shows that every check here can fail.

    peak_lag(c)               checkAlignment's scan: float32 power, exact zeros skipped, first maximum, fold above n // 2
    phases(a, b)              Phase(complex128(a * conj(b))) per pair, the product as Go's complex64 arithmetic forms it
    mean_phase_exact(a, b)    math.fsum of those phases / n: the correctly rounded sum, no summation order at all
    kernel_order_mean(ph)     the order hzsdr_mean_phase sums in: per-thread strided sum, tree of 256, workgroups in order
    closure_want64(kind,x,y)  forward, forward, (conjugated) product, unnormalised backward in complex128
    closure_yardstick(...)    the same three steps in single precision, spectra rounded to complex64 in between

The grid of the two reductions, from csrc/hz_kerberos.hip and csrc/hz_common.h (kThreads = 256, kRedBlocks = 1024;
blocks_for's own cap of 128 workgroups per CU is above 1024 on any device with 8 CUs or more): min(ceil(n / 256), 1024)
workgroups of 256 threads, so above n = S = 262144 a thread takes a second element, at its index + S.

The second half of the file builds the inputs that both test files use, so that the CPU file holds the restatements to
the oracle on exactly the classes the GPU file runs."""
import math

import numpy as np

from util import FFT_FLOOR, FFT_K, fft_bin_errors, fft_want64, fft_worst_bin, fft_yardstick

THREADS = 256  # kThreads, csrc/hz_common.h
RED_BLOCKS = 1024  # kRedBlocks, csrc/hz_kerberos.hip
S = THREADS * RED_BLOCKS  # the grid-stride of a full grid: 262144

PI = math.pi
CENSUS_TOL = 2.0 ** -49  # |mean * n - expected sum| of the exactly-once sweeps


def red_blocks(n):
    return max(1, min(-(-n // THREADS), RED_BLOCKS))


# ---- peak search -----------------------------------------------------------------------------------------------------

def powers(c):
    """float64(float32(re * re) + float32(im * im)): numpy's float32 products and sum round once each, nothing fused."""
    v = np.ascontiguousarray(c, np.complex64).view(np.float32).reshape(-1, 2)
    re, im = v[:, 0], v[:, 1]
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        rr = re * re
        ii = im * im
        s = rr + ii
    assert rr.dtype == ii.dtype == s.dtype == np.float32
    return s.astype(np.float64)


def fold(i, n):
    """align.go:145-147: an index above n // 2 is a negative lag."""
    return i - n if i > n // 2 else i


def peak_lag(c):
    """The lag of align.go:128-149.  The scan `if pow > max: max = pow`, started at -inf, keeps the first of equal
    maxima and never takes a NaN; np.argmax over the eligible powers (NaN and skipped ones set to -inf, which no power
    equals) picks the same element.  peak_lag_scan is that loop written out; the CPU tests hold the two together."""
    c = np.ascontiguousarray(c, np.complex64)
    n = len(c)
    if n == 0:
        return -1
    p = powers(c)
    ok = ~((c.real == 0) & (c.imag == 0)) & ~np.isnan(p)  # (-0.0 == 0 is true: both signs of zero are skipped)
    if not ok.any():
        return -1
    return fold(int(np.argmax(np.where(ok, p, -np.inf))), n)


def peak_lag_scan(c, wins=lambda p, best: p > best, skipped=lambda re, im: re == 0 and im == 0,
                  power=None, folds=lambda i, n: i > n // 2):
    """The reference's loop, one element at a time; the keyword arguments exist for the mutants of the CPU tests."""
    c = np.ascontiguousarray(c, np.complex64)
    n = len(c)
    p = powers(c) if power is None else power(c)
    v = c.view(np.float32).reshape(-1, 2)
    best, best_i = -math.inf, -1
    for i in range(n):
        if skipped(v[i, 0], v[i, 1]):
            continue
        if wins(p[i], best):
            best, best_i = p[i], i
    return best_i - n if folds(best_i, n) else best_i


def assert_peak(got, c, orc=None, want=None, what=""):
    """`got` is the restatement's lag of `c`, the oracle's where one is given, and `want` where the case knows it."""
    ref = peak_lag(c)
    if want is not None:
        assert ref == want, (what, "the restatement itself misses the expected lag", ref, want)
    if orc is not None:
        o = orc.peak_lag(np.ascontiguousarray(c, np.complex64))
        assert o == ref, (what, "oracle and restatement disagree", o, ref)
    assert got == ref, (what, "peak_lag", got, "want", ref)


# ---- mean phase ------------------------------------------------------------------------------------------------------

def phases(a, b):
    """atan2 in float64 of the complex64 product a * conj(b).  Go forms a complex64 product from float32 parts widened
    to float64 (the products are then exact), one float64 subtraction or addition, and one narrowing to float32."""
    a = np.ascontiguousarray(a, np.complex64).view(np.float32).reshape(-1, 2).astype(np.float64)
    b = np.ascontiguousarray(b, np.complex64).view(np.float32).reshape(-1, 2).astype(np.float64)
    ar, ai, br, bi = a[:, 0], a[:, 1], b[:, 0], -b[:, 1]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        re = (ar * br - ai * bi).astype(np.float32)
        im = (ar * bi + ai * br).astype(np.float32)
    return np.arctan2(im.astype(np.float64), re.astype(np.float64))


def mean_phase_exact(a, b):
    ph = phases(a, b)
    if np.isnan(ph).any():
        return math.nan
    return math.fsum(ph.tolist()) / len(ph)


def _sum2_add(hi, lo, x, xlo):
    """Sum2 of csrc/hz_kerberos.hip: (hi, lo) += (x, xlo), the addition's rounding error kept in lo (Knuth's two-sum)."""
    with np.errstate(invalid="ignore"):
        t = hi + x
        z = t - hi
        return t, lo + (((hi - (t - z)) + (x - z)) + xlo)


def kernel_order_mean(ph, compensated=True):
    """The mean of `ph` summed as hzsdr_mean_phase sums: each thread its elements a grid-stride apart, in order, from
    +0.0; the fixed tree over a workgroup's 256 threads; the workgroups' sums in order on the host; one division.
    Every addition carries its rounding error along (compensated=False: the plain sums the kernel made before)."""
    ph = np.asarray(ph, np.float64)
    n = len(ph)
    blocks = red_blocks(n)
    stride = blocks * THREADS
    trips = -(-n // stride)
    pad = np.zeros(trips * stride)
    pad[:n] = ph
    hi, lo = np.zeros(stride), np.zeros(stride)
    for t in range(trips):
        hi, lo = _sum2_add(hi, lo, pad[t * stride:(t + 1) * stride], 0.0)
    keep = 1.0 if compensated else 0.0
    hi, lo = hi.reshape(blocks, THREADS).copy(), lo.reshape(blocks, THREADS) * keep
    k = THREADS // 2
    while k:
        h, l = _sum2_add(hi[:, :k], lo[:, :k], hi[:, k:2 * k], lo[:, k:2 * k])
        hi[:, :k], lo[:, :k] = h, l * keep
        k //= 2
    th, tl = np.float64(0.0), np.float64(0.0)
    for p, q in zip(hi[:, 0], lo[:, 0]):
        th, tl = _sum2_add(th, tl, p, q)
        tl = tl * keep
    return float((th + tl) / n)


def mean_bound(n):
    """|mean - mean_phase_exact| allowed: any order of summing n float64 terms of size <= pi errs by at most
    (n - 1) u sum|x| <= (n - 1) n pi u with u = 2^-53, that is (n - 1) pi u on the mean; each atan2 is within a few
    ulp(pi) = 2^-51 of the true value in OCML and in libm, and the division rounds once: pi (n + 16) 2^-53."""
    return PI * (n + 16) * 2.0 ** -53


def assert_mean(got, a, b, what="", exact=None):
    """-> error / bound.  A NaN expected is a NaN required."""
    want = mean_phase_exact(a, b) if exact is None else exact
    if math.isnan(want):
        assert math.isnan(got), (what, "mean_phase: want NaN, got", got)
        return 0.0
    n = len(a)
    err = abs(got - want)
    assert err <= mean_bound(n), (what, "mean_phase", got, "want", want, "error", err, "bound", mean_bound(n))  # (a NaN fails)
    return err / mean_bound(n)


def assert_census(got, n, total, what=""):
    """The exactly-once sweeps: every phase but a few is +0, so mean * n is the sum of the few, to 2^-49."""
    assert abs(got * n - total) <= CENSUS_TOL, (what, "mean * n", got * n, "want", total)  # (a NaN fails)


# ---- the closures ----------------------------------------------------------------------------------------------------

KINDS = ("freq", "convolve", "xcorr")


def closure_want64(kind, x, y):
    """fft/convolution.go in complex128: `y` is the filter's spectrum (freq), a second signal (convolve) or the signal
    whose spectrum is conjugated (xcorr).  The backward transform is unnormalised, as fft_want64 has it."""
    assert kind in KINDS
    X = fft_want64(x, True)
    Y = np.asarray(y).astype(np.complex128) if kind == "freq" else fft_want64(y, True)
    return fft_want64(X * (np.conj(Y) if kind == "xcorr" else Y), False)


def closure_yardstick(kind, x, y, spoil=None):
    """The same in single precision: tests/util.py's yardstick for each transform, the spectra and their product
    rounded to complex64.  spoil = (bin, factor): one bin of x's spectrum multiplied by `factor` (the CPU tests'
    model of a wrong table entry)."""
    assert kind in KINDS
    X = fft_yardstick(x, True).astype(np.complex64)
    Y = np.ascontiguousarray(y, np.complex64) if kind == "freq" else fft_yardstick(y, True).astype(np.complex64)
    if spoil is not None:
        X = X.copy()
        X[spoil[0]] = X[spoil[0]] * np.complex64(spoil[1])
    P = X * (np.conj(Y) if kind == "xcorr" else Y)
    assert P.dtype == np.complex64
    return fft_yardstick(P, False)


def closure_ratios(got, kind, x, y, want64=None):
    """-> ((max_sample, rel_l2) of `got`, of the yardstick, got / max(yardstick, 2^-23)) against closure_want64."""
    w = closure_want64(kind, x, y) if want64 is None else want64
    mine = fft_bin_errors(got, w)
    yard = fft_bin_errors(closure_yardstick(kind, x, y), w)
    return mine, yard, tuple(m / max(v, FFT_FLOOR) for m, v in zip(mine, yard))


def assert_closure(got, kind, x, y, what="", k=FFT_K, want64=None):
    """m(kernel) <= k * max(m(yardstick), 2^-23) for m in (max_sample, rel_l2), as util.assert_fft_close.  -> ratios."""
    w = closure_want64(kind, x, y) if want64 is None else want64
    mine, yard, ratio = closure_ratios(got, kind, x, y, w)
    for name, m, v, r in zip(("max_sample", "rel_l2"), mine, yard, ratio):
        assert m <= k * max(v, FFT_FLOOR), "%s: %s %.3e > %g * max(yardstick %.3e, 2^-23), ratio %.1f, worst sample %d" % (
            what, name, m, k, v, r, fft_worst_bin(got, w))
    return ratio


def rotate(a, d):
    """`a` delayed by d samples, circularly: out[t] = a[t - d]."""
    return np.roll(np.asarray(a), d)


def implied_lag(n, d):
    """Where cross_correlate(a, rotate(a, d)) peaks: ifft(A conj(B)) with B_k = A_k e^(-2 pi i k d / n) is the
    autocorrelation moved to -d mod n, and checkAlignment folds an index above n // 2."""
    return fold((-d) % n, n)


def assert_lag(got, corr_want64, n, d, what=""):
    """`got` is the restatement's lag of the float64 correlation and the lag the delay implies."""
    ref = peak_lag(np.asarray(corr_want64).astype(np.complex64))
    assert ref == implied_lag(n, d), (what, "the float64 correlation does not peak where the delay says", ref, implied_lag(n, d))
    assert got == ref, (what, "lag", got, "want", ref)


# ---- inputs shared by tests/test_sync_ref_cpu.py and tests/test_gpu_sync.py -------------------------------------------

LENGTHS = [1, 2, 3, 255, 256, 257, 1000, 65536, S - 1, S, S + 1, 2 * S + 256, 3 * S + 77]


def cval(re, im):
    """One complex64 with exactly these float32 components (signed zeros and NaN kept)."""
    return np.array([re, im], np.float32).view(np.complex64)[0]


def hot_positions(n):
    """Where the one-hot and exactly-once sweeps put their sample: both ends, either side of a workgroup edge, of
    n // 2, of the grid-stride S and of the last (partial) workgroup."""
    tail = n - n % THREADS
    ps = [0, 1, 255, 256, n // 2 - 1, n // 2, n // 2 + 1, n - 2, n - 1, S - 1, S, S + 255, 2 * S, tail - 1, tail]
    return sorted({p for p in ps if 0 <= p < n})


def low_noise(seed, n):
    """White noise of power below 0.02: the floor under the planted samples."""
    from util import rand_c64
    return (np.float32(0.1) * rand_c64(seed, n).view(np.float32)).view(np.complex64)


TIE_FORMS = [cval(3, 4), cval(5, 0), cval(-5, 0), cval(0, -5)]  # four ways to a float32 power of exactly 25


def tie_placements(n):
    out = []
    if n > S + 7:
        out.append(("one thread, trips 1 and 2", 7, 7 + S))
    if n > 2 * S + 300:
        out.append(("one thread, trips 1 and 3", 300, 300 + 2 * S))
    if n > 200:
        out.append(("two threads of a workgroup", 5, 200))
    if n > 256:
        out.append(("last thread of a workgroup, first of the next", 255, 256))
    if n > S + 256:
        out.append(("the same in the second trip", S + 255, S + 256))
    if n >= 1000:
        out.append(("far-apart workgroups", 263, n - 200))
    if n >= 2:
        out.append(("first and last element", 0, n - 1))
    return out


def tie_cases(n):
    """-> (name, buffer, expected lag): two equal powers of 25 over low noise, each placement with either form in
    front; the smaller index wins."""
    base = low_noise(41, n)
    for k, (name, p, q) in enumerate(tie_placements(n)):
        for u, v in ((TIE_FORMS[k % 4], TIE_FORMS[(k + 1) % 4]), (TIE_FORMS[(k + 1) % 4], TIE_FORMS[k % 4])):
            c = base.copy()
            c[q] = v
            c[p] = u
            yield "tie %s (%d, %d) n=%d %s first" % (name, p, q, n, u), c, fold(p, n)


ARITH_A = cval(1 + 2.0 ** -12, 2.0 ** -12)
ARITH_C = cval(1 + 2.0 ** -12, 0.0)


def arithmetic_case(n):
    """C in front of A: their un-fused float32 powers are both 1 + 2^-11 (each of (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24
    and the sum with 2^-24 is a tie that rounds to even), so the first one, C, wins; a fused sum or a float64 power
    keeps the 2^-24 of A's imaginary part and picks A."""
    assert n >= 2
    c = low_noise(42, n)
    ic, ia = n // 3, n - 1
    c[ic], c[ia] = ARITH_C, ARITH_A
    return "float32 arithmetic n=%d" % n, c, fold(ic, n), ic, ia


def extreme_cases(n):
    """-> (name, buffer, expected lag), n >= 8."""
    assert n >= 8
    p, q = n // 4, n - 3
    for big in ((3e19, 2e19), (2e19, 3e19)):  # both powers overflow float32 to +Inf: equal, the first wins
        c = low_noise(43, n)
        c[p], c[q] = cval(big[0], 0), cval(big[1], 0)
        yield "overflow %g before %g n=%d" % (big[0], big[1], n), c, fold(p, n)
    c = np.full(n, cval(1e-20, 0), np.complex64)  # powers 1e-40 and 4e-40: float32 denormals, not to be flushed
    c[n - 2] = cval(2e-20, 0)
    yield "denormal powers n=%d" % n, c, fold(n - 2, n)
    yield "every power underflows to 0 n=%d" % n, np.full(n, cval(1e-30, 0), np.complex64), 0
    for before, after in ((cval(np.nan, 1), cval(1, np.nan)), (cval(1, np.nan), cval(np.nan, 1))):
        c = low_noise(44, n)
        c[p] = cval(50, 0)
        c[0] = c[p - 1] = before
        c[p + 1] = c[n - 1] = after
        yield "NaN around the peak n=%d %s" % (n, before), c, fold(p, n)
    yield "NaN only n=%d" % n, np.full(n, cval(np.nan, np.nan), np.complex64), -1
    zs = np.array([cval(-0.0, 0.0), cval(0.0, -0.0), cval(-0.0, -0.0), cval(0.0, 0.0)], np.complex64)
    c = np.resize(zs, n)
    yield "zeros of every sign n=%d" % n, c, -1
    c = c.copy()
    c[q] = cval(1e-30, 0)  # its power underflows to 0, the power a zero would have: only the skip tells them apart
    yield "zeros of every sign in front of a power of 0 n=%d" % n, c, fold(q, n)
    yield "all zeros n=%d" % n, np.zeros(n, np.complex64), -1


ONE = cval(1, 0)
QUARTER = cval(0, 1)  # against ONE: a phase of +pi/2; cval(0, -1): -pi/2


def census_pair(n, plus=(), minus=()):
    """a = b = (1, 0) everywhere (phase +0) but a = (0, 1) at `plus` and (0, -1) at `minus`."""
    a = np.full(n, ONE, np.complex64)
    b = a.copy()
    for p in plus:
        a[p] = QUARTER
    for p in minus:
        a[p] = cval(0, -1)
    return a, b


def cut_pair(n, negative_zero):
    """a = (1, 0), b = (-1, +0): the product is (-1, -0), every phase -pi.  b = (-1, -0): (-1, +0), +pi."""
    return np.full(n, ONE, np.complex64), np.full(n, cval(-1, -0.0 if negative_zero else 0.0), np.complex64)


def zero_pair(n):
    """a = (+-0, +-0) in its four sign combinations against b = (+-1, +-1) in its four: sixteen products of signed
    zeros, whose phases are +0, -0 and +pi: atan2 of two signed zeros."""
    za = np.array([cval(0.0, 0.0), cval(-0.0, 0.0), cval(0.0, -0.0), cval(-0.0, -0.0)], np.complex64)
    zb = np.array([cval(1, 1), cval(-1, 1), cval(1, -1), cval(-1, -1)], np.complex64)
    i = np.arange(n)
    return za[i % 4], zb[(i // 4) % 4]


def noise_pair(n):
    from util import rand_c64
    return rand_c64(1000 + n, n), rand_c64(2000 + n, n)


IMPULSE_VALUE = cval(0.75, -0.5)


def closure_inputs(n):
    """-> [(class, x, y, d or None)]: the time-domain pairs of one length.  y is an impulse IMPULSE_VALUE at d, or x
    delayed by d, where d is given."""
    from util import impulse, rand_c64
    x = rand_c64(3000 + n, n)
    out = [("noise", x, rand_c64(4000 + n, n), None)]
    for d in sorted({0, 1 % n, n // 2, n - 1}):
        out.append(("impulse", x, impulse(n, d, IMPULSE_VALUE), d))
    t = np.arange(n, dtype=np.float64)
    f = n // 3
    ang = 2.0 * np.pi * ((t * f) % n) / n
    tone = np.cos(ang) + 1j * np.sin(ang)
    out.append(("tone", tone.astype(np.complex64), (tone * (0.5 - 0.25j)).astype(np.complex64), None))
    burst = x.copy()
    burst[max(1, n // 4):] = 0
    d = n // 3
    out.append(("burst", burst, rotate(burst, d), d))
    return out


def closure_operand(kind, y):
    """What the closure of `kind` is given for y: the signal itself, or (freq) its float64 spectrum rounded once."""
    return fft_want64(y, True).astype(np.complex64) if kind == "freq" else np.ascontiguousarray(y, np.complex64)


def impulse_closure_want64(kind, x, d):
    """convolve / xcorr of x with an impulse IMPULSE_VALUE at d, analytically: x delayed by d times the value, or x
    advanced by d times its conjugate -- times n, the backward transform being unnormalised."""
    x = np.asarray(x).astype(np.complex128)
    v = complex(IMPULSE_VALUE) * len(x)
    return rotate(x, d) * v if kind == "convolve" else rotate(x, -d) * np.conj(v)


def closure_family(n):
    if n < 4:
        return "tiny"
    if n & (n - 1):
        return "bluestein"
    return "radix-4" if n < 256 else ("radix-16" if n <= 8192 else "two-step")


def _rand(seed, n):
    from util import rand_c64
    return rand_c64(seed, n)


def peak_cases(n):
    """Every buffer class of section P at length n -> (name, buffer, expected lag or None)."""
    for p in hot_positions(n):
        c = np.zeros(n, np.complex64)
        c[p] = cval(3, -4)
        yield "one-hot n=%d p=%d" % (n, p), c, fold(p, n)
    yield from tie_cases(n)
    if n >= 2:
        yield arithmetic_case(n)[:3]
    if n >= 8:
        yield from extreme_cases(n)
    yield "white noise n=%d" % n, _rand(50 + n, n), None


def mean_pairs(n):
    """Every pair class of section M at length n -> (name, a, b)."""
    for p in hot_positions(n):
        yield ("census n=%d p=%d" % (n, p),) + census_pair(n, plus=[p])
    yield ("cut -pi n=%d" % n,) + cut_pair(n, False)
    yield ("cut +pi n=%d" % n,) + cut_pair(n, True)
    yield ("zeros n=%d" % n,) + zero_pair(n)
    yield ("noise n=%d" % n,) + noise_pair(n)
    a, b = noise_pair(n)
    yield "noise, a is b n=%d" % n, a, a
    a = a.copy()
    a[n - 1] = cval(np.nan, 0)
    yield "NaN last n=%d" % n, a, b

"""tests/sync_ref.py, the checker of tests/test_gpu_sync.py, checked on the CPU.

1. The restatements equal the oracle (oracle/hzsdr_oracle.c, itself a restatement of rtl/kerberos/internal/align.go and
   fft/convolution.go) on every input class the GPU module uses: peak_lag exactly, mean_phase within the bound of
   sync_ref.mean_bound (the oracle sums in order), closure_want64 within the oracle's own float32 roundings.
2. The mean-phase bound pi (n + 16) 2^-53 holds, against math.fsum, for the oracle's sequential sum and for a numpy
   model of the kernel's summation order.  Measured here over n = 1, 257, 65536, 262145, 3 * 262144 + 77 and 2^20 + 3
   on white noise: the worst error / bound is printed (`pytest -s`) and was 1.2e-3 for the oracle and 0 for the
   kernel's order, whose sums are compensated (1.1e-7 for the same order summed plainly) -- the references alone are
   far inside: the bound is derived, not measured.
3. Ten models of a subtly wrong kernel, in numpy, each reported by the helper the GPU module calls.  The last one, a
   spectrum bin off by 1e-5 relative, is seen where the spectrum has few bins to hide behind: a tone pair at any length
   (ratios 40 ... 84 at 4096 points, 18 ... 45 at 1000) and white noise at short lengths (8 ... 20 at 64 points).  On white noise the error of ONE bin is a
   tone of 1e-5 / sqrt(n) of the output's level, below single precision itself from a few thousand points on; the test
   says so by asserting that the noise pair at 4096 points does not see it."""
import math

import numpy as np
import pytest

import sync_ref as R
from sync_ref import S
from util import FFT_K, fft_bin_errors, rand_c64

SMALL = [8, 255, 256, 257, 1000]  # every class at these; the classes that need a second trip at S + 1 and 2 S + 256 too


def orc_lag(orc, c):
    return orc.peak_lag(np.ascontiguousarray(c, np.complex64))


# ---- 1. the restatements equal the oracle ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3] + SMALL + [S + 1, 2 * S + 256])
def test_peak_lag_equals_the_oracle_and_the_written_out_scan(orc, n):
    count = 0
    for name, c, want in R.peak_cases(n):
        ref = R.peak_lag(c)
        assert ref == orc_lag(orc, c), name
        if want is not None:
            assert ref == want, name
        if n <= 1000:
            assert R.peak_lag_scan(c) == ref, name
        R.assert_peak(ref, c, orc, want, name)
        count += 1
    assert count >= 2
    assert R.peak_lag(np.zeros(0, np.complex64)) == -1


def test_float32_arithmetic_case_is_what_it_claims():
    p = R.powers(np.array([R.ARITH_A, R.ARITH_C]))
    assert p[0] == p[1] == 1 + 2.0 ** -11
    a = np.array([R.ARITH_A, R.ARITH_C]).view(np.float32).reshape(2, 2).astype(np.float64)
    f64 = a[:, 0] ** 2 + a[:, 1] ** 2  # exact: both squares fit a float64
    assert f64[0] > f64[1]
    assert np.float32(f64[0]) > np.float32(f64[1])  # a fused multiply-add rounds the exact sum once: A stays larger


@pytest.mark.parametrize("n", [1, 2, 3] + SMALL + [S + 1])
def test_mean_phase_equals_the_oracle_within_the_bound(orc, n):
    for name, a, b in R.mean_pairs(n):
        R.assert_mean(orc.mean_phase(a, b), a, b, name)
        R.assert_mean(R.kernel_order_mean(R.phases(a, b)), a, b, name)


def test_phases_of_the_planted_pairs():
    """What section M relies on: a = b = (1, 0) has phase +0 (not -0), the hot pair +-pi/2 to the bit, the two cuts
    -pi and +pi, and the sixteen products of signed zeros every one of +0, -0 and +pi (-pi would take a real and an
    imaginary part of -0 at once, which no product of a zero with a finite sample has; the cut pairs reach it)."""
    a, b = R.census_pair(4, plus=[1], minus=[2])
    ph = R.phases(a, b)
    assert ph.tolist() == [0.0, math.pi / 2, -math.pi / 2, 0.0] and not np.signbit(ph[[0, 3]]).any()
    assert (R.phases(*R.cut_pair(5, False)) == -math.pi).all()
    assert (R.phases(*R.cut_pair(5, True)) == math.pi).all()
    z = R.phases(*R.zero_pair(16))
    assert {(float(abs(v)), bool(np.signbit(v))) for v in z} == {(0.0, False), (0.0, True), (math.pi, False)}


@pytest.mark.parametrize("n", [1, 2, 3, 4, 8, 12, 64, 256, 1000, 4096, 4099])
def test_closure_want64_equals_the_oracle_within_its_float32_roundings(orc, n):
    """The oracle transforms in float64 and rounds three times on the way: each spectrum, the Go complex64 product,
    the output.  To first order that is a relative error of at most 3 * 2^-24 on every bin of the product and one more
    2^-24 on every output sample: |err_t| <= 3 * 2^-24 * sum_k |P_k| + 2^-24 |want_t|, and 4 * 2^-24 in relative L2
    (asserted with 1 % for the second-order terms).  4096 is the power of two that pins the closures' scaling (n times the circular convolution)."""
    u = 2.0 ** -24
    for cls, x, y, d in R.closure_inputs(n):
        for kind in R.KINDS:
            yk = R.closure_operand(kind, y)
            want = R.closure_want64(kind, x, yk)
            got = np.zeros(n, np.complex64)
            rc = orc.convolve_freq(got, x, yk) if kind == "freq" else orc.convolve(got, x, yk, conj=(kind == "xcorr"))
            assert rc == 0
            X = np.fft.fft(x.astype(np.complex128))
            Y = yk.astype(np.complex128) if kind == "freq" else np.fft.fft(yk.astype(np.complex128))
            err = np.abs(got.astype(np.complex128) - want)
            assert (err <= 1.01 * (3 * u * np.abs(X * Y).sum() + u * np.abs(want))).all(), (n, cls, kind, err.max())
            assert fft_bin_errors(got, want)[1] <= 1.01 * 4 * u, (n, cls, kind)
            if cls == "impulse" and kind != "freq":
                assert np.abs(want - R.impulse_closure_want64(kind, x, d)).max() <= 1e-12 * max(1, n), (n, kind, d)


@pytest.mark.parametrize("n", [4, 8, 12, 255, 256, 1000, 4096, 4099])
def test_lag_of_a_delayed_copy(orc, n):
    """The sign convention and the fold, on the float64 correlation and on the oracle's."""
    a = rand_c64(60 + n, n)
    for d in (0, 1, -1, n // 2, n // 2 + 1, -(n // 2)):
        b = R.rotate(a, d)
        want = R.closure_want64("xcorr", a, b)
        got = np.zeros(n, np.complex64)
        orc.convolve(got, a, b, conj=True)
        R.assert_lag(orc_lag(orc, got), want, n, d, (n, d))


@pytest.mark.parametrize("n", [1, 2, 3, 4, 64, 1000, 4096])
def test_closure_yardstick_passes_at_k_1_and_stays_single(n):
    for cls, x, y, d in R.closure_inputs(n):
        for kind in R.KINDS:
            yk = R.closure_operand(kind, y)
            g = R.closure_yardstick(kind, x, yk)
            assert g.dtype == np.complex64
            R.assert_closure(g, kind, x, yk, (n, cls, kind), k=1.0)
            assert fft_bin_errors(g, R.closure_want64(kind, x, yk))[1] <= 2e-6, (n, cls, kind)


# ---- 2. the mean-phase bound ------------------------------------------------------------------------------------------

def test_mean_phase_bound_holds_for_both_summation_orders(orc):
    worst = {"oracle": 0.0, "kernel order": 0.0}
    for n in (1, 257, 65536, 262145, 3 * 262144 + 77, (1 << 20) + 3):
        a, b = R.noise_pair(n)
        ph = R.phases(a, b)
        exact = math.fsum(ph.tolist()) / n
        for who, got in (("oracle", orc.mean_phase(a, b)), ("kernel order", R.kernel_order_mean(ph))):
            worst[who] = max(worst[who], R.assert_mean(got, a, b, (who, n), exact=exact))
    print("mean phase, worst error / bound: oracle %.2e, kernel order %.2e" % (worst["oracle"], worst["kernel order"]))
    assert max(worst.values()) <= 1.0


def test_branch_cut_mean_in_the_kernels_order():
    """262145 phases of -pi: the kernel's compensated sums give -pi to 2^-49 (the GPU module's check); the plain sums
    it made before, in the same order, ended 8.5 * 2^-49 away, the 1024 workgroup sums rounding one after another."""
    for negative_zero, want in ((False, -math.pi), (True, math.pi)):
        for n in (257, S + 1):
            ph = R.phases(*R.cut_pair(n, negative_zero))
            assert abs(R.kernel_order_mean(ph) - want) <= 2.0 ** -49, (n, want)
    assert abs(R.kernel_order_mean(ph, compensated=False) - math.pi) * 2.0 ** 49 == 8.5


def test_kernel_order_model_is_a_sum():
    """On integers every order is exact: the model drops and doubles nothing at each grid shape."""
    for n in (1, 255, 256, 257, 1000, S - 1, S, S + 1, 2 * S + 256, 3 * S + 77):
        v = np.arange(n, dtype=np.float64) % 1000.0
        assert R.kernel_order_mean(v) == float(v.sum()) / n


# ---- 3. mutants -------------------------------------------------------------------------------------------------------

def _bits_zero(re, im):
    return not (np.signbit(re) or np.signbit(im)) and re == 0 and im == 0


def _power64(c):
    v = np.ascontiguousarray(c, np.complex64).view(np.float32).reshape(-1, 2).astype(np.float64)
    return v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]


def _power_fused(c):
    with np.errstate(over="ignore"):
        return _power64(c).astype(np.float32).astype(np.float64)  # the exact sum (it fits a float64 here) rounded once


PEAK_MUTANTS = {
    ">=": dict(wins=lambda p, best: p >= best),
    "(-0, +0) not skipped": dict(skipped=_bits_zero),
    "float64 power": dict(power=_power64),
    "fused power": dict(power=_power_fused),
    "fold at >= n/2": dict(folds=lambda i, n: i >= n / 2),
}


@pytest.mark.parametrize("mutant", sorted(PEAK_MUTANTS))
def test_peak_mutants_fail(orc, mutant):
    n = 1000
    caught = []
    for name, c, want in R.peak_cases(n):
        got = R.peak_lag_scan(c, **PEAK_MUTANTS[mutant])
        try:
            R.assert_peak(got, c, orc, want, name)
        except AssertionError:
            caught.append(name)
    print("%s: caught by %d cases, the first: %s" % (mutant, len(caught), caught[:1]))
    assert caught, mutant
    kinds = {">=": "tie", "(-0, +0) not skipped": "zeros of every sign", "float64 power": "float32 arithmetic",
             "fused power": "float32 arithmetic", "fold at >= n/2": "one-hot n=1000 p=500"}
    assert any(c.startswith(kinds[mutant]) for c in caught), (mutant, caught)


def _mean_drop_last(a, b):
    ph = R.phases(a, b)
    return R.kernel_order_mean(ph[:-1]) * (len(ph) - 1) / len(ph)


def _mean_double(a, b):
    ph = R.phases(a, b)
    return (R.kernel_order_mean(ph) * len(ph) + ph[S]) / len(ph)


def _mean_conj_a(a, b):
    return R.kernel_order_mean(R.phases(np.conj(a), np.conj(b)))  # conj(a) * b


MEAN_MUTANTS = {"drops the last element": _mean_drop_last, "counts element 262144 twice": _mean_double,
                "conjugates a": _mean_conj_a}


@pytest.mark.parametrize("mutant", sorted(MEAN_MUTANTS))
def test_mean_mutants_fail(mutant):
    n = S + 1
    f = MEAN_MUTANTS[mutant]
    # the census: one hot pair at the last element, which is element 262144, the first of a second trip
    a, b = R.census_pair(n, plus=[n - 1])
    R.assert_census(R.kernel_order_mean(R.phases(a, b)), n, math.pi / 2)
    with pytest.raises(AssertionError):
        R.assert_census(f(a, b), n, math.pi / 2, mutant)
    # random data against the bound
    a, b = R.noise_pair(n)
    R.assert_mean(R.kernel_order_mean(R.phases(a, b)), a, b)
    with pytest.raises(AssertionError):
        R.assert_mean(f(a, b), a, b, mutant)
    # the smallest structural error, one element of the smallest phase the census uses, is far outside the bound
    assert (math.pi / 2) / n > 1e4 * R.mean_bound(n)


@pytest.mark.parametrize("n", [64, 1000, 4096, 4099])
def test_cross_correlation_conjugating_the_other_operand_fails(n):
    for cls, x, y, d in R.closure_inputs(n):
        # (even the tone pair on ONE bin: conj(X) Y and X conj(Y) differ by the sign of the pair's relative phase)
        X, Y = np.fft.fft(x.astype(np.complex128)), np.fft.fft(y.astype(np.complex128))
        wrong = (np.fft.ifft(np.conj(X) * Y) * n).astype(np.complex64)
        with pytest.raises(AssertionError):
            R.assert_closure(wrong, "xcorr", x, y, (n, cls))
    a = rand_c64(70 + n, n)
    b = R.rotate(a, 5)
    wrong = (np.fft.ifft(np.conj(np.fft.fft(a.astype(np.complex128))) * np.fft.fft(b.astype(np.complex128))) * n).astype(np.complex64)
    with pytest.raises(AssertionError):
        R.assert_lag(R.peak_lag(wrong), R.closure_want64("xcorr", a, b), n, 5)


@pytest.mark.parametrize("kind", R.KINDS)
def test_one_spectrum_bin_off_by_1e_5_fails(kind):
    seen = {}
    for n, cls in ((4096, "tone"), (1000, "tone"), (64, "noise"), (4096, "noise")):
        _, x, y, _ = [c for c in R.closure_inputs(n) if c[0] == cls][0]
        yk = R.closure_operand(kind, y)
        k = n // 3  # the tone's bin
        got = R.closure_yardstick(kind, x, yk, spoil=(k, 1 + 1e-5))
        ratio = R.closure_ratios(got, kind, x, yk)[2]
        seen[(n, cls)] = ratio
        if (n, cls) == (4096, "noise"):
            continue
        assert max(ratio) > 8.0, (n, cls, "not seen even by the largest factor a family may get", ratio)
        with pytest.raises(AssertionError):
            R.assert_closure(got, kind, x, yk, (n, cls), k=FFT_K)
    print(kind, "ratios (max_sample, rel_l2) of a bin off by 1e-5:", {k: "%.1f %.1f" % v for k, v in seen.items()})
    assert max(seen[(4096, "noise")]) < FFT_K  # (the docstring's caveat, kept true)

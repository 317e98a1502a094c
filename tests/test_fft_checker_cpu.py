"""The per-bin FFT checker of tests/util.py, tested on the CPU: what K = 4 lets pass and what it catches.

An independent textbook float32 transform (iterative radix-2, decimation in time, written here in numpy: complex64
products and sums, one rounding each) stands in for an honest single-precision kernel.  Its twiddles come either from
one table rounded from float64 (`plain`) or, as in the kernels' big_twiddle (csrc/hz_fft.hip), as the complex64 PRODUCT
of two rounded table entries, W^m = hi[m >> s] * lo[m & (2^s - 1)] (`split`).  Both must pass the assertion of
util.assert_fft_close at K = 4 on every input class of util.fft_inputs; the split form with ONE entry of `lo` multiplied
by 1 + 1e-5i must fail it on every impulse position and on random input -- a defect whose relative L2 error (2.8e-7 ...
1.3e-6) the suite's older bound 3e-7 log2 N + 1e-7 lets through at every size.

Measured here (ratios to max(yardstick, 2^-23), N = 2^12 and 2^16, forward and backward; printed by the tests):
    honest transform, plain and split, over all classes:  max_bin <= 1.7, rel_l2 <= 1.5
    float32 Bluestein over the honest transform (n = 1000, 4099), against the yardstick's Bluestein over scipy:
                                                          max_bin <= 1.6, rel_l2 <= 1.5
    one perturbed entry:                                  max_bin 23 ... 44 on impulses and on random input
DC and the alternating sequence are transformed exactly by every radix-2 / radix-4 transform (all intermediate values
are small multiples of the input), so they separate nothing by value: they stay in the GPU module as a check of
placement (bin 0 / bin N/2 only, every other bin exactly zero) under the same assertion, which the floor makes 4.8e-7
of the peak."""
import numpy as np
import pytest

from util import (FFT_FLOOR, FFT_K, assert_fft_close, bluestein_f32, fft_bin_errors, fft_inputs, fft_ratios, fft_want64,
                  fft_yardstick, impulse, impulse_want64)

SIZES = [1 << 12, 1 << 16]


def _tables(n, split, perturb):
    """-> W[m], m < N/2, as complex64: rounded from float64, or the product of two rounded entries."""
    m = np.arange(n // 2, dtype=np.int64)
    if not split:
        ang = -2.0 * np.pi * m / n
        return (np.cos(ang) + 1j * np.sin(ang)).astype(np.complex64)
    L = n.bit_length() - 1
    s = L // 2
    a = np.arange(1 << (L - s), dtype=np.int64)
    b = np.arange(1 << s, dtype=np.int64)
    hi = np.exp(-2j * np.pi * (a << s) / n).astype(np.complex64)
    lo = np.exp(-2j * np.pi * b / n).astype(np.complex64)
    if perturb:
        lo[5] = lo[5] * np.complex64(1 + 1e-5j)
    return hi[m >> s] * lo[m & ((1 << s) - 1)]


def textbook_fft32(x, forward=True, split=False, perturb=False):
    """Radix-2 decimation in time in complex64; backward unnormalised."""
    x = np.asarray(x, np.complex64)
    n = len(x)
    L = n.bit_length() - 1
    assert n == 1 << L
    w = _tables(n, split, perturb)
    if not forward:
        w = np.conj(w)
    idx = np.arange(n)
    rev = np.zeros(n, np.int64)
    for bit in range(L):
        rev |= ((idx >> bit) & 1) << (L - 1 - bit)
    y = x[rev].copy()
    half = 1
    while half < n:
        y = y.reshape(-1, 2, half)
        t = y[:, 1, :] * w[::n // (2 * half)][None, :]
        y = np.stack([y[:, 0, :] + t, y[:, 0, :] - t], axis=1).astype(np.complex64)
        half *= 2
    return y.reshape(n)


def _want(x, wf, wb, forward):
    w = wf if forward else wb
    return fft_want64(x, forward) if w is None else w


def test_textbook_transform_is_a_transform():
    x = fft_inputs(64)[0][1]
    for split in (False, True):
        for fwd in (True, False):
            assert fft_bin_errors(textbook_fft32(x, fwd, split), fft_want64(x, fwd))[1] < 1e-6


@pytest.mark.parametrize("n", [4, 12, 1000, 4096, 4099, 100_003, (1 << 20) + 7])
def test_analytic_impulse_equals_numpy(n):
    for p in (0, 1, n - 1, n // 2 + 1, (n // 3) | 1):
        for fwd in (True, False):
            x = impulse(n, p)
            assert np.abs(impulse_want64(n, p, forward=fwd) - fft_want64(x, fwd)).max() <= 1e-12, (n, p, fwd)


@pytest.mark.parametrize("n", SIZES + [1000, 4099])
def test_yardstick_passes_at_k_1_and_stays_single(n):
    """By construction (ratio <= 1), and its own values stay where they were measured: max_bin <= 1.1e-6 and
    rel_l2 <= 3.3e-7 (powers of two: 4.9e-7 and 1.8e-7), so that a changed scipy is noticed."""
    pow2 = n & (n - 1) == 0
    for name, x, wf, wb in fft_inputs(n):
        for fwd in (True, False):
            w = _want(x, wf, wb, fwd)
            y = fft_yardstick(x, fwd)
            assert y.dtype == np.complex64
            assert_fft_close(y, x, w, fwd, (n, name, fwd), k=1.0)
            mb, l2 = fft_bin_errors(y, w)
            assert mb <= (4.9e-7 if pow2 else 1.1e-6) and l2 <= (1.8e-7 if pow2 else 3.3e-7), (n, name, fwd, mb, l2)


@pytest.mark.parametrize("split", [False, True], ids=["plain", "split"])
@pytest.mark.parametrize("n", SIZES)
def test_honest_float32_transform_passes_at_k_4(n, split):
    worst = [0.0, 0.0]
    for name, x, wf, wb in fft_inputs(n):
        for fwd in (True, False):
            r = assert_fft_close(textbook_fft32(x, fwd, split), x, _want(x, wf, wb, fwd), fwd, (n, name, fwd, split))
            worst = [max(a, b) for a, b in zip(worst, r)]
    print("honest n=%d split=%s: worst ratios max_bin %.2f rel_l2 %.2f" % (n, split, worst[0], worst[1]))


@pytest.mark.parametrize("n", [1000, 4099])
def test_honest_float32_bluestein_passes_at_k_4(n):
    """The chirp transform over the textbook transform against the yardstick's chirp transform over scipy."""
    worst = [0.0, 0.0]
    for name, x, wf, wb in fft_inputs(n):
        for fwd in (True, False):
            got = bluestein_f32(x, fwd, lambda a: textbook_fft32(a, True, True),
                                lambda a: textbook_fft32(a, False, True) / np.float32(len(a)))
            r = assert_fft_close(got, x, _want(x, wf, wb, fwd), fwd, (n, name, fwd))
            worst = [max(a, b) for a, b in zip(worst, r)]
    print("honest bluestein n=%d: worst ratios max_bin %.2f rel_l2 %.2f" % (n, worst[0], worst[1]))


@pytest.mark.parametrize("n", SIZES)
def test_one_perturbed_table_entry_fails_on_impulses_and_random(n):
    seen = []
    for name, x, wf, wb in fft_inputs(n):
        if not (name == "random" or name.startswith("impulse")):
            continue
        for fwd in (True, False):
            w = _want(x, wf, wb, fwd)
            got = textbook_fft32(x, fwd, True, perturb=True)
            mine, yard, ratio = fft_ratios(got, x, w, fwd)
            seen.append((name, fwd, ratio))
            assert ratio[0] > FFT_K, (n, name, fwd, "max_bin does not see the perturbed entry", mine, yard)
            assert ratio[0] > 8.0, (n, name, fwd, "nor would the largest factor a kernel family may get", ratio)
            with pytest.raises(AssertionError):
                assert_fft_close(got, x, w, fwd, (n, name, fwd))
            # ... and the older bound lets it through
            assert mine[1] < 3e-7 * np.log2(n) + 1e-7
    print("perturbed n=%d: max_bin ratios %.1f ... %.1f" % (n, min(r[2][0] for r in seen), max(r[2][0] for r in seen)))


def test_floor_is_one_float32_ulp():
    assert FFT_FLOOR == np.finfo(np.float32).eps

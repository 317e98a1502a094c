"""The per-bin bar of tests/spectrum_ref.py, tested on the CPU: what it lets pass and what it catches.

An honest float32 spectrum stands in for the kernels: the frames as the kernel forms them, the textbook radix-2
transform of tests/test_fft_checker_cpu.py with the kernels' split twiddle form, float32 re*re + im*im (three roundings),
float32 sums in frame order and a float32 scale.  It must lie under the bar on every input class (white, comb, tones,
tone_off_bin) at N in {256, 2048, 8192}, avg in {1, 5}, with a rectangular and with the asymmetric window, from c64 and
from u8 samples.

Measured here (worst |got - want| / bound over every bin; printed by the tests):
    honest spectrum     white 0.33 ... 0.37   comb 0.29 ... 0.31   tones 0.20 ... 0.30   tone_off_bin 0.19 ... 0.26
    pinned: <= 0.5 on every class and size, as a trial with fewer cases suggested (0.17 ... 0.28) and this run of every
    class, size, avg, window and two source formats supports: the largest seen is 0.37
    planted errors (ratio to the bar | what the older row-L1 bound of tests/test_gpu_spectrum.py says):
      two adjacent bins swapped, comb     N = 2048: 230     N = 8192: 46         | passes (6.2e-7 of 7.1e-6, 2.0e-7 of 8.3e-6)
      one window entry x 1.001, white     N = 8192, avg = 5: 5.8                 | passes (6.2e-6 of 8.5e-6)
      a frame one sample late, white      3.5e3 ... 4.3e4                        | fails
      a row's last frame in the next row  4.7e5 ... 9.2e5                        | fails
      one bin of one frame x (1 + 1e-4)   comb, N = 2048 / 8192: 28 ... 31 (avg = 1), 5.3 ... 5.8 (avg = 5)
                                                                                 | passes (1.7e-7 ... 2.3e-7)
      NegativeFirst rotated by one bin    comb: 5.9e5 and more                   | fails (1.3e-3, 3.1e-4)
(the figures are printed again by every run; the assertions are "over the bar" for each, and "the older bound passes"
for the first two and for the single bin.)

The exact impulse streams of the GPU module's bit-for-bit tests are checked here too: every prefix of every row's
float64 sum is a float32 value, for every avg those tests use."""
import numpy as np
import pytest

import spectrum_ref as sr
from test_fft_checker_cpu import textbook_fft32

SIZES = [256, 2048, 8192]
AVGS = [1, 5]


def honest_rows(c, n, hop, avg, w, scale, frame_shift=0, w_used=None, bump=None):
    """the honest float32 spectrum of the converted stream c, ZeroFirst (rows, n) float32.  Planted errors: frames taken
    `frame_shift` samples late (frame 1 only), another window in use, (frame, bin, factor) on one frame's power."""
    F, rows = sr.counts(c.shape[0] - (1 if frame_shift else 0), n, hop, avg)
    f = sr.frames32(c, n, hop, w if w_used is None else w_used, rows * avg)
    if frame_shift:
        f[1] = sr.frames32(c[frame_shift:], n, hop, w, 2)[1]
    p = np.empty((rows * avg, n), np.float32)
    for j in range(rows * avg):
        X = textbook_fft32(f[j], True, split=True)
        re, im = X.real.astype(np.float32), X.imag.astype(np.float32)
        p[j] = re * re + im * im
    if bump is not None:
        p[bump[0], bump[1]] *= np.float32(bump[2])
    return sum_rows(p, avg, scale)


def sum_rows(p, avg, scale):
    rows = p.shape[0] // avg
    p = p.reshape(rows, avg, -1)
    acc = np.zeros((rows, p.shape[2]), np.float32)
    for t in range(avg):
        acc = acc + p[:, t]
    return np.float32(scale) * acc


def stream_len(n, hop, avg):
    frames = max(8, 2 * avg) // avg * avg  # every tone of the `tones` class once
    return (frames - 1) * hop + n + 1


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("cls", sr.CLASSES)
def test_honest_spectrum_is_under_the_bar(orc, cls, n):
    worst = 0.0
    for fmt in ("c64", "u8"):
        for avg in AVGS:
            for w in (None, sr.asym_window(n)):
                hop = n if cls == "tones" or w is None else n // 2
                x, c = sr.class_input(orc, cls, fmt, n, stream_len(n, hop, avg), seed=n + avg)
                scale = 1.0 / (avg * n)
                want, bound = sr.spectrum_bar(c, n, hop, avg, w, scale)
                assert want.shape[0] >= 2
                got = honest_rows(c, n, hop, avg, w, scale)
                worst = max(worst, sr.check_bar(got, want, bound, (cls, fmt, n, avg, w is not None)))
                nf = sr.check_bar(sr.negative_first(got), sr.negative_first(want), sr.negative_first(bound), "NegativeFirst")
                assert nf <= worst
    print("honest %-12s n=%d: worst ratio %.2f" % (cls, n, worst))
    assert worst <= 0.5, "an honest float32 spectrum uses more than half of the bar"


def test_tones_are_where_they_should_be(orc):
    """the tones class puts frame j's power into bin tone_bins[j mod 8]"""
    n = 256
    x, c = sr.class_input(orc, "tones", "c64", n, 8 * n, seed=1)
    want, _ = sr.spectrum_bar(c, n, n, 1, None, 1.0)
    assert list(want.argmax(axis=1)) == sr.tone_bins(n)
    assert (np.sort(want, axis=1)[:, -2] < 1e-9 * want.max(axis=1)).all()


def test_comb_bins_differ_by_2_over_n():
    n = 2048
    P = np.abs(np.fft.fft(sr.comb_period(n, 3))) ** 2
    P = P / P[0]
    assert (np.diff(P) >= 2.0 / n * 0.999).all()


def _over(got, want, bound):
    r = sr.bar_ratio(got, want, bound)
    assert not np.isnan(r).any()
    return float(r.max())


@pytest.mark.parametrize("n", [2048, 8192])
def test_swapped_bins_fail_on_the_comb(orc, n):
    avg, hop = 1, n
    x, c = sr.class_input(orc, "comb", "c64", n, 2 * n + 1, seed=n)
    scale = 1.0 / n
    want, bound = sr.spectrum_bar(c, n, hop, avg, None, scale)
    got = honest_rows(c, n, hop, avg, None, scale)
    k = n // 16 + 3  # (the second register slot of lane 3, and lane 4's first: a wrong lane + q * TPT)
    got[1, [k, k + 1]] = got[1, [k + 1, k]]
    ratio, l1 = _over(got, want, bound), sr.row_l1(got, want).max()
    print("swapped bins n=%d: ratio %.1f, row L1 %.2e of %.2e" % (n, ratio, l1, sr.row_l1_bound(n, avg)))
    assert ratio > 1.0
    with pytest.raises(AssertionError, match="row 1 bin %d" % k):
        sr.check_bar(got, want, bound)
    assert l1 <= sr.row_l1_bound(n, avg), "the older bound sees it after all"


def test_one_window_entry_off_fails_on_white(orc):
    n, avg, hop = 8192, 5, 8192
    x, c = sr.class_input(orc, "white", "c64", n, 2 * avg * hop, seed=9)
    w = sr.asym_window(n)
    scale = 1.0 / (avg * n)
    want, bound = sr.spectrum_bar(c, n, hop, avg, w, scale)
    off = w.copy()
    off[n // 2 + 3] *= np.float32(1.001)
    got = honest_rows(c, n, hop, avg, w, scale, w_used=off)
    ratio, l1 = _over(got, want, bound), sr.row_l1(got, want).max()
    print("window entry x 1.001: ratio %.1f, row L1 %.2e of %.2e" % (ratio, l1, sr.row_l1_bound(n, avg)))
    assert ratio > 1.0
    assert l1 <= sr.row_l1_bound(n, avg), "the older bound sees it after all"


@pytest.mark.parametrize("n", SIZES)
def test_late_frame_and_misplaced_frame_fail(orc, n):
    avg, hop = 5, n + 37
    x, c = sr.class_input(orc, "white", "i16", n, 2 * avg * hop + n, seed=n)
    scale = 1.0 / (avg * n)
    want, bound = sr.spectrum_bar(c, n, hop, avg, None, scale)
    late = honest_rows(c, n, hop, avg, None, scale, frame_shift=1)
    ratio = _over(late, want, bound)
    print("late frame n=%d: ratio %.3g, row L1 %.2e of %.2e" % (n, ratio, sr.row_l1(late, want).max(), sr.row_l1_bound(n, avg)))
    assert ratio > 1.0
    # row 0's last frame summed into row 1
    f = sr.frames32(c, n, hop, None, 2 * avg)
    p = np.stack([np.abs(textbook_fft32(v, True, split=True)).astype(np.float32) ** 2 for v in f])
    moved = np.float32(scale) * np.stack([p[:avg - 1].sum(axis=0), p[avg - 1:].sum(axis=0)])
    ratio = _over(moved, want, bound)
    print("misplaced frame n=%d: ratio %.3g, row L1 %.2e" % (n, ratio, sr.row_l1(moved, want).max()))
    assert ratio > 1.0


@pytest.mark.parametrize("n,avg", [(2048, 1), (2048, 5), (8192, 1), (8192, 5)])
def test_one_bin_of_one_frame_off_fails_on_the_comb(orc, n, avg):
    hop = n
    x, c = sr.class_input(orc, "comb", "c64", n, 2 * avg * hop, seed=n + 1)
    scale = 1.0 / (avg * n)
    want, bound = sr.spectrum_bar(c, n, hop, avg, None, scale)
    got = honest_rows(c, n, hop, avg, None, scale, bump=(avg, n // 2 + 5, 1.0 + 1e-4))
    ratio, l1 = _over(got, want, bound), sr.row_l1(got, want).max()
    print("one bin x (1 + 1e-4) n=%d avg=%d: ratio %.1f, row L1 %.2e of %.2e" % (n, avg, ratio, l1, sr.row_l1_bound(n, avg)))
    assert ratio > 1.0
    with pytest.raises(AssertionError, match="row 1 bin %d" % (n // 2 + 5)):
        sr.check_bar(got, want, bound)
    assert l1 <= sr.row_l1_bound(n, avg), "the older bound sees it after all"


@pytest.mark.parametrize("n", [2048, 8192])
def test_negative_first_rotated_fails_on_the_comb(orc, n):
    x, c = sr.class_input(orc, "comb", "c64", n, 2 * n, seed=n + 2)
    want, bound = sr.spectrum_bar(c, n, n, 1, None, 1.0 / n)
    got = sr.negative_first(honest_rows(c, n, n, 1, None, 1.0 / n))
    wn, bn = sr.negative_first(want), sr.negative_first(bound)
    assert _over(got, wn, bn) <= 0.5
    rot = np.roll(got, 1, axis=1)
    ratio = _over(rot, wn, bn)
    print("NegativeFirst rotated n=%d: ratio %.1f, row L1 %.2e of %.2e" % (n, ratio, sr.row_l1(rot, wn).max(), sr.row_l1_bound(n, 1)))
    assert ratio > 1.0


def test_a_nan_fails():
    want, bound = np.ones((2, 4)), np.ones((2, 4))
    got = np.ones((2, 4), np.float32)
    assert sr.check_bar(got, want, bound) == 0.0
    got[1, 2] = np.nan
    with pytest.raises(AssertionError, match="row 1 bin 2"):
        sr.check_bar(got, want, bound)


# ---- the exact impulse streams ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", sr.EXACT_FORMATS)
def test_exact_streams_have_exact_prefix_sums(fmt):
    for avg in (1, 2, 3, 7, 16, 1024 + 5, 32768 + 5):
        m = sr.exact_period(fmt, avg)
        assert m >= (3 if avg > 4096 else 5)
        raw, p = sr.impulse_stream(fmt, 4, 4, np.zeros(3 * avg + 1, np.int64), m)
        assert sr.prefix_sums_exact(p, avg), (fmt, avg, m)
        for w2 in (1.0, 0.25):
            rows = sr.exact_rows(p, avg, w2, 0.125)
            assert rows.shape == ((3 * avg + 1) // avg,) and (rows.astype(np.float32).astype(np.float64) == rows).all()
    # ... and the condition is not empty: all of c64's amplitudes over a long row are not exact
    _, p = sr.impulse_stream("c64", 4, 4, np.zeros(40000, np.int64), 8)
    assert not sr.prefix_sums_exact(p, 40000)


def test_impulse_stream_layout_and_conversion(orc):
    for fmt in sr.EXACT_FORMATS:
        pos = np.array([0, 5, 15, 7])
        raw, p = sr.impulse_stream(fmt, 16, 21, pos, 4, tail=3)
        c = sr.converted(orc, raw)
        assert c.shape[0] == 3 * 21 + 16 + 3
        at = np.flatnonzero(c)
        assert list(at) == [0, 26, 57, 70]
        got = c[at].real.astype(np.float64) ** 2 + c[at].imag.astype(np.float64) ** 2
        assert (got == p).all()


def test_pending_after_restates_the_walkthrough():
    assert sr.pending_after(200, 256, 300, 4) == (0, 200)
    assert sr.pending_after(260, 256, 300, 4) == (1, 0)
    assert sr.pending_after(301, 256, 300, 4) == (1, 1)
    assert sr.pending_after(256 + 128, 256, 128, 2) == (0, 128)


def test_slot_positions():
    for n in (256, 2048):
        assert (sr.slot_positions(n) == np.arange(n)).all()
    for n in (4096, 8192):
        p = sr.slot_positions(n)
        t = n // 16
        assert p.shape[0] == 2048 == np.unique(p).shape[0]
        assert set(range(64)) <= set(p) and set(range(n - 64, n)) <= set(p)
        for q in range(16):
            assert {int(v) % 64 for v in p if v // t == q} == set(range(64))

"""tests/conv_ref.py on the CPU: the dispatch restatement reaches all six forms with the shapes the GPU tests run, the
float64 reference is the oracle's ConvolutionReader (+ DecimateReader) within float32 rounding, an honest float32
convolution passes the per-block bar at K = 4 on every input class, and every model of a subtly wrong kernel fails it.

Also pinned: why the older tests could not see a wrong filter bin.  With the suite's low-pass filter and white input,
two stop-band bins swapped move a block by less than 1e-7 relative L2 (the older bar: 2e-6); with an all-pass filter
the same swap moves it by more than 1e-2.  And why the tone class exists: one filter bin, or one bin of the spectrum,
off by 1e-5 passes on white input at n = 8192 and fails on a tone that sits on the bin."""
import numpy as np
import pytest

import conv_ref as cr
from test_fft_checker_cpu import textbook_fft32
from test_gpu_fft_plans import _lowpass_bins
from util import FFT_K, rand_c64, zeros


def test_form_maps_the_gpu_shapes_onto_all_six_forms():
    for f, shapes in cr.SHAPES.items():
        for n, fmt, stages, dec in shapes:
            assert cr.form(n, fmt, stages, dec) == f, (n, fmt, stages, dec)
    assert set(cr.SHAPES) == set(cr.FORMS)
    four = [s[0] for s in cr.SHAPES[4]]
    assert any(2048 <= n <= 8192 for n in four) and any(256 <= n <= 1024 for n in four)
    # a c64 source in front of a decimated convolution below 256 stays the direct kernel
    assert cr.form(64, "c64", 0, 8) == 1 and cr.form(64, "c64", 1, 8) == 2


def test_blocks_per_trip_and_workgroup_sizes():
    cus = 256
    assert [cr.xpb(1, n) for n in (4, 8, 16, 32, 64, 128)] == [64, 32, 16, 8, 4, 2]
    assert [cr.xpb(5, n) for n in (256, 512, 1024, 2048, 8192)] == [4, 2, 1, 1, 1]
    assert [cr.xpw(n) for n in (256, 512, 1024)] == [4, 2, 1]
    assert [cr.blocks_per_trip(3, n, cus) for n in (256, 512, 1024)] == [cus * 64, cus * 32, cus * 16]
    assert [cr.blocks_per_trip(4, n, cus) for n in (256, 512, 1024, 2048, 4096, 8192)] == [cus * 64, cus * 32, cus * 16, cus * 8, cus * 4, cus]
    assert cr.blocks_per_trip(5, 4096, cus) is None
    assert cr.unit(1000, 8) == 4_096_000 and cr.unit(65536, 3) == 65536 and cr.unit(512, 10) == 32768 and cr.unit(512, 1) == 512


def oracle_blocks(orc, xc, H, n, dec):
    cons = cr.whole(len(xc), n, dec)
    conv = zeros("c64", cons)
    assert orc.convolution_reader(conv, np.ascontiguousarray(xc[:cons]), H) == cons
    if dec <= 1:
        return conv
    per = cr.READER // dec
    out = zeros("c64", cons // cr.READER * per)
    for r in range(cons // cr.READER):
        assert orc.decimate(out[r * per:(r + 1) * per], conv[r * cr.READER:(r + 1) * cr.READER], dec) == per
    return out


@pytest.mark.parametrize("n", [8, 256, 1000])
@pytest.mark.parametrize("dec", [1, 8, 10])
def test_want64_is_the_oracles_reader_chain(orc, n, dec):
    """The oracle is itself a float32 convolution: it has to pass the bar it is the reference of (K = 4), every block,
    and its layout behind the pick (whole lcm(n, 32 Ki) units, per = 32768 // dec outputs per reader block) has to be
    want64's.  A ragged rest is dropped by both.  At 1000 bins a decimated call's unit is 4096 blocks, a quarter of a
    minute of the oracle's transform: there the two readers are held to want64 one after the other -- the oracle's
    ConvolutionReader by the dec = 1 case, and here the oracle's DecimateReader over want64's own undecimated stream,
    which has to pick exactly the samples want64 picks."""
    if n == 1000 and dec > 1:
        count = cr.unit(n, dec) + n + n // 2
        xc = rand_c64(n + dec, count)
        H = cr.graded(n, 5)
        full = cr.want64(xc, H, n).astype(np.complex64).reshape(-1)
        per, blocks = cr.READER // dec, cr.unit(n, dec) // cr.READER
        out = zeros("c64", blocks * per)
        for r in range(blocks):
            assert orc.decimate(out[r * per:(r + 1) * per], full[r * cr.READER:(r + 1) * cr.READER], dec) == per
        assert np.array_equal(out.reshape(blocks, per), cr.want64(xc, H, n, dec).astype(np.complex64))
        return
    count = cr.unit(n, dec) * 2 + n + n // 2
    xc = rand_c64(n + dec, count)
    H = cr.graded(n, 5)
    got = oracle_blocks(orc, xc, H, n, dec)
    w = cr.want64(xc, H, n, dec)
    assert w.size == got.size and w.shape[1] == (n if dec == 1 else cr.READER // dec)
    cr.assert_conv_blocks(got, xc, H, n, dec, what="oracle n=%d dec=%d" % (n, dec))


@pytest.mark.parametrize("n", [12, 64, 1000, 4096])
def test_analytic_impulse_want_equals_the_numeric_one(n):
    for fmt in ("c64", "i8", "i16"):
        nblk = 40
        raw, conv, pos, amps = cr.impulses(fmt, nblk, n)
        H = cr.allpass(n, 3)
        a, b = cr.impulse_want64(H, n, pos, amps), cr.want64(conv, H, n)
        assert np.abs(a - b).max() <= 1e-13 * np.abs(b).max(), (n, fmt)
        assert np.count_nonzero(conv) == nblk and np.count_nonzero(conv.reshape(nblk, n), axis=1).tolist() == [1] * nblk


@pytest.mark.parametrize("n", [64, 512, 2048, 4096, 16384, 1000])
def test_tone_blocks_cover_the_spectrum(n):
    cr.assert_tone_coverage(n)
    assert cr.tone_stride(n) % 2 == 1
    x = cr.tones(4, n, bins=[0, 1, n // 2, n - 1]).reshape(4, n)
    X = np.fft.fft(x.astype(np.complex128), axis=1) / n
    assert np.abs(X - np.eye(n)[[0, 1, n // 2, n - 1]]).max() < 1e-6


def classes(n, few=True):
    """-> [(class, xc, H, analytic want or None)] of one length, c64."""
    nb = cr.tone_blocks(n)
    bins = cr.tone_bins(nb, n)[::max(1, nb // 16)] if few else cr.tone_bins(nb, n)
    raw, conv, pos, amps = cr.impulses("c64", 16, n)
    Ha = cr.allpass(n, 11)
    return [("white", cr.white("c64", 8, n, n + 1), Ha, None),
            ("impulses", conv, Ha, cr.impulse_want64(Ha, n, pos, amps)),
            ("tones", cr.tones(len(bins), n, bins), cr.graded(n, 12), None)]


@pytest.mark.parametrize("n", [64, 1024, 8192, 1000])
def test_yardstick_passes_at_k_1(n):
    for cls, xc, H, w in classes(n):
        assert cr.assert_conv_blocks(cr.yardstick32(xc, H, n), xc, H, n, k=1.0, what=cls, want=w) <= (1.0, 1.0)


def textbook_conv(xc, H, n):
    out = np.empty((len(xc) // n, n), np.complex64)
    for b, x in enumerate(xc.reshape(-1, n)):
        P = textbook_fft32(x, True, split=True) * H
        assert P.dtype == np.complex64
        out[b] = textbook_fft32(P, False, split=True)
    return out


@pytest.mark.parametrize("n", [64, 1024, 8192])
def test_honest_float32_convolution_passes_at_k_4(n):
    """An independent radix-2 float32 transform with the kernels' split twiddles, a complex64 product, the transform
    back: the arithmetic of an honest kernel."""
    for cls, xc, H, w in classes(n):
        r = cr.assert_conv_blocks(textbook_conv(xc, H, n), xc, H, n, k=FFT_K, what="%s n=%d" % (cls, n), want=w)
        print("honest n=%d %-8s worst ratios max_sample %.2f rel_l2 %.2f" % (n, cls, r[0], r[1]))


def fails(got, xc, H, n, dec=1, want=None):
    with pytest.raises(AssertionError):
        cr.assert_conv_blocks(got, xc, H, n, dec, want=want)
    return True


@pytest.mark.parametrize("n", [64, 256, 8192])
def test_block_and_bin_mutants_fail_on_white(n):
    """Mutants 1, 4, 5, 6 and 7 on white input through an all-pass filter."""
    xw = cr.xpw(n) if 256 <= n <= 1024 else 4
    nblk = 5 * xw + 3
    xc, H = cr.white("c64", nblk, n, 77), cr.allpass(n, 7)
    cr.assert_conv_blocks(cr.yardstick32(xc, H, n), xc, H, n, k=1.0)
    assert fails(cr.mutant_swapped_bins(xc, H, n, n // 2 + 3, n // 2 + 5), xc, H, n), "1"
    assert fails(cr.mutant_block_from(xc, H, n, 2, xw), xc, H, n), "4"
    assert fails(cr.mutant_wave_permuted(xc, H, n, 1, xw), xc, H, n), "5"
    assert fails(cr.mutant_last_unwritten(xc, H, n), xc, H, n), "6"
    assert fails(cr.mutant_rotated(xc, H, n, nblk - 2), xc, H, n), "7"
    nan = cr.yardstick32(xc, H, n)
    nan[3, 5] = complex(np.nan, 0.0)
    assert fails(nan, xc, H, n), "NaN"


@pytest.mark.parametrize("n,dec", [(64, 8), (512, 10), (512, 3), (1000, 10), (65536, 3)])
def test_pick_mutants_fail_on_white(n, dec):
    """Mutants 8 and 9 (the latter where the factor does not divide 32768), and mutant 6 behind a pick."""
    count = cr.unit(n, dec) * (1 if n == 1000 else 3) + n + 1
    xc, H = cr.white("c64", count // n + 1, n, 78)[:count], cr.allpass(n, 8)
    cr.assert_conv_blocks(cr.yardstick32(xc, H, n, dec), xc, H, n, dec, k=1.0)
    assert fails(cr.mutant_pick_plus_one(xc, H, n, dec), xc, H, n, dec), "8"
    assert fails(cr.mutant_last_unwritten(xc, H, n, dec), xc, H, n, dec), "6"
    if cr.READER % dec and count >= 2 * cr.READER:
        assert fails(cr.mutant_pick_past_per(xc, H, n, dec), xc, H, n, dec), "9"


@pytest.mark.parametrize("n", [64, 1024, 8192])
def test_one_bin_off_by_1e_5_fails_on_tones(n):
    """Mutants 2 and 3 with the tone class through the graded filter: the block whose tone sits on the bin."""
    bins = cr.tone_bins(cr.tone_blocks(n), n)[5::max(1, cr.tone_blocks(n) // 64)]
    a = int(bins[len(bins) // 3])
    xc, H = cr.tones(len(bins), n, bins), cr.graded(n, 9)
    cr.assert_conv_blocks(cr.yardstick32(xc, H, n), xc, H, n, k=1.0)
    for name, got in (("2", cr.mutant_filter_bin(xc, H, n, a)), ("3", cr.mutant_spectrum_bin(xc, H, n, a))):
        with pytest.raises(AssertionError, match="block %d " % (len(bins) // 3)):
            cr.assert_conv_blocks(got, xc, H, n, what=name)


def test_one_bin_off_by_1e_5_passes_on_white_at_8192():
    """... which is why the tone class exists: on white input at n = 8192 the same two mutants pass K = 4."""
    n, a = 8192, 8192 // 2 + 3
    xc, H = cr.white("c64", 8, n, 79), cr.allpass(n, 10)
    for got in (cr.mutant_filter_bin(xc, H, n, a), cr.mutant_spectrum_bin(xc, H, n, a)):
        r = cr.assert_conv_blocks(got, xc, H, n)
        assert r[0] < FFT_K and r[1] < FFT_K


def test_the_low_pass_blind_spot():
    """Two swapped stop-band bins of the suite's low-pass filter, white input, float64 throughout: below 1e-7 relative
    L2, a twentieth of the older 2e-6 bar.  The same swap in an all-pass filter: above 1e-2."""
    n, a, b = 1024, 1024 // 2 + 3, 1024 // 2 + 5
    xc = cr.white("c64", 8, n, 80)
    seen = {}
    for name, H in (("lowpass", _lowpass_bins(n)), ("allpass", cr.allpass(n, 13))):
        Hs = H.copy()
        Hs[[a, b]] = Hs[[b, a]]
        seen[name] = float(cr.block_metrics(cr.want64(xc, Hs, n), cr.want64(xc, H, n))[1].max())
    print("swap of two bins, white, n=1024: rel_l2 lowpass %.2e allpass %.2e" % (seen["lowpass"], seen["allpass"]))
    assert seen["lowpass"] < 1e-7 < 2e-6 and seen["allpass"] > 1e-2
    # ... and through the single-precision arithmetic the low-pass swap passes the new bar too: it is the filter,
    # not the bar, that hides the bin
    H = _lowpass_bins(n)
    cr.assert_conv_blocks(cr.mutant_swapped_bins(xc, H, n, a, b), xc, H, n)

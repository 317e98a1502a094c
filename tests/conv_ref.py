"""The block-circular convolution (hzsdr_convolution_blocks and the convolution(...) chain terminal) restated in numpy:
which of its six kernel forms a call takes, a float64 reference of every block, the single-precision yardstick, the
per-block checker, filters and inputs that make every bin and every block count, and numpy models of a subtly wrong
kernel.  numpy and scipy only: no GPU, no library.  tests/test_conv_ref_cpu.py holds all of it to the oracle and shows
that every mutant fails the checker; tests/test_gpu_conv_blocks.py runs the kernels against it.

The dispatch (form, xpb, xpw, blocks_per_trip) is a RESTATEMENT BY READING of launch_conv_n and conv_blocks_device in
csrc/hz_conv.hip and of the kernels in csrc/hz_chain_dev.h, not something measured: the tests use it to size their
calls (a whole trip of a walking grid, a trip that ends inside a workgroup) and to prove that their shapes reach every
form.  If the launch code changes, this changes with it.

    form  kernel                                   reached by
    1     conv_blocks_kernel<N, c64, false>        N 4 ... 128, c64 source, no elementwise stage (any decimation)
    2     conv_blocks_kernel<N, FMT, true>         N 4 ... 128, a byte / i16 source or a stage
    3     conv_blocks_shared_kernel<N, 16, FMT>    N 256 ... 1024, no stage, no decimation (any source format)
    4     conv_blocks_kernel16<N, c64, false>      N 2048 ... 8192 c64 without stages; N 256 ... 1024 likewise, decimated
    5     conv_blocks_kernel16<N, FMT, true>       N 256 ... 8192, whatever forms 3 and 4 do not take
    6     conv_blocks_generic_fmt                  every other length

The bar (assert_conv_blocks): for EVERY block b of a call, with want the float64 convolution of the block as stored
and the yardstick the same three steps in complex64 (scipy's transforms, a complex64 product),

    m_b(kernel) <= K * max(m_b(yardstick), 2**-23)    for m in (max_sample, rel_l2),    K = util.FFT_K = 4,

max_sample the block's worst sample error over its largest |want|.  Behind a decimating pick a "block" is one 32 Ki
reader block's picked outputs."""
import math
import os

import numpy as np

from util import FFT_FLOOR, FFT_K, _chirp, rand_c64, rand_i8, rand_i16, rand_u8

READER = 32768  # kReaderBlock: the DecimateReader's block
SENT32 = 0xA5A5A5A5  # what util.Guarded fills a slice with, as a 32-bit word
FORMS = (1, 2, 3, 4, 5, 6)
WORKERS = max(1, min(8, os.cpu_count() or 1))  # threads of the host transforms (rows are independent: the same values)


# ---- the dispatch, restated -------------------------------------------------------------------------------------------

def lds_length(n):
    """fft_lds_ok: the lengths the fused kernels take."""
    return 4 <= n <= 8192 and n & (n - 1) == 0


def form(n, fmt, n_stages, dec):
    """-> 1 ... 6 (the table above).  fmt: "c64", "u8", "i8", "i16"; n_stages: Shift / Gain / Rotate stages in front."""
    if not lds_length(n):
        return 6
    direct = fmt == "c64" and n_stages == 0
    if n < 256:
        return 1 if direct else 2
    if n <= 1024 and n_stages == 0 and dec <= 1:
        return 3
    return 4 if direct else 5


def xpb(f, n):
    """Blocks one workgroup holds side by side (forms 1, 2: fft_xpb; 4, 5: fv::xpb; 3: sixteen waves of xpw)."""
    if f in (1, 2):
        tpt = min(max(n // 4, 1), 256)
        return max(64, tpt) // tpt
    if f == 3:
        return 16 * xpw(n)
    if f in (4, 5):
        return max(64, n // 16) // (n // 16)
    return 1


def xpw(n):
    """ConvShared<N>::XPW: blocks one wave of form 3 transforms side by side."""
    return 64 // (n // 16)


def blocks_per_trip(f, n, cus):
    """Blocks one trip of the grid holds.  Forms 3 and 4 walk (grid <= what the chip holds at once, stride = this
    number); forms 1, 2 and 5 launch one workgroup per xpb blocks and never walk: None."""
    if f == 3:
        return cus * 16 * (64 // (n // 16))
    if f == 4:
        block = max(64, n // 16)
        occ = 2 if block >= 512 else 4
        return cus * (occ * 256 // block) * (block // (n // 16))
    return None


def unit(n, dec):
    """What a chain's plan() consumes in whole: a block, or with a DecimateReader behind it lcm(n, 32 Ki)."""
    return n if dec <= 1 else n * READER // math.gcd(n, READER)


# ---- reference and yardstick ------------------------------------------------------------------------------------------

def whole(count, n, dec=1):
    """Samples of `count` that a call consumes."""
    return count // unit(n, dec) * unit(n, dec)


def pick(y, n, dec):
    """The DecimateReader behind the blocks: out[r * per + q] = y[r * 32768 + q * dec], q < per = 32768 // dec, over
    the whole reader blocks of whole lcm(n, 32768) units.  -> (reader blocks, per); dec <= 1: y as (blocks, n)."""
    if dec <= 1:
        return y.reshape(-1, n)
    per = READER // dec
    flat = y.reshape(-1)
    flat = flat[:whole(flat.shape[0], n, dec)]
    return np.ascontiguousarray(flat.reshape(-1, READER)[:, :per * dec:dec])


def _rows(xc, n):
    xc = np.ascontiguousarray(xc, np.complex64).reshape(-1)
    nblk = xc.shape[0] // n  # (a partial block is dropped)
    return xc[:nblk * n].reshape(nblk, n)


def want64(xc, H, n, dec=1):
    """Block-circular ifft(fft(x_b) * H) * n in complex128, all blocks at once: xc the complex64 stream as stored behind
    the elementwise stages, H the complex64 bins as stored.  (pocketfft in double precision, numpy's own algorithm,
    through scipy so that the rows go over a few threads.)"""
    import scipy.fft
    x = _rows(xc, n).astype(np.complex128)
    h = np.ascontiguousarray(H, np.complex64).astype(np.complex128)
    assert h.shape == (n,)
    X = scipy.fft.fft(x, axis=1, workers=WORKERS)
    X *= h[None, :]
    y = scipy.fft.ifft(X, axis=1, norm="forward", workers=WORKERS)
    assert y.dtype == np.complex128
    return pick(y, n, dec)


def impulse_want64(H, n, positions, amps):
    """The analytic block of an impulse `amp` at `p`: amp * roll(ifft(H) * n, p) -> (blocks, n) complex128."""
    g = np.fft.ifft(np.ascontiguousarray(H, np.complex64).astype(np.complex128)) * n
    idx = (np.arange(n)[None, :] - np.asarray(positions, np.int64)[:, None]) % n
    return np.asarray(amps, np.complex128)[:, None] * g[idx]


def _fft32_rows(a, forward):
    """Single-precision transforms along the rows, backward unnormalised: scipy's complex64 pocketfft for a power of
    two, for any other length util.bluestein_f32's arithmetic (the algorithm the kernels implement) over it."""
    import scipy.fft
    a = np.ascontiguousarray(a, np.complex64)
    n = a.shape[1]
    if n & (n - 1) == 0:
        y = scipy.fft.fft(a, axis=1, workers=WORKERS) if forward else scipy.fft.ifft(a, axis=1, norm="forward", workers=WORKERS)
    else:
        c, B = _chirp(n, bool(forward))
        m = B.shape[0]
        y = np.empty_like(a)
        step = max(1, (1 << 22) // m)
        for r0 in range(0, a.shape[0], step):
            z = np.zeros((min(step, a.shape[0] - r0), m), np.complex64)
            z[:, :n] = a[r0:r0 + step] * c[None, :]
            z = scipy.fft.ifft(scipy.fft.fft(z, axis=1, workers=WORKERS) * B[None, :], axis=1, workers=WORKERS)
            assert z.dtype == np.complex64
            y[r0:r0 + step] = z[:, :n] * c[None, :]
    assert y.dtype == np.complex64, "the yardstick left single precision: %s" % y.dtype
    return y


def yardstick_blocks(xc, H, n, spoil=None):
    """Every block's convolution in single precision, undecimated -> (blocks, n) complex64: the arithmetic of
    sync_ref.closure_yardstick("freq", ...) over all blocks.  spoil = (bin, factor): that bin of every block's
    spectrum times `factor`."""
    X = _fft32_rows(_rows(xc, n), True)
    if spoil is not None:
        X[:, spoil[0]] = X[:, spoil[0]] * np.complex64(spoil[1])
    P = X * np.ascontiguousarray(H, np.complex64)[None, :]
    assert P.dtype == np.complex64
    return _fft32_rows(P, False)


def yardstick32(xc, H, n, dec=1, spoil=None):
    return pick(yardstick_blocks(xc, H, n, spoil), n, dec)


# ---- the checker ------------------------------------------------------------------------------------------------------

def block_metrics(got, want):
    """-> (max_sample, rel_l2) per row."""
    d = np.abs(np.asarray(got).astype(np.complex128) - want)
    peak = np.maximum(np.abs(want).max(axis=1), 1e-300)
    norm = np.maximum(np.linalg.norm(want, axis=1), 1e-300)
    return d.max(axis=1) / peak, np.linalg.norm(d, axis=1) / norm


def assert_conv_blocks(got, xc, H, n, dec=1, k=FFT_K, what="", want=None, yard=None):
    """The bar of the module docstring on EVERY block of the call (dec > 1: on every reader block's picked outputs).
    `got`: the call's output, as long as the reference's; NaN or a word of the sentinel pattern in it fails.
    `want` / `yard`: an analytic float64 reference / a yardstick already computed.  -> the worst ratios
    (max_sample, rel_l2) over the blocks; a failure names the worst block and its worst sample."""
    w = want64(xc, H, n, dec) if want is None else np.asarray(want, np.complex128)
    y = yardstick32(xc, H, n, dec) if yard is None else yard
    g = np.ascontiguousarray(got, np.complex64).reshape(-1)
    assert g.shape[0] == w.size, (what, "output samples", g.shape[0], "expected", w.size)
    g = g.reshape(w.shape)
    words = g.view(np.uint32).reshape(w.shape[0], -1)
    left = np.flatnonzero((words == SENT32).any(axis=1))
    assert left.size == 0, "%s: %d blocks hold sentinel words (never written), the first block %d" % (what, left.size, left[0])
    worst = []
    for name, mg, my in zip(("max_sample", "rel_l2"), block_metrics(g, w), block_metrics(y, w)):
        bound = k * np.maximum(my, FFT_FLOOR)
        ratio = mg / np.maximum(my, FFT_FLOOR)
        bad = np.flatnonzero(~(mg <= bound))  # (a NaN fails)
        if bad.size:
            b = int(bad[np.argmax(np.where(np.isnan(ratio[bad]), np.inf, ratio[bad]))])
            d = np.abs(g[b].astype(np.complex128) - w[b])
            s = int(np.argmax(np.where(np.isnan(d), np.inf, d)))
            raise AssertionError("%s: block %d (%d of %d blocks fail): %s %.3e > %g * max(yardstick %.3e, 2^-23), ratio %.1f, "
                                 "worst sample %d: got %s want %s" % (what, b, bad.size, w.shape[0], name, mg[b], k, my[b],
                                                                      ratio[b], s, g[b, s], w[b, s]))
        worst.append(float(ratio.max()) if ratio.size else 0.0)
    return tuple(worst)


# ---- filters (no low-pass: a stop band hides half the bins) --------------------------------------------------------------

def _unit(u):
    return np.cos(2.0 * np.pi * u) + 1j * np.sin(2.0 * np.pi * u)


def allpass(n, seed):
    """exp(2 pi i u_k) / n, u_k uniform: every bin moves the output by the same amount."""
    return (_unit(np.random.default_rng(seed).random(n)) / n).astype(np.complex64)


def graded(n, seed):
    """(0.5 + ((37 k) mod n) / n) exp(2 pi i u_k) / n: every bin has a gain of its own."""
    k = np.arange(n, dtype=np.int64)
    return ((0.5 + ((37 * k) % n) / n) * _unit(np.random.default_rng(seed).random(n)) / n).astype(np.complex64)


def delay(n, d):
    """exp(-2 pi i k d / n) / n: the output is the input rotated by d inside its block."""
    k = np.arange(n, dtype=np.int64)
    return (_unit(-((k * d) % n) / n) / n).astype(np.complex64)


# ---- inputs: whole (nblk, n) streams ----------------------------------------------------------------------------------

def white(fmt, nblk, n, seed):
    """-> the raw samples of the format (c64: re / im uniform in [-1, 1))."""
    return {"c64": rand_c64, "u8": rand_u8, "i8": rand_i8, "i16": rand_i16}[fmt](seed, nblk * n)


def impulse_positions(nblk, n):
    return (7 * np.arange(nblk, dtype=np.int64) + 3) % n


def impulses(fmt, nblk, n):
    """Block b is zero but for one sample at (7 b + 3) mod n of amplitude readout.train_amp(fmt, b) (c64:
    2^-(b mod 8) (1 - 0.5j)) -> (raw samples, their converted complex64 values, positions, amplitudes as complex).
    u8 has no zero: not offered."""
    from readout import train_amp
    from util import DT
    period = [train_amp(fmt, b) for b in range(24)]  # (a multiple of every format's period)
    b = np.arange(nblk)
    at = b * n + impulse_positions(nblk, n)
    raw = np.zeros(nblk * n, np.complex64) if fmt == "c64" else np.zeros((nblk * n, 2), DT[fmt])
    conv = np.zeros(nblk * n, np.complex64)
    raw[at] = np.array([r for r, _ in period], raw.dtype)[b % 24]
    amps = np.array([a for _, a in period], np.complex128)[b % 24]
    conv[at] = amps.astype(np.complex64)
    assert np.array_equal(conv[at].astype(np.complex128), amps), "an amplitude is not exact in float32"
    return raw, conv, impulse_positions(nblk, n), amps


def tone_stride(n):
    """g of k_b = (g b) mod n: 1 up to 2048 bins; above, odd, so that no bin repeats within n blocks."""
    return 1 if n <= 2048 else 2 * n // 2048 + 1


def tone_bins(nblk, n):
    return (tone_stride(n) * np.arange(nblk, dtype=np.int64)) % n


def tone_blocks(n):
    return min(n, 2048)


def assert_tone_coverage(n, nblk=None):
    """min(n, 2048) blocks visit every bin up to 2048; above, every k mod 16 and every sixteenth of the spectrum."""
    k = tone_bins(tone_blocks(n) if nblk is None else nblk, n)
    if n <= 2048:
        assert np.array_equal(np.sort(k), np.arange(n)), (n, "a bin is not visited")
    else:
        assert np.unique(k).shape[0] == k.shape[0], (n, "a bin repeats")
        assert set(k % 16) == set(range(16)) and set(k // (n // 16)) == set(range(16)), (n, "coverage")


def tones(nblk, n, bins=None):
    """Block b is exp(2 pi i k_b t / n) as complex64 (c64 only), k_b = tone_bins (or `bins`): the whole tone sits on
    ONE bin of the block's spectrum, where one wrong filter or table entry is the whole error."""
    bins = tone_bins(nblk, n) if bins is None else np.asarray(bins, np.int64)
    w = _unit(np.arange(n, dtype=np.float64) / n).astype(np.complex64)
    t = np.arange(n, dtype=np.int64)
    out = np.empty((bins.shape[0], n), np.complex64)
    for r0 in range(0, bins.shape[0], 256):
        out[r0:r0 + 256] = w[(bins[r0:r0 + 256, None] * t[None, :]) % n]
    return out.reshape(-1)


# ---- mutants: a subtly wrong kernel, modelled on the yardstick's arithmetic ---------------------------------------------

def _sentinel(count):
    return np.full(2 * count, SENT32, np.uint32).view(np.complex64)


def mutant_swapped_bins(xc, H, n, a, b, dec=1):
    """1. two filter bins swapped"""
    Hs = np.array(H, np.complex64)
    Hs[[a, b]] = Hs[[b, a]]
    return yardstick32(xc, Hs, n, dec)


def mutant_filter_bin(xc, H, n, a, dec=1, factor=1 + 1e-5):
    """2. one filter bin times 1 + 1e-5"""
    Hs = np.array(H, np.complex64)
    Hs[a] = Hs[a] * np.complex64(factor)
    return yardstick32(xc, Hs, n, dec)


def mutant_spectrum_bin(xc, H, n, a, dec=1, factor=1 + 1e-5):
    """3. one bin of every block's spectrum times 1 + 1e-5 (a wrong twiddle-table entry)"""
    return yardstick32(xc, H, n, dec, spoil=(a, factor))


def mutant_block_from(xc, H, n, b, stride, dec=1):
    """4. block b computed from block b + stride's input (a prefetch one trip ahead of its block)"""
    x = _rows(xc, n).copy()
    x[b] = x[b + stride]
    return yardstick32(x, H, n, dec)


def mutant_wave_permuted(xc, H, n, group, xpw_, dec=1):
    """5. the blocks inside one wave's group of xpw rotated by one"""
    y = yardstick_blocks(xc, H, n)
    y[group * xpw_:(group + 1) * xpw_] = np.roll(y[group * xpw_:(group + 1) * xpw_], 1, axis=0)
    return pick(y, n, dec)


def mutant_last_unwritten(xc, H, n, dec=1):
    """6. the last (ragged) block left unwritten: the output slice's sentinel fill"""
    y = yardstick32(xc, H, n, dec)
    y[-1] = _sentinel(y.shape[1])
    return y


def mutant_rotated(xc, H, n, b, dec=1):
    """7. a block's output rotated by one sample"""
    y = yardstick_blocks(xc, H, n)
    y[b] = np.roll(y[b], 1)
    return pick(y, n, dec)


def mutant_pick_plus_one(xc, H, n, dec):
    """8. the decimating pick taken at i + 1"""
    assert dec > 1
    per = READER // dec
    flat = yardstick_blocks(xc, H, n).reshape(-1)
    flat = flat[:whole(flat.shape[0], n, dec)].reshape(-1, READER)
    return np.ascontiguousarray(flat[:, (np.arange(per) * dec + 1) % READER])


def mutant_pick_past_per(xc, H, n, dec=10):
    """9. the pick without `q < per`: with dec = 10 a reader block's sample 32760 = 3276 * 10 is written as output
    q = per, which is the next reader block's output 0 (behind the last reader block: the guard)"""
    per = READER // dec
    assert per * dec < READER, "this factor divides 32768: there is no output q = per"
    flat = yardstick_blocks(xc, H, n).reshape(-1)
    flat = flat[:whole(flat.shape[0], n, dec)].reshape(-1, READER)
    y = np.ascontiguousarray(flat[:, :per * dec:dec])
    y[1:, 0] = flat[:-1, per * dec]
    return y


# ---- the shapes of tests/test_gpu_conv_blocks.py: (n, source format, elementwise stages, decimation) -> form --------------
SHAPES = {
    1: [(n, "c64", 0, 1) for n in (4, 8, 16, 32, 64, 128)],
    2: [(n, "i16", 2, 1) for n in (8, 64, 128)] + [(n, "u8", 0, 1) for n in (8, 64, 128)]
       + [(64, "i16", 1, d) for d in (8, 10, 3)],
    3: [(n, f, 0, 1) for n in (256, 512, 1024) for f in ("c64", "u8", "i8", "i16")],
    4: [(n, "c64", 0, 1) for n in (2048, 4096, 8192)] + [(n, "c64", 0, 8) for n in (256, 512, 1024)]
       + [(512, "c64", 0, d) for d in (10, 3)],
    5: [(256, "u8", 1, 1), (512, "u8", 1, 1), (2048, "u8", 1, 1), (8192, "u8", 1, 1), (1024, "c64", 1, 1),
        (4096, "i8", 0, 1)] + [(4096, "u8", 1, d) for d in (8, 10, 3)],
    6: [(n, "c64", 0, 1) for n in (1, 2, 3, 12, 1000, 16384)] + [(n, "c64", 0, d) for n in (1000, 65536) for d in (8, 10, 3)],
}

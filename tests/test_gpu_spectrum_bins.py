"""The fused power spectrum (include/hzsdr_spectrum.h) per bin, per frame and per row, in both kernel forms.

What tests/test_gpu_spectrum.py cannot see: it scores a row by ONE relative-L1 number over white input, a bound that two
swapped bins, one wrong window entry or one bin of one frame off by 1e-4 pass (tests/test_spectrum_checker_cpu.py keeps
those experiments), and everything else it asserts compares the kernels with themselves.

The bar (tests/spectrum_ref.py, spectrum_bar): with want the float64 spectrum of the frames as the kernel forms them
(complex64 sample times float32 window) and, per frame, e = FFT_K max(max_bin(yardstick), 2^-23) max_k |X_k| the
amplitude bar the FFT core already meets (tests/test_gpu_fft_plans.py, K = 4 over scipy's complex64 transform),

    |got - want| <= scale * ( sum over the row's frames of (2 sqrt(P) e + e^2 + 3 2^-24 P)  +  (avg + 1) 2^-24 sum P )

for EVERY bin of every row.  An honest textbook float32 spectrum measures <= 0.37 of it on the CPU; two swapped bins
measure 46 and more, one window entry off by 1e-3 measures 5.8.

Sections:  B   every size, source format, kernel form and order against the bar: white, comb, one tone per frame, an
               off-bin tone; rectangular, asymmetric and Hann windows; hop n/2, n, n + 37; avg 1 and 5; 2 xpb + 1 rows
               and an open one
           C1  window and staging read-out: one impulse per frame, the position walking through the frame under an
               asymmetric window -- row j is (w[p_j] |a_j|)^2 scale in every bin
           C2  row bookkeeping BIT FOR BIT against the analytic value: impulses at position 0 whose squared magnitudes
               sum exactly in float32 in any order; rows around the rows-per-workgroup edge, cuts that leave 1 and K - 1
               frames in the open row, cuts inside a skip gap and one sample behind a frame start, one sample per push,
               pending() after every push; the chunk edges of the frame-parallel form (kSpecChunkFloats)
           D   isolation: guard rows behind rows_written, a NaN kept to the rows of its frames, input sub-slices one to
               three samples off an allocation's start, host context for every format and form
           E   stream.spectrum_rows over a Reader with short reads; fft::Spectrum of cxx/hzsdr.hpp

Observed worst |got - want| / bound over sections B and C1 on an MI355X (row walk | frame parallel: the same bits, so the
same figures; printed when the module ends, `pytest -s`):

    N       white         comb          tones         tone_off_bin  impulse (C1)
    256     0.31 | 0.31   0.35 | 0.35   0.19 | 0.19   0.20 | 0.20   0.42 | 0.42
    512     0.32 | 0.32   0.35 | 0.35   0.19 | 0.19   0.21 | 0.21   0.42 | 0.42
    1024    0.33 | 0.33   0.30 | 0.30   0.21 | 0.21   0.25 | 0.25   0.50 | 0.50
    2048    0.32 | 0.32   0.33 | 0.33   0.16 | 0.16   0.31 | 0.31   0.44 | 0.44
    4096    0.31 | 0.31   0.29 | 0.29   0.24 | 0.24   0.22 | 0.22   0.44 | 0.44
    8192    0.32 | 0.32   0.33 | 0.33   0.26 | 0.26   0.21 | 0.21   0.46 | 0.46
    The worst is 0.50 (an impulse at N = 1024): the kernels use half of the bar, as the honest spectrum on the CPU does.

Tried once against the bar and not kept: bins 37 and 38 exchanged in spec_pos fail B at every size and format; the
last frame of a chunk left out of spectrum_sum_kernel's j1 fails B, C1 and C2 throughout; the open row's frame count not
carried from chunk to chunk (fc) fails only the chunk-edge cases of C2 here, with avg = 3 and with avg = C + 5 -- the
latter only because every push of this module writes into rows that hold SENTINEL beforehand (push() below): the row
walk's correct rows of the run before were still in the allocator's block.
"""
import importlib
import os
import subprocess

import numpy as np
import pytest

import spectrum_ref as sr
from conftest import ROOT
from util import FMT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIZES = [256, 512, 1024, 2048, 4096, 8192]
FORMATS = ["u8", "i8", "i16", "c64"]
SENTINEL = 0x7F7F7F7F  # a float32 of 3.39e38: no row of these tests holds it
CHUNK_FLOATS = 1 << 23  # kSpecChunkFloats of csrc/hz_spectrum.hip: the frame-parallel form's scratch, in float32 values
RATIOS = {}  # (n, input class, form) -> worst |got - want| / bound


def xpb(n):
    """rows (and frames) per workgroup: fv::xpb of csrc/hz_fftv.h"""
    return {256: 4, 512: 2}.get(n, 1)


@pytest.fixture(scope="module")
def hz():
    return importlib.import_module("go-sdr_amd")


@pytest.fixture(scope="module")
def sp():
    return importlib.import_module("go-sdr_amd.spectrum")


@pytest.fixture(scope="module")
def ctx(hz):
    c = hz.Context(0, hz.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


@pytest.fixture(scope="module")
def hctx(hz):
    c = hz.Context(0, hz.MEM_HOST)
    yield c
    c.close()


@pytest.fixture(scope="module", autouse=True)
def report_ratios():
    """Prints what the module measured (`pytest -s`): the table of the docstring and of DESIGN.md section 4."""
    yield
    for (n, cls, form), r in sorted(RATIOS.items()):
        print("\nRATIO n=%-5d %-12s form %d  %5.2f" % (n, cls, form, r), end="")


def note(n, cls, form, ratio):
    RATIOS[(n, cls, form)] = max(RATIOS.get((n, cls, form), 0.0), ratio)


def forms(hz):
    return (hz.SPECTRUM_FORM_ROW_WALK, hz.SPECTRUM_FORM_FRAME_PARALLEL)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def ibits(t):
    t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    a, b = ibits(a).cpu(), ibits(b).cpu()
    return a.shape == b.shape and bool(torch.equal(a, b))


def push(s, x):
    """s.push(x) into rows that hold SENTINEL beforehand: a row the kernels leave unwritten cannot pass for written by
    what an earlier run left in the allocator's block"""
    rows = s.rows_for(x.shape[0])
    if isinstance(x, torch.Tensor):
        out = torch.full((rows, s.n), SENTINEL, dtype=torch.int32, device=x.device).view(torch.float32)
    else:
        out = np.full((rows, s.n), SENTINEL, np.int32).view(np.float32)
    got = s.push(x, out=out)
    assert got.shape == (rows, s.n)
    return got


def push_cuts(s, x, cuts, shape=None):
    """push x[cuts[i]:cuts[i + 1]] in turn, pending() checked against the stream position after every push (`shape`:
    (n, hop, avg)); -> the rows of all pushes, concatenated"""
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        out.append(push(s, x[a:b]))
        if shape is not None:
            assert s.pending() == sr.pending_after(b, *shape), (cuts, b)
    if isinstance(out[0], torch.Tensor):
        return torch.cat(out, 0)
    return np.concatenate(out, 0)


def rows_equal_columns(got, col):
    """every bin of row r of `got` (a device tensor or numpy rows) has the bits of float32 col[r]"""
    col = np.asarray(col, np.float64)
    c32 = col.astype(np.float32)
    assert (c32.astype(np.float64) == col).all(), "the analytic rows are not float32 values"
    if got.shape[0] != c32.shape[0]:
        return False
    if isinstance(got, torch.Tensor):
        want = torch.from_numpy(c32).to(got.device).view(torch.int32)[:, None]
        return bool((got.view(torch.int32) == want).all().item())
    return bool((np.ascontiguousarray(got).view(np.int32) == c32.view(np.int32)[:, None]).all())


# ---- B. per bin against the bar --------------------------------------------------------------------------------------

def bar_cases(n):
    """(class, window name, hop, avg) of one size and format"""
    out = []
    for cls in sr.CLASSES:
        for win in ("rect", "asym"):
            for hop in ((n,) if cls == "tones" else (n // 2, n, n + 37)):
                for avg in (1, 5):
                    out.append((cls, win, hop, avg))
    out.append(("white", "hann", n // 2, 5))
    return out


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("n", SIZES)
def test_every_bin_against_the_bar(hz, sp, orc, ctx, n, fmt):
    windows = {"rect": None, "asym": sr.asym_window(n), "hann": sp.hann(n)}
    for i, (cls, win, hop, avg) in enumerate(bar_cases(n)):
        w = windows[win]
        rows = 2 * xpb(n) + 1
        frames = rows * avg + (avg - 1 if avg > 1 else 0)  # ... and an open row (avg = 1: held samples only)
        L = (frames - 1) * hop + n + hop // 3
        x, c = sr.class_input(orc, cls, fmt, n, L, seed=n * 31 + i)
        scale = sp.spectrum_scale("power", n, avg, w)
        want, bound = sr.spectrum_bar(c, n, hop, avg, w, scale)
        assert want.shape == (rows, n) and (bound > 0).all()
        dx = dev(x)
        for order in (sp.ZeroFirst, sp.NegativeFirst):
            wo, bo = (want, bound) if order == sp.ZeroFirst else (sr.negative_first(want), sr.negative_first(bound))
            with ctx.spectrum(FMT[fmt], n, hop=hop, avg=avg, window=w, scale="power", order=order) as s:
                assert s.scale == scale
                for form in forms(hz):
                    s.reset()
                    s.options(form)
                    got = push(s, dx).cpu().numpy()
                    assert s.last_form() == form
                    assert s.pending() == sr.pending_after(L, n, hop, avg)
                    what = "%s n=%d %s %s hop=%d avg=%d form %d order %d" % (fmt, n, cls, win, hop, avg, form, order)
                    note(n, cls, form, sr.check_bar(got, wo, bo, what))


# ---- C1. window and staging read-out ---------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", sr.EXACT_FORMATS)
@pytest.mark.parametrize("n", SIZES)
def test_window_read_out(hz, sp, orc, ctx, n, fmt):
    """hop = n, avg = 1, frame j zero except a_j at position p_j under the asymmetric window (w[0] = 0.25): every bin
    of row j is (w[p_j] |a_j|)^2 scale.  Every position up to N = 2048; beyond, 2048 positions: the first and last 64
    of each of a lane's sixteen register slots (the frame's first and last 64 among them)."""
    pos = sr.slot_positions(n)
    w = sr.asym_window(n)
    scale = 2.0 ** -3
    x, p = sr.impulse_stream(fmt, n, n, pos, 24)
    want = (scale * w.astype(np.float64)[pos] ** 2 * p)[:, None] * np.ones((1, n))
    restated, bound = sr.spectrum_bar(sr.converted(orc, x), n, n, 1, w, scale)
    assert np.abs(restated - want).max() <= 1e-12 * want.max()  # (the analytic value is the definition's)
    dx = dev(x)
    with ctx.spectrum(FMT[fmt], n, hop=n, avg=1, window=w, scale=scale, order=sp.ZeroFirst) as s:
        for form in forms(hz):
            s.reset()
            s.options(form)
            got = push(s, dx).cpu().numpy()
            assert s.last_form() == form and s.pending() == (0, 0)
            note(n, "impulse", form, sr.check_bar(got, want, bound, "%s n=%d form %d (row j: position %s ...)" % (fmt, n, form, pos[:3])))


# ---- C2. row bookkeeping, bit for bit --------------------------------------------------------------------------------

def total_rows(n):
    return sorted({r for r in (1, xpb(n) - 1, xpb(n), xpb(n) + 1, 2 * xpb(n) + 1) if r > 0})


def cut_sets(n, hop, avg, frames, L):
    """one push; two pushes cut so that the second starts with 1 and K - 1 frames in the open row: at the frame's last
    sample, inside the skip gap behind it, one sample behind the next frame's start"""
    out = [[0, L]]
    for f0 in sorted({1, avg - 1} - {0}):
        if f0 >= frames:
            continue
        at = [(f0 - 1) * hop + n, f0 * hop + 1]
        if hop > n + 1:
            at.append((f0 - 1) * hop + n + (hop - n) // 2)
        out += [[0, a, L] for a in at if 0 < a < L]
    return out


@pytest.mark.parametrize("avg", [1, 3, 7, 16])
@pytest.mark.parametrize("n", [256, 512, 1024])
def test_rows_bit_for_bit_against_the_analytic_value(hz, sp, ctx, n, avg):
    """An impulse at each frame's position 0: the transform of a_j delta is a_j in every bin through multiplications by
    1 and additions of 0 alone, |w[0] a_j|^2 sums exactly in any order (tests/test_spectrum_checker_cpu.py), so row r
    is scale * sum_t |w[0] a_{r K + t}|^2 to the bit in both forms, however the stream is cut."""
    scale = 2.0 ** -3
    half = np.ones(n, np.float32)
    half[0] = 0.5
    runs = 0
    for fmt in sr.EXACT_FORMATS:
        period = sr.exact_period(fmt, avg)
        for hop in (n, n + 37, 3 * n + 1):
            specs = [(w2, ctx.spectrum(FMT[fmt], n, hop=hop, avg=avg, window=w, scale=scale)) for w2, w in ((1.0, None), (0.25, half))]
            for rows in total_rows(n):
                for open_row in (False, True):
                    frames = rows * avg + (min(avg - 1, 2) if open_row else 0)
                    x, p = sr.impulse_stream(fmt, n, hop, np.zeros(frames, np.int64), period, tail=n // 3 if open_row else 0)
                    assert sr.prefix_sums_exact(p, avg)
                    L, dx = x.shape[0], dev(x)
                    for w2, s in specs:
                        want = sr.exact_rows(p, avg, w2, scale)
                        assert want.shape == (rows,)
                        for form in forms(hz):
                            s.options(form)
                            for cuts in cut_sets(n, hop, avg, frames, L):
                                s.reset()
                                got = push_cuts(s, dx, cuts, (n, hop, avg))
                                assert rows_equal_columns(got, want), (fmt, hop, rows, open_row, w2, form, cuts)
                                runs += 1
            for _, s in specs:
                s.close()
    assert runs >= 2 * 3 * len(total_rows(n)) * 2 * 2 * 2


@pytest.mark.parametrize("n", [256, 512, 1024])
def test_rows_bit_for_bit_host(hz, sp, hctx, n):
    """the same in a HOST context: xpb + 1 rows and an open one, every avg, a cut one sample behind a frame start"""
    scale = 2.0 ** -3
    half = np.ones(n, np.float32)
    half[0] = 0.5
    for i, avg in enumerate((1, 3, 7, 16)):
        hop = (n, n + 37, 3 * n + 1)[i % 3]
        for fmt in sr.EXACT_FORMATS:
            frames = (xpb(n) + 1) * avg + min(avg - 1, 2)
            x, p = sr.impulse_stream(fmt, n, hop, np.zeros(frames, np.int64), sr.exact_period(fmt, avg), tail=n // 3)
            want = sr.exact_rows(p, avg, 0.25, scale)
            with hctx.spectrum(FMT[fmt], n, hop=hop, avg=avg, window=half, scale=scale) as s:
                for form in forms(hz):
                    s.options(form)
                    for cuts in ([0, x.shape[0]], [0, hop + 1, x.shape[0]]):
                        s.reset()
                        assert rows_equal_columns(push_cuts(s, x, cuts, (n, hop, avg)), want), (fmt, avg, hop, form, cuts)


@pytest.mark.parametrize("hop", [256, 258])
@pytest.mark.parametrize("form", [1, 2])
def test_one_sample_per_push(hz, sp, ctx, form, hop):
    """2 n + 3 samples one by one (hop = n + 2: two of the pushes fall into the skip gap and launch nothing)"""
    n, avg = 256, 2
    L = 2 * n + 3
    x, p = sr.impulse_stream("i8", n, hop, np.zeros(2, np.int64), 6, tail=3 - (hop - n))
    assert x.shape[0] == L
    dx = dev(x)
    with ctx.spectrum(hz.FMT_I8, n, hop=hop, avg=avg, scale=2.0 ** -3) as s:
        s.options(form)
        got = push_cuts(s, dx, list(range(L + 1)), (n, hop, avg))
        assert rows_equal_columns(got, sr.exact_rows(p, avg, 1.0, 2.0 ** -3)) and got.shape[0] == 1


@pytest.mark.parametrize("avg_kind", ["1", "3", "C+5"])
@pytest.mark.parametrize("n", [256, 8192])
def test_chunk_edges_of_the_frame_parallel_form(hz, sp, ctx, n, avg_kind):
    """The frame-parallel form walks a push in chunks of C = kSpecChunkFloats / N frames and carries the open row's
    frame count and sums from chunk to chunk: pushes of C - 1, C, C + 1 and 2 C + 3 frames, behind a first push that
    leaves 0 or 2 frames in the open row; rows of 1 and 3 frames (the open row is cut by every chunk edge for avg = 3
    whenever 3 does not divide the frames in front of it) and of C + 5 (a row that spans a whole chunk).  The row walk
    gives the same bits: the analytic ones."""
    C = CHUNK_FLOATS // n
    avg = {"1": 1, "3": 3, "C+5": C + 5}[avg_kind]
    scale = 2.0 ** -3
    period = sr.exact_period("i8", avg)
    x, p = sr.impulse_stream("i8", n, n, np.zeros(2 * C + 5, np.int64), period)
    assert sr.prefix_sums_exact(p, avg) or avg > 2 * C + 5
    dx = dev(x)
    with ctx.spectrum(hz.FMT_I8, n, hop=n, avg=avg, scale=scale) as s:
        for F in (C - 1, C, C + 1, 2 * C + 3):
            for f0 in ((0, 2) if avg > 2 else (0,)):
                want = sr.exact_rows(p[:f0 + F], avg, 1.0, scale)
                for form in forms(hz):
                    s.reset()
                    s.options(form)
                    if f0:
                        assert push(s, dx[:f0 * n]).shape[0] == 0
                        assert s.pending() == (f0, 0)
                    got = push(s, dx[f0 * n:(f0 + F) * n])
                    assert s.last_form() == form
                    assert s.pending() == ((f0 + F) % avg, 0)
                    assert rows_equal_columns(got, want), (n, avg, F, f0, form)
                    del got


# ---- D. isolation ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("space", ["device", "host"])
def test_rows_behind_the_count_stay_untouched(hz, sp, ctx, hctx, space):
    n, hop, avg = 512, 512, 3
    frames = (2 * xpb(n) + 1) * avg + 1
    x = sr.white_raw("u8", (frames - 1) * hop + n + 5, seed=7)
    on_dev = space == "device"
    c = ctx if on_dev else hctx
    xin = dev(x) if on_dev else x

    def guarded(rows):
        if on_dev:
            return torch.full((rows, n), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
        return np.full((rows, n), SENTINEL, np.int32).view(np.float32)

    def ints(t):
        return t.cpu().numpy().view(np.int32) if on_dev else t.view(np.int32)

    for form in forms(hz):
        with c.spectrum(hz.FMT_U8, n, hop=hop, avg=avg, window=sp.hann(n)) as s, \
                c.spectrum(hz.FMT_U8, n, hop=hop, avg=avg, window=sp.hann(n)) as plain:
            s.options(form)
            plain.options(form)
            # a push that completes no row writes nothing
            out = guarded(2)
            assert s.rows_for(2 * hop) == 0 and s.push(xin[:2 * hop], out=out).shape[0] == 0
            assert (ints(out) == SENTINEL).all()
            rest = x.shape[0] - 2 * hop
            rows = s.rows_for(rest)
            assert rows == 2 * xpb(n) + 1
            out = guarded(rows + 2)
            got = s.push(xin[2 * hop:], out=out)
            assert got.shape[0] == rows
            assert (ints(out)[rows:] == SENTINEL).all(), "rows behind rows_written were written"
            want = push_cuts(plain, xin, [0, x.shape[0]])
            assert same_bits(out[:rows], want) and not (ints(out)[:rows] == SENTINEL).any()


@pytest.mark.parametrize("db", [False, True], ids=["power", "db"])
@pytest.mark.parametrize("n", [512, 2048])
def test_a_nan_stays_in_the_rows_of_its_frames(hz, sp, ctx, n, db):
    hop, avg, rows = n // 2, 3, 6
    L = (rows * avg) * hop + n  # (an open row of one frame behind the last)
    clean = sr.white_raw("c64", L, seed=n)
    for at in (8 * hop + 5, 9 * hop + 5, 0, L - 1):  # (frames 7, 8: row 2; frames 8, 9: rows 2 and 3; frame 0; the open row)
        x = clean.copy()
        x[at] = np.complex64(complex(np.nan, 0.5))
        hit = sorted({j // avg for j in range(rows * avg) if j * hop <= at < j * hop + n})
        dx, dc = dev(x), dev(clean)
        for form in forms(hz):
            with ctx.spectrum(hz.FMT_C64, n, hop=hop, avg=avg, window=sp.hann(n), db=db) as s:
                s.options(form)
                want = push_cuts(s, dc, [0, L]).cpu().numpy()
                assert want.shape == (rows, n) and not np.isnan(want).any()
                for cuts in ([0, L], [0, min(L - 1, at + 3), L], [0, max(1, at), L]):
                    s.reset()
                    got = push_cuts(s, dx, cuts).cpu().numpy()
                    assert got.shape == (rows, n)
                    for r in range(rows):
                        if r in hit:
                            assert np.isnan(got[r]).all(), (at, form, cuts, "row %d is not all NaN" % r)
                        else:
                            assert same_bits(got[r], want[r]), (at, form, cuts, "row %d differs from the clean run" % r)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("n", [512, 2048])
def test_input_sub_slices(hz, sp, ctx, n, fmt):
    """the input 1, 2 and 3 samples into a larger allocation gives the bits of an aligned copy"""
    hop, avg = n // 2 + 3, 2
    L = 11 * hop + n + 9
    big = sr.white_raw(fmt, L + 8, seed=n + 3)
    dbig = dev(big)
    assert dbig.data_ptr() % 256 == 0
    for form in forms(hz):
        with ctx.spectrum(FMT[fmt], n, hop=hop, avg=avg, window=sr.asym_window(n)) as s:
            s.options(form)
            for off in (1, 2, 3):
                s.reset()
                aligned = dev(big[off:off + L])
                assert aligned.data_ptr() % 256 == 0
                want = push_cuts(s, aligned, [0, L])
                assert want.shape[0] == 6
                for cuts in ([0, L], [0, n + 1, L]):
                    s.reset()
                    view = dbig[off:off + L]
                    assert view.data_ptr() == dbig.data_ptr() + off * big[0:1].nbytes
                    assert same_bits(push_cuts(s, view, cuts), want), (fmt, n, form, off, cuts)


@pytest.mark.parametrize("fmt", FORMATS)
def test_host_context_every_format_and_form(hz, sp, ctx, hctx, fmt):
    n, hop, avg = 512, 300, 3
    L = 16 * hop + n + 17
    x = sr.white_raw(fmt, L, seed=19)
    for form in forms(hz):
        with ctx.spectrum(FMT[fmt], n, hop=hop, avg=avg, window=sp.hann(n)) as d, \
                hctx.spectrum(FMT[fmt], n, hop=hop, avg=avg, window=sp.hann(n)) as h:
            d.options(form)
            h.options(form)
            rd = push_cuts(d, dev(x), [0, L])
            rh = push_cuts(h, x, [0, 1000, 1001, L], (n, hop, avg))
            assert h.last_form() == form and isinstance(rh, np.ndarray)
            assert rd.shape[0] == 5 and same_bits(rd, rh)


# ---- E. the other layers ---------------------------------------------------------------------------------------------

def test_spectrum_rows_over_a_reader(hz, sp, hctx):
    """stream.spectrum_rows over a BufferReader with short reads is one push of the whole stream."""
    st = importlib.import_module("go-sdr_amd.stream")
    n, hop, avg, rate = 256, 200, 3, 2_048_000
    x = sr.white_raw("i16", 20_000, seed=5)
    with hctx.spectrum(hz.FMT_I16, n, hop=hop, avg=avg, window=sp.hann(n), order=sp.ZeroFirst, sample_rate=rate) as one:
        want = np.array(one.push(x))
    with hctx.spectrum(hz.FMT_I16, n, hop=hop, avg=avg, window=sp.hann(n), order=sp.ZeroFirst, sample_rate=rate) as s:
        blocks = [(np.array(r), fs, order) for r, fs, order in st.spectrum_rows(st.BufferReader(x, rate, max_read=777), s, block=1024)]
        assert s.pending() == sr.pending_after(x.shape[0], n, hop, avg)
        assert s.frequency_slice() == (n, rate, sp.ZeroFirst)
    assert len(blocks) > 3 and all(r.dtype == np.float32 and r.shape[1] == n and r.shape[0] > 0 for r, _, _ in blocks)
    assert all((fs, order) == (rate, sp.ZeroFirst) for _, fs, order in blocks)
    assert want.shape[0] == sr.counts(x.shape[0], n, hop, avg)[1] and same_bits(np.concatenate([r for r, _, _ in blocks]), want)
    with hctx.spectrum(hz.FMT_U8, n, hop=hop, avg=avg) as s, pytest.raises(hz.ErrSampleFormatMismatch):
        list(st.spectrum_rows(st.BufferReader(x, rate), s))


def test_cxx_spectrum(hz):
    """tests/cxx/test_spectrum.cpp (hzsdr::fft::Spectrum of go-sdr_amd/cxx/hzsdr.hpp) built with g++ and run."""
    build = os.path.join(ROOT, "build")
    exe = os.path.join(build, "test_spectrum_cxx")
    os.makedirs(build, exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + ROOT, os.path.join(ROOT, "tests", "cxx", "test_spectrum.cpp"),
                           "-L" + os.path.join(ROOT, "go-sdr_amd"), "-lhzsdr_hip", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "go-sdr_amd") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "spectrum-cxx ok" in p.stdout

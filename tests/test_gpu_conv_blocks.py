"""The block-circular convolution per sample, per block and per kernel form (through the C ABI, device context).

hzsdr_convolution_blocks and the convolution(...) chain terminal have six kernel forms (tests/conv_ref.py restates the
dispatch), each with its own block walk and LDS layout.  What the older tests of it share -- tests/test_gpu_parity.py,
check_conv_blocks of tests/test_gpu_fft_plans.py -- is a low-pass filter, white input and ONE relative-L2 number < 2e-6,
mostly on a sample of the blocks: half of the filter's bins can be indexed wrongly under that bar
(tests/test_conv_ref_cpu.py pins the experiment).  They stay as checks of the reference's semantics.

The bar here (conv_ref.assert_conv_blocks), on EVERY block of every call, nothing sampled:

    m_b(kernel) <= K * max(m_b(yardstick), 2**-23)    for m in (max_sample, rel_l2),    K = util.FFT_K = 4

against the float64 convolution of the stream as stored behind the elementwise stages (which are bit-exact: the
oracle's convert, Shift, scale and rotate produce it), the yardstick the same three steps in complex64.  Filters are
all-pass, graded (every bin a gain of its own) or a pure delay, never a low-pass; inputs are white, one impulse per
block (an analytic reference, every filter bin in every sample) or one on-bin tone per block (the block's whole energy
through ONE bin of the filter and of the transform tables, visiting every bin up to 2048).

Sections:  A  walks of forms 3 and 4: two full trips of the grid and a ragged third, exactly one trip, 1, xpw + 1
           B  workgroup edges of forms 1, 2 and 5; Shift with the clock's 2 pi wrap inside the call; two run() calls
           C  per-bin read-out of all six forms (tones x graded, impulses x all-pass), and pure delays
           D  the decimating pick at factors 8, 10 and 3 into a slice of exactly plan()'s length
           E  a block's bits do not depend on its neighbours, on NaN / Inf beside it, or on how often the call runs
           F  sub-slices one sample off 16-byte (c64) / pair (bytes, i16) alignment
           G  the generic form: past a Bluestein piece, 16384 bins, lengths 1, 2, 3 and 12
           H  one host-context call

Observed worst ratio kernel / max(yardstick, 2^-23), max_sample | rel_l2, over all sections on an MI355X (printed when
the module ends, `pytest -s`):

    form                                            white         impulses      tones
    1  conv_blocks_kernel<N, c64, false>            1.45 | 1.15   1.23 | 1.01   1.51 | 0.94
    2  conv_blocks_kernel<N, FMT, true>             1.43 | 1.14   1.65 | 1.03   1.51 | 0.94
    3  conv_blocks_shared_kernel<N, 16, FMT>        2.49 | 1.33   2.13 | 1.52   3.45 | 2.07
    4  conv_blocks_kernel16<N, c64, false>          1.81 | 1.14   1.88 | 1.38   2.63 | 2.33
    5  conv_blocks_kernel16<N, FMT, true>           1.44 | 1.18   2.13 | 1.52   3.45 | 2.33
    6  conv_blocks_generic_fmt                      1.98 | 1.53   1.85 | 1.42   2.35 | 2.24

K = 4 for every form: none needs a factor of its own.  The largest number, 3.45, is a tone block of 512 points (forms
3 and 5 run the same transform passes and measure the same).  106 tests, 20 s of wall time in one visit.

What the bar sees that the older one does not, tried once in a scratch build: with the bins N/2 + 3 and N/2 + 5 swapped
where conv_blocks_shared_kernel copies the filter into LDS, every older GPU test of a convolution passes (the 766 tests
that `-k conv` selects in test_gpu_parity, test_gpu_fft_plans, test_gpu_fullsize and test_gpu_subslices); here every
accuracy case of form 3 fails (19 tests: section A at 256 ... 1024 in all four formats, C at 512, F at 256), in the white-input
walks with every block of a call over the bar."""
import importlib

import numpy as np
import pytest

import conv_ref as cr
from util import SENT, Guarded, bits_equal, zeros

pytestmark = pytest.mark.gpu

RATE, SHIFT = 2_400_000, 3.1e5
TAU = 2.0 * np.pi
RATIOS = {}  # (form, input class) -> [worst max_sample ratio, worst rel_l2 ratio]
CHUNK = 1 << 22  # samples of one checker call (undecimated blocks are independent: a long call is checked in pieces)


@pytest.fixture(scope="module")
def hz():
    return importlib.import_module("go-sdr_amd")


@pytest.fixture(scope="module")
def torch():
    return importlib.import_module("torch")


@pytest.fixture(scope="module")
def ctx(hz, torch):
    c = hz.Context(0, hz.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cus(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count  # (ctx->num_cus)


@pytest.fixture(scope="module", autouse=True)
def report_ratios():
    """Prints what the module measured (`pytest -s`): the table of the docstring."""
    yield
    for (f, cls), (ms, l2) in sorted(RATIOS.items()):
        print("\nRATIO form %d %-9s max_sample %5.2f  rel_l2 %5.2f" % (f, cls, ms, l2), end="")


def check(f, cls, got, xc, H, n, dec=1, what="", want=None):
    """Every block of the call through the bar; the worst ratios go into the module's table."""
    got = np.asarray(got).reshape(-1)
    if dec > 1 or got.shape[0] <= CHUNK:
        rs = [cr.assert_conv_blocks(got, xc, H, n, dec, what=what, want=want)]
    else:
        rows = max(1, CHUNK // n)
        rs = []
        for b0 in range(0, got.shape[0] // n, rows):
            s = slice(b0 * n, (b0 + rows) * n)
            rs.append(cr.assert_conv_blocks(got[s], xc[s], H, n, what="%s blocks %d..." % (what, b0),
                                            want=None if want is None else want[b0:b0 + rows]))
    r = RATIOS.setdefault((f, cls), [0.0, 0.0])
    r[0], r[1] = max([r[0]] + [a for a, _ in rs]), max([r[1]] + [b for _, b in rs])


# ---- running the two entry points -------------------------------------------------------------------------------------

def run_blocks(torch, ctx, x, H, n, off=0, what=""):
    """convolution_blocks over len(x) samples (whole blocks and a partial one) of a guarded c64 slice into another: the
    guards and the input intact, the partial block's output still sentinel.  -> the whole blocks' output"""
    count, nblk = len(x), len(x) // n
    src, out = Guarded(torch, "c64", count, off, x), Guarded(torch, "c64", count, off)
    assert ctx.convolution_blocks(out.t, src.t, torch.from_numpy(np.ascontiguousarray(H)).cuda()) == nblk * n, what
    ctx.synchronize()
    raw = out.check(None, what)[out.lo:out.hi]
    src.check(x, what + " input")
    assert (raw[nblk * n * 8:] == SENT).all(), (what, "the partial block was written")
    return raw[:nblk * n * 8].view(np.complex64).copy()


def stream_of(orc, fmt, raw, stages, ts0=0.0):
    """The complex64 stream as stored behind the elementwise stages, by the oracle's bit-exact operators.
    stages: ("shift", hz) / ("gain", r) / ("rotate", m) in order.  -> (xc, the clock behind the call)"""
    xc = zeros("c64", len(raw))
    if fmt == "c64":
        xc[:] = raw
    else:
        assert orc.convert(xc, np.ascontiguousarray(raw)) == len(raw)
    ts = ts0
    for kind, v in stages:
        if kind == "shift":
            sh = orc.Shifter(RATE)
            sh.ts.value = ts0
            sh(v, xc)
            ts = sh.ts.value
        elif kind == "gain":
            orc.scale(xc, v)
        else:
            orc.rotate(xc, v)
    return xc, ts


def make_chain(hz, torch, ctx, fmt, H, stages, dec, ts0=0.0):
    ch = ctx.chain(getattr(hz, "FMT_" + fmt.upper()), RATE)
    for kind, v in stages:
        ch = ch.shift(v) if kind == "shift" else (ch.gain(v) if kind == "gain" else ch.rotate(v))
    ch = ch.convolution(torch.from_numpy(np.ascontiguousarray(H)).cuda(), decimate=dec)
    if ts0:
        ch.set_time(ts0)
    return ch


def outputs_of(samples, n, dec):
    return samples if dec <= 1 else samples // cr.READER * (cr.READER // dec)


def run_chain(hz, torch, ctx, fmt, raw, H, n, stages=(), dec=1, ts0=0.0, cut=None, off=0, what="", ts_after=None):
    """chain(fmt) [stages] convolution(H, decimate=dec) over the guarded slice `raw` into a guarded slice of EXACTLY
    plan()'s length; `cut`: two run() calls that continue the stream, the first over `cut` samples (whole units).
    plan()'s two numbers, run()'s, the guards, the input and the clock are asserted.  -> the output"""
    count = len(raw)
    ch = make_chain(hz, torch, ctx, fmt, H, stages, dec, ts0)
    cons = cr.whole(count, n, dec)
    outn = outputs_of(cons, n, dec)
    assert ch.plan(count) == (cons, outn), (what, "plan", ch.plan(count), (cons, outn))
    src, out = Guarded(torch, fmt, count, off, raw), Guarded(torch, "c64", outn, off)
    if cut:
        assert 0 < cut < cons and cut % cr.unit(n, dec) == 0
        a = outputs_of(cut, n, dec)
        assert ch.run(src.t[:cut], out.t[:a]) == (cut, a), what
        assert ch.run(src.t[cut:], out.t[a:]) == (cons - cut, outn - a), what
    else:
        assert ch.run(src.t, out.t) == (cons, outn), what
    ctx.synchronize()
    got = out.check(None, what)[out.lo:out.hi].view(np.complex64).copy()
    src.check(raw, what + " input")
    if ts_after is not None:
        assert ch.time() == ts_after, (what, "the clock behind the call", ch.time(), ts_after)
    ch.close()
    return got


def wrap_start(samples):
    """A clock start that puts the 2 pi wrap in the middle of `samples` samples."""
    return TAU - (samples // 2 + 0.5) / RATE


def edge_counts(x):
    return [1, 2, 3] if x == 1 else sorted({1, x - 1, x, x + 1, 2 * x + 1})


# ---- A. walks ---------------------------------------------------------------------------------------------------------

def walk_counts(bpt, xw):
    """Two full trips and a third that ends inside a workgroup and inside a wave's group; exactly one trip; 1; xpw + 1."""
    return [2 * bpt + 5 * xw + max(1, xw - 1), bpt, 1, xw + 1]


@pytest.mark.parametrize("fmt", ["c64", "u8", "i8", "i16"])
@pytest.mark.parametrize("n", [256, 512, 1024])
def test_shared_table_kernel_walks(hz, torch, ctx, orc, cus, n, fmt):
    """Form 3: c64 through convolution_blocks, byte and i16 sources through chain(fmt).convolution(H)."""
    assert cr.form(n, fmt, 0, 1) == 3
    H = cr.allpass(n, n + 1)
    for nblk in walk_counts(cr.blocks_per_trip(3, n, cus), cr.xpw(n)):
        what = "form 3 n=%d %s blocks=%d" % (n, fmt, nblk)
        raw = cr.white(fmt, nblk, n, n * 131 + nblk)
        raw = np.concatenate([raw, raw[:n // 2]])  # (and half a block that nothing consumes)
        if fmt == "c64":
            got, xc = run_blocks(torch, ctx, raw, H, n, what=what), raw
        else:
            got = run_chain(hz, torch, ctx, fmt, raw, H, n, what=what)
            xc, _ = stream_of(orc, fmt, raw, ())
        check(3, "white", got, xc[:nblk * n], H, n, what=what)


@pytest.mark.parametrize("n", [2048, 4096, 8192])
def test_prefetching_kernel_walks(torch, ctx, cus, n):
    """Form 4 at 2048 ... 8192 through convolution_blocks: blockIdx.x, + gridDim.x, ... with the next block in registers."""
    assert cr.form(n, "c64", 0, 1) == 4
    H = cr.allpass(n, n + 2)
    for nblk in walk_counts(cr.blocks_per_trip(4, n, cus), cr.xpb(4, n)):
        what = "form 4 n=%d blocks=%d" % (n, nblk)
        x = cr.white("c64", nblk, n, n * 137 + nblk)
        x = np.concatenate([x, x[:n // 2]])
        check(4, "white", run_blocks(torch, ctx, x, H, n, what=what), x[:nblk * n], H, n, what=what)


@pytest.mark.parametrize("n", [256, 512, 1024])
def test_prefetching_kernel_walks_below_2048_when_decimated(hz, torch, ctx, cus, n):
    """Form 4 at 256 ... 1024 (xpb 4, 2, 1): a c64 chain convolution(H, decimate=8).  A decimated call consumes whole
    lcm(n, 32 Ki) = 32 Ki units: two full trips of the grid and one more unit, plus a ragged rest that plan() refuses."""
    assert cr.form(n, "c64", 0, 8) == 4
    H = cr.allpass(n, n + 3)
    bpt, per_unit = cr.blocks_per_trip(4, n, cus), cr.READER // n
    for units in (2 * bpt // per_unit + 1, bpt // per_unit, 1):
        count = units * cr.READER + 5 * n + n // 2
        what = "form 4 n=%d dec=8 units=%d" % (n, units)
        x = cr.white("c64", -(-count // n), n, n * 139 + units)[:count]
        got = run_chain(hz, torch, ctx, "c64", x, H, n, dec=8, what=what)
        assert len(got) == units * 4096
        check(4, "white", got, x, H, n, 8, what=what)


# ---- B. workgroup edges -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [4, 8, 16, 32, 64, 128])
def test_direct_radix4_kernel_either_side_of_a_workgroup(torch, ctx, n):
    """Form 1: 1, X - 1, X, X + 1 and 2 X + 1 blocks, X = fft_xpb(n)."""
    H = cr.allpass(n, n + 4)
    for nblk in edge_counts(cr.xpb(1, n)):
        what = "form 1 n=%d blocks=%d" % (n, nblk)
        x = cr.white("c64", nblk + 1, n, n * 149 + nblk)[:nblk * n + n // 2]
        check(1, "white", run_blocks(torch, ctx, x, H, n, what=what), x[:nblk * n], H, n, what=what)


STAGED_EDGES = [(2, n, "i16", (("shift", SHIFT), ("gain", 0.5))) for n in (8, 64, 128)] + [(2, n, "u8", ()) for n in (8, 64, 128)] + \
               [(5, n, "u8", (("shift", SHIFT),)) for n in (256, 512, 2048, 8192)] + \
               [(5, 1024, "c64", (("rotate", 0.5 - 0.25j),)), (5, 4096, "i8", ())]


@pytest.mark.parametrize("f,n,fmt,stages", STAGED_EDGES, ids=lambda v: str(v) if isinstance(v, (int, str)) else "+".join(s[0] for s in v) or "bare")
def test_staged_kernels_either_side_of_a_workgroup(hz, torch, ctx, orc, f, n, fmt, stages):
    """Forms 2 and 5 (one workgroup per xpb blocks, staged through LDS): the same counts, in one run() and in two that
    continue the stream; where there is a Shift its clock wraps past 2 pi inside the call."""
    assert cr.form(n, fmt, len(stages), 1) == f
    H = cr.allpass(n, n + 5)
    shifted = any(k == "shift" for k, _ in stages)
    for nblk in edge_counts(cr.xpb(f, n)):
        count = nblk * n + n // 2
        raw = cr.white(fmt, nblk + 1, n, n * 151 + nblk)[:count]
        ts0 = wrap_start(nblk * n) if shifted else 0.0
        xc, ts1 = stream_of(orc, fmt, raw[:nblk * n], stages, ts0)
        if shifted:
            assert ts1 < ts0, "the clock did not wrap inside the call"
        for cut in ((None, (nblk // 2) * n) if nblk > 1 else (None,)):
            what = "form %d n=%d %s blocks=%d cut=%s" % (f, n, fmt, nblk, cut)
            got = run_chain(hz, torch, ctx, fmt, raw, H, n, stages, ts0=ts0, cut=cut, what=what, ts_after=ts1 if shifted else None)
            check(f, "white", got, xc, H, n, what=what)


# ---- C. per-bin read-out ----------------------------------------------------------------------------------------------

GAIN = (("gain", 0.5),)
READOUT = [(1, 64, "c64", (), 1), (2, 64, "c64", GAIN, 1), (3, 512, "c64", (), 1), (4, 512, "c64", (), 8), (5, 512, "c64", GAIN, 1),
           (4, 4096, "c64", (), 1), (5, 4096, "c64", GAIN, 1), (6, 1000, "c64", (), 1), (6, 16384, "c64", (), 1)]
# the impulse class from the byte formats as well, where a form takes them (their conversion is the kernel's own)
READOUT_BYTES = [(2, 64, "i8", (), 1), (2, 64, "i16", GAIN, 1), (3, 512, "i8", (), 1), (3, 512, "i16", (), 1), (5, 512, "i8", GAIN, 1),
                 (5, 4096, "i8", (), 1), (6, 1000, "i16", (), 1)]


def run_any(hz, torch, ctx, f, fmt, raw, H, n, stages, dec, what):
    if fmt == "c64" and not stages and dec == 1:
        return run_blocks(torch, ctx, raw, H, n, what=what)
    return run_chain(hz, torch, ctx, fmt, raw, H, n, stages, dec, what=what)


@pytest.mark.parametrize("f,n,fmt,stages,dec", READOUT, ids=lambda v: str(v) if isinstance(v, (int, str)) else ("gain" if v else "bare"))
def test_tones_read_out_every_bin_through_a_graded_filter(hz, torch, ctx, orc, f, n, fmt, stages, dec):
    """Block b is a tone on bin k_b, the filter has a gain of its own on every bin: min(n, 2048) blocks put every bin
    (above 2048 bins: every k mod 16 in every sixteenth of the spectrum) alone in front of the bar."""
    assert cr.form(n, fmt, len(stages), dec) == f
    nblk = cr.tone_blocks(n)
    cr.assert_tone_coverage(n, nblk)
    assert (nblk * n) % cr.unit(n, dec) == 0
    raw, H = cr.tones(nblk, n), cr.graded(n, n + 6)
    xc, _ = stream_of(orc, fmt, raw, stages)
    what = "form %d n=%d tones dec=%d" % (f, n, dec)
    check(f, "tones", run_any(hz, torch, ctx, f, fmt, raw, H, n, stages, dec, what), xc, H, n, dec, what=what)


@pytest.mark.parametrize("f,n,fmt,stages,dec", READOUT + READOUT_BYTES,
                         ids=lambda v: str(v) if isinstance(v, (int, str)) else ("gain" if v else "bare"))
def test_impulses_read_out_the_filter_against_an_analytic_reference(hz, torch, ctx, orc, f, n, fmt, stages, dec):
    """Block b holds one sample at (7 b + 3) mod n: its output is amp * roll(ifft(H) n, p), every bin of the all-pass
    filter in every sample, the reference analytic."""
    assert cr.form(n, fmt, len(stages), dec) == f
    nblk = cr.tone_blocks(n)
    raw, conv, pos, amps = cr.impulses(fmt, nblk, n)
    H = cr.allpass(n, n + 7)
    xc, _ = stream_of(orc, fmt, raw, stages)
    scale = 0.5 if stages else 1.0  # (Gain 0.5: exact)
    assert bits_equal(xc, (conv * np.float32(scale)).astype(np.complex64)), "the converted impulses are not the expected amplitudes"
    want = cr.pick(cr.impulse_want64(H, n, pos, amps * scale), n, dec)
    what = "form %d n=%d %s impulses dec=%d" % (f, n, fmt, dec)
    check(f, "impulses", run_any(hz, torch, ctx, f, fmt, raw, H, n, stages, dec, what), xc, H, n, dec, what=what, want=want)


@pytest.mark.parametrize("f,n,fmt,stages,dec", [r for r in READOUT if r[4] == 1],
                         ids=lambda v: str(v) if isinstance(v, (int, str)) else ("gain" if v else "bare"))
def test_a_pure_delay_rotates_every_block(hz, torch, ctx, orc, f, n, fmt, stages, dec):
    """delay(n, d), d in {1, n / 2, n - 1}, on white input: the output is the input rotated by d inside its block, per
    sample (the float64 reference is that rotation to the rounding of the filter's bins)."""
    nblk = 2 * cr.xpb(f, n) + 1 if f != 3 else 16 * cr.xpw(n) + cr.xpw(n) + 1
    raw = cr.white(fmt, nblk, n, n + 8)
    xc, _ = stream_of(orc, fmt, raw, stages)
    for d in (1, n // 2, n - 1):
        H = cr.delay(n, d)
        rolled = np.roll(xc.reshape(nblk, n), d, axis=1).astype(np.complex128)
        assert np.abs(cr.want64(xc, H, n) - rolled).max() <= 4e-7 * np.sqrt(n), "the reference is not the rotation"
        what = "form %d n=%d delay %d" % (f, n, d)
        check(f, "white", run_any(hz, torch, ctx, f, fmt, raw, H, n, stages, dec, what), xc, H, n, what=what)


# ---- D. the decimating pick -------------------------------------------------------------------------------------------

PICK = [(2, 64, "i16", GAIN), (4, 512, "c64", ()), (5, 4096, "u8", (("shift", SHIFT),)), (6, 1000, "c64", ()), (6, 65536, "c64", ())]


@pytest.mark.parametrize("dec", [8, 10, 3])
@pytest.mark.parametrize("f,n,fmt,stages", PICK, ids=lambda v: str(v) if isinstance(v, (int, str)) else "+".join(s[0] for s in v) or "bare")
def test_decimating_pick(hz, torch, ctx, orc, f, n, fmt, stages, dec):
    """conv_store's `q * dec == i && q < per` (form 6: chain_decimate_kernel) at a factor that divides 32768 and at two
    that do not, into a guarded slice of exactly plan()'s length: an output q = per lands in the next reader block or
    in the guard.  One sample less of output is refused and leaves the chain as it was."""
    assert cr.form(n, fmt, len(stages), dec) == f
    units = 1 if n == 1000 else 2
    count = units * cr.unit(n, dec) + n // 2 + 1  # (a ragged rest that plan() refuses)
    raw = cr.white(fmt, -(-count // n), n, n * 157 + dec)[:count]
    H = cr.allpass(n, n + 9)
    shifted = any(k == "shift" for k, _ in stages)
    ts0 = wrap_start(count) if shifted else 0.0
    cons = units * cr.unit(n, dec)
    xc, ts1 = stream_of(orc, fmt, raw[:cons], stages, ts0)
    what = "form %d n=%d %s dec=%d" % (f, n, fmt, dec)
    got = run_chain(hz, torch, ctx, fmt, raw, H, n, stages, dec, ts0=ts0, what=what, ts_after=ts1 if shifted else None)
    assert len(got) == cons // cr.READER * (cr.READER // dec)
    check(f, "white", got, xc, H, n, dec, what=what)
    # one sample less: refused, and the next full run is a fresh chain's bit for bit
    ch = make_chain(hz, torch, ctx, fmt, H, stages, dec, ts0)
    src = Guarded(torch, fmt, count, 0, raw)
    short, full = Guarded(torch, "c64", len(got) - 1, 0), Guarded(torch, "c64", len(got), 0)
    with pytest.raises(hz.ErrDstTooSmall):
        ch.run(src.t, short.t)
    ctx.synchronize()
    short.check(None, what + " refused")
    assert (short.bytes() == SENT).all(), (what, "a refused call wrote")
    assert ch.time() == ts0
    assert ch.run(src.t, full.t) == (cons, len(got))
    ctx.synchronize()
    full.check(got, what + " after a refused call")
    ch.close()


# ---- E. independence --------------------------------------------------------------------------------------------------

def poison(n):
    x = cr.white("c64", 1, n, 9)
    x[0] = complex(float("nan"), 1.0)
    x[n // 2] = complex(float("inf"), -1.0)
    x[n - 1] = complex(1e30, 1e30)
    return x


def sampled_blocks(f, n, nblk, bpt):
    """The first, one per trip, every block of the ragged tail, one per sub and per wave."""
    group = cr.xpb(f, n)
    trip = bpt or nblk
    tail = range(nblk - nblk % trip if nblk % trip else nblk - min(nblk, group), nblk)
    per_sub = range(min(nblk, 2 * group))
    per_trip = [t * trip + (7 * t) % group for t in range(-(-nblk // trip))]
    return sorted({0} | set(tail) | set(per_sub) | {b for b in per_trip if b < nblk})


INDEPENDENT = [(1, 16, ()), (2, 64, GAIN), (3, 256, ()), (3, 1024, ()), (4, 2048, ()), (5, 512, GAIN), (6, 12, ()), (6, 1000, ())]


@pytest.mark.parametrize("f,n,stages", INDEPENDENT, ids=lambda v: str(v) if isinstance(v, int) else ("gain" if v else "bare"))
def test_a_block_is_bit_identical_beside_any_neighbours(hz, torch, ctx, cus, f, n, stages):
    """Block b of a long call == the same samples as a one-block call, bit for bit; a block of NaN, Inf and 1e30 in a
    wave (n = 256) and a workgroup of live ones changes no other block's bits; the call run twice gives the same bits."""
    assert cr.form(n, "c64", len(stages), 1) == f
    bpt = cr.blocks_per_trip(f, n, cus)
    group = cr.xpb(f, n)
    nblk = 2 * bpt + 5 * (cr.xpw(n) if f == 3 else group) + 1 if bpt else 4 * group + 3
    H = cr.graded(n, n + 10)
    x = cr.white("c64", nblk, n, n + 11)
    what = "form %d n=%d blocks=%d" % (f, n, nblk)
    run = (lambda v, w: run_any(hz, torch, ctx, f, "c64", v, H, n, stages, 1, w))
    clean = run(x, what).reshape(nblk, n)
    assert bits_equal(run(x, what + " again").reshape(nblk, n), clean), (what, "a second call gives other bits")
    assert np.isfinite(clean.view(np.float32)).all()
    # (the poisoned block: the second of a wave's group / of a workgroup, and one in the last trip)
    bad = sorted({1 % nblk, nblk - 2})
    xp = x.reshape(nblk, n).copy()
    for b in bad:
        xp[b] = poison(n)
    dirty = run(xp.reshape(-1), what + " poisoned").reshape(nblk, n)
    keep = np.ones(nblk, bool)
    keep[bad] = False
    assert not np.isfinite(dirty[bad].view(np.float32)).all(axis=1).any(), (what, "a poisoned block came out finite")
    diff = np.flatnonzero((dirty[keep].view(np.uint64) != clean[keep].view(np.uint64)).any(axis=1))
    assert diff.size == 0, (what, "blocks changed by a poisoned neighbour", np.flatnonzero(keep)[diff][:8])
    for b in sampled_blocks(f, n, nblk, bpt):
        alone = run(x[b * n:(b + 1) * n].copy(), what + " block %d alone" % b)
        if not bits_equal(alone, clean[b]):
            d = np.flatnonzero(alone.view(np.uint64) != clean[b].view(np.uint64))
            raise AssertionError("%s: block %d differs from the same samples as a one-block call in %d of %d samples, the "
                                 "first at %d" % (what, b, d.size, n, d[0]))


# ---- F. off alignment -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("f,n,fmt,stages", [(2, 64, "i16", GAIN), (2, 64, "u8", ()), (3, 256, "c64", ()), (3, 256, "i8", ()), (4, 2048, "c64", ()),
                                            (5, 512, "u8", (("shift", SHIFT),)), (5, 2048, "i16", ())],
                         ids=lambda v: str(v) if isinstance(v, (int, str)) else "+".join(s[0] for s in v) or "bare")
def test_sub_slices_one_sample_off_alignment(hz, torch, ctx, orc, f, n, fmt, stages):
    """What a Go caller's buf[1:] hands over: c64 input and output 8 bytes past 16-byte alignment; byte and i16 inputs
    one sample past pair alignment (stage_block's vec_ok == false leg).  The same bar, the guards intact."""
    assert cr.form(n, fmt, len(stages), 1) == f
    group = cr.xpb(f, n)
    nblk = 2 * group + 1
    raw = cr.white(fmt, nblk + 1, n, n + 12)[:nblk * n + n // 2]
    H = cr.allpass(n, n + 13)
    xc, _ = stream_of(orc, fmt, raw[:nblk * n], stages)
    what = "form %d n=%d %s off=1" % (f, n, fmt)
    if fmt == "c64" and not stages:
        got = run_blocks(torch, ctx, raw, H, n, off=1, what=what)
    else:
        got = run_chain(hz, torch, ctx, fmt, raw, H, n, stages, off=1, what=what)
    check(f, "white", got, xc, H, n, what=what)


# ---- G. the generic form ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,nblk", [(1000, (1 << 25) // 2048 + 7), (16384, 3), (1, 37), (2, 37), (3, 37), (12, 37)])
def test_generic_form_every_block(torch, ctx, n, nblk):
    """conv_blocks_generic_fmt: 1000 bins (M = 2048, pieces of 16384 blocks) over a piece and 7 blocks; 16384 bins (the
    two-step transform) over 3; the shortest lengths.  Every block goes through the bar."""
    assert cr.form(n, "c64", 0, 1) == 6
    H = cr.allpass(n, n + 14)
    x = cr.white("c64", nblk + 1, n, n + 15)[:nblk * n + n // 2]
    what = "form 6 n=%d blocks=%d" % (n, nblk)
    check(6, "white", run_blocks(torch, ctx, x, H, n, what=what), x[:nblk * n], H, n, what=what)


# ---- H. host memory ---------------------------------------------------------------------------------------------------

def test_host_context_gives_the_device_contexts_bits(hz, torch, ctx):
    n, nblk = 64, 9
    H = cr.graded(n, 16)
    x = cr.white("c64", nblk + 1, n, 17)[:nblk * n + n // 2]
    host = hz.Context(0, hz.MEM_HOST)
    out = np.full(len(x), np.complex64(7.0))
    assert host.convolution_blocks(out, x.copy(), H) == nblk * n
    host.close()
    assert (out[nblk * n:] == np.complex64(7.0)).all(), "the partial block was written"
    check(1, "white", out[:nblk * n], x[:nblk * n], H, n, what="host")
    assert bits_equal(out[:nblk * n], run_blocks(torch, ctx, x, H, n, what="device"))

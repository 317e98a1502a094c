"""The overlap-save FIR-decimate (the transform form of the chain terminal) per block, at form, call, run and slow-list
edges: through Chain.run in a device context, every output a guarded slice of exactly plan()'s length.

fir_run (csrc/hz_chain_fir.hip) instantiates fir_decimate_kernel16<N, FMT, FOLD, LATE> and fir_synth_kernel16<N, FOLD,
LATE> for 19 forms (N, FOLD) x two mixer orders x four source formats (tests/fir_ref.py restates the dispatch;
fir_decimate_kernel, the radix-4 predecessor in csrc/hz_chain_dev.h, is no longer launched by anything).  What the
older tests of it share -- test_gpu_parity.py::test_chain_fir_decimate_overlap_save, test_gpu_latemix.py,
test_gpu_fir_fuzz.py, the transform cases of test_gpu_firmm.py -- is a windowed-sinc low-pass, white input, ONE bound
over a whole call and call lengths that are powers of two, multiples of 1000 D or random.  By the geometry of their
fixed case tables (the fuzz seeds left aside, which reach a form by chance): no fixed case has N = 8192 with FOLD 0, 2 or 4 or N = 4096
with FOLD 4 at all; N = 8192 with FOLD 8, N = 4096 with FOLD 0 and N = 2048 with FOLD 0 occur only as matrix-eligible
byte chains of test_gpu_firmm.py, which take the transforms where a call falls back to them.  None runs a call of
exactly k hop samples or hop +- D, a call shorter than `off` (let alone several in a row), or n = D; a binade edge or
the 2 pi wrap meets a block edge only by luck; and with at most 2047 taps no slow list has more than about a dozen
entries: the upper half of the ballot and the give-up above 96 entries never ran.

The bar here (fir_ref.assert_fir_blocks), on EVERY overlap-save block of every call, nothing sampled:

    m_b(kernel) <= K * max(m_b(yardstick), 2**-23)    for m in (max_sample, l2),    K = util.FFT_K = 4

both over sum|h| * max|x|, against y[m] = sum_k h[k] x[D m - k] in float64 over the stream as stored behind the
elementwise stages (the oracle's bit-exact convert, Shift, scale and rotate), the yardstick the same block in complex64.
Filters are graded (white complex taps), ends-only or a pure delay, never a low-pass; inputs white or impulses.

Sections and the forms (N, FOLD) each runs:

    A  every form in both mixer orders, graded x white and ends-only x impulses, formats rotated; N = 256 and 512 at
       1, X - 1, X, X + 1 and 2 X + 1 blocks                                                        all 19 forms
    B  calls of D, hop - D, hop, hop + D, 2 hop, 3 hop, off - D, off, off + D, one with n % D != 0, seven shorter than
       off / 3 and a long one, as ONE stream; reset() and a fresh chain                            (1024, 0) (1024, 2) (2048, 4) (2048, 8) (4096, 16)
    C  the binade edge at 1 s on the five places around a middle block's span and around n - off - N, both orders; the
       2 pi wrap inside a call; a call of more than 32 runs                                        (1024, 0) (2048, 4) (4096, 16) (8192, 0)
    D  every class of the slow list (none, 1-4, 5-64, 65-96, given up) with rest % 8 in {0, 1, 7}, and rest < 8
                                                    (1024, 0) (1024, 4) (2048, 2) (2048, 4) (2048, 8) (4096, 0) (4096, 16) and all five folds at 8192

Measured on an MI355X (`pytest -s` prints the table when the module ends):
    worst ratio kernel / max(yardstick, 2^-23), max_sample | l2, over all sections:

    form (N, FOLD)    white         impulses
    ( 256,  0)        0.31 | 0.95   0.50 | 0.73
    ( 512,  0)        0.25 | 1.12   0.36 | 0.66
    (1024,  0)        1.45 | 1.18   0.46 | 0.87
    (1024,  2)        1.34 | 1.11   0.60 | 1.02
    (1024,  4)        0.24 | 1.04   0.23 | 0.32
    (2048,  0)        0.22 | 1.12   0.48 | 0.65
    (2048,  2)        0.18 | 1.00   0.25 | 0.47
    (2048,  4)        1.08 | 1.08   0.38 | 0.75
    (2048,  8)        1.43 | 1.09   0.50 | 0.59
    (4096,  0)        0.18 | 1.17   0.56 | 0.74
    (4096,  2)        0.13 | 1.02   0.79 | 1.17
    (4096,  4)        0.16 | 0.98   0.23 | 0.32
    (4096,  8)        0.13 | 0.87   0.42 | 0.69
    (4096, 16)        1.58 | 1.05   0.56 | 0.67
    (8192,  0)        0.15 | 1.12   0.40 | 0.63
    (8192,  2)        0.11 | 1.11   0.23 | 0.50
    (8192,  4)        0.14 | 1.12   0.37 | 0.71
    (8192,  8)        0.11 | 1.03   0.23 | 0.38
    (8192, 16)        0.11 | 0.74   0.40 | 0.49

K = 4 for every form: none needs a factor of its own, and no test found a fault in the kernels.  (A max_sample ratio
below 1 is the floor's doing: over sum|h| * max|x| a single sample's error of a white filter lies under 2^-23, and it
is the l2 number that carries those cases.)  78 tests, 3.2 s of wall time for the whole module in one visit, the
slowest test 0.33 s.

What a wrong value costs, tried once in a scratch build: in fir_decimate_kernel16's transform path (every FOLD 0 form
and the four folds of N = 8192; the polyphase forms do not pass there) lane 5's spectrum slots 4 and 4 + 16 / FOLD --
two bins that fold onto one output bin -- exchanged in front of the filter multiply, registers only.  Of the older
tests (test_gpu_latemix, test_gpu_parity -k fir_decimate, test_gpu_fir_fuzz, test_gpu_firmm: 169 tests) 131 still pass;
the 38 that fail are the fixed cases at (256, 0), (512, 0), (1024, 0) and (8192, 16) -- test_small_overlap_save_blocks
x 4, test_chain_fir_decimate_overlap_save[129-10], [1-1] and [2048-16] on both contexts -- and 28 runs of the two
fuzzers (18 seeds); no older fixed case fails for (2048, 0), (4096, 0), (8192, 0), (8192, 2), (8192, 4) or (8192, 8),
because none runs them.  Here 45 of the 78 tests fail: section A
for all ten planted forms (the six FOLD 0 forms with every block count of N = 256 and 512, and N = 8192 with FOLD 2,
4, 8 and 16 in every format), and every case of B, C and D that runs one of them; the 33 that pass run polyphase
forms only."""
import importlib

import numpy as np
import pytest

import fir_ref as fr
from util import Guarded, bits_equal

pytestmark = pytest.mark.gpu

RATIOS = {}  # ((N, FOLD), input class) -> [worst max_sample ratio, worst l2 ratio]


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


@pytest.fixture(scope="module", autouse=True)
def report_ratios():
    """Prints what the module measured (`pytest -s`): the table of the docstring."""
    yield
    for (f, cls), (ms, l2) in sorted(RATIOS.items()):
        print("\nRATIO form %-10s %-9s max_sample %5.2f  l2 %5.2f" % (f, cls, ms, l2), end="")


def make_chain(hz, ctx, fmt, rate, stages, h, g, nfft_min, in_order=False, ts0=0.0):
    ch = ctx.chain(getattr(hz, "FMT_" + fmt.upper()), rate)
    for kind, v in stages:
        ch = ch.shift(v) if kind == "shift" else (ch.gain(v) if kind == "gain" else ch.rotate(v))
    ch.fir_options(impl=hz.FIR_IMPL_TRANSFORMS, nfft_min=nfft_min)  # (byte sources: not the matrix form)
    ch.fir_decimate(h, g.D)
    ch.mix_in_order(in_order)
    if ts0:
        ch.set_time(ts0)
    return ch


def run_call(hz, torch, ctx, ch, fmt, raw, g, what):
    """One run() over the guarded slice `raw` into a guarded slice of exactly plan()'s length: the counts, the path,
    the guards and the input asserted.  -> (samples consumed, the output)"""
    n = len(raw)
    cons, outn = n // g.D * g.D, n // g.D
    assert ch.plan(n) == (cons, outn), (what, "plan", ch.plan(n))
    src, out = Guarded(torch, fmt, n, 0, raw), Guarded(torch, "c64", outn, 0)
    assert ch.run(src.t, out.t) == (cons, outn), what
    ctx.synchronize()
    assert ch.last_fir_path() == hz.FIR_PATH_TRANSFORM, what
    got = out.check(None, what)[out.lo:out.hi].view(np.complex64).copy()
    src.check(raw, what + " input")  # (the samples behind n // D * D, which the call leaves for the next, among them)
    return cons, got


def check(g, cls, got, xc, a, b, h, xmax, what):
    """The call over xc[a:b] of a stream through the bar; the worst ratios go into the module's table."""
    want = fr.want64(xc[a:b], h, g.D, xc[:a])
    yard = fr.yardstick32(g, xc[a:b], h, xc[:a])
    r = fr.assert_fir_blocks(got, want, yard, h, xmax, g, what=what)
    t = RATIOS.setdefault((fr.form(g)[:2], cls), [0.0, 0.0])
    t[0], t[1] = max(t[0], r[0]), max(t[1], r[1])


def run_stream(hz, torch, ctx, orc, c, h, raw, lens, cls, in_order=False, what=""):
    """A chain of case c over the stream `raw` in calls of `lens` samples (a call consumes n // D * D of them and the
    next begins behind those), every call through the bar.  -> [the outputs of every call]"""
    g = c["g"]
    ch = make_chain(hz, ctx, c["fmt"], c["rate"], c["stages"], h, g, c["nfft_min"], in_order, c["ts0"])
    xc = fr.stream_of(orc, c["fmt"], raw, c["stages"], c["rate"], c["ts0"])
    xmax = float(np.abs(xc).max())
    a, outs = 0, []
    for i, n in enumerate(lens):
        w = "%s %s order call %d of %d samples at %d" % (what, "reference" if in_order else "late", i, n, a)
        cons, got = run_call(hz, torch, ctx, ch, c["fmt"], raw[a:a + n], g, w)
        check(g, cls, got, xc, a, a + cons, h, xmax, w)
        outs.append(got)
        a += cons
    ch.close()
    return outs


def ident(c):
    return "N%d-F%d-%s" % (c["N"], c["fold"], c["fmt"]) + ("-b%d" % c["blocks"] if "blocks" in c else "")


# ---- A. forms ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", fr.form_cases() + fr.small_block_cases(), ids=ident)
def test_every_form_in_both_mixer_orders(hz, torch, ctx, orc, c):
    """Five blocks and a ragged sixth (N = 256, 512: around a workgroup's worth): graded taps x white input and
    ends-only taps x one impulse per block, both mixer orders."""
    g, n = c["g"], c["n"]
    assert fr.form(g)[:2] == (c["N"], c["fold"])
    seed = c["N"] + 31 * c["fold"] + fr.FMTS.index(c["fmt"])
    for in_order in (False, True):
        p = fr.plan_call(hz, g, c["rate"] if c["stages"][0][0] == "shift" else 0, c["ts0"], n, in_order)
        if not in_order and c["N"] >= 1024:
            assert any(p["late"]) and not all(p["late"]), "blocks of both kinds in the call"
        run_stream(hz, torch, ctx, orc, c, fr.graded_taps(g.ntaps, seed), fr.white(c["fmt"], n, seed + 1), [n], "white", in_order, ident(c))
        run_stream(hz, torch, ctx, orc, c, fr.ends_taps(g.ntaps), fr.impulse_input(c["fmt"], n, fr.block_places(g, n, 3)), [n], "impulses",
                   in_order, ident(c) + " ends")


@pytest.mark.parametrize("N,fold,fmt,D", fr.EDGE_FORMS, ids=lambda v: str(v))
def test_pure_delays(hz, torch, ctx, orc, N, fold, fmt, D):
    """A single tap at 0, 1, ntaps / 2, ntaps - 2 and ntaps - 1 on white input: the output is the input, delayed."""
    g, nmin = fr.geom_for(N, fold, None, D)
    n = 3 * g.hop + g.hop // 2 // D * D
    c = dict(N=N, fold=fold, fmt=fmt, g=g, nfft_min=nmin, stages=(), rate=0, ts0=0.0)
    raw = fr.white(fmt, n, N + 5)
    for k0 in fr.delay_places(g.ntaps):
        run_stream(hz, torch, ctx, orc, c, fr.delay_taps(g.ntaps, k0), raw, [n], "white", False, "delay %d" % k0)


# ---- B. call edges -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("in_order", [False, True], ids=["late", "reference"])
@pytest.mark.parametrize("i", range(len(fr.EDGE_FORMS)), ids=lambda i: "N%d-F%d-%s" % fr.EDGE_FORMS[i][:3])
def test_call_lengths_and_histories(hz, torch, ctx, orc, i, in_order):
    """ONE stream in calls of D, hop - D, hop, hop + D, 2 hop, 3 hop, off - D, off, off + D, hop + D + 1 (n % D != 0: the
    call consumes hop + D and the next begins behind that), seven calls shorter than off / 3 (history built from history
    three times over) and a long one; white input through graded taps, then impulses on the last sample before every
    cut and the first behind it through ends-only taps.  reset() and a fresh chain reproduce the first call's bits."""
    N, fold, fmt, D = fr.EDGE_FORMS[i]
    g, nmin = fr.geom_for(N, fold, None, D)
    first, tail = fr.call_lengths(g)
    lens = first + [g.hop + D + 1] + tail
    cuts = np.cumsum([0] + [v // D * D for v in lens])
    total = int(cuts[-1]) + D
    c = dict(N=N, fold=fold, fmt=fmt, g=g, nfft_min=nmin, stages=fr.SHIFT_GAIN if i % 2 == 0 else (), rate=fr.RATE, ts0=1.3 if i % 2 == 0 else 0.0)
    what = "N%d F%d %s" % (N, fold, fmt)
    h = fr.graded_taps(g.ntaps, N + i)
    raw = fr.white(fmt, total, N + i + 1)
    outs = run_stream(hz, torch, ctx, orc, c, h, raw, lens, "white", in_order, what)
    run_stream(hz, torch, ctx, orc, c, fr.ends_taps(g.ntaps), fr.impulse_input(fmt, total, fr.cut_places([int(v) for v in cuts])), lens, "impulses",
               in_order, what + " ends")
    # reset() reproduces the first calls bit for bit, and so does a fresh chain
    ch = make_chain(hz, ctx, fmt, c["rate"], c["stages"], h, g, nmin, in_order, c["ts0"])
    for rounds in range(2):
        a = 0
        for k in range(4):
            cons, got = run_call(hz, torch, ctx, ch, fmt, raw[a:a + lens[k]], g, what + " again")
            assert bits_equal(got, outs[k]), (what, "call %d differs %s" % (k, "after reset()" if rounds else "on a fresh chain"))
            a += cons
        ch.reset()
        if c["ts0"]:
            ch.set_time(c["ts0"])
    ch.close()


# ---- C. run edges ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1024, 2048, 4096, 8192])
def test_a_binade_edge_on_every_place_around_a_span(hz, torch, ctx, orc, N):
    """The clock's run boundary at 1 s on p0 - 1, p0, p0 + 1, p0 + N - 1 and p0 + N of a middle block and of the last
    span inside the call, both mixer orders: late_block and slow_blocks compare at equality."""
    cases = [c for c in fr.run_edge_cases(hz) if c["N"] == N]
    assert len(cases) == 10
    g, n = cases[0]["g"], cases[0]["n"]
    h = fr.graded_taps(g.ntaps, N + 7)
    raw = fr.white(cases[0]["fmt"], n, N + 8)
    for c in cases:
        p = fr.plan_call(hz, g, c["rate"], c["ts0"], n)
        assert [r[0] for r in p["runs"]] == [0, c["edge"]] and any(p["late"])
        for in_order in (False, True):
            run_stream(hz, torch, ctx, orc, c, h, raw, [n], "white", in_order, "edge %s%+d" % c["where"])


@pytest.mark.parametrize("N,fold,fmt", [(1024, 0, "i16"), (2048, 8, "u8"), (8192, 4, "c64")])
def test_the_2_pi_wrap_inside_a_call(hz, torch, ctx, orc, N, fold, fmt):
    """The short runs behind the wrap have no filter: their blocks, and the two that straddle a boundary, stay on the
    reference order."""
    c = fr.find_case(hz, N, fold, "5-64" if N < 8192 else "given_up", 1)
    c.update(N=N, fold=fold, fmt=fmt, stages=(("shift", 3.1e5), ("gain", 0.5)))
    g, n, p = c["g"], c["n"], c["plan"]
    assert c["scenario"] == "wrap" and len(p["runs"]) > 10 and not all(p["has"]) and any(p["late"])
    assert any(b[2] < a[2] for a, b in zip(p["runs"], p["runs"][1:])), "the clock wraps inside the call"
    h = fr.graded_taps(g.ntaps, N + 9)
    for in_order in (False, True):
        run_stream(hz, torch, ctx, orc, c, h, fr.white(fmt, n, N + 10), [n], "white", in_order, "wrap")


def test_neighbouring_runs_have_their_own_taps(hz, torch, ctx, orc):
    """20 Msps, a Shift of 8 MHz, 2047 taps, the binade edge at 4 s on a block's first sample: the steps of the two
    runs differ by 2^-51 s, a phase slip of 2e-5 rad at the last tap if a block took the other run's spectrum -- 34 x
    over the bar in tests/test_fir_ref_cpu.py's model, and invisible at the rates and tap counts of the other cases."""
    rate = 20_000_000
    g, nmin = fr.geom_for(8192, 0, 2047, 1)
    n = 6 * g.hop + g.N
    ts0 = fr.edge_start(hz, rate, 4.0, g.p0(4), n)
    c = dict(N=8192, fold=0, fmt="c64", g=g, nfft_min=nmin, stages=(("shift", 8.0e6),), rate=rate, ts0=ts0)
    p = fr.plan_call(hz, g, rate, ts0, n)
    assert [r[0] for r in p["runs"]] == [0, g.p0(4)] and p["runs"][0][3] != p["runs"][1][3] and p["has"] == [True, True]
    assert p["late"] == [False, True, True, False, True, True, True, False]
    run_stream(hz, torch, ctx, orc, c, fr.graded_taps(2047, 6), fr.white("c64", n, 5), [n], "white", False, "two runs")


def test_more_than_32_runs_stay_on_the_reference_order(hz, torch, ctx, orc):
    """A clock so slow that one call holds two wraps: 40 runs, the device-table form of the clock.  No block mixes late:
    the default order gives the reference order's bits."""
    g, nmin = fr.geom_for(1024, 4)
    n = fr.SLOW_N // g.D * g.D
    c = dict(N=1024, fold=4, fmt="c64", g=g, nfft_min=nmin, stages=(("shift", 310.0),), rate=fr.SLOW_RATE, ts0=0.0)
    p = fr.plan_call(hz, g, c["rate"], 0.0, n)
    assert len(p["runs"]) > fr.MAX_RUNS and p["has"] is None and not any(p["late"])
    assert max(r[1] for r in p["runs"]) >= 2 * g.N, "long runs there are: it is the table's form that keeps the order"
    h, raw = fr.graded_taps(g.ntaps, 11), fr.white("c64", n, 12)
    outs = [run_stream(hz, torch, ctx, orc, c, h, raw, [n], "white", in_order, "40 runs")[0] for in_order in (False, True)]
    assert bits_equal(outs[0], outs[1])


# ---- D. the slow list --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(16), ids=["%s-rest%d" % (cls, r) for cls in fr.CLASSES for r in (0, 1, 7)] + ["rest-below-8"])
def test_every_class_of_the_slow_list(hz, torch, ctx, orc, k):
    """No list, the scalar scan (1 ... 4 entries), the ballot's lower half (5 ... 64), its upper half (65 ... 96) and
    the give-up above 96, each with the rest of the blocks 0, 1 and 7 mod 8 over the eight runs they are dealt in."""
    c = fr.slow_cases(hz)[k]
    g, n = c["g"], c["n"]
    p = fr.plan_call(hz, g, c["rate"], c["ts0"], n)
    assert p["cls"] == c["cls"] and p["has"] is not None, "the LATE kernel with the class the case is named for"
    count = len(p["slow"])
    assert {"none": count == 0, "1-4": 1 <= count <= 4, "5-64": 5 <= count <= 64, "65-96": 65 <= count <= 96, "given_up": count == 0}[c["cls"]]
    assert (p["rest"] < 8) if c["residue"] is None else (p["rest"] % 8 == c["residue"])
    assert any(p["late"]) and (c["cls"] == "none" or not all(p["late"]))
    hit = sorted(b for b in (fr.block_of_workgroup(g, n, p["slow"], i) for i in range(fr.grid_of(g, n, p["slow"], True))) if b is not None)
    assert hit == list(range(g.nblocks(n)))
    run_stream(hz, torch, ctx, orc, c, fr.graded_taps(g.ntaps, 100 + k), fr.white(c["fmt"], n, 200 + k), [n], "white", False,
               "slow list %s (%d entries, rest %d)" % (c["cls"], count, p["rest"]))
    if k % 5 == 0:
        run_stream(hz, torch, ctx, orc, c, fr.ends_taps(g.ntaps), fr.impulse_input(c["fmt"], n, fr.block_places(g, n, 1)), [n], "impulses", False,
                   "slow list %s ends" % c["cls"])

"""The chains without a FIR or convolution terminal, per program, vector width and clock run: chain_map_kernel,
chain_decimate_kernel and chain_downsample_kernel (csrc/hz_chain_dev.h) through launch_map and run_fmt
(csrc/hz_chain.hip), against tests/chain_ref.py -- the oracle's separate operations, bit for bit.  Every device
comparison is util.Guarded.check: the slice byte for byte and both guards intact; a failure adds chain_ref.first_diff's
line (the sample, its W, tile and lane, its clock run).

What the older tests leave open: [Shift] and [Shift, Gain] have kernels of their own (shift_exact_kernel, the *_ULP1
shapes) and carry test_shift_*, test_map_chain_subslices and the pipelined-map cases; the INTERPRETED program
(SHAPE_ANY: ew_apply_n<W> in the map, the rolled ew_apply in the terminals) ran through the map once, aligned, at one
length, with two stages.  Here: nine programs (none, one, two, three and the limit of six stages; a gain in front of
a Shift; two Shifts on one clock; gains that are no powers of two and rotations off both axes, so that a wrong order
shows; rotate(1 + 0j), which the library drops) x four source formats x six (source, destination) offsets that reach
W = 4, W = 2 and W = 1 x lengths with tails of 0 to 3 samples and ragged tiles; ten clocks that put one run, a binade
edge, the 2 pi wrap (late, in the first tile, three samples before a tile's end, at 200 MHz), a fresh stream and a device
table of 48 and of 222 runs under the tiles (nco_ts's scan, inline search and table branch; chain_ref.clock_cases,
each asserted before it runs);
the clock after every call, across three calls, in a HOST context, under shift_ulp1 and behind the refused seventh
stage.  Decimate and Downsample: four programs x four formats x factors 1, 2, 3, 10, 4096, 32767 and 32768 x four
clocks over 3 * 32768 + 1234 samples, into guarded outputs longer than needed; plan() against run(); calls below a
block; two calls whose clock must advance over the CONSUMED samples; decimate(1) against the map; a c64 block of -0,
Inf and NaN; the refusals.  The pipelined map (hzsdr_chain_pipeline + run_after) over three rotating buffer pairs, and
once with the 222-run clock, which takes run_fmt's draining path.

tests/test_chain_ref_cpu.py proves on the CPU that these inputs see every planted fault (swapped stages, a tail's
clock from 0, a neighbouring run's line, a tile's first run only, the dropped rotation applied, a pick off by one, a
sum from -0 or in reverse, a clock advanced over the offered samples) in at least three outputs.

Left out: the second trip of the map's grid-stride loop.  blocks_for gives a call as many workgroups as it has tiles
up to a cap that a call of less than 2^25 samples does not reach; a test of that size does not belong in a suite that
runs for every change.  tests/test_gpu_subslices.py's 2^24 + 3 sample cases are the nearest.

What a wrong value costs, tried in scratch builds on the MI355X (145 tests):
    the W = 1 tail launched with base = 0 (csrc/hz_chain.hip)            68 of the then 141 fail: every map test that has a
                                                                         tail behind a vector body; no terminal test
    Downsample's sum started at -0 (csrc/hz_chain_dev.h)                 11 fail: the -0 block at all four factors, and the
                                                                         c64 and i8 streams, whose zeros sum to -0 by 1
    nco_ts's scan taking a run from `j > first` (csrc/hz_nco.h)          8 fail: wrap_at_tile_end in all four formats, in
                                                                         one call and in three -- and nothing else: on a
                                                                         binade edge the boundary sample lies on the
                                                                         previous run's line too, only the wrap tells, and
                                                                         only where a tile holds at most four runs.  That
                                                                         clock case was added for it.
The first failure names its sample: "3 of 1500 samples differ, the first at 1021: W = 4, tile 0, lane 255, slot 1,
clock run 1 of 12 (first 1021)".  No test found a fault in the kernels as they are.

Measured on an MI355X, the module alone: 145 tests in 6.2 s of wall time, 1.7 s of it the first context.  The slowest
test 0.35 s (test_terminal_per_factor_and_clock[*-downsample-gain_shift_rotate]: 28 calls of 98 304 samples), a map
test 0.12 s."""
import importlib

import numpy as np
import pytest

import chain_ref as cr
from test_gpu_subslices import ULP1_BOUND, _close_to_factor
from util import SENT, Guarded

pytestmark = pytest.mark.gpu

B = cr.B
PROGRAM_NAMES = tuple(cr.programs())
SHIFTED = tuple(k for k, p in cr.programs().items() if cr.has_shift(p))
ONE_RUN = cr.clock_cases()[0]
CASES = {c["name"]: c for c in cr.clock_cases()}
TCASES = {c["name"]: c for c in cr.terminal_clock_cases()}


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
def host(hz):
    c = hz.Context(0, hz.MEM_HOST)
    yield c
    c.close()


# ---- helpers -------------------------------------------------------------------------------------------------------------

def build(hz, ctx, fmt, rate, program, term=None, factor=0):
    ch = ctx.chain(getattr(hz, "FMT_" + fmt.upper()), rate)
    for kind, v in program:
        ch = ch.shift(v) if kind == "shift" else (ch.gain(v) if kind == "gain" else ch.rotate(v))
    if term:
        ch = ch.decimate(factor) if term == "decimate" else ch.downsample(factor)
    return ch


_WANT = {}


def want_of(orc, fmt, name, case, n, terminal=False, start=0, ts0=None):
    """chain_ref.want of samples [start, start + n) of the format's stream, computed once and left read-only."""
    ts0 = case["ts0"] if ts0 is None else ts0
    key = (fmt, name, terminal, case["rate"], case["shift"], ts0, n, start)
    if key not in _WANT:
        p = (cr.terminal_programs if terminal else cr.programs)(case["shift"])[name]
        w, te = cr.want(orc, fmt, cr.inputs(fmt, n, start), p, case["rate"], ts0)
        w.flags.writeable = False
        _WANT[key] = (w, te)
    return _WANT[key]


def sentinel(n):
    return np.full(n * 8, SENT, np.uint8).view(np.complex64)


def check(d, want, what, widths=None, runs=()):
    try:
        d.check(want, what)
    except AssertionError as e:
        if widths is None or len(want) != d.n:
            raise
        raise AssertionError("%s | %s" % (e, cr.first_diff(d.values(), want, widths, list(runs)))) from None


def run_map(hz, torch, ctx, orc, ch, fmt, name, case, n, so, do, ulp1=False):
    """One call of a map chain over guarded slices from the case's clock -> the destination, checked."""
    x = cr.inputs(fmt, n)
    w, te = want_of(orc, fmt, name, case, n)
    s, d = Guarded(torch, fmt, n, so, x), Guarded(torch, "c64", n, do)
    ch.set_time(case["ts0"])
    assert ch.run(s.t, d.t) == (n, n)
    assert ch.time() == te, (fmt, name, case["name"], n, ch.time(), te)
    widths = cr.map_widths(so * cr.RAW[fmt], do * 8, fmt, n, cr.programs()[name], ulp1)
    runs = cr.clock_runs(hz, case["rate"], case["ts0"], n) if name in SHIFTED else []
    check(d, w, ("map", fmt, name, case["name"], "src@%d dst@%d" % (so, do), "n=%d" % n), widths, runs)
    s.check(x, "map source")
    return d


lengths_of = cr.clock_lengths


# ---- the map, interpreted programs -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", PROGRAM_NAMES)
@pytest.mark.parametrize("fmt", cr.FMTS)
def test_map_program_at_every_offset_and_length(hz, torch, ctx, orc, fmt, name):
    """One clock run (1 s at 20 MHz): every width, tail and ragged tile of launch_map."""
    ch = build(hz, ctx, fmt, ONE_RUN["rate"], cr.programs()[name])
    try:
        for n in cr.LENGTHS:
            for so, do in cr.OFFSETS:
                run_map(hz, torch, ctx, orc, ch, fmt, name, ONE_RUN, n, so, do)
    finally:
        ch.close()


@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
@pytest.mark.parametrize("fmt", cr.FMTS)
def test_map_clock_case(hz, torch, ctx, orc, fmt, case):
    """Every program with a Shift under every clock: the class is asserted first (a drift of hzsdr_nco_segments shows
    here, not as a case that quietly tests something else)."""
    c = CASES[case]
    count, most, cls = cr.classify(hz, c["rate"], c["ts0"], c["n"])
    assert (cls, cr.class_of(most)) == (c["cls"], c["tile"]), (case, count, most)
    offsets = cr.OFFSETS if c["n"] <= cr.N_MAP else ((0, 0), (2, 2), (1, 0))
    for name in SHIFTED:
        ch = build(hz, ctx, fmt, c["rate"], cr.programs(c["shift"])[name])
        try:
            for n in lengths_of(c):
                for so, do in offsets:
                    x = cr.inputs(fmt, n)
                    w, te = want_of(orc, fmt, name, c, n)
                    s, d = Guarded(torch, fmt, n, so, x), Guarded(torch, "c64", n, do)
                    ch.set_time(c["ts0"])
                    assert ch.run(s.t, d.t) == (n, n)
                    assert ch.time() == te, (fmt, name, case, n)
                    widths = cr.map_widths(so * cr.RAW[fmt], do * 8, fmt, n, cr.programs()[name])
                    check(d, w, ("map", fmt, name, case, "src@%d dst@%d" % (so, do), "n=%d" % n), widths,
                          cr.clock_runs(hz, c["rate"], c["ts0"], n))
        finally:
            ch.close()


@pytest.mark.parametrize("fmt", cr.FMTS)
def test_map_clock_carries_across_three_calls(hz, torch, ctx, orc, fmt):
    """4099 samples as calls of 1366, 1367 and 1366: the outputs of one call over the buffer, the clock after each
    call the reference's (the later calls start 2 and 1 samples off the vector grid)."""
    x = cr.inputs(fmt, cr.N_MAP)
    for case, c in CASES.items():
        if c["n"] != cr.N_MAP:
            continue
        for name in PROGRAM_NAMES:
            if case != "one_run" and name not in SHIFTED:
                continue
            w, te = want_of(orc, fmt, name, c, cr.N_MAP)
            ch = build(hz, ctx, fmt, c["rate"], cr.programs(c["shift"])[name])
            s, d = Guarded(torch, fmt, cr.N_MAP, 0, x), Guarded(torch, "c64", cr.N_MAP, 0)
            ch.set_time(c["ts0"])
            ts, at = c["ts0"], 0
            for m in cr.CUTS:
                assert ch.run(s.t[at:at + m], d.t[at:at + m]) == (m, m)
                ts = cr.want(orc, fmt, x[at:at + m], cr.programs(c["shift"])[name], c["rate"], ts)[1]
                assert ch.time() == ts, (fmt, name, case, at)
                at += m
            assert ts == te
            ch.close()
            d.check(w, ("map in three calls", fmt, name, case))


@pytest.mark.parametrize("fmt", ["c64", "u8"])
def test_map_ulp1_on_an_interpreted_program(hz, torch, ctx, orc, fmt):
    """shift_ulp1 on [Gain 0.5, Shift], which has no ULP1 shape: the output within test_map_chain_subslices' bound of
    the reference (c64: unit inputs, whose output is half the factor; u8: the converted sample's |I| + |Q| times
    3.5 / 1.5, as there), whichever factor the code takes."""
    c = ONE_RUN
    program = (("gain", 0.5), ("shift", c["shift"]))
    ch = build(hz, ctx, fmt, c["rate"], program)
    ch.shift_ulp1()
    try:
        for n in cr.LENGTHS:
            x = np.ones(n, np.complex64) if fmt == "c64" else cr.inputs(fmt, n)
            w, te = cr.want(orc, fmt, x, program, c["rate"], c["ts0"])
            xc = cr.to_c64(orc, fmt, x)
            mag = (np.abs(xc.real) + np.abs(xc.imag)).astype(np.float64) * 0.5
            scale = np.repeat(mag if fmt == "c64" else mag * (3.5 / 1.5), 2)
            for so, do in cr.OFFSETS:
                s, d = Guarded(torch, fmt, n, so, x), Guarded(torch, "c64", n, do)
                ch.set_time(c["ts0"])
                assert ch.run(s.t, d.t) == (n, n)
                assert ch.time() == te
                what = ("ulp1 interpreted", fmt, so, do, "n=%d" % n)
                d.check(None, what)
                _close_to_factor(d.values(), w, scale, what)
    finally:
        ch.close()
    assert ULP1_BOUND == 1.5 * 2.0 ** -24


def test_seventh_stage_is_refused_and_the_six_still_run(hz, torch, ctx, orc):
    ch = build(hz, ctx, "i16", ONE_RUN["rate"], cr.programs()["six"])
    try:
        for add in (lambda: ch.gain(2.0), lambda: ch.rotate(0.5j), lambda: ch.shift(1e5)):
            with pytest.raises(hz.ErrInvalidArgument):
                add()
        ch.rotate(1 + 0j)  # (dropped: takes no place)
        run_map(hz, torch, ctx, orc, ch, "i16", "six", ONE_RUN, cr.N_MAP, 0, 0)
    finally:
        ch.close()


@pytest.mark.parametrize("name", PROGRAM_NAMES)
def test_map_in_a_host_context(hz, host, orc, name):
    """Go slices: the library stages them.  Formats rotated over the programs; a sentinel either side of the output."""
    fmt = cr.FMTS[PROGRAM_NAMES.index(name) % 4]
    c = CASES["wrap_late"]
    n = cr.N_MAP
    x = np.array(cr.inputs(fmt, n))
    w, te = want_of(orc, fmt, name, c, n)
    buf = sentinel(n + 16)
    ch = build(hz, host, fmt, c["rate"], cr.programs(c["shift"])[name])
    ch.set_time(c["ts0"])
    assert ch.run(x, buf[8:8 + n]) == (n, n)
    assert ch.time() == te
    ch.close()
    assert cr.same(buf[:8], sentinel(8)).all() and cr.same(buf[8 + n:], sentinel(8)).all()
    widths = cr.map_widths(0, 0, fmt, n, cr.programs()[name])  # (the staging buffers are aligned)
    msg = cr.first_diff(buf[8:8 + n], w, widths, cr.clock_runs(hz, c["rate"], c["ts0"], n) if name in SHIFTED else [])
    assert msg is None, (fmt, name, msg)
    assert np.array_equal(x.view(np.uint8), np.array(cr.inputs(fmt, n)).view(np.uint8))


# ---- Decimate and Downsample -----------------------------------------------------------------------------------------------

def terminal_want(orc, fmt, name, case, term, factor, blocks=3, start=0, ts0=None):
    c, te = want_of(orc, fmt, name, case, blocks * B, True, start, ts0)
    return cr.want_terminal(orc, term, factor, c), te


@pytest.mark.parametrize("name", cr.TERMINAL_PROGRAMS)
@pytest.mark.parametrize("term", ["decimate", "downsample"])
@pytest.mark.parametrize("fmt", cr.FMTS)
def test_terminal_per_factor_and_clock(hz, torch, ctx, orc, fmt, term, name):
    """3 * 32768 + 1234 samples: three blocks consumed, the outputs in a guarded slice five samples longer than needed
    (the rest must stay unwritten), the clock advanced over the three blocks."""
    x = cr.inputs(fmt, cr.N_TERM)
    shifted = cr.has_shift(cr.terminal_programs()[name])
    s = Guarded(torch, fmt, cr.N_TERM, 1, x)
    for k, (case, c) in enumerate(TCASES.items()):
        if not shifted and case != "one_run":
            continue
        count, _, cls = cr.classify(hz, c["rate"], c["ts0"], 3 * B)
        assert cls == c["cls"], (case, count)
        for factor in cr.FACTORS:
            per = B // factor
            w, te = terminal_want(orc, fmt, name, c, term, factor)
            ch = build(hz, ctx, fmt, c["rate"], cr.terminal_programs(c["shift"])[name], term, factor)
            ch.set_time(c["ts0"])
            assert ch.plan(cr.N_TERM) == (3 * B, 3 * per)
            d = Guarded(torch, "c64", 3 * per + 5, (k + factor) % 2)
            assert ch.run(s.t, d.t) == (3 * B, 3 * per)
            assert ch.time() == te, (fmt, term, name, case, factor)
            ch.close()
            d.check(np.concatenate([w, sentinel(5)]), (term, fmt, name, case, "by %d" % factor))
    s.check(x, "terminal source")


@pytest.mark.parametrize("term", ["decimate", "downsample"])
def test_terminal_plan_is_what_run_returns_and_short_calls_do_nothing(hz, torch, ctx, orc, term):
    c = TCASES["one_run"]
    for fmt, factor in (("u8", 3), ("c64", 4096), ("i16", 32768), ("i8", 1)):
        per = B // factor
        ch = build(hz, ctx, fmt, c["rate"], cr.terminal_programs(c["shift"])["shift"], term, factor)
        ch.set_time(c["ts0"])
        for n in (0, 32767, 32768, 32769, cr.N_TERM):
            x = cr.inputs(fmt, n)
            s, d = Guarded(torch, fmt, n, 0, x), Guarded(torch, "c64", n // B * per + 3, 1)
            ch.set_time(c["ts0"])
            assert ch.plan(n) == (n // B * B, n // B * per)
            assert ch.run(s.t, d.t) == ch.plan(n)
            if n < B:  # below one block: nothing consumed, nothing written, the clock where it was
                assert ch.plan(n) == (0, 0) and ch.time() == c["ts0"]
                d.check(sentinel(3), (term, fmt, "short call", n))
            else:
                w, te = terminal_want(orc, fmt, "shift", c, term, factor, n // B)
                assert ch.time() == te
                d.check(np.concatenate([w, sentinel(3)]), (term, fmt, "plan", n))
        ch.close()


@pytest.mark.parametrize("term", ["decimate", "downsample"])
@pytest.mark.parametrize("fmt", cr.FMTS)
def test_terminal_clock_advances_over_the_consumed_samples(hz, torch, ctx, orc, fmt, term):
    """Two calls: the first is offered 2 * 32768 + 77 samples and takes two blocks, the second starts at sample
    2 * 32768.  Outputs and clock are the reference's over the one stream."""
    x = cr.inputs(fmt, cr.N_TERM)
    s = Guarded(torch, fmt, cr.N_TERM, 0, x)
    for case, c in TCASES.items():
        for name in ("shift", "gain_shift_rotate"):
            for factor in (10, 4096):
                per = B // factor
                w, te = terminal_want(orc, fmt, name, c, term, factor)
                _, t2 = want_of(orc, fmt, name, c, 2 * B, True)
                ch = build(hz, ctx, fmt, c["rate"], cr.terminal_programs(c["shift"])[name], term, factor)
                ch.set_time(c["ts0"])
                d = Guarded(torch, "c64", 3 * per, 0)
                assert ch.run(s.t[:2 * B + 77], d.t[:2 * per + 1]) == (2 * B, 2 * per)
                assert ch.time() == t2, (fmt, term, name, case, "after the first call")
                assert ch.run(s.t[2 * B:], d.t[2 * per:]) == (B, per)
                assert ch.time() == te, (fmt, term, name, case, "after the second call")
                ch.close()
                d.check(w, (term, fmt, name, case, "by %d" % factor, "two calls"))


@pytest.mark.parametrize("fmt", cr.FMTS)
def test_decimate_by_one_is_the_map(hz, torch, ctx, orc, fmt):
    """The rolled one-sample ew_apply of the terminals against ew_apply_n of the map, on the device: decimate(1) gives
    the map chain's output over the consumed samples, for every program of the map and a clock with a wrap."""
    c = CASES["wrap_late"]
    n = B + 100
    x = cr.inputs(fmt, n)
    s = Guarded(torch, fmt, n, 0, x)
    for name in PROGRAM_NAMES:
        p = cr.programs(c["shift"])[name]
        m, t = build(hz, ctx, fmt, c["rate"], p), build(hz, ctx, fmt, c["rate"], p, "decimate", 1)
        dm, dt = Guarded(torch, "c64", B, 0), Guarded(torch, "c64", B + 2, 1)
        m.set_time(c["ts0"])
        t.set_time(c["ts0"])
        assert m.run(s.t[:B], dm.t) == (B, B) and t.run(s.t, dt.t) == (B, B)
        assert m.time() == t.time()
        m.close()
        t.close()
        w, te = cr.want(orc, fmt, x[:B], p, c["rate"], c["ts0"])
        dm.check(w, ("map", fmt, name))
        dt.check(np.concatenate([dm.values(), sentinel(2)]), ("decimate(1) against the map", fmt, name))


@pytest.mark.parametrize("factor", [2, 3, 10, 4096])
def test_downsample_of_minus_zero_inf_and_nan(hz, torch, ctx, orc, factor):
    """Windows of nothing but -0 sum to +0 (the sum starts at +0), an Inf and a NaN stay in their windows."""
    x = cr.minus_zero_block(factor)
    w = cr.want_terminal(orc, "downsample", factor, x)
    assert not np.signbit(w[1].real) and not np.signbit(w[6].imag) and np.isinf(w[2].real) and np.isnan(w[4].imag)
    ch = build(hz, ctx, "c64", 0, (), "downsample", factor)
    s, d = Guarded(torch, "c64", B, 1, x), Guarded(torch, "c64", B // factor, 1)
    assert ch.run(s.t, d.t) == (B, B // factor)
    ch.close()
    d.check(w, ("downsample of -0, Inf, NaN", factor))


def test_terminal_refusals(hz, torch, ctx, orc):
    for term in ("decimate", "downsample"):
        for factor in (0, 32769):
            ch = build(hz, ctx, "u8", cr.RATE, ())
            with pytest.raises(hz.ErrInvalidArgument):
                getattr(ch, term)(factor)
            ch.close()
        ch = build(hz, ctx, "u8", cr.RATE, (("shift", cr.SHIFT),), term, 8)
        for more in (lambda: ch.decimate(2), lambda: ch.downsample(2), lambda: ch.gain(0.5), lambda: ch.rotate(1j),
                     lambda: ch.shift(1.0)):
            with pytest.raises(hz.ErrInvalidArgument):
                more()
        # a destination one sample short: refused, nothing written, the clock where it was
        x = cr.inputs("u8", B)
        s, d = Guarded(torch, "u8", B, 0, x), Guarded(torch, "c64", B // 8 - 1, 0)
        ch.set_time(1.0)
        with pytest.raises(hz.ErrDstTooSmall):
            ch.run(s.t, d.t)
        assert ch.time() == 1.0
        d.check(sentinel(B // 8 - 1), (term, "short destination"))
        ch.close()
    ch = ctx.chain(hz.FMT_C64)  # no sample rate
    with pytest.raises(hz.ErrInvalidArgument):
        ch.shift(1.0)
    ch.close()


# ---- the pipelined map -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["wrap", "table"])
def test_pipelined_map_of_an_interpreted_program(hz, torch, orc, case):
    """hzsdr_chain_pipeline + run_after on [Gain 0.3, Shift, Rotate] from i16 over three rotating (input, output)
    pairs, nine calls of one stream: every call's output and the clock are the plain chain's and the reference's.
    `table`: the 222-run clock -- its table lives in one scratch slot, so run_fmt drains and runs in order."""
    c = dict(TCASES["table"]) if case == "table" else dict(rate=cr.RATE, shift=cr.SHIFT, ts0=cr.TAU - 2.5 * B / cr.RATE)
    n, sets, calls = 3 * B, 3, 9 if case == "wrap" else 4
    p = cr.terminal_programs(c["shift"])["gain_shift_rotate"]
    if case == "table":
        assert cr.classify(hz, c["rate"], c["ts0"], n)[2] == ">32"
    xs = [cr.GEN["i16"](900 + i, n) for i in range(sets)]
    wants, clocks, ts = [], [], c["ts0"]
    for i in range(calls):
        w, ts = cr.want(orc, "i16", xs[i % sets], p, c["rate"], ts)
        wants.append(w)
        clocks.append(ts)
    kept = {}
    for piped in (False, True):
        st = torch.cuda.Stream()
        cx = hz.Context(0, hz.MEM_DEVICE, stream=st.cuda_stream)
        ch = build(hz, cx, "i16", c["rate"], p)
        if piped:
            ch.pipeline(True)
        ch.set_time(c["ts0"])
        ins = [Guarded(torch, "i16", n, 0, x) for x in xs]
        outs = [Guarded(torch, "c64", n, 0) for _ in range(sets)]
        keep = [torch.zeros(n, dtype=torch.complex64, device="cuda") for _ in range(calls)]
        copied = [torch.cuda.Event() for _ in range(sets)]
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            for i in range(calls):
                k = i % sets
                if piped:
                    assert ch.run_after(ins[k].t, outs[k].t, copied[k] if i >= sets else None) == (n, n)
                else:
                    assert ch.run(ins[k].t, outs[k].t) == (n, n)
                assert ch.time() == clocks[i], (case, piped, i)
                keep[i].copy_(outs[k].t)  # (on the context's stream: behind the call)
                copied[k].record(st)
        cx.synchronize()
        torch.cuda.synchronize()
        kept[piped] = [t.cpu().numpy() for t in keep]
        for k in range(sets):  # the guards, and the last call each pair took
            last = max(i for i in range(calls) if i % sets == k)
            outs[k].check(wants[last], ("pipelined map" if piped else "plain map", case, "pair %d" % k))
            ins[k].check(xs[k], "pipelined map source")
        ch.close()
        cx.close()
    widths = cr.map_widths(0, 0, "i16", n, p)
    for i in range(calls):
        ts0 = c["ts0"] if i == 0 else clocks[i - 1]
        for piped in (False, True):
            msg = cr.first_diff(kept[piped][i], wants[i], widths, cr.clock_runs(hz, c["rate"], ts0, n))
            assert msg is None, (case, "piped" if piped else "plain", "call %d" % i, msg)

"""tests/chain_ref.py on the CPU: the reference carries its clock across calls, the numpy restatement of the stages is
the oracle bit for bit, the restated launch_map reaches every width and tail with the offsets and lengths of
tests/test_gpu_chain_terminals.py, every clock case is in its class, and every planted fault changes at least
chain_ref.MIN_SEEN outputs of the very inputs the GPU module compares -- per program, format and clock case where the
fault can occur at all.

Where a fault cannot occur (`pytest -s` prints the counts):
    the W = 1 tail's clock from 0     needs a tail behind a vector body: the aligned calls whose length is 3 mod 4
                                      (4099, 303, 3 * 32768 + 3), every format, every program with a Shift
    the previous run's line,          need two clock runs in the call / in one tile: every clock case but one_run
    the tile's first run only
    rotate(1 + 0j) applied            needs NaN, Inf or -0 in the stream: c64 only (the converters of u8, i8 and i16
                                      produce none), lengths that hold the specials (>= 10 samples)
    the sum from -0                   needs windows of nothing but -0: the c64 block of chain_ref.minus_zero_block
    the sum in reverse                needs three terms: factors >= 3
    the clock over the offered        needs a Shift: the two terminal programs that have one
Every pair of adjacent stages, the two gains 0.3 and 1.7 included (their products round differently in either order),
is seen by every format.  Pairs that cannot reach MIN_SEEN and what stands in for them:
    tail x clock `fresh`              2.5 MHz at 20 MHz turns by pi / 4 a sample, so from 0 s sample 4096 + k has sample
                                      k's factor: replaced by `fresh_off_grid`, the same start at 2 345 678.9 Hz
    sum in reverse                    i8 behind no stage (every partial sum exact), c64 behind no stage by 3 (two white
                                      terms add exactly), c64 by 32767 / 32768 (three outputs, the first NaN either
                                      way): the same formats behind a rotation and the integer formats stand in
                                      (chain_ref.sum_reversed_unseen)
Two things the listed lengths and clocks did not reach, added: lengths 6 and 1026 (the two-sample tail behind W = 4),
and the clock `wrap_at_tile_end` -- a run boundary taken one sample late shows only at the 2 pi wrap, and in nco_ts's
rolled scan only where the wrap shares a tile with at most three more runs
(test_only_the_wrap_tells_a_boundary_one_sample_late).

Counts (`pytest -s`): swap 800 pairs, fewest outputs changed 129; tail 180 / 3; previous run's line 300 / 5; tile's
first run 300 / 3; rotate(1 + 0j) 7 / 3; pick off by one 280 / 3; sum in reverse 174 / 3; sum from -0 4 / 4; clock over
the offered samples 128 / 8."""
import importlib

import numpy as np
import pytest

import chain_ref as cr


@pytest.fixture(scope="module")
def hz():
    return importlib.import_module("go-sdr_amd")


PROGRAMS = cr.programs()
SHIFTED = [k for k, p in PROGRAMS.items() if cr.has_shift(p)]


lengths_of = cr.clock_lengths


# ---- the reference -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", cr.FMTS)
def test_want_over_three_calls_is_want_over_the_buffer(hz, orc, fmt):
    x = cr.inputs(fmt, cr.N_MAP)
    for case in cr.clock_cases():
        for name, p in cr.programs(case["shift"]).items():
            whole, te = cr.want(orc, fmt, x, p, case["rate"], case["ts0"])
            ts, at, parts = case["ts0"], 0, []
            for m in cr.CUTS:
                y, ts = cr.want(orc, fmt, x[at:at + m], p, case["rate"], ts)
                parts.append(y)
                at += m
            assert at == cr.N_MAP and ts == te, (case["name"], name)
            assert cr.same(np.concatenate(parts), whole).all(), (case["name"], name)
            if not cr.has_shift(p):
                assert te == case["ts0"]


def test_the_dropped_rotation_is_the_empty_program(orc):
    x = cr.inputs("c64", 64)
    a, _ = cr.want(orc, "c64", x, PROGRAMS["rotate_one"], 0, 0.0)
    assert cr.same(a, x).all() and cr.effective(PROGRAMS["rotate_one"]) == ()
    assert len(cr.effective(PROGRAMS["six"])) == cr.MAX_STAGES


@pytest.mark.parametrize("fmt", cr.FMTS)
def test_numpy_stages_are_the_oracle_bit_for_bit(orc, fmt):
    """apply_with_clock, which the clock faults are built on, over the true clock: the oracle's bytes, NaNs included."""
    for case in cr.clock_cases():
        n = min(case["n"], cr.N_MAP)
        x = cr.inputs(fmt, n)
        ts = cr.clock_of(orc, case["rate"], case["ts0"], n)
        for name, p in cr.programs(case["shift"]).items():
            w, te = cr.want(orc, fmt, x, p, case["rate"], case["ts0"])
            v = cr.apply_with_clock(orc, cr.to_c64(orc, fmt, x), cr.effective(p), ts)
            assert cr.same(v, w).all(), (case["name"], name)
            assert te == (ts[-1] if cr.has_shift(p) else case["ts0"])


def test_clock_of_is_the_runs_line(hz, orc):
    for case in cr.clock_cases(hz):
        n = min(case["n"], 20_000)
        runs = cr.clock_runs(hz, case["rate"], case["ts0"], n)
        ts = cr.clock_of(orc, case["rate"], case["ts0"], n)
        for r in runs:
            j = np.arange(r[0], r[0] + r[1])
            assert np.array_equal(cr.line_of(r, j), ts[j]), (case["name"], r)


@pytest.mark.parametrize("factor", cr.FACTORS)
def test_numpy_downsample_is_the_oracle(orc, factor):
    for fmt in ("c64", "u8"):
        c = cr.to_c64(orc, fmt, cr.inputs(fmt, cr.N_TERM))
        assert cr.same(cr.downsample_np(c, factor), cr.want_terminal(orc, "downsample", factor, c)).all()
    if cr.B // factor >= 8:
        c = cr.minus_zero_block(factor)
        assert cr.same(cr.downsample_np(c, factor), cr.want_terminal(orc, "downsample", factor, c)).all()


def test_want_terminal_known_values(orc):
    c = (np.arange(2 * cr.B + 5) % 1000).astype(np.complex64)
    d = cr.want_terminal(orc, "decimate", 10, c)
    assert len(d) == 2 * 3276 and d[1] == 10 and d[3276] == c[cr.B] and d[3277] == c[cr.B + 10]
    s = cr.want_terminal(orc, "downsample", 32768, c)
    assert len(s) == 2
    assert cr.want_terminal(orc, "decimate", 32767, c)[1] == c[cr.B]


# ---- launch_map, restated ----------------------------------------------------------------------------------------------

def test_map_widths_known_values():
    p = PROGRAMS["shift_rotate"]
    assert cr.map_widths(0, 0, "c64", 4099, p) == [(4, 0, 4096), (1, 4096, 3)]
    assert cr.map_widths(16, 16, "c64", 4099, p) == [(2, 0, 4098), (1, 4098, 1)]
    assert cr.map_widths(8, 0, "c64", 4099, p) == [(1, 0, 4099)]
    assert cr.map_widths(0, 8, "u8", 5, p) == [(1, 0, 5)]
    assert cr.map_widths(4, 0, "u8", 5, p) == [(2, 0, 4), (1, 4, 1)]  # two u8 samples in: aligned to two, not to four
    assert cr.map_widths(0, 0, "i16", 3, p) == [(2, 0, 2), (1, 2, 1)]  # n < 4: two-sample vectors
    assert cr.map_widths(0, 0, "i8", 1, p) == [(1, 0, 1)]
    assert cr.map_widths(0, 0, "i8", 0, p) == []
    assert cr.map_widths(0, 0, "u8", 4099, (("shift", 1.0),)) == [("exact", 0, 4098), (1, 4098, 1)]
    assert cr.map_widths(0, 0, "u8", 4099, (("shift", 1.0),), ulp1=True) == [(4, 0, 4096), (1, 4096, 3)]
    assert cr.place([(4, 0, 4096), (1, 4096, 3)], 1030) == (4, 1, 1, 2)
    assert cr.place([(4, 0, 4096), (1, 4096, 3)], 4098) == (1, 0, 2, 0)
    assert cr.place([(2, 0, 4098), (1, 4098, 1)], 1027) == (2, 1, 1, 1)


def test_map_widths_reach_every_width_tail_and_ragged_tile():
    bodies, tails, whole_w1, ragged, full = set(), set(), False, set(), set()
    for fmt in cr.FMTS:
        for name, p in PROGRAMS.items():
            for so, do in cr.OFFSETS:
                for n in cr.LENGTHS:
                    ws = cr.map_widths(so * cr.RAW[fmt], do * 8, fmt, n, p)
                    assert sum(c for _, _, c in ws) == n and all(W != "exact" for W, _, _ in ws), (fmt, name, so, do, n)
                    for W, first, count in ws:
                        if W == 1 and first > 0:
                            tails.add(count)
                        elif W == 1:
                            whole_w1 = True
                        if first == 0:
                            bodies.add((fmt, W))
                        if count > cr.TILE[W] and count % cr.TILE[W]:
                            ragged.add(W)
                        if count % cr.TILE[W] == 0:
                            full.add(W)
    assert bodies == {(f, W) for f in cr.FMTS for W in (4, 2, 1)}
    assert tails == {1, 2, 3} and whole_w1
    assert ragged == {4, 2, 1} and full == {4, 2, 1}
    # shift_exact_kernel: only for the two programs the GPU module leaves to the older tests, and only with ulp1 off
    for p in ((("shift", 1.0),), (("shift", 1.0), ("gain", 0.3)), (("rotate", 1 + 0j), ("shift", 1.0))):
        assert cr.map_widths(0, 0, "c64", 4099, p)[0][0] == "exact"
        assert cr.map_widths(0, 0, "c64", 4099, p, ulp1=True)[0][0] == 4
        assert cr.map_widths(8, 0, "c64", 4099, p) == [(1, 0, 4099)]


# ---- clock cases ----------------------------------------------------------------------------------------------------------

def test_every_clock_case_is_in_its_class(hz):
    cases = cr.clock_cases(hz)  # (asserts each)
    assert {c["cls"] for c in cases} == set(cr.CLASSES) and {c["tile"] for c in cases} == set(cr.CLASSES)
    counts = {c["name"]: cr.classify(hz, c["rate"], c["ts0"], c["n"])[:2] for c in cases}
    assert counts == {"one_run": (1, 1), "boundary_in_tile": (2, 2), "wrap_late": (13, 13), "wrap_first_tile": (14, 11),
                      "wrap_at_tile_end": (15, 10), "fresh": (14, 12), "fresh_off_grid": (14, 12), "table_short": (48, 48),
                      "table_long": (222, 12), "wrap_fast": (11, 11)}, counts
    assert cr.clock_runs(hz, cr.RATE, 4 - 500 * cr.TAU / cr.RATE, cr.N_MAP)[1][0] == 3141
    end = cr.clock_runs(hz, cr.RATE, cr.TAU - 1021.5 / cr.RATE, cr.N_MAP)
    assert [r[0] for r in end[:5]] == [0, 1021, 1022, 1023, 1026] and end[1][2] < end[0][2], "tile 0: four runs, the wrap inside"
    for c in cases:  # the length with a three-sample tail stays in the class
        for n in lengths_of(c)[-1:]:
            assert cr.classify(hz, c["rate"], c["ts0"], n)[2] == c["cls"], c["name"]
    terms = cr.terminal_clock_cases(hz)
    assert {c["cls"] for c in terms} == {"1", "5-32", ">32"}
    wrap = cr.clock_runs(hz, cr.RATE, terms[1]["ts0"], 3 * cr.B)
    assert cr.B < wrap[1][0] < 2 * cr.B, "the wrap lies inside the second block"


def test_only_the_wrap_tells_a_boundary_one_sample_late(hz, orc):
    """Why wrap_at_tile_end exists: a lookup that takes a run from `j > first` gives the boundary sample the previous
    run's line.  On the binade edge at 4 s that line still holds the sample's clock; at the 2 pi wrap it is 2 pi off.
    nco_ts's rolled scan serves windows of at most four runs, so the wrap has to share a tile with at most three more."""
    def late(case):
        c = next(k for k in cr.clock_cases() if k["name"] == case)
        runs = cr.clock_runs(hz, c["rate"], c["ts0"], c["n"])
        ts = cr.clock_of(orc, c["rate"], c["ts0"], c["n"])
        return runs, [r[0] for i, r in enumerate(runs[1:]) if cr.line_of(runs[i], r[0]) != ts[r[0]]]
    assert late("boundary_in_tile")[1] == []
    runs, wrong = late("wrap_at_tile_end")
    assert wrong[:3] == [1021, 1022, 1023]
    firsts = [r[0] for r in runs]
    assert sum(1 for f in firsts if f < 1024) == 4 and cr.run_of(runs, 1023) - cr.run_of(runs, 0) <= 3


# ---- planted faults -------------------------------------------------------------------------------------------------------

SEEN = {}  # fault -> [pairs checked, fewest outputs changed]


def note(fault, count, what):
    assert count >= cr.MIN_SEEN, (fault, what, count)
    s = SEEN.setdefault(fault, [0, count])
    s[0] += 1
    s[1] = min(s[1], count)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for k, (pairs, fewest) in sorted(SEEN.items()):
        print("\nFAULT %-28s %5d pairs, fewest outputs changed %d" % (k, pairs, fewest), end="")


@pytest.mark.parametrize("fmt", cr.FMTS)
def test_planted_map_faults_are_seen(hz, orc, fmt):
    kept = {k: 0 for k in ("swap", "tail", "previous_run", "tile_first_run")}
    for case in cr.clock_cases(hz):
        for n in lengths_of(case):
            x = cr.inputs(fmt, n)
            runs, most, _ = cr.classify(hz, case["rate"], case["ts0"], n)
            widths = cr.map_widths(0, 0, fmt, n, PROGRAMS["six"])
            tail = sum(c for W, f, c in widths if W == 1 and f > 0)
            for name in SHIFTED:
                p = cr.programs(case["shift"])[name]
                what = (fmt, name, case["name"], n)
                w, _ = cr.want(orc, fmt, x, p, case["rate"], case["ts0"])
                for i in cr.swaps(p):
                    note("swap", cr.seen(cr.fault_stages_swapped(orc, fmt, x, p, case["rate"], case["ts0"], i), w), what + (i,))
                    kept["swap"] += 1
                if tail >= cr.MIN_SEEN and ("tail", case["name"]) not in cr.REPLACED:
                    note("tail", cr.seen(cr.fault_tail_clock_from_zero(orc, fmt, x, p, case["rate"], case["ts0"], widths), w), what)
                    kept["tail"] += 1
                if runs >= 2:
                    note("previous_run", cr.seen(cr.fault_previous_run_line(orc, hz, fmt, x, p, case["rate"], case["ts0"]), w), what)
                    kept["previous_run"] += 1
                if most >= 2:
                    note("tile_first_run", cr.seen(cr.fault_tile_first_run(orc, hz, fmt, x, p, case["rate"], case["ts0"]), w), what)
                    kept["tile_first_run"] += 1
    assert all(kept.values()), kept


def test_the_tail_fault_applies_to_every_clock_case(hz, orc):
    names = [c["name"] for c in cr.clock_cases(hz)]
    for case in cr.clock_cases(hz):
        n = lengths_of(case)[-1]
        assert cr.map_widths(0, 0, "u8", n, PROGRAMS["six"])[-1] == (1, n - 3, 3), case["name"]
    # the one replaced pair: from 0 s at 2.5 MHz the tail's factors repeat the call's first ones
    assert cr.REPLACED == {("tail", "fresh"): "fresh_off_grid"} and "fresh_off_grid" in names
    x = cr.inputs("i16", cr.N_MAP)
    p = PROGRAMS["gain_shift"]
    widths = cr.map_widths(0, 0, "i16", cr.N_MAP, p)
    bad = cr.fault_tail_clock_from_zero(orc, "i16", x, p, cr.RATE, 0.0, widths)
    assert cr.seen(bad, cr.want(orc, "i16", x, p, cr.RATE, 0.0)[0]) < cr.MIN_SEEN


def test_unit_rotate_applied_is_seen_on_c64(orc):
    p = PROGRAMS["rotate_one"]
    for n in cr.LENGTHS:
        x = cr.inputs("c64", n)
        w, _ = cr.want(orc, "c64", x, p, 0, 0.0)
        got = cr.seen(cr.fault_unit_rotate_applied(orc, "c64", x, p, 0, 0.0), w)
        if n >= 10:
            note("unit_rotate", got, n)
        else:
            assert got <= n
    for fmt in ("u8", "i8", "i16"):  # (no NaN, Inf or -0 behind an integer converter: the fault cannot show)
        x = cr.inputs(fmt, cr.N_MAP)
        assert cr.seen(cr.fault_unit_rotate_applied(orc, fmt, x, p, 0, 0.0), cr.want(orc, fmt, x, p, 0, 0.0)[0]) == 0


@pytest.mark.parametrize("fmt", cr.FMTS)
def test_planted_terminal_faults_are_seen(hz, orc, fmt):
    x = cr.inputs(fmt, cr.N_TERM)
    for case in cr.terminal_clock_cases(hz):
        for name, p in cr.terminal_programs(case["shift"]).items():
            if case["name"] != "one_run" and not cr.has_shift(p):
                continue  # (no clock in the program: one case holds it)
            c, _ = cr.want(orc, fmt, x[:3 * cr.B], p, case["rate"], case["ts0"])
            for factor in cr.FACTORS:
                what = (fmt, name, case["name"], factor)
                note("pick_off_by_one", cr.seen(cr.fault_pick_off_by_one(c, factor), cr.want_terminal(orc, "decimate", factor, c)), what)
                if factor >= 3:
                    count = cr.seen(cr.fault_sum_reversed(c, factor), cr.want_terminal(orc, "downsample", factor, c))
                    if cr.sum_reversed_unseen(fmt, name, factor):
                        assert count < cr.MIN_SEEN, what  # (the documented blind pairs: others stand in for them)
                    else:
                        note("sum_reversed", count, what)
            if cr.has_shift(p):
                x2 = x[2 * cr.B:3 * cr.B]
                bad = cr.fault_clock_over_offered(orc, fmt, x2, p, case["rate"], case["ts0"], 2 * cr.B, 2 * cr.B + 77)
                good = c[2 * cr.B:]
                for term in ("decimate", "downsample"):
                    for factor in (10, 4096):
                        note("clock_over_offered", cr.seen(cr.want_terminal(orc, term, factor, bad),
                                                           cr.want_terminal(orc, term, factor, good)), (fmt, name, case["name"], term, factor))


def test_sum_from_minus_zero_is_seen_on_the_minus_zero_block(orc):
    for factor in (2, 3, 10, 4096):
        c = cr.minus_zero_block(factor)
        w = cr.want_terminal(orc, "downsample", factor, c)
        note("sum_from_minus_zero", cr.seen(cr.fault_sum_from_minus_zero(c, factor), w), factor)
        assert np.isinf(w[2].real) and np.isnan(w[4].imag) and np.signbit(w[1].real) == False  # noqa: E712
    c = cr.to_c64(orc, "c64", cr.inputs("c64", cr.B))  # (on white data the fault changes nothing: why the block exists)
    assert cr.seen(cr.fault_sum_from_minus_zero(c, 10), cr.want_terminal(orc, "downsample", 10, c)) == 0

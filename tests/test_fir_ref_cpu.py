"""tests/fir_ref.py on the CPU: the float64 reference is the direct sum and the oracle's FIR, an honest complex64
overlap-save "kernel" on the restated geometry passes the per-block bar, every planted fault fails it, and the
restatement of the late flags, the slow list and the workgroup-to-block map agrees with a brute-force walk over every
block, with the clock's run boundary swept over both ends of a block's span and of the call.  Every case list of
tests/test_gpu_fir_blocks.py is produced and checked here: a drift in geometry or class shows without a GPU.

What the older bar makes of the same faults (util.assert_fir_close: ONE max-abs and ONE relative-L2 number per call,
behind the suite's Hamming-windowed sinc low-pass, white input), by how many times each fault misses either bar, recorded
by test_planted_faults_fail_the_bar_and_what_the_old_bar_sees (`pytest -s` prints the figures):

    fault                                                     new bar       old bar
    the last tap dropped                                      46 895 x      1 426 x
    the history one sample late                              468 987 x    166 286 x
    a history taken from two calls back                      461 201 x    628 249 x
    two alias bins of a folded form swapped (N 2048, D 8)     46 979 x         25 x   (two stop-band bins)
    one block left unwritten                               1 230 317 x  1 693 467 x
    one block with its neighbour run's modulated taps             34 x         28 x   (20 Msps, 8 MHz, 2047 taps, edge at 4 s)

So on a shape it RUNS the older bar fails every one of the six: it is not blind to them, but the filter takes three
orders of magnitude off a wrong alias bin and one and a half off a wrong edge tap, and the neighbour's taps show in
either bar only at the top of the clock's range (the step of two neighbouring binades differs by 2^-51 s at most: a
phase slip of omega * k * 2^-51 at tap k).  The gap the GPU module closes is the forms, call lengths, run edges and
slow-list classes that no older test runs at all."""
import importlib

import numpy as np
import pytest

import fir_ref as fr
from test_fft_checker_cpu import textbook_fft32
from util import FFT_K, FIR_REL_L2, assert_fir_close, fir_errors, rand_c64


@pytest.fixture(scope="module")
def hz():
    return importlib.import_module("go-sdr_amd")


# ---- geometry and dispatch -------------------------------------------------------------------------------------------------

def test_geometry_known_values_and_the_refusal():
    g = fr.Geom(1024, 8)
    assert (g.N, g.off, g.hop, g.ok) == (4096, 1024, 3072, True)
    g = fr.Geom(257, 4)
    assert (g.N, g.off, g.hop) == (2048, 256, 1792)
    g = fr.Geom(50, 3, 256)
    assert (g.N, g.off, g.hop) == (256, 51, 204)
    assert fr.Geom(100, 8, 300).N == 1024, "a nfft_min that is no power of two falls back to 1024"
    assert fr.Geom(8185, 8).ok and fr.Geom(8185, 8).hop == 8 and not fr.Geom(8186, 8).ok
    assert fr.Geom(8192, 1).ok and fr.Geom(8192, 1).hop == 1 and not fr.Geom(8193, 1).ok


def test_every_form_is_reachable_and_nothing_else():
    seen = set()
    for D in (1, 2, 3, 4, 5, 8, 10, 16, 32):
        for ntaps in (1, 30, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 5000):
            for nmin in (0, 256, 512, 1024, 2048, 4096, 8192):
                g = fr.Geom(ntaps, D, nmin)
                if g.ok:
                    f = fr.form(g)
                    seen.add(f[:2])
                    assert f[2] == (f[1] != 0 and f[0] <= 4096) and f[3] == (f[0] >= 1024) and f[4] == {256: 4, 512: 2}.get(f[0], 1)
    assert seen == set(fr.FORMS) and len(fr.FORMS) == 19
    for N, fold in fr.FORMS:
        if N >= 1024:
            g, _ = fr.geom_for(N, fold)
            assert fr.form(g)[:2] == (N, fold)


# ---- the reference ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ntaps,D", [(1, 1), (2, 3), (37, 4), (100, 8)])
def test_want64_is_the_direct_sum_and_the_oracles_fir(orc, ntaps, D):
    h = fr.graded_taps(ntaps, ntaps)
    x = rand_c64(ntaps + D, 700)
    hist = rand_c64(ntaps + 99, 150)
    for hs in (None, hist, hist[:ntaps // 2]):
        a, b = fr.want64(x, h, D, hs), fr.want64_direct(x, h, D, hs)
        assert a.shape == b.shape == (700 // D,)
        assert np.abs(a - b).max() <= 1e-12 * np.abs(h).sum()
    out = np.zeros(700 // D, np.complex64)
    orc.fir_decimate_f64(out, x, h, D)
    assert np.abs(out - fr.want64(x, h, D)).max() <= 2e-7 * np.abs(fr.want64(x, h, D)).max()
    # a stream cut anywhere, the history handed on: the same outputs
    cut = 333 // D * D
    two = np.concatenate([fr.want64(x[:cut], h, D), fr.want64(x[cut:], h, D, x[:cut])])
    assert np.abs(two - fr.want64(x, h, D)).max() <= 1e-12 * np.abs(h).sum()


def test_impulses_read_the_taps_out():
    g = fr.Geom(135, 3)
    n = 4 * g.hop
    places = fr.block_places(g, n, 5)
    x = fr.impulse_input("c64", n, places)
    h = fr.graded_taps(135, 1)
    y = fr.want64(x, h, 3)
    for i, p in enumerate(places):
        for m in range(-(-p // 3), min((p + 135 + 2) // 3, n // 3)):
            k = 3 * m - p
            if 0 <= k < 135 and all(not (0 <= 3 * m - q < 135) for q in places if q != p):
                assert abs(y[m] - complex(x[p]) * complex(h[k])) <= 1e-12
    assert len(places) == 4 and [p // g.hop for p in places] == [0, 1, 2, 3]


# ---- the checker -----------------------------------------------------------------------------------------------------------

def streams(g, ncalls, seed, taps="graded"):
    """A stream cut into calls -> (taps, [(xc, the stream in front of it)])."""
    h = fr.graded_taps(g.ntaps, seed) if taps == "graded" else fr.lowpass_taps(g.ntaps)
    lens = [3 * g.hop + g.hop // 2 // g.D * g.D, 2 * g.hop, 4 * g.hop - g.D][:ncalls]
    x = rand_c64(seed + 1, sum(lens))
    cuts = np.cumsum([0] + lens)
    return h, x, [(x[a:b], x[:a]) for a, b in zip(cuts[:-1], cuts[1:])]


def check(g, got, xc, front, h, k=FFT_K):
    return fr.assert_fir_blocks(got, fr.want64(xc, h, g.D, front), fr.yardstick32(g, xc, h, front), h, float(np.abs(xc).max()), g, k=k)


@pytest.mark.parametrize("ntaps,D,nmin", [(50, 3, 256), (135, 2, 0), (263, 8, 0), (1031, 16, 0), (7808, 4, 0)])
def test_yardstick_passes_at_k_1_on_every_call(ntaps, D, nmin):
    g = fr.Geom(ntaps, D, nmin)
    h, x, calls = streams(g, 3, ntaps)
    for xc, front in calls:
        assert check(g, fr.yardstick32(g, xc, h, front), xc, front, h, k=1.0) <= (1.0, 1.0)
    for h2 in [fr.ends_taps(ntaps)] + [fr.delay_taps(ntaps, k0) for k0 in fr.delay_places(ntaps)]:
        xi = fr.impulse_input("c64", len(calls[0][0]), fr.block_places(g, len(calls[0][0]), 11))
        check(g, fr.yardstick32(g, xi, h2, None), xi, None, h2, k=1.0)


@pytest.mark.parametrize("ntaps,D", [(135, 3), (263, 8)])
def test_honest_float32_overlap_save_passes_at_k_4(ntaps, D):
    """An independent radix-2 float32 transform with split twiddles, a complex64 product, the transform back, on the
    restated geometry: the arithmetic of an honest kernel."""
    g = fr.Geom(ntaps, D)
    h, x, calls = streams(g, 2, ntaps + 1)
    H = fr.filter_bins(g, h)
    for xc, front in calls:
        rows = fr.block_rows(g, xc, front)
        y = np.stack([textbook_fft32((textbook_fft32(r, True, split=True) * H).astype(np.complex64), False, split=True) for r in rows])
        r = check(g, fr.pick_outputs(g, y, len(xc)), xc, front, h)
        print("honest N=%d D=%d worst ratios max_sample %.2f l2 %.2f" % (g.N, D, r[0], r[1]))


def late_case(hz, taps):
    """A Shift chain across the binade edge at 4 s, every block of the middle late: (g, converted samples, the stream
    as stored, taps, runs, omega)."""
    rate, shift = 20_000_000, 8.0e6
    g = fr.Geom(2047, 1)
    n = 6 * g.hop + g.N
    ts0 = fr.edge_start(hz, rate, 4.0, g.p0(4), n)  # block 4 begins the run behind the edge
    runs = fr.clock_runs(hz, rate, ts0, n)
    assert len(runs) == 2 and runs[1][0] == g.p0(4) and runs[0][3] != runs[1][3]
    raw = rand_c64(5, n)
    omega = 2.0 * np.pi * shift
    ts = fr.clock_of(runs, n)
    ph = omega * ts
    xc = (raw * (np.cos(ph) + 1j * np.sin(ph)).astype(np.complex64)).astype(np.complex64)
    h = fr.graded_taps(2047, 6) if taps == "graded" else fr.lowpass_taps(2047)
    return g, raw, xc, h, runs, omega


FAULTS = ("last_tap", "history_late", "stale_history", "alias_swap", "unwritten", "neighbour_taps")
OLD_BAR_SEES = {"last_tap": True, "history_late": True, "stale_history": True, "alias_swap": True, "unwritten": True,
                "neighbour_taps": True}


def faulty(hz, name, taps):
    """-> (g, got, want, yard, h, xmax) of the call the fault shows in."""
    if name == "neighbour_taps":
        g, raw, xc, h, runs, omega = late_case(hz, taps)
        n = len(xc)
        honest = fr.late_mixed32(g, raw, h, runs, omega)
        steps = [runs[0][3] if g.p0(b) + g.N // 2 < runs[1][0] else runs[1][3] for b in range(g.nblocks(n))]
        steps[4] = runs[0][3]  # block 4, the first of the second run, with the first run's taps
        bad = fr.late_mixed32(g, raw, h, runs, omega, steps)
        yard = fr.yardstick32(g, xc, h)
        per = g.hop // g.D
        # (the stream's edges and the block across the boundary mix in reference order: the yardstick there)
        flags = fr.late_flags(g, runs, n, fr.run_filters(g, runs, n))
        assert flags[4] and flags[5] and not flags[3] and sum(flags) >= 4
        for y in (honest, bad):
            for b, late in enumerate(flags):
                if not late:
                    y[b * per:(b + 1) * per] = yard[b * per:(b + 1) * per]
        want = fr.want64(xc, h, g.D)
        if taps == "graded":  # the honest late mixer passes: the model and the bar agree on what is right
            fr.assert_fir_blocks(honest, want, yard, h, float(np.abs(xc).max()), g, what="honest late mixer")
        return g, bad, want, yard, h, float(np.abs(xc).max())
    g = fr.Geom(263, 8)  # N = 2048, FOLD 8
    h, x, calls = streams(g, 3, 21, taps)
    xc, front = calls[2]
    two_back = calls[1][1]  # the stream in front of the call before
    got = {"last_tap": lambda: fr.fault_last_tap_dropped(g, xc, h, front),
           "history_late": lambda: fr.fault_history_late(g, xc, h, front),
           "stale_history": lambda: fr.fault_stale_history(g, xc, h, two_back),
           "alias_swap": lambda: fr.fault_alias_bins_swapped(g, xc, h, front, k0=3, q1=3, q2=4),
           "unwritten": lambda: fr.fault_block_unwritten(g, xc, h, front, 2)}[name]()
    return g, got, fr.want64(xc, h, g.D, front), fr.yardstick32(g, xc, h, front), h, float(np.abs(xc).max())


@pytest.mark.parametrize("name", FAULTS)
def test_planted_faults_fail_the_bar_and_what_the_old_bar_sees(hz, name):
    g, got, want, yard, h, xmax = faulty(hz, name, "graded")
    with pytest.raises(AssertionError):
        fr.assert_fir_blocks(got, want, yard, h, xmax, g, what=name)
    clean = np.where(got.view(np.uint32).reshape(-1, 2) == fr.SENT32, 0.0, got.view(np.float32).reshape(-1, 2)).view(np.complex64).reshape(-1)
    new = max(fr.assert_fir_blocks(clean, want, yard, h, xmax, g, k=np.inf)) / FFT_K
    # the same fault behind the older tests' low-pass, white input, one bound over the whole call
    g, got, want, yard, h, xmax = faulty(hz, name, "lowpass")
    err, bound, rel = fir_errors(got, want, h, xmax)
    old = max(err / bound, rel / FIR_REL_L2)
    try:
        assert_fir_close(got, want, h, xmax, name)
        seen = False
    except AssertionError:
        seen = True
    print("fault %-15s over the new bar by %9.1f x   over the old bar by %9.1f x (%s)" % (name, new, old, "fails" if seen else "PASSES"))
    assert seen == (old > 1.0) and new > 1.0
    assert seen == OLD_BAR_SEES[name], "the record in this file's docstring is out of date"


# ---- the restatement against a brute-force walk ------------------------------------------------------------------------------

def brute_late(g, firsts, has, n, b):
    """late_block sample by sample."""
    p0 = g.p0(b)
    if p0 < 0 or p0 + g.N > n - g.off:
        return False
    runs_of = {max(i for i, f in enumerate(firsts) if f <= p) for p in (p0, p0 + g.N - 1)} | \
              {i for i, f in enumerate(firsts) if p0 < f <= p0 + g.N - 1}
    return len(runs_of) == 1 and has[next(iter(runs_of))]


def brute_slow(g, firsts, has, n, b):
    """slow_blocks' conditions block by block: a span that leaves [0, n - off], touches a run without a filter, or has
    a boundary of a run with a filter at p0 ... p0 + N (both ends included: the host compares at equality)."""
    p0 = g.p0(b)
    if p0 < 0 or b * g.hop > n - g.N:
        return True
    ends = firsts[1:] + [n]
    for r, (f, e) in enumerate(zip(firsts, ends)):
        if not has[r] and f <= p0 + g.N - 1 and e - 1 >= p0 and e > f:
            return True
        if has[r] and r > 0 and p0 <= f <= p0 + g.N:
            return True
    return False


def fake_runs(firsts):
    return [(f, 0, 0.0, 1.0) for f in firsts]


@pytest.mark.parametrize("ntaps,D", [(135, 3), (263, 8), (7808, 4), (1031, 1)])
def test_late_flags_and_slow_list_against_a_walk_over_every_block(ntaps, D):
    g = fr.Geom(ntaps, D)
    b_mid = 2 * g.N // g.hop + 3  # a block with room for a long run in front
    checked = 0
    for n0 in (g.p0(b_mid + 2 * g.N // g.hop + 6) + g.N + g.off,):
        base = g.p0(b_mid)
        # the run boundary over both ends of a block's span; the same five around n - off - N (n moves, the boundary stays)
        sweeps = [(n0, base + d) for d in (-1, 0, 1, g.N - 1, g.N)] + [(n0 + d, base) for d in (-1, 0, 1, g.N - 1, g.N)]
        # ... and a boundary on each of the five around the last span inside the call
        sweeps += [(n0, n0 - g.off - g.N + d) for d in (-1, 0, 1, g.N - 1, g.N)]
        for n, s in sweeps:
            for firsts in ([0, s], [0, s, s + 2 * g.N], [0, s, s + 100], [0]):
                runs = fake_runs(firsts)
                has = fr.run_filters(g, runs, n)
                if has is None:
                    continue
                flags = fr.late_flags(g, runs, n, has)
                lst, cls = fr.slow_list(g, runs, n, has)
                nb = g.nblocks(n)
                assert flags == [brute_late(g, firsts, has, n, b) for b in range(nb)], (n, firsts)
                want = [b for b in range(nb) if brute_slow(g, firsts, has, n, b)]
                if cls == "given_up":
                    assert lst == [] and len(want) > fr.MAX_SLOW - 40, (n, firsts, len(want))
                    continue
                assert lst == want, (n, firsts, lst, want)
                assert cls == fr.slow_class(len(lst))
                # every block that does not mix late is on the list; what is on it and still late sits AT a boundary
                assert {b for b in range(nb) if not flags[b]} <= set(lst)
                for b in set(lst) - {b for b in range(nb) if not flags[b]}:
                    assert any(f in (g.p0(b), g.p0(b) + g.N) for f in firsts[1:]), (n, firsts, b)
                checked += 1
    assert checked >= 30


def test_more_than_32_runs_or_no_long_run_means_no_late_kernel(hz):
    g = fr.Geom(135, 3)
    runs = fr.clock_runs(hz, fr.SLOW_RATE, 0.0, fr.SLOW_N)
    assert len(runs) > fr.MAX_RUNS and fr.run_filters(g, runs, fr.SLOW_N) is None
    assert fr.run_filters(g, fake_runs([0, 1000, 2000]), 3000) is None
    assert fr.run_filters(g, [], 3000) == [True] and fr.run_filters(g, [], 3000, in_order=True) is None
    assert fr.run_filters(fr.Geom(50, 3, 256), [], 3000) is None, "blocks that share a workgroup never mix late"


def assert_map_is_a_bijection(g, n, lst, what):
    nb = g.nblocks(n)
    hit = [fr.block_of_workgroup(g, n, lst, i) for i in range(fr.grid_of(g, n, lst, True))]
    blocks = [b for b in hit if b is not None]
    assert sorted(blocks) == list(range(nb)), (what, "blocks missed", sorted(set(range(nb)) - set(blocks))[:8], "hit twice",
                                               sorted({b for b in blocks if blocks.count(b) > 1})[:8])
    assert hit[:len(lst)] == lst
    # the c-th block not in the list, the kernel's three ways against a plain walk
    free = [b for b in range(nb) if b not in set(lst)]
    assert [fr.nth_unlisted(lst, c) for c in range(len(free))] == free, what
    if 0 < len(lst) <= 4 or len(lst) > 4:
        k = [c + sum(1 for i, e in enumerate(lst) if e - i <= c) for c in range(len(free))]
        assert k == free, (what, "the ballot's formula")


def test_synthetic_lists_of_every_length_map_onto_every_block():
    g = fr.Geom(7808, 8)
    rng = np.random.default_rng(3)
    for count in list(range(0, 8)) + [63, 64, 65, 66, 95, 96]:
        for nb in (count + 1, count + 7, count + 8, count + 9, count + 100):
            lst = sorted(rng.choice(nb, count, replace=False).tolist())
            assert_map_is_a_bijection(g, nb * g.hop, lst, (count, nb))


# ---- the case lists of the GPU tests -------------------------------------------------------------------------------------------

def test_form_cases_cover_every_form_and_rotate_the_formats():
    cases = fr.form_cases()
    assert {(c["N"], c["fold"]) for c in cases} == {f for f in fr.FORMS if f[0] >= 1024}
    for c in cases:
        assert fr.form(c["g"])[:2] == (c["N"], c["fold"]) and c["n"] % c["g"].D == 0
        assert c["g"].nblocks(c["n"]) == 6 and c["n"] % c["g"].hop != 0
        assert c["n"] <= 25_000 or c["N"] == 8192
        assert c["nfft_min"] == 0, "the library's own choice of N"
    for fold in (0, 2, 4, 8, 16):
        fmts = {c["fmt"] for c in cases if c["fold"] == fold} | ({c["fmt"] for c in fr.small_block_cases()} if fold == 0 else set())
        assert fmts == set(fr.FMTS), (fold, fmts)
    small = fr.small_block_cases()
    assert {c["N"] for c in small} == {256, 512}
    for N, x in ((256, 4), (512, 2)):
        assert {c["blocks"] for c in small if c["N"] == N} == {1, x - 1, x, x + 1, 2 * x + 1} - {0}
    for c in small:
        assert c["g"].nblocks(c["n"]) == c["blocks"] and c["n"] % c["g"].D == 0 and fr.form(c["g"])[4] == {256: 4, 512: 2}[c["N"]]


def test_call_edge_lengths():
    for N, fold, fmt, D in fr.EDGE_FORMS:
        g, _ = fr.geom_for(N, fold, None, D)
        first, stream = fr.call_lengths(g)
        assert {g.D, g.hop - g.D, g.hop, g.hop + g.D, 2 * g.hop, 3 * g.hop, g.off - g.D, g.off, g.off + g.D} == set(first)
        assert all(v % g.D == 0 and v > 0 for v in first + stream)
        assert len(stream) == 8 and all(v < g.off / 3 for v in stream[:7]) and stream[7] > 2 * g.hop
    assert {f[1] for f in fr.EDGE_FORMS} == {0, 2, 4, 8, 16} and {f[2] for f in fr.EDGE_FORMS} == set(fr.FMTS)


def test_run_edge_cases_put_the_edge_where_they_say(hz):
    cases = fr.run_edge_cases(hz)
    assert len(cases) == 40
    for c in cases:
        g, n = c["g"], c["n"]
        p = fr.plan_call(hz, g, c["rate"], c["ts0"], n)
        assert [r[0] for r in p["runs"]] == [0, c["edge"]], (c["where"], p["runs"])
        name, d = c["where"]
        base = g.p0(4) if name == "middle" else n - g.off - g.N
        assert c["edge"] == base + d
        firsts = [0, c["edge"]]
        assert p["late"] == [brute_late(g, firsts, p["has"], n, b) for b in range(g.nblocks(n))]
        assert p["slow"] == [b for b in range(g.nblocks(n)) if brute_slow(g, firsts, p["has"], n, b)]
        assert_map_is_a_bijection(g, n, p["slow"], c["where"])
        if name == "middle":  # both runs have a filter; the block is late exactly when the edge is at or outside its ends
            assert p["has"] == [True, True] and p["late"][4] == (d in (-1, 0, g.N)), (c["where"], p["late"])
            assert (4 in p["slow"]) == (d != -1), "the host lists the block at equality, the device mixes it late"


def test_slow_cases_have_their_class_and_residue(hz):
    cases = fr.slow_cases(hz)
    assert [(c["cls"], c["residue"]) for c in cases[:-1]] == [(k, r) for k in fr.CLASSES for r in (0, 1, 7)]
    for c in cases:
        g, n, p = c["g"], c["n"], c["plan"]
        assert fr.form(g)[:2] == (c["N"], c["fold"]) and n % g.D == 0 and n <= 100_000
        assert p["cls"] == c["cls"] and p["has"] is not None
        assert c["residue"] is None or (p["rest"] % 8 == c["residue"] and p["rest"] >= 1)
        count = len(p["slow"])
        assert {"none": count == 0, "1-4": 1 <= count <= 4, "5-64": 5 <= count <= 64, "65-96": 65 <= count <= 96,
                "given_up": count == 0}[c["cls"]]
        firsts = [r[0] for r in p["runs"]] or [0]
        brute = [b for b in range(g.nblocks(n)) if brute_slow(g, firsts, p["has"], n, b)]
        if c["cls"] == "given_up":
            assert len(brute) > fr.MAX_SLOW and any(not f for f in p["late"]) and any(p["late"])
        else:
            assert p["slow"] == brute
        assert p["late"] == [brute_late(g, firsts, p["has"], n, b) for b in range(g.nblocks(n))]
        assert_map_is_a_bijection(g, n, p["slow"], (c["cls"], c["residue"]))
    assert cases[-1]["plan"]["rest"] < 8
    assert any(len(c["plan"]["slow"]) > 64 for c in cases), "the upper half of the ballot"
    for N in (1024, 2048, 4096):
        for cls in ("65-96", "given_up"):
            assert not fr.reachable(N, cls) and fr.find_case(hz, N, 0, cls, 0) is None

"""The symbol-timing recovery bank's ABI and arithmetic, without a GPU: include/hzsdr_symsync.h is C99 and declares exactly
its ten entries, the C walkthrough names them all and compiles, the library exports them and _capi.SYMSYNC_SIGNATURES
binds them exactly; exact read-outs of the bit-exact restatement (tests/host/symsync_ref.cpp over the header the kernel
evaluates) with the loop held still; the interpolator on samples of a cubic; acquisition of the five cases of the
definition, by the program and by the independent float64 restatement (tests/symsync_ref.py); the counter and the bound
under saturating input; refused parameters; cuts."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import symsync_ref as ref
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "hzsdr_symsync.h")
WALK = os.path.join(ROOT, "tests", "c", "test_symsync_abi.c")
ENTRIES = {"hzsdr_symsync_create", "hzsdr_symsync_push", "hzsdr_symsync_max_symbols", "hzsdr_symsync_set_params", "hzsdr_symsync_get_state",
           "hzsdr_symsync_set_state", "hzsdr_symsync_position", "hzsdr_symsync_plan", "hzsdr_symsync_reset", "hzsdr_symsync_free"}
GCC = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include")]


@pytest.fixture(scope="module")
def hz():
    return importlib.import_module("go-sdr_amd")


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("symsync_ref"))


def symsync_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(hzsdr_[a-z0-9_]+)\s*\(", text)))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the ABI ---------------------------------------------------------------------------------------

def test_header_is_c99(tmp_path):
    src = tmp_path / "inc.c"
    src.write_text('#include "hzsdr_symsync.h"\n'
                   "int main(void) { hzsdr_symsync *f = 0; return (f != 0) + HZSDR_SYMSYNC_REAL_F32 - HZSDR_SYMSYNC_FORM_PER_ROW"
                   " - HZSDR_SYMSYNC_FORM_COMPLEX - HZSDR_SYMSYNC_MAX_ROWS; }\n")
    subprocess.check_call(GCC + ["-c", str(src), "-o", str(tmp_path / "inc.o")])


def test_header_declares_exactly_the_entries():
    assert len(ENTRIES) == 10 and set(symsync_symbols()) == ENTRIES


def test_c_walkthrough_names_every_entry():
    text = open(WALK).read()
    missing = [s for s in symsync_symbols() if not re.search(r"\b" + s + r"\s*\(", text)]
    assert missing == []
    assert "symsync-abi ok" in text


def test_c_walkthrough_compiles_as_c99(tmp_path):
    subprocess.check_call(GCC + ["-c", WALK, "-o", str(tmp_path / "w.o")])


def test_library_exports_and_ctypes_table(hz):
    capi = importlib.import_module("go-sdr_amd._capi")
    syms = symsync_symbols()
    for s in syms:
        assert hasattr(capi.lib, s), f"{s} declared in hzsdr_symsync.h but not exported"
    assert sorted(capi.SYMSYNC_SIGNATURES) == syms
    others = (set(capi.SIGNATURES) | set(capi.SPECTRUM_SIGNATURES) | set(capi.CHANNELIZER_SIGNATURES) | set(capi.SYNTHESIZER_SIGNATURES)
              | set(capi.RESAMPLER_SIGNATURES) | set(capi.DEMOD_SIGNATURES) | set(capi.TUNER_SIGNATURES) | set(capi.CHANBANK_SIGNATURES)
              | set(capi.COVAR_SIGNATURES) | set(capi.IIR_SIGNATURES))
    assert not set(capi.SYMSYNC_SIGNATURES) & others
    for name, (res, args) in capi.SYMSYNC_SIGNATURES.items():
        fn = getattr(capi.lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_signatures_have_the_header_arity(hz):
    capi = importlib.import_module("go-sdr_amd._capi")
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    found = re.findall(r"\bint (hzsdr_symsync_[a-z_]+)\s*\(([^)]*)\)", text)
    assert {name for name, _ in found} == ENTRIES
    for name, params in found:
        assert len(capi.SYMSYNC_SIGNATURES[name][1]) == len(params.split(",")), name


def test_constants_match_header(hz):
    defs = dict(re.findall(r"#define (HZSDR_\w+) (\d+)", open(HEADER).read()))
    iir = dict(re.findall(r"#define (HZSDR_\w+) (\d+)", open(os.path.join(ROOT, "include", "hzsdr_iir.h")).read()))
    assert int(defs["HZSDR_SYMSYNC_REAL_F32"]) == hz.SYMSYNC_REAL_F32 == ref.REAL_F32 == 32 == int(iir["HZSDR_IIR_REAL_F32"]) == hz.IIR_REAL_F32
    assert "HZSDR_IIR_REAL_F32" in open(HEADER).read(), "the header does not say that the kind is the IIR bank's"
    assert hz.SYMSYNC_REAL_F32 not in (hz.FMT_C64, hz.FMT_U8, hz.FMT_I16, hz.FMT_I8)
    assert int(defs["HZSDR_SYMSYNC_FORM_PER_ROW"]) == hz.SYMSYNC_FORM_PER_ROW == ref.FORM_PER_ROW == 1
    assert int(defs["HZSDR_SYMSYNC_FORM_COMPLEX"]) == hz.SYMSYNC_FORM_COMPLEX == ref.FORM_COMPLEX == 2
    assert int(defs["HZSDR_SYMSYNC_MAX_ROWS"]) == hz.SYMSYNC_MAX_ROWS == ref.MAX_ROWS == 8192
    csrc = os.path.join(ROOT, "go-sdr_amd", "csrc")
    assert "kMaxRows = 8192, kLanes = 64" in open(os.path.join(csrc, "hz_rowwave_plan.h")).read()  # (the row-wave banks')
    assert "kParams = 4;" in open(os.path.join(csrc, "hz_symsync_plan.h")).read()
    assert hz.SYMSYNC_REAL_F32 is importlib.import_module("go-sdr_amd.symsync").SYMSYNC_REAL_F32


def test_python_layers_are_exported(hz):
    st = importlib.import_module("go-sdr_amd.stream")
    mod = importlib.import_module("go-sdr_amd.symsync")
    assert hz.SymbolSync is mod.SymbolSync and hz.loop_gains is mod.loop_gains and callable(hz.Context.symbol_sync) and callable(st.symbol_rows)
    for name in ("push", "ragged", "max_symbols", "set_params", "state", "set_state", "position", "reset", "plan", "close", "__enter__", "__exit__"):
        assert callable(getattr(hz.SymbolSync, name)), name
    hpp = open(os.path.join(ROOT, "go-sdr_amd", "cxx", "hzsdr.hpp")).read()
    assert "class SymbolSync" in hpp and '#include "../../include/hzsdr_symsync.h"' in hpp
    assert "hzsdr_symsync.h" in open(os.path.join(ROOT, "go-sdr_amd", "csrc", "Makefile")).read()
    # the real float32 rows go through the rows helper by the kind's value
    rows = importlib.import_module("go-sdr_amd._rows")
    x = np.zeros((3, 40), np.float32)[:, :33]
    assert rows.rows_input(x, hz.SYMSYNC_REAL_F32, 3, "symbol sync") == (x.ctypes.data, 33, 40)


def test_loop_gains(hz):
    g_mu, g_omega = hz.loop_gains(5.0)
    assert g_mu == pytest.approx(0.06 * 5.0 / 2.7, rel=1e-15) and g_omega == pytest.approx(g_mu * 0.06 / 4.0, rel=1e-15)
    assert hz.loop_gains(8.0, alpha=0.1, ted_gain=2.0) == pytest.approx((0.4, 0.01), rel=1e-15)
    doc = hz.loop_gains.__doc__
    assert "ted_gain" in doc and "NOMINAL" in doc and "not been measured" in doc
    for bad in ((0.0,), (5.0, 0.0), (5.0, 0.06, -1.0)):
        with pytest.raises(ValueError):
            hz.loop_gains(*bad)


# ---- exact read-outs: the loop held still ------------------------------------------------------------

def integers(n, seed):
    """nonzero small integers, exact in float32"""
    rng = np.random.default_rng(seed)
    return (rng.integers(1, 111, n) * (2 * rng.integers(0, 2, n) - 1)).astype(np.float32)


@pytest.mark.parametrize("sps", [4, 6, 8])
def test_even_sps_reads_samples_out(build_dir, sps):
    """g_mu = g_omega = limit = 0: every advance is sps / 2 exactly, every strobe falls ON a sample (mu = 0), and symbol
    k is x[sps k + sps / 2 - 2], bit for bit."""
    x = integers(50 * sps, seed=sps)
    ((y, counts, z, neg),) = ref.exact(build_dir, [(np.array([sps, 0, 0, 0], np.float32), x)])
    k = np.arange(counts[0])
    assert counts[0] == len(x) // sps and neg == 0
    assert np.array_equal(bits(y[0, :counts[0]]), bits(x[sps * k + sps // 2 - 2]))
    assert z[0, 1] == np.float32(sps / 2) and not y[0, counts[0]:].any()


def test_sps_5_reads_midpoints_out(build_dir):
    """sps = 5, the loop held still: the mid-symbol strobe falls on a sample and the symbol strobe half way between
    two, where the cubic is (-x[i-1] + 9 x[i] + 9 x[i+1] - x[i+2]) / 16, i = 5 k, samples before the stream 0: within 4
    float32 ulps of that value, symbol by symbol.  The samples are integers of one sign, 60 ... 110, so that no
    symbol is a small difference of large terms (an ulp of such a value would say nothing about the arithmetic)."""
    x = np.abs(integers(500, seed=55)) % 51 + 60
    assert x.dtype == np.float32 and x.min() >= 60 and x.max() <= 110
    ((y, counts, _, neg),) = ref.exact(build_dir, [(np.array([5, 0, 0, 0], np.float32), x)])
    assert neg == 0 and counts[0] == 100
    xp = np.concatenate([[0.0], x.astype(np.float64), [0.0, 0.0]])  # xp[j + 1] = x[j]
    i = 5 * np.arange(counts[0])
    want = (-xp[i] + 9.0 * xp[i + 1] + 9.0 * xp[i + 2] - xp[i + 3]) / 16.0
    err = np.abs(y[0, :counts[0]].astype(np.float64) - want)
    ulps = err / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    print(f"sps 5: max error {err.max():.3e} = {ulps.max():.2f} ulps of its value, values {np.abs(want).min():.1f} ... {np.abs(want).max():.1f}")
    assert ulps.max() <= 4.0


def test_interpolator_on_a_cubic(build_dir):
    """interp on samples of a cubic returns the cubic at mu.  sps = 2.125 with the loop held still walks the symbol
    strobes' mu through the odd sixteenths (every counter value is a small multiple of 1 / 16, exact in float32); the
    input is p(n) = 0.001 n^3 - 0.02 n^2 + 0.3 n + 50 over n < 60 (50 ... 210: of one sign and away from 0, so that an ulp
    of a value says something about the arithmetic), and every symbol behind the first three samples must be within
    4 float32 ulps OF ITS OWN VALUE of the exact cubic through the float32 samples, and within one ulp more of p
    itself, whose samples are rounded (half an ulp each, times the basis' sum of at most 1.25 on [0, 1])."""
    n = np.arange(60, dtype=np.float64)
    px = lambda t: 0.001 * t ** 3 - 0.02 * t ** 2 + 0.3 * t + 50.0  # noqa: E731
    x = px(n).astype(np.float32)
    ((y, counts, _, _),) = ref.exact(build_dir, [(np.array([2.125, 0, 0, 0], np.float32), x)])
    # strobe j is at time 1.0625 j - 2 (samples): mid-symbol ones at even j, symbols at odd j
    t = 1.0625 * (2 * np.arange(counts[0]) + 1) - 2.0
    ok = t >= 1.0  # (x3 is a sample of the stream, not the 0 before it)
    # the samples are float32 roundings of p: interpolate THEM exactly (float64 Lagrange) for the comparison
    want = []
    for tt in t[ok]:
        i = int(np.floor(tt))
        want.append(ref.lagrange(float(x[i - 1]), float(x[i]), float(x[i + 1]), float(x[i + 2]), tt - i))
    want = np.array(want)
    got = y[0, :counts[0]][ok].astype(np.float64)
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    exact, cubic = np.abs(got - want) / ulp, np.abs(got - px(t[ok])) / ulp
    print(f"interp: {exact.max():.2f} ulps of its value from the cubic through the samples, {cubic.max():.2f} from p itself; "
          f"values {want.min():.1f} ... {want.max():.1f}")
    assert ok.sum() >= 24 and {float(m) for m in (t[ok] % 1.0)} == {k / 16.0 for k in range(1, 16, 2)}
    assert want.min() > 50.0
    assert exact.max() <= 4.0
    assert cubic.max() <= 5.0


# ---- acquisition -----------------------------------------------------------------------------------

# (sps, clock offset in ppm, off, complex)
ACQ = [(5.0, 200.0, 0.37, False), (4.0, -300.0, 0.9, False), (8.0, 500.0, 0.5, True), (2.5, 100.0, 0.2, False), (10.0, -1000.0, 0.77, False)]
SKIP, LAST = 1000, 2980


def acquisition_case(hz, sps, ppm, off, cplx, noise_db=None):
    a = ref.symbols(3000, 7 + int(sps * 10), cplx)
    sps_true = sps * (1.0 + ppm * 1e-6)
    x = ref.signal(a, sps_true, off, noise_db, seed=3)
    return a, sps_true, x, np.array([sps, 0.01, *hz.loop_gains(sps)], np.float32)


def check_acquired(name, y, hs, a, sps_true, cplx):
    """the conditions of the definition on the symbols y (and h at every symbol) behind the first SKIP"""
    assert len(y) >= LAST
    lag, bad, n = ref.best_lag(y[:LAST], a, SKIP)
    level = np.abs(y[SKIP:LAST].real).min() if cplx else np.abs(y[SKIP:LAST]).min()
    rel = abs(float(np.mean(hs[-200:])) / (sps_true / 2.0) - 1.0)
    print(f"{name}: lag {lag}, {bad} of {n} signs differ, min level {level:.4f}, mean h over the last 200 symbols off by {rel:.2e} relative")
    assert n == LAST - SKIP and bad == 0, f"{name}: {bad} symbols differ at the best lag {lag}"
    assert level >= (0.6 if cplx else 0.85), f"{name}: the eye is {level}"
    assert rel <= 1e-4, f"{name}: h is off by {rel}"


def h_trace(build_dir, params, x, count):
    """h over the last symbols of the program's run: the program gives the state behind a run, so the stream is run up
    to about 230 symbols before its end in one piece and from there in pieces of about 5 symbols, the state carried,
    and every symbol of a piece is given the h behind the piece"""
    sps = float(params[0])
    first, step = len(x) - int(230 * sps), int(5 * sps)
    ((_, c, state, _),) = ref.exact(build_dir, [(params, x[:first])])
    hs, done = [np.nan] * int(c[0]), first
    while done < len(x):
        ((_, c, state, _),) = ref.exact(build_dir, [(params, x[done:done + step], state)])
        hs += [float(state[0, 1])] * int(c[0])
        done += step
    assert len(hs) == count and not np.isnan(hs[-200:]).any()
    return np.array(hs)


@pytest.mark.parametrize("sps,ppm,off,cplx", ACQ)
def test_acquisition_exact(hz, build_dir, sps, ppm, off, cplx):
    a, sps_true, x, params = acquisition_case(hz, sps, ppm, off, cplx)
    ((y, counts, z, neg),) = ref.exact(build_dir, [(params, x)])
    assert neg == 0
    y = y[0, :counts[0]]
    check_acquired(f"float32 sps {sps}", y, h_trace(build_dir, params, x, len(y)), a, sps_true, cplx)


@pytest.mark.parametrize("sps,ppm,off,cplx", ACQ)
def test_acquisition_float64(hz, sps, ppm, off, cplx):
    a, sps_true, x, params = acquisition_case(hz, sps, ppm, off, cplx)
    y, hs = ref.float64(params, x)
    check_acquired(f"float64 sps {sps}", y, hs, a, sps_true, cplx)


@pytest.mark.parametrize("sps,ppm,off,cplx", [ACQ[0], ACQ[2]])
def test_acquisition_in_noise(hz, build_dir, sps, ppm, off, cplx):
    """white noise 15 dB under the symbols: at most 5 of the 1980 symbols behind the first 1000 differ"""
    a, _, x, params = acquisition_case(hz, sps, ppm, off, cplx, noise_db=-15.0)
    ((y, counts, _, _),) = ref.exact(build_dir, [(params, x)])
    y64, _ = ref.float64(params, x)
    for name, v in (("float32", y[0, :counts[0]]), ("float64", y64)):
        lag, bad, n = ref.best_lag(v[:LAST], a, SKIP)
        print(f"{name} sps {sps} in noise: lag {lag}, {bad} of {n} signs differ")
        assert n == 1980 and bad <= 5


def test_the_restatements_agree(hz, build_dir):
    """the program's float32 symbols against the float64 loop's over the first 300 symbols of a locked-in case: the
    same count, and symbols within 1e-3 (the loops are coupled to their own rounding through e, so this is a
    consistency check of two implementations, not a rounding bound)"""
    a, _, x, params = acquisition_case(hz, 5.0, 200.0, 0.37, False)
    ((y, counts, _, _),) = ref.exact(build_dir, [(params, x[:1500])])
    y64, _ = ref.float64(params, x[:1500])
    assert counts[0] == len(y64) and np.abs(y[0, :counts[0]] - y64).max() <= 1e-3


# ---- the bound and the invariants --------------------------------------------------------------------

SATURATING = [(2.5, 0.1, 0.1), (2.25, 0.0, 0.125), (3.0, 0.25, 0.125)]


@pytest.mark.parametrize("sps,limit,g_mu", SATURATING)
def test_counter_and_bound_under_saturating_input(build_dir, sps, limit, g_mu):
    """20 000 white samples of amplitude 4 drive e to both rails: the counter never goes below 0 and the count stays
    inside max_symbols, for the whole stream and for every push of a stream cut into pushes of 1 ... 700 samples."""
    rng = np.random.default_rng(int(sps * 100))
    x = rng.uniform(-4.0, 4.0, 20_000).astype(np.float32)
    params = np.array([sps, limit, g_mu, 0.05], np.float32)
    assert ref.accepted(params)
    ((y, counts, z, neg),) = ref.exact(build_dir, [(params, x)])
    bound = ref.max_symbols(len(x), params)
    (_, _, hmin, hmax, least), = ref.derive(build_dir, [params])
    assert bound == ref.bound(build_dir, len(x), least)
    print(f"sps {sps} limit {limit} g_mu {g_mu}: {counts[0]} symbols, bound {bound}, h ends at {z[0, 1]} in [{hmin}, {hmax}]")
    assert neg == 0 and counts[0] <= bound and hmin <= z[0, 1] <= hmax
    assert counts[0] > 0.5 * bound, "the input does not press on the bound"
    state, done, size, total = None, 0, 1, 0
    while done < len(x):
        case = (params, x[done:done + size]) if state is None else (params, x[done:done + size], state)
        ((_, c, state, ng),) = ref.exact(build_dir, [case])
        n = len(x[done:done + size])
        assert ng == 0 and c[0] <= ref.max_symbols(n, params), f"a push of {n} samples at {done} wrote {c[0]}"
        total, done, size = total + int(c[0]), done + size, size * 3 + 1 if size < 700 else 1
    assert total == counts[0] and np.array_equal(bits(state), bits(z))


def test_refused_parameters(hz, build_dir):
    """each parameter just outside its range, and hmin - g_mu one ulp under 1: by csrc/hz_symsync_plan.h's validation
    (the library's) and by the restatement of the header's text"""
    up = lambda v, to=np.inf: np.nextafter(np.float32(v), np.float32(to))  # noqa: E731
    sets = [((5, 0.01, 0.1, 0.002), True), ((2.0, 0, 0, 0), False), ((up(2.0), 0, 0, 0), True), ((256.0, 0, 0, 0), True), ((up(256.0), 0, 0, 0), False),
            ((5, 0.25, 0, 0), True), ((5, up(0.25), 0, 0), False), ((5, -1e-9, 0, 0), False), ((5, 0, -1e-9, 0), False), ((5, 0, 0, -1e-9), False),
            ((5, 0, 1.5, 0), True), ((5, 0, up(1.5), 0), False), ((2.25, 0, 0.125, 0), True), ((2.25, 0, 0.125 + 2.0 ** -24, 0), False),
            ((np.nan, 0, 0, 0), False), ((5, np.inf, 0, 0), False), ((5, 0, np.nan, 0), False), ((5, 0, 0, np.inf), False)]
    q = np.array([s for s, _ in sets], np.float32)
    # hmin - g_mu of the one-ulp case is 1 - 2^-24 exactly
    assert np.float32(1.125) - q[13, 2] == np.float32(1.0) - np.float32(2.0 ** -24)
    got = ref.derive(build_dir, q)
    for (s, want), (ok, h0, hmin, hmax, _) in zip(sets, got):
        assert ok == want == ref.accepted(s), f"{s}: the library says {ok}, the header's text {ref.accepted(s)}"
        if ok:
            assert (h0, hmin, hmax) == ref.loop_constants(np.array(s, np.float32)), s


# ---- cuts ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cplx", [False, True])
def test_cuts(hz, build_dir, cplx):
    """any partition of a stream, pushes of 0, 1, 2 and 3 samples included, gives the symbols, the total counts and the
    final state of one push"""
    a, _, x, params = acquisition_case(hz, 5.0, 200.0, 0.37, cplx)
    x = x[:900]
    ((y, counts, z, _),) = ref.exact(build_dir, [(params, x)])
    rng = np.random.default_rng(1)
    for trial in range(3):
        sizes = [0, 1, 2, 3] + [int(v) for v in rng.integers(0, 90, 14)]
        rng.shuffle(sizes)
        state, done, parts = None, 0, []
        for size in sizes + [len(x)]:
            case = (params, x[done:done + size]) if state is None else (params, x[done:done + size], state)
            ((yy, c, state, _),) = ref.exact(build_dir, [case])
            parts.append(yy[0, :c[0]])
            done += size
        got = np.concatenate(parts)
        assert len(got) == counts[0] and np.array_equal(bits(got), bits(y[0, :counts[0]])) and np.array_equal(bits(state), bits(z))

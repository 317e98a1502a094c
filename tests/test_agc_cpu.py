"""The AGC bank (include/hzsdr_agc.h) without a GPU: the ABI's header, exports and bindings; the validation at every
bound's edge and one ulp outside; the host program tests/host/agc_ref.cpp (the bits the device must produce) on exact
read-outs, on settling from four levels, against the float64 restatement of tests/agc_ref.py, on every branch of the
step, on cuts, new parameters, a NaN and an infinity kept to their sample."""
import importlib
import math
import os
import re
import subprocess

import numpy as np
import pytest

import agc_ref as ref
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "hzsdr_agc.h")
ENTRIES = {"hzsdr_agc_create", "hzsdr_agc_push", "hzsdr_agc_set_params", "hzsdr_agc_get_state", "hzsdr_agc_set_state", "hzsdr_agc_position",
           "hzsdr_agc_plan", "hzsdr_agc_reset", "hzsdr_agc_free"}
GCC = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include")]

# the loop of the settling tests: ref 1, down fast, up slowly, no gate, a range wide enough for every level
ATTACK, DECAY = 0.1, 0.01
PARAMS = np.array([1.0, ATTACK, DECAY, 0.0, 1.0, 2.0 ** -20, 2.0 ** 20], np.float32)
LEVELS = (1e-3, 0.03, 30.0, 1e3)
N = 3000

# the program against the float64 restatement over the settling rows and noisy QPSK (test_program_against_float64),
# as DESIGN.md records them
DEV_OUTPUT, DEV_GAIN = 5.67e-06, 5.67e-06


@pytest.fixture(scope="module")
def hz():
    return importlib.import_module("go-sdr_amd")


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("agc_ref"))


def agc_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(hzsdr_[a-z0-9_]+)\s*\(", text)))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def up(v):
    return np.nextafter(np.float32(v), np.float32(np.inf))


def down(v):
    return np.nextafter(np.float32(v), np.float32(-np.inf))


# ---- the ABI ---------------------------------------------------------------------------------------

def test_header_is_c99(tmp_path):
    src = tmp_path / "inc.c"
    src.write_text('#include "hzsdr_agc.h"\n'
                   "int main(void) { hzsdr_agc *f = 0; return (f != 0) + HZSDR_AGC_REAL_F32 - HZSDR_AGC_FORM_PER_ROW - HZSDR_AGC_FORM_COMPLEX"
                   " - HZSDR_AGC_MAX_ROWS - HZSDR_AGC_PARAMS; }\n")
    subprocess.check_call(GCC + ["-c", str(src), "-o", str(tmp_path / "inc.o")])


def test_header_declares_exactly_the_entries():
    assert len(ENTRIES) == 9 and set(agc_symbols()) == ENTRIES


def test_library_exports_and_ctypes_table(hz):
    capi = importlib.import_module("go-sdr_amd._capi")
    syms = agc_symbols()
    for s in syms:
        assert hasattr(capi.lib, s), f"{s} declared in hzsdr_agc.h but not exported"
    assert sorted(capi.AGC_SIGNATURES) == syms
    for name, (res, args) in capi.AGC_SIGNATURES.items():
        fn = getattr(capi.lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    found = re.findall(r"\bint (hzsdr_agc_[a-z_]+)\s*\(([^)]*)\)", text)
    assert {name for name, _ in found} == ENTRIES
    for name, params in found:
        assert len(capi.AGC_SIGNATURES[name][1]) == len(params.split(",")), name


def test_constants_and_python_layers(hz):
    defs = dict(re.findall(r"#define (HZSDR_\w+) (\d+)", open(HEADER).read()))
    assert int(defs["HZSDR_AGC_REAL_F32"]) == hz.AGC_REAL_F32 == hz.IIR_REAL_F32 == hz.SYMSYNC_REAL_F32 == ref.REAL_F32 == 32
    assert hz.FMT_C64 == ref.C64
    assert int(defs["HZSDR_AGC_FORM_PER_ROW"]) == hz.AGC_FORM_PER_ROW == ref.FORM_PER_ROW == 1
    assert int(defs["HZSDR_AGC_FORM_COMPLEX"]) == hz.AGC_FORM_COMPLEX == ref.FORM_COMPLEX == 2
    assert int(defs["HZSDR_AGC_MAX_ROWS"]) == hz.AGC_MAX_ROWS == ref.MAX_ROWS == 8192
    assert int(defs["HZSDR_AGC_PARAMS"]) == 7
    st = importlib.import_module("go-sdr_amd.stream")
    mod = importlib.import_module("go-sdr_amd.agc")
    assert hz.Agc is mod.Agc and hz.agc_rates is mod.agc_rates and callable(mod.level) and callable(hz.Context.agc) and callable(st.agc_rows)
    for name in ("push", "set_params", "state", "set_state", "position", "reset", "plan", "close", "__enter__", "__exit__"):
        assert callable(getattr(hz.Agc, name)), name
    hpp = open(os.path.join(ROOT, "go-sdr_amd", "cxx", "hzsdr.hpp")).read()
    assert "class Agc" in hpp and '#include "../../include/hzsdr_agc.h"' in hpp
    make = open(os.path.join(ROOT, "go-sdr_amd", "csrc", "Makefile")).read()
    assert "hzsdr_agc.h" in make and "hz_agc" not in make.split("MFMA_UNITS =")[1].splitlines()[0]
    # the sentences that said there was no AGC point to the bank
    for path in (os.path.join(ROOT, "include", "hzsdr_carrier.h"), os.path.join(ROOT, "go-sdr_amd", "carrier.py")):
        text = open(path).read()
        assert "hzsdr_agc.h" in text and "Not here: AGC" not in text, path


def test_agc_rates_and_level(hz):
    mod = importlib.import_module("go-sdr_amd.agc")
    assert hz.agc_rates(10, 100) == pytest.approx(ref.rates(10, 100), rel=1e-14)
    a, d = hz.agc_rates(1.0 / math.log(2.0) * (1 + 1e-9), 1e9)
    assert a <= 0.5 and a == pytest.approx(0.5, rel=1e-8) and d == pytest.approx(1e-9, rel=1e-6)
    for bad in ((1.4, 100), (100, 1.0), (0.0, 10), (10, -1.0)):
        with pytest.raises(ValueError):
            hz.agc_rates(*bad)
    g = np.array([0.5, 4.0, 1.0], np.float32)
    assert np.array_equal(mod.level(g, 2.0), np.array([4.0, 0.5, 2.0], np.float32))


# ---- the validation --------------------------------------------------------------------------------

GOOD = [1.0, 0.1, 0.01, 0.0, 1.0, 0.5, 2.0]


def with_(**kw):
    names = ["ref", "attack", "decay", "floor", "g0", "gmin", "gmax"]
    q = [np.float32(v) for v in GOOD]
    for k, v in kw.items():
        q[names.index(k)] = np.float32(v)
    return q


def test_restated_validation(build_dir):
    """Each bound at its edge (accepted) and one ulp outside (refused), the order gmin <= g0 <= gmax, the values that
    are not finite: csrc/hz_agc_plan.h against the rules restated in Python; and iref, computed in float64."""
    lo, hi = np.float32(ref.LOW), np.float32(ref.HIGH)
    edges = [
        (with_(), True),
        (with_(ref=lo, gmin=lo, g0=lo, gmax=lo), True), (with_(ref=hi, gmin=hi, g0=hi, gmax=hi), True),
        (with_(ref=down(lo)), False), (with_(ref=up(hi)), False), (with_(ref=0.0), False), (with_(ref=-1.0), False),
        (with_(attack=0.0, decay=0.0), True), (with_(attack=0.5, decay=0.5), True),
        (with_(attack=up(0.5)), False), (with_(decay=up(0.5)), False), (with_(attack=down(0.0)), False), (with_(decay=down(0.0)), False),
        (with_(floor=0.0), True), (with_(floor=-0.0), True), (with_(floor=down(0.0)), False), (with_(floor=np.finfo(np.float32).max), True),
        (with_(gmin=lo), True), (with_(gmin=down(lo)), False), (with_(gmax=hi), True), (with_(gmax=up(hi)), False),
        (with_(gmin=1.0, g0=1.0, gmax=1.0), True), (with_(gmin=up(1.0)), False), (with_(gmax=down(1.0)), False),
        (with_(gmin=2.0, gmax=0.5), False),
    ]
    for k in range(7):
        for bad in (np.nan, np.inf, -np.inf):
            q = with_()
            q[k] = np.float32(bad)
            edges.append((q, False))
    rng = np.random.default_rng(5)
    rand = np.exp(rng.uniform(-50, 50, (200, 7))).astype(np.float32)
    rand[:, 1:3] = rng.uniform(-0.1, 0.6, (200, 2))
    rand[:, 3] = rng.uniform(-0.1, 1.0, 200)
    rand[:100, 4:] = np.sort(rand[:100, 4:], axis=1)[:, [1, 0, 2]]
    sets = np.array([e[0] for e in edges] + list(rand), np.float32)
    got = ref.derive(build_dir, sets)
    for q, want in edges:
        assert ref.accepted(q) == want, q
    assert sum(g[0] for g in got) > 30 and sum(not g[0] for g in got) > 30
    for p, (ok, iref) in zip(sets, got):
        assert ok == ref.accepted(p), p
        if ok:
            assert iref == ref.iref_of(p) and ref.LOW <= iref <= ref.HIGH, p


# ---- exact read-outs ---------------------------------------------------------------------------------

@pytest.mark.parametrize("cplx", [False, True])
def test_exact_readouts(build_dir, cplx):
    """attack = decay = 0 returns x g0 bit for bit; a floor above every level holds g; a constant level equal to ref
    leaves g at g0."""
    x = ref.white((2, 300), 31, cplx)
    g0 = np.float32(1.7)
    frozen = np.array([1.0, 0.0, 0.0, 0.0, g0, 0.5, 2.0], np.float32)
    gated = np.array([0.25, 0.5, 0.5, 2.0, g0, 0.5, 2.0], np.float32)
    (y, tr, z), (yg, tg, zg) = ref.exact(build_dir, [(frozen, x), (gated, x)])
    want = (x.view(np.float32) * g0).view(x.dtype)
    for got_y, got_t, got_z in ((y, tr, z), (yg, tg, zg)):
        assert np.array_equal(bits(got_y), bits(want)) and (got_t == g0).all() and (got_z == g0).all()
    # a constant level equal to ref: b g0 = 1 exactly for powers of two, e = 0, g stays
    for level, g0 in ((0.5, 2.0), (4.0, 0.25), (1.0, 1.0)):
        p = np.array([1.0, 0.5, 0.5, 0.0, g0, 2.0 ** -10, 2.0 ** 10], np.float32)
        xc = ref.constant_modulus(300, level, 3, False)
        if cplx:
            xc = (xc * (1j ** np.arange(300))).astype(np.complex64)  # on the axes: the modulus is exact
        (y, tr, z), = ref.exact(build_dir, [(p, xc)])
        assert (tr == np.float32(g0)).all() and z[0] == np.float32(g0) and (np.abs(y) == 1.0).all()


# ---- settling, and the program against float64 -----------------------------------------------------------

@pytest.fixture(scope="module")
def settle_runs(build_dir):
    """[(level, complex, x, program's (y, track, state), float64's (y, track, g))]: every level, both kinds, and noisy
    QPSK at level 0.2, computed once"""
    rows = [(lev, cplx, ref.constant_modulus(N, lev, 40 + k, cplx)) for k, lev in enumerate(LEVELS) for cplx in (True, False)]
    rows.append((0.2, True, ref.noisy_qpsk(N, 0.2, 50)))
    got = ref.exact(build_dir, [(PARAMS, x) for _, _, x in rows])
    return [(lev, cplx, x, g, ref.float64(PARAMS, x)) for (lev, cplx, x), g in zip(rows, got)]


def test_settling_does_not_depend_on_the_level(settle_runs):
    """Constant-modulus rows at 1e-3, 0.03, 30 and 1e3 with attack 0.1, decay 0.01, ref 1: from the sample
    agc_ref.settle_bound gives -- the geometric approach and the last 5 %, times 1.1 -- |y| stays within 5 % of ref."""
    for lev, cplx, x, (y, tr, z), _ in settle_runs[:-1]:
        bound = math.ceil(ref.settle_bound(lev, 1.0, ATTACK, DECAY))
        off = np.nonzero(np.abs(np.abs(y[0].astype(np.complex128)) - 1.0) > 0.05)[0]
        last = int(off.max()) + 1 if len(off) else 0
        print(f"level {lev} complex {cplx}: within 5 % from sample {last} (bound {bound})")
        assert bound < N and last <= bound
        assert abs(float(z[0]) * lev - 1.0) < 0.05


def test_program_against_float64(settle_runs):
    """Outputs and gain of the program against the float64 restatement over the settling rows and noisy QPSK at level
    0.2.  The two trajectories differ by float32 roundings: while the gain slews (up to 700 steps of a factor 1.01) one
    rounding of g per step adds up, and the settled loop contracts the sum at the rates attack and decay.  Measured:
    outputs 5.67e-06 of max(ref, |y|), gain 5.67e-06 of the gain (both in the quietest row, at the end of its slew).
    Asserted: four times that."""
    dy = dg = 0.0
    for lev, cplx, x, (y, tr, z), (y64, tr64, g64) in settle_runs:
        scale = np.maximum(1.0, np.abs(y64))
        dy = max(dy, float((np.abs(y[0].astype(y64.dtype) - y64) / scale).max()))
        dg = max(dg, float((np.abs(tr[0].astype(np.float64) - tr64) / tr64).max()), abs(float(z[0]) - g64) / g64)
    print(f"largest deviations: outputs {dy:.3e} of max(ref, |y|), gain {dg:.3e} of the gain")
    assert dy <= 4 * DEV_OUTPUT and dg <= 4 * DEV_GAIN
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert f"{DEV_OUTPUT:.2e}" in design and f"{DEV_GAIN:.2e}" in design


# ---- every branch ------------------------------------------------------------------------------------

@pytest.mark.parametrize("cplx", [False, True])
def test_white_rows_reach_every_branch(build_dir, cplx):
    """White rows of 255 samples, four seeds: the loud set reaches attack, decay, the clip at -1, the gate and the clamp
    at gmin, the quiet set the clamp at gmax, counted by the host program from the header's step.  (How often depends on
    the generator; with this one, complex rows: attack >= 202, decay >= 30, clip >= 55, gate >= 7, gmin >= 199,
    gmax >= 241; real rows: 125, 65, 5, 44, 115, 195.)"""
    for seed in (1, 2, 3, 4):
        x = ref.white((255,), seed, cplx)
        (_, _, _, loud), (_, _, _, quiet) = ref.exact(build_dir, [(ref.LOUD, x), (ref.QUIET, x)], branches=True)
        print(f"seed {seed}: loud {loud}, quiet {quiet}")
        for name in ("attack", "decay", "clip", "gate", "gmin"):
            assert loud[name] >= 5, name
        assert quiet["gmax"] >= 190
        assert loud["attack"] + loud["decay"] + loud["gate"] <= 255


# ---- cuts, new parameters, NaN -----------------------------------------------------------------------------

@pytest.mark.parametrize("cplx", [False, True])
def test_track_is_the_gain_applied(build_dir, cplx):
    """track[n] is the gain BEFORE sample n's step, y[n] = x[n] * track[n], and the state behind n samples is
    track[n] of a longer run"""
    x = ref.white((41,), 3, cplx)
    (y, tr, z), = ref.exact(build_dir, [(ref.LOUD, x)])
    assert tr[0, 0] == ref.LOUD[4]
    want = (x.view(np.float32).reshape(41, -1) * tr[0][:, None]).reshape(-1)
    assert np.array_equal(bits(y).reshape(-1), bits(want))
    for n, (yn, trn, zn) in zip(range(1, 41), ref.exact(build_dir, [(ref.LOUD, x[:n]) for n in range(1, 41)])):
        assert zn[0] == tr[0, n] and np.array_equal(bits(trn), bits(tr[:, :n]))


def test_cuts_and_new_parameters(build_dir):
    """one run equals the same stream cut at 1, 255, 256 and 257 samples with the state carried; new parameters between
    two pushes keep g, and g is held to the new range BEHIND the next sample"""
    x = np.stack([ref.noisy_qpsk(1000, 0.2, 11), ref.white((1000,), 12)])
    (y, tr, z), = ref.exact(build_dir, [(PARAMS, x)])
    for cut in (1, 255, 256, 257):
        (ya, ta, za), = ref.exact(build_dir, [(PARAMS, x[:, :cut])])
        (yb, tb, zb), = ref.exact(build_dir, [(PARAMS, x[:, cut:], za)])
        assert np.array_equal(bits(np.hstack([ya, yb])), bits(y)) and np.array_equal(bits(np.hstack([ta, tb])), bits(tr)) and np.array_equal(zb, z)
    narrow = np.array([1.0, ATTACK, DECAY, 0.0, 1.0, 0.5, 2.0], np.float32)
    (y2, t2, z2), = ref.exact(build_dir, [([(0, PARAMS), (600, narrow)], x)])
    (ya, ta, za), = ref.exact(build_dir, [(PARAMS, x[:, :600])])
    (yb, tb, zb), = ref.exact(build_dir, [(narrow, x[:, 600:], za)])
    assert np.array_equal(bits(np.hstack([ya, yb])), bits(y2)) and np.array_equal(zb, z2)
    assert np.array_equal(bits(y2[:, :601]), bits(y[:, :601]))  # (sample 600 still sees the gain it had)
    assert t2[0, 600] > 2.0 and t2[0, 601] == 2.0 and t2[:, 601:].max() <= 2.0 and t2[:, 601:].min() >= 0.5


@pytest.mark.parametrize("cplx", [False, True])
def test_nan_and_infinity_stay_in_their_sample(build_dir, cplx):
    """A NaN sample: a NaN output for that sample, and g holds as it does for a sample of zero error (a sample whose
    level times the gain is exactly ref cannot be made in general, so: the row with the sample GATED, which holds g as
    well).  An infinity: e = -1, the gain falls by the factor 1 - attack, the row goes on finite.  The other rows are
    untouched.  A NaN gain stays."""
    x = ref.white((3, 300), 21, cplx)
    p = np.array([0.5, 0.25, 0.125, 1e-3, 1.0, 2.0 ** -10, 2.0 ** 10], np.float32)
    bad, held, inf = x.copy(), x.copy(), x.copy()
    bad[1, 100], held[1, 100], inf[1, 100] = np.nan, 0.0, np.inf
    (yb, tb, zb), (yh, th, zh), (yi, ti, zi), (y, tr, z) = ref.exact(build_dir, [(p, bad), (p, held), (p, inf), (p, x)])
    assert np.isnan(yb[1, 100])
    keep = np.ones(x.shape, bool)
    keep[1, 100] = False
    assert np.array_equal(bits(yb[keep]), bits(yh[keep])) and np.array_equal(bits(tb), bits(th)) and np.array_equal(zb, zh)
    assert tb[1, 101] == tb[1, 100] and not np.isnan(yb[keep]).any()
    assert np.array_equal(bits(yi[[0, 2]]), bits(y[[0, 2]])) and np.array_equal(zi[[0, 2]], z[[0, 2]])
    assert not np.isfinite(yi[1, 100]) and np.isfinite(yi[keep]).all() and np.isfinite(ti).all()
    assert ti[1, 101] == np.float32(ti[1, 100] * np.float32(0.75))  # fmaf(g, -0.25, g): exact in float64, rounded once
    (yn, tn, zn), = ref.exact(build_dir, [(p, x, np.array([1.0, np.nan, 2.0], np.float32))])
    assert np.isnan(yn[1]).all() and np.isnan(tn[1]).all() and np.isnan(zn[1]) and np.isfinite(yn[[0, 2]]).all()

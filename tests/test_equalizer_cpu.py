"""The equalizer bank (include/hzsdr_equalizer.h) without a GPU: the ABI's header, exports and bindings; the validation
at every bound's edge and one ulp outside; the host program tests/host/equalizer_ref.cpp (the bits the device must
produce) on exact read-outs, on one hand-computed update per mode, bit for bit against the numpy restatement of
tests/equalizer_ref.py for every tap count that changes the butterfly, on cuts, on ragged counts, on a NaN kept to its
row; and the convergence case on the restatement."""
import importlib
import math
import os
import re
import subprocess

import numpy as np
import pytest

import equalizer_ref as ref
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "hzsdr_equalizer.h")
ENTRIES = {"hzsdr_equalizer_create", "hzsdr_equalizer_push", "hzsdr_equalizer_set_params", "hzsdr_equalizer_get_state", "hzsdr_equalizer_set_state",
           "hzsdr_equalizer_plan", "hzsdr_equalizer_reset", "hzsdr_equalizer_free"}
GCC = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include")]
TAPS = (1, 2, 3, 5, 8, 11, 17, 32, 33, 64)
f32 = np.float32


@pytest.fixture(scope="module")
def hz():
    return importlib.import_module("go-sdr_amd")


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("equalizer_ref"))


def header_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(hzsdr_[a-z0-9_]+)\s*\(", text)))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def up(v):
    return np.nextafter(f32(v), f32(np.inf))


def down(v):
    return np.nextafter(f32(v), f32(-np.inf))


def modes_of(cplx):
    return (ref.CMA, ref.DD_BPSK, ref.DD_QPSK) if cplx else (ref.CMA, ref.DD_BPSK)


# ---- the ABI ---------------------------------------------------------------------------------------

def test_header_is_c99(tmp_path):
    src = tmp_path / "inc.c"
    src.write_text('#include "hzsdr_equalizer.h"\n'
                   "int main(void) { hzsdr_equalizer *f = 0; return (f != 0) + HZSDR_EQUALIZER_REAL_F32 - HZSDR_EQUALIZER_FORM_PER_ROW"
                   " - HZSDR_EQUALIZER_FORM_COMPLEX - HZSDR_EQUALIZER_MAX_ROWS - HZSDR_EQUALIZER_MAX_TAPS - HZSDR_EQUALIZER_PARAMS"
                   " - HZSDR_EQUALIZER_CMA - HZSDR_EQUALIZER_DD_BPSK - HZSDR_EQUALIZER_DD_QPSK; }\n")
    subprocess.check_call(GCC + ["-c", str(src), "-o", str(tmp_path / "inc.o")])


def test_header_declares_exactly_the_entries():
    assert len(ENTRIES) == 8 and set(header_symbols()) == ENTRIES


def test_library_exports_and_ctypes_table(hz):
    capi = importlib.import_module("go-sdr_amd._capi")
    syms = header_symbols()
    for s in syms:
        assert hasattr(capi.lib, s), f"{s} declared in hzsdr_equalizer.h but not exported"
    assert sorted(capi.EQUALIZER_SIGNATURES) == syms
    for name, (res, args) in capi.EQUALIZER_SIGNATURES.items():
        fn = getattr(capi.lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    found = re.findall(r"\bint (hzsdr_equalizer_[a-z_]+)\s*\(([^)]*)\)", text)
    assert {name for name, _ in found} == ENTRIES
    for name, params in found:
        assert len(capi.EQUALIZER_SIGNATURES[name][1]) == len(params.split(",")), name


def test_constants_and_python_layers(hz):
    defs = dict(re.findall(r"#define (HZSDR_\w+) (\d+)", open(HEADER).read()))
    assert int(defs["HZSDR_EQUALIZER_REAL_F32"]) == hz.EQUALIZER_REAL_F32 == hz.IIR_REAL_F32 == hz.SYMSYNC_REAL_F32 == hz.AGC_REAL_F32 == ref.REAL_F32 == 32
    assert hz.FMT_C64 == ref.C64
    assert int(defs["HZSDR_EQUALIZER_CMA"]) == hz.EQUALIZER_CMA == ref.CMA == 0
    assert int(defs["HZSDR_EQUALIZER_DD_BPSK"]) == hz.EQUALIZER_DD_BPSK == ref.DD_BPSK == 1
    assert int(defs["HZSDR_EQUALIZER_DD_QPSK"]) == hz.EQUALIZER_DD_QPSK == ref.DD_QPSK == 2
    assert int(defs["HZSDR_EQUALIZER_FORM_PER_ROW"]) == hz.EQUALIZER_FORM_PER_ROW == ref.FORM_PER_ROW == 1
    assert int(defs["HZSDR_EQUALIZER_FORM_COMPLEX"]) == hz.EQUALIZER_FORM_COMPLEX == ref.FORM_COMPLEX == 2
    assert int(defs["HZSDR_EQUALIZER_MAX_ROWS"]) == hz.EQUALIZER_MAX_ROWS == ref.MAX_ROWS == 8192
    assert int(defs["HZSDR_EQUALIZER_MAX_TAPS"]) == hz.EQUALIZER_MAX_TAPS == ref.MAX_TAPS == 64
    assert int(defs["HZSDR_EQUALIZER_PARAMS"]) == 2
    # the same values in the headers the kernel is built from
    math_h = open(os.path.join(ROOT, "go-sdr_amd", "csrc", "hz_equalizer_math.h")).read()
    plan_h = open(os.path.join(ROOT, "go-sdr_amd", "csrc", "hz_equalizer_plan.h")).read()
    assert "kCma = 0, kDdBpsk = 1, kDdQpsk = 2" in math_h and "kRealF32 = 32, kC64 = 1" in plan_h and "kMaxTaps = 64" in plan_h
    st = importlib.import_module("go-sdr_amd.stream")
    mod = importlib.import_module("go-sdr_amd.equalizer")
    assert hz.Equalizer is mod.Equalizer and callable(hz.Context.equalizer) and callable(st.equalized_rows)
    for name in ("push", "set_params", "state", "set_state", "reset", "plan", "close", "__enter__", "__exit__"):
        assert callable(getattr(hz.Equalizer, name)), name
    hpp = open(os.path.join(ROOT, "go-sdr_amd", "cxx", "hzsdr.hpp")).read()
    assert "class Equalizer" in hpp and '#include "../../include/hzsdr_equalizer.h"' in hpp
    for name, value in re.findall(r"#define (HZSDR_EQUALIZER_\w+) (\d+)", open(HEADER).read()):
        assert int(value) == getattr(hz, name[len("HZSDR_"):], int(value)), name
    make = open(os.path.join(ROOT, "go-sdr_amd", "csrc", "Makefile")).read()
    assert "hzsdr_equalizer.h" in make and "hz_equalizer" not in make.split("MFMA_UNITS =")[1].splitlines()[0]


# ---- the validation --------------------------------------------------------------------------------

def test_restated_validation(build_dir):
    """Each bound at its edge (accepted) and one ulp outside (refused), the values that are not finite, the geometry at
    its edges: csrc/hz_equalizer_plan.h against the rules restated in Python."""
    lo, hi = f32(ref.LOW), f32(ref.HIGH)
    sets = [((0.0, lo), True), ((1.0, hi), True), ((-0.0, 1.0), True), ((up(1.0), 1.0), False), ((down(0.0), 1.0), False),
            ((0.5, down(lo)), False), ((0.5, up(hi)), False), ((0.5, 0.0), False), ((0.5, -1.0), False)]
    sets += [((bad, 1.0), False) for bad in (np.nan, np.inf, -np.inf)] + [((0.5, bad), False) for bad in (np.nan, np.inf, -np.inf)]
    rng = np.random.default_rng(5)
    rand = [((float(f32(rng.uniform(-0.2, 1.2))), float(f32(np.exp(rng.uniform(-50, 50))))), None) for _ in range(200)]
    geoms = [((1, 0, ref.CMA, c), True) for c in (0, 1)] + [((64, 63, ref.DD_BPSK, c), True) for c in (0, 1)]
    geoms += [((0, 0, ref.CMA, 1), False), ((65, 0, ref.CMA, 1), False), ((8, 8, ref.CMA, 1), False), ((8, -1, ref.CMA, 1), False),
              ((8, 4, -1, 1), False), ((8, 4, 3, 1), False), ((8, 4, ref.DD_QPSK, 1), True), ((8, 4, ref.DD_QPSK, 0), False)]
    records = [(q[0], q[1], 8, 4, ref.CMA, 1) for q, _ in sets + rand] + [(0.5, 1.0) + g for g, _ in geoms]
    got = ref.check(build_dir, records)
    for (q, want), (ok, gok) in zip(sets + rand, got):
        assert ref.accepted(q) == ok and gok and (want is None or ok == want), q
    assert sum(ok for ok, _ in got[len(sets):len(sets) + 200]) > 30 and sum(not ok for ok, _ in got[len(sets):len(sets) + 200]) > 30
    for (g, want), (ok, gok) in zip(geoms, got[len(sets) + 200:]):
        assert ok and gok == want == ref.geometry_accepted(*g), g


# ---- exact read-outs ---------------------------------------------------------------------------------

@pytest.mark.parametrize("cplx", [False, True])
def test_one_tap_with_mu_0_is_a_copy_times_w(build_dir, cplx):
    x = ref.white((3, 200), 31, cplx)
    w = (f32(0.75), f32(-1.5)) if cplx else (f32(-1.25),)
    z = np.tile(np.array(w, f32), (3, 1))
    (fresh, _, z0), (y, _, z1) = ref.exact(build_dir, [(ref.CMA, 1, 0, (0.0, 1.0), x), (ref.CMA, 1, 0, (0.0, 1.0), x, z)])
    assert np.array_equal(bits(fresh), bits(x)) and np.array_equal(z0, ref.initial_state(3, 1, 0, cplx)) and np.array_equal(z1, z)
    if cplx:
        xr, xi = x.real, x.imag
        want = ref.fmaf(-w[1], xi, w[0] * xr) + 1j * ref.fmaf(w[1], xr, w[0] * xi)
        assert np.array_equal(bits(y), bits(want.astype(np.complex64)))
    else:
        assert np.array_equal(bits(y), bits(w[0] * x))


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("taps", [3, 11, 33, 64])
def test_an_impulse_reads_out_the_taps(build_dir, cplx, taps):
    """mu = 0, taps of small integers over 4 (sums exact in float32): a unit impulse gives the taps in order, an impulse
    of i (complex rows) gives them turned by a quarter; the state behind holds the inputs newest first."""
    rng = np.random.default_rng(taps)
    w = (rng.integers(-8, 9, taps) / 4.0 + (1j * rng.integers(-8, 9, taps) / 4.0 if cplx else 0)).astype(np.complex64 if cplx else f32)
    z = np.zeros((1, ref.state_width(taps, cplx)), f32)
    z[0, :w.view(f32).size] = w.view(f32)
    x = np.zeros(taps + 5, w.dtype)
    x[2] = 1j if cplx else 1.0
    ((y, tr, z1),) = ref.exact(build_dir, [(ref.DD_BPSK, taps, 0, (0.0, 1.0), x, z)])
    want = np.zeros_like(x)
    want[2:2 + taps] = w * x[2]
    assert np.array_equal(y[0], want) and np.array_equal(z1[0, :w.view(f32).size], w.view(f32))
    hist = np.ascontiguousarray(x[::-1][:taps - 1])
    assert np.array_equal(z1[0, w.view(f32).size:], hist.view(f32))


def test_one_hand_computed_update_per_mode(build_dir):
    """N = 2, c = 0, the state w = (1, 0), history 0.5 (complex: 0.5 - 0.25i), mu = 0.5: every value below is exact in
    float32, worked out by hand from the header's step."""
    # complex rows: x = 0.5 + 0.5i, y = w0 x = 0.5 + 0.5i, |y|^2 = 0.5
    x = np.array([0.5 + 0.5j], np.complex64)
    z = np.array([[1, 0, 0, 0, 0.5, -0.25]], f32)
    cases = [(ref.CMA, 2, 0, (0.5, 1.0), x, z), (ref.DD_QPSK, 2, 0, (0.5, 0.75), x, z), (ref.DD_BPSK, 2, 0, (0.5, 0.75), x, z)]
    (yc, tc, zc), (yq, tq, zq), (yb, tb, zb) = ref.exact(build_dir, cases)
    assert yc[0, 0] == yq[0, 0] == yb[0, 0] == 0.5 + 0.5j
    # CMA: c = 1 - 0.5 = 0.5, e = (0.25, 0.25), g = (0.125, 0.125); w0 += g conj(x) = (0.125 + 0.125i)(0.5 - 0.5i) = 0.125;
    # w1 += g conj(0.5 - 0.25i) = (0.125 + 0.125i)(0.5 + 0.25i) = 0.03125 + 0.09375i; track = 0.125
    assert np.array_equal(zc[0], np.array([1.125, 0, 0.03125, 0.09375, 0.5, 0.5], f32)) and tc[0, 0] == 0.125
    # DD_QPSK: e = (0.25, 0.25) again (0.75 - 0.5): the same update and track
    assert np.array_equal(zq[0], zc[0]) and tq[0, 0] == 0.125
    # DD_BPSK: e = (0.25, -0.5), g = (0.125, -0.25); w0 += (0.125 - 0.25i)(0.5 - 0.5i) = -0.0625 - 0.1875i;
    # w1 += (0.125 - 0.25i)(0.5 + 0.25i) = 0.125 - 0.09375i; track = 0.0625 + 0.25
    assert np.array_equal(zb[0], np.array([0.9375, -0.1875, 0.125, -0.09375, 0.5, 0.5], f32)) and tb[0, 0] == 0.3125
    # real rows: x = 0.5, history 0.25: y = 0.5; CMA e = (1 - 0.25) 0.5 = 0.375, g = 0.1875: w = (1.09375, 0.046875);
    # DD e = 0.75 - 0.5 = 0.25, g = 0.125: w = (1.0625, 0.03125)
    xr, zr = np.array([0.5], f32), np.array([[1, 0, 0.25]], f32)
    (y1, t1, z1), (y2, t2, z2) = ref.exact(build_dir, [(ref.CMA, 2, 0, (0.5, 1.0), xr, zr), (ref.DD_BPSK, 2, 0, (0.5, 0.75), xr, zr)])
    assert y1[0, 0] == y2[0, 0] == 0.5 and t1[0, 0] == f32(0.140625) and t2[0, 0] == 0.0625
    assert np.array_equal(z1[0], np.array([1.09375, 0.046875, 0.5], f32)) and np.array_equal(z2[0], np.array([1.0625, 0.03125, 0.5], f32))
    # the clip: a level of 16 gives e = 15.5 -> 1, g = 0.5: w = (1.25, 0.125)
    ((_, t3, z3),) = ref.exact(build_dir, [(ref.DD_BPSK, 2, 0, (0.5, 16.0), xr, zr)])
    assert np.array_equal(z3[0], np.array([1.25, 0.125, 0.5], f32)) and t3[0, 0] == 1.0


# ---- the program against the numpy restatement --------------------------------------------------------------

def test_fmaf_emulation_is_exact():
    """the emulation against exact rational arithmetic on random operands and on operands aimed at ties"""
    from fractions import Fraction
    rng = np.random.default_rng(1)
    a = (rng.standard_normal(3000) * np.exp(rng.uniform(-8, 8, 3000))).astype(f32)
    b = (rng.standard_normal(3000) * np.exp(rng.uniform(-8, 8, 3000))).astype(f32)
    c = np.where(rng.random(3000) < 0.5, -(a.astype(np.float64) * b).astype(f32), (rng.standard_normal(3000)).astype(f32)).astype(f32)
    # ties: a b = an odd multiple of half an ulp of c, plus or minus a little
    a[:500] = (1 + rng.integers(0, 2 ** 12, 500) * 2.0 ** -12).astype(f32)
    b[:500] = (2.0 ** -24 * (1 + 2.0 ** -11 * rng.integers(-1, 2, 500))).astype(f32)
    c[:500] = (1 + rng.integers(0, 2 ** 22, 500) * 2.0 ** -22).astype(f32)
    got = ref.fmaf(a, b, c)

    def nearest(fr):
        v = f32(float(fr))  # (may be doubly rounded: fix up against its neighbours)
        best = min((f32(np.nextafter(v, f32(-np.inf))), v, f32(np.nextafter(v, f32(np.inf)))), key=lambda u: (abs(Fraction(float(u)) - fr), int(f32(u).view(np.uint32)) & 1))
        return best
    for k in range(3000):
        want = nearest(Fraction(float(a[k])) * Fraction(float(b[k])) + Fraction(float(c[k])))
        assert got[k] == want, (a[k], b[k], c[k])


@pytest.mark.parametrize("cplx", [False, True])
def test_program_against_numpy_bit_for_bit(build_dir, cplx):
    """N in {1, 2, 3, 5, 8, 11, 17, 32, 33, 64}, every mode of the kind: outputs, track and state of 120 white symbols,
    then 40 more from the state carried, a step large enough for the taps to move and for the clip to be reached."""
    cases, runs = [], []
    for taps in TAPS:
        for mode in modes_of(cplx):
            x = ref.white((160,), 100 * taps + mode, cplx, 1.5)
            p = np.array([0.05, 0.5 if mode else 0.6], f32)
            cases.append((mode, taps, taps // 2, p, x))
    for case, (y, tr, z) in zip(cases, ref.exact(build_dir, cases)):
        mode, taps, c, p, x = case
        y1, t1, z1 = ref.restated(mode, taps, c, p, x[:120])
        y2, t2, z2 = ref.restated(mode, taps, c, p, x[120:], z1)
        what = f"taps {taps} mode {mode}"
        assert np.array_equal(bits(np.concatenate([y1, y2])), bits(y[0])), what
        assert np.array_equal(bits(np.concatenate([t1, t2])), bits(tr[0])) and np.array_equal(bits(z2), bits(z[0])), what
        runs.append(float(tr.max()))
        assert not np.array_equal(z[0], ref.initial_state(1, taps, c, cplx)[0])
    assert max(runs) >= 1.0  # (the clip was reached)


# ---- cuts, counts, NaN -------------------------------------------------------------------------------

@pytest.mark.parametrize("cplx", [False, True])
def test_cuts_and_counts(build_dir, cplx):
    """one run equals the same stream cut at 0, 1, N - 2, 255, 256 and 257 symbols with the state carried; a row with a
    count consumes min(count, n) symbols and leaves the rest alone"""
    taps, n = 9, 600
    x = np.stack([ref.white((n,), 11 + r, cplx, 0.8) for r in range(3)])
    p = np.array([[0.02, 0.5], [0.05, 0.3], [0.0, 1.0]], f32)
    mode = ref.DD_QPSK if cplx else ref.DD_BPSK
    ((y, tr, z),) = ref.exact(build_dir, [(mode, taps, 4, p, x)])
    for cut in (0, 1, taps - 2, 255, 256, 257):
        ((ya, ta, za),) = ref.exact(build_dir, [(mode, taps, 4, p, x[:, :cut])])
        ((yb, tb, zb),) = ref.exact(build_dir, [(mode, taps, 4, p, x[:, cut:], za)])
        assert np.array_equal(bits(np.hstack([ya, yb])), bits(y)) and np.array_equal(bits(np.hstack([ta, tb])), bits(tr)) and np.array_equal(bits(zb), bits(z))
    counts = np.array([0, 257, n + 5], np.uint32)
    ((yc, tc, zc),) = ref.exact(build_dir, [(mode, taps, 4, p, x, None, counts)])
    ((y257, t257, z257),) = ref.exact(build_dir, [(mode, taps, 4, p, x[:, :257])])
    assert np.array_equal(zc[0], ref.initial_state(1, taps, 4, cplx)[0]) and not yc[0].any()
    assert np.array_equal(bits(yc[1, :257]), bits(y257[1])) and not yc[1, 257:].any() and np.array_equal(bits(zc[1]), bits(z257[1]))
    assert np.array_equal(bits(yc[2]), bits(y[2])) and np.array_equal(bits(zc[2]), bits(z[2]))


@pytest.mark.parametrize("cplx", [False, True])
def test_nan_stays_in_its_row(build_dir, cplx):
    """a NaN in one symbol of one row: that row's outputs are NaN from there on (CMA feeds it into every tap) until the
    state is replaced; the rows beside it are bit-equal to a run without it"""
    x = ref.white((3, 100), 21, cplx)
    bad = x.copy()
    bad[1, 40] = np.nan
    (y, tr, z), (yb, tb, zb) = ref.exact(build_dir, [(ref.CMA, 5, 2, (0.05, 0.5), x), (ref.CMA, 5, 2, (0.05, 0.5), bad)])
    assert np.array_equal(bits(yb[[0, 2]]), bits(y[[0, 2]])) and np.array_equal(bits(zb[[0, 2]]), bits(z[[0, 2]])) and np.array_equal(bits(tb[[0, 2]]), bits(tr[[0, 2]]))
    assert np.array_equal(bits(yb[1, :40]), bits(y[1, :40])) and np.isnan(yb[1, 40:].view(f32)).all() and np.isnan(zb[1, :5]).all()
    assert np.isfinite(yb[[0, 2]].view(f32)).all()


# ---- convergence -------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_convergence_on_the_restatement(build_dir, seed):
    """6000 QPSK symbols through h = [0.2 - 0.1i, 1, 0.45 + 0.3i, -0.2 + 0.15i] with noise of deviation 0.02: N = 11,
    c = 5; CMA with mu = 0.01, level = 1 over all of them, then the taps carried into a DD_QPSK bank with mu = 0.01,
    level = 1 / sqrt 2 over symbols 3000 ... 5999.  In the last 2000 symbols: more than 100 wrong sign decisions
    unequalized, exactly 0 behind CMA (best of the four rotations, best delay 4 ... 8) and 0 behind DD."""
    r, a = ref.qpsk_through_channel(6000, seed)
    raw, cma, dd, wmax = ref.converge(lambda *case: ref.exact(build_dir, [case])[0], r, a)
    print(f"seed {seed}: wrong decisions of 2000: unequalized {raw}, CMA {cma}, DD {dd}; largest |w| {wmax:.3f}")
    assert raw > 100 and cma == 0 and dd == 0

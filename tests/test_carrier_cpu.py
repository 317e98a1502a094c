"""The carrier recovery bank (include/hzsdr_carrier.h) without a GPU: the ABI's header, exports and bindings; car_unit of
csrc/hz_carrier_math.h against float64 and against the tuner's three-table rotator; the host program
tests/host/carrier_ref.cpp (the bits the device must produce) against the float64 restatement of tests/carrier_ref.py:
outputs, track and state, lock, the clamp, a NaN kept to its sample, cuts, new parameters, the validation."""
import importlib
import math
import os
import re
import subprocess

import numpy as np
import pytest

import carrier_ref as ref
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "hzsdr_carrier.h")
ENTRIES = {"hzsdr_carrier_create", "hzsdr_carrier_push", "hzsdr_carrier_set_params", "hzsdr_carrier_get_state", "hzsdr_carrier_set_state",
           "hzsdr_carrier_position", "hzsdr_carrier_plan", "hzsdr_carrier_reset", "hzsdr_carrier_free"}
GCC = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include")]

# car_unit's and the tuner rotator's largest |(c, s) - exact| over ALL 2^32 phase words (`carrier_ref unit 1 16`),
# as csrc/hz_carrier_math.h and DESIGN.md record them
CAR_UNIT_MAX, TUNER_ROTATE_MAX = 1.294e-07, 1.605e-07

# the loop of these tests: a noise bandwidth of 0.02 cycles per sample, the range +-0.01
ALPHA, BETA = ref.gains(0.02)
PARAMS = np.array([ALPHA, BETA, 0.0, -0.01, 0.01], np.float32)
N = 4096
# (mode, offsets inside and at the edge of [fmin, fmax])
LOCK_CASES = [(ref.TONE, 0.0), (ref.TONE, 0.004), (ref.TONE, -0.01), (ref.BPSK, 0.003), (ref.BPSK, 0.01), (ref.QPSK, -0.002), (ref.QPSK, -0.01)]


@pytest.fixture(scope="module")
def hz():
    return importlib.import_module("go-sdr_amd")


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("carrier_ref"))


def carrier_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(hzsdr_[a-z0-9_]+)\s*\(", text)))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the ABI ---------------------------------------------------------------------------------------

def test_header_is_c99(tmp_path):
    src = tmp_path / "inc.c"
    src.write_text('#include "hzsdr_carrier.h"\n'
                   "int main(void) { hzsdr_carrier *f = 0; return (f != 0) + HZSDR_CARRIER_TONE + HZSDR_CARRIER_BPSK + HZSDR_CARRIER_QPSK"
                   " - HZSDR_CARRIER_FORM_PER_ROW - HZSDR_CARRIER_FORM_MODE - HZSDR_CARRIER_MAX_ROWS; }\n")
    subprocess.check_call(GCC + ["-c", str(src), "-o", str(tmp_path / "inc.o")])


def test_header_declares_exactly_the_entries():
    assert len(ENTRIES) == 9 and set(carrier_symbols()) == ENTRIES


def test_library_exports_and_ctypes_table(hz):
    capi = importlib.import_module("go-sdr_amd._capi")
    syms = carrier_symbols()
    for s in syms:
        assert hasattr(capi.lib, s), f"{s} declared in hzsdr_carrier.h but not exported"
    assert sorted(capi.CARRIER_SIGNATURES) == syms
    for name, (res, args) in capi.CARRIER_SIGNATURES.items():
        fn = getattr(capi.lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    found = re.findall(r"\bint (hzsdr_carrier_[a-z_]+)\s*\(([^)]*)\)", text)
    assert {name for name, _ in found} == ENTRIES
    for name, params in found:
        assert len(capi.CARRIER_SIGNATURES[name][1]) == len(params.split(",")), name


def test_constants_and_python_layers(hz):
    defs = dict(re.findall(r"#define (HZSDR_\w+) (\d+)", open(HEADER).read()))
    assert int(defs["HZSDR_CARRIER_TONE"]) == hz.CARRIER_TONE == ref.TONE == 0
    assert int(defs["HZSDR_CARRIER_BPSK"]) == hz.CARRIER_BPSK == ref.BPSK == 1
    assert int(defs["HZSDR_CARRIER_QPSK"]) == hz.CARRIER_QPSK == ref.QPSK == 2
    assert int(defs["HZSDR_CARRIER_FORM_PER_ROW"]) == hz.CARRIER_FORM_PER_ROW == ref.FORM_PER_ROW == 1
    assert int(defs["HZSDR_CARRIER_FORM_MODE"]) == hz.CARRIER_FORM_MODE == ref.FORM_MODE == 2
    assert int(defs["HZSDR_CARRIER_MAX_ROWS"]) == hz.CARRIER_MAX_ROWS == ref.MAX_ROWS == 8192
    st = importlib.import_module("go-sdr_amd.stream")
    mod = importlib.import_module("go-sdr_amd.carrier")
    assert hz.CarrierLoop is mod.CarrierLoop and hz.carrier_gains is mod.carrier_gains and callable(hz.Context.carrier_loop) and callable(st.carrier_rows)
    for name in ("push", "set_params", "state", "set_state", "position", "reset", "plan", "close", "__enter__", "__exit__"):
        assert callable(getattr(hz.CarrierLoop, name)), name
    hpp = open(os.path.join(ROOT, "go-sdr_amd", "cxx", "hzsdr.hpp")).read()
    assert "class CarrierLoop" in hpp and '#include "../../include/hzsdr_carrier.h"' in hpp
    make = open(os.path.join(ROOT, "go-sdr_amd", "csrc", "Makefile")).read()
    assert "hzsdr_carrier.h" in make and "hz_carrier" not in make.split("MFMA_UNITS =")[1].splitlines()[0]
    assert "amplitude" in open(HEADER).read().lower()


def test_carrier_gains(hz):
    alpha, beta = hz.carrier_gains(0.02)
    tn = 0.02 / (0.7071 + 1.0 / (4.0 * 0.7071))
    d = 1.0 + 2.0 * 0.7071 * tn + tn * tn
    assert alpha == pytest.approx(4.0 * 0.7071 * tn / d / (2.0 * math.pi), rel=1e-15) and beta == pytest.approx(4.0 * tn * tn / d / (2.0 * math.pi), rel=1e-15)
    assert (alpha, beta) == pytest.approx(ref.gains(0.02), rel=1e-15)
    assert hz.carrier_gains(0.05, 1.0) == pytest.approx(ref.gains(0.05, 1.0), rel=1e-15)
    for bad in ((0.0,), (0.01, 0.0), (-1.0,)):
        with pytest.raises(ValueError):
            hz.carrier_gains(*bad)


# ---- the unit vector -----------------------------------------------------------------------------------

def test_car_unit_accuracy(build_dir):
    """Every 64th phase word (2^26 of them) and the axes, the diagonals and their 64 neighbours on either side, against
    float64: car_unit stays inside its recorded bound (1.294e-07 over all 2^32 words; the tuner's three-table rotator:
    1.605e-07 over the same words), is no worse than the rotator over these words, and is exact on the four axes."""
    words, car, car_at, tab, tab_at, bad_axes = ref.unit(build_dir, 64, 8)
    print(f"{words} words: car_unit {car:.4e} at {car_at:#010x}, tuner_rotate {tab:.4e} at {tab_at:#010x}")
    assert words == (1 << 26) + 8 * 129
    assert bad_axes == 0
    assert car <= CAR_UNIT_MAX and tab <= TUNER_ROTATE_MAX
    assert car <= tab
    assert CAR_UNIT_MAX <= TUNER_ROTATE_MAX
    text = open(os.path.join(ROOT, "go-sdr_amd", "csrc", "hz_carrier_math.h")).read()
    assert "1.294e-07" in text and "1.605e-07" in text


# ---- the program against the float64 restatement ---------------------------------------------------------

@pytest.fixture(scope="module")
def lock_runs(build_dir):
    """[(mode, offset, noise, x, program's (y, track, state), float64's (y, track, (theta, F)))]: every lock case without
    noise and with it, computed once"""
    runs = []
    for noise in (0.0, 0.02):
        cases = [(mode, PARAMS, ref.signal(mode, N, off, 1.0, 100 * mode + k, noise=noise)) for k, (mode, off) in enumerate(LOCK_CASES)]
        for (mode, off), (_, _, x), got in zip(LOCK_CASES, cases, ref.exact(build_dir, cases)):
            runs.append((mode, off, noise, x, got, ref.float64(mode, PARAMS, x)))
    return runs


def test_program_against_float64(lock_runs):
    """Outputs, track and final state of the program against the float64 restatement, TONE, BPSK and QPSK rows at
    offsets inside and at the edge of [fmin, fmax], without noise and with it.  The two trajectories differ by the
    float32 roundings of y and by the integer truncations that follow them, a few phase units that the loop contracts.
    Measured over these cases: outputs 9.70e-06 (the BPSK row at the edge, while it acquires; 1.6e-07 elsewhere), track
    2.38e-08 cycles per sample, theta 26 phase units, F 2 phase units per sample.  Asserted: four times that."""
    dy = dt = dth = df = 0.0
    for mode, off, noise, x, (y, tr, z), (y64, tr64, (th, f)) in lock_runs:
        dy = max(dy, float(np.abs(y[0].astype(np.complex128) - y64).max()))
        dt = max(dt, float(np.abs(tr[0].astype(np.float64) - tr64).max()))
        dth = max(dth, abs((int(z[0, 0]) - th + (1 << 31)) % (1 << 32) - (1 << 31)))
        df = max(df, abs(int(np.int32(z[0, 1])) - f))
    print(f"largest deviations: outputs {dy:.3e}, track {dt:.3e}, theta {dth} units, F {df} units")
    assert dy <= 4 * 9.70e-06 and dt <= 4 * 2.38e-08 and dth <= 4 * 26 and df <= 4 * 2


def test_lock(lock_runs):
    """The condition: the offset is inside the loop's pull-in range, confirmed on the float64 restatement first (its
    frequency estimate over the last quarter is within 2e-5 cycles per sample of the offset and y^m keeps to one
    half-plane).  Then the mean of the last quarter of the program's track is the true offset, and y, y^2, y^4 (TONE,
    BPSK, QPSK) has a constant phase: both against the float64 restatement's own residuals, four times them."""
    q = 3 * N // 4
    for mode, off, noise, x, (y, tr, z), (y64, tr64, _) in lock_runs:
        if noise == 0.0:
            continue  # (without noise the residuals are the roundings themselves: test_program_against_float64 has them)
        ref_freq, ref_spread = abs(float(tr64[q:].mean()) - off), ref.phase_spread(mode, y64[q:])
        assert ref_freq < 2e-5 and ref_spread < math.pi / 2, f"the reference does not lock: mode {mode}, offset {off}"
        got_freq, got_spread = abs(float(tr[0, q:].astype(np.float64).mean()) - off), ref.phase_spread(mode, y[0, q:])
        print(f"mode {mode} offset {off}: frequency residual {got_freq:.3e} (float64 {ref_freq:.3e}), phase spread {got_spread:.3e} ({ref_spread:.3e})")
        assert got_freq <= 4 * ref_freq and got_spread <= 4 * ref_spread


def test_clamp_holds(build_dir):
    """An offset outside [fmin, fmax]: F never leaves the range, reaches the edge on the offset's side and spends the
    last quarter near it, in the program as in the float64 restatement."""
    _, _, _, fmin, fmax = ref.loop_constants(PARAMS)
    for mode in (ref.TONE, ref.QPSK):
        for off, edge in ((0.03, fmax), (-0.03, fmin)):
            x = ref.signal(mode, N, off, 0.3, 7)
            (y, tr, z), = ref.exact(build_dir, [(mode, PARAMS, x)])
            _, tr64, (_, f64) = ref.float64(mode, PARAMS, x)
            lo, hi = np.float32(fmin) * np.float32(2.0 ** -32), np.float32(fmax) * np.float32(2.0 ** -32)
            assert tr.min() >= lo and tr.max() <= hi and tr64.min() >= fmin / ref.TWO32 and tr64.max() <= fmax / ref.TWO32
            assert fmin <= int(np.int32(z[0, 1])) <= fmax
            if mode == ref.TONE:
                assert (tr == np.float32(edge) * np.float32(2.0 ** -32)).any() and (tr64 == edge / ref.TWO32).any()
                assert abs(tr[0, 3 * N // 4:].mean() - edge / ref.TWO32) < 0.002 and abs(tr64[3 * N // 4:].mean() - edge / ref.TWO32) < 0.002


def test_track_is_the_state(build_dir):
    """track[n] is (float) F * 2^-32 of the state behind sample n: cut behind every sample of a short row"""
    x = ref.signal(ref.QPSK, 40, 0.004, 2.0, 3, noise=0.1)
    (y, tr, z), = ref.exact(build_dir, [(ref.QPSK, PARAMS, x)])
    cases = [(ref.QPSK, PARAMS, x[:n]) for n in range(1, 41)]
    for n, (yn, trn, zn) in zip(range(1, 41), ref.exact(build_dir, cases)):
        assert trn[0, -1] == np.float32(np.int32(zn[0, 1])) * np.float32(2.0 ** -32)
        assert np.array_equal(bits(yn), bits(y[:, :n])) and np.array_equal(bits(trn), bits(tr[:, :n]))


def test_cuts_and_new_parameters(build_dir):
    """one run equals the same stream cut at 1, 255, 256 and 257 samples with the state carried; new parameters between
    two pushes keep theta and F and hold F to the new range at the next sample"""
    x = np.stack([ref.signal(ref.BPSK, 1000, 0.004, 0.5, 11, noise=0.05), ref.white((1000,), 12)])
    (y, tr, z), = ref.exact(build_dir, [(ref.BPSK, PARAMS, x)])
    for cut in (1, 255, 256, 257):
        (ya, ta, za), = ref.exact(build_dir, [(ref.BPSK, PARAMS, x[:, :cut])])
        (yb, tb, zb), = ref.exact(build_dir, [(ref.BPSK, PARAMS, x[:, cut:], za)])
        assert np.array_equal(bits(np.hstack([ya, yb])), bits(y)) and np.array_equal(bits(np.hstack([ta, tb])), bits(tr)) and np.array_equal(zb, z)
    narrow = np.array([ALPHA, BETA, 0.0, -0.001, 0.001], np.float32)
    (y2, t2, z2), = ref.exact(build_dir, [(ref.BPSK, [(0, PARAMS), (600, narrow)], x)])
    (ya, ta, za), = ref.exact(build_dir, [(ref.BPSK, PARAMS, x[:, :600])])
    (yb, tb, zb), = ref.exact(build_dir, [(ref.BPSK, narrow, x[:, 600:], za)])
    assert np.array_equal(bits(np.hstack([ya, yb])), bits(y2)) and np.array_equal(zb, z2)
    assert np.array_equal(bits(y2[:, :601]), bits(y[:, :601]))  # (theta of sample 600 is the old one: y[600] is unchanged)
    edge = np.float32(ref.loop_constants(narrow)[4]) * np.float32(2.0 ** -32)  # (float) Fmax * 2^-32, as the track is made
    assert abs(t2[0, 599]) > 0.003 and np.abs(t2[:, 600:]).max() <= edge and t2[0, 600] == edge


def test_nan_stays_in_its_sample(build_dir):
    """A NaN sample: a NaN output for that sample, and theta and F move on as they do for a sample of zero error (a
    zero sample: e = 0): every other output, the track and the state are those of the row with a zero in its place.
    An infinity clips: its row goes on, the other rows are untouched."""
    for mode in (ref.TONE, ref.BPSK, ref.QPSK):
        x = np.stack([ref.signal(mode, 300, 0.002, 0.1, 21 + k, noise=0.05) for k in range(3)])
        bad, zero, inf = x.copy(), x.copy(), x.copy()
        bad[1, 100] = complex(np.nan, 0.5)
        zero[1, 100] = 0.0
        inf[1, 100] = complex(np.inf, 0.5)
        (yb, tb, zb), (yz, tz, zz), (yi, ti, zi), (y, tr, z) = ref.exact(build_dir, [(mode, PARAMS, bad), (mode, PARAMS, zero), (mode, PARAMS, inf), (mode, PARAMS, x)])
        assert np.isnan(yb[1, 100].real) and np.isnan(yb[1, 100].imag)
        keep = np.ones(x.shape, bool)
        keep[1, 100] = False
        assert np.array_equal(bits(yb)[np.repeat(keep, 2, axis=1)], bits(yz)[np.repeat(keep, 2, axis=1)])
        assert np.array_equal(bits(tb), bits(tz)) and np.array_equal(zb, zz)
        assert not np.isnan(yb[keep]).any()
        assert np.array_equal(bits(yi[[0, 2]]), bits(y[[0, 2]])) and np.array_equal(zi[[0, 2]], z[[0, 2]])
        assert not np.isfinite(yi[1, 100]) and np.isfinite(yi[keep]).all() and np.isfinite(ti).all()


def test_restated_validation(build_dir):
    """the acceptance rules, restated in Python, against csrc/hz_carrier_plan.h; and the derived constants"""
    up, qup = np.nextafter(np.float32(0.125), np.float32(1)), np.nextafter(np.float32(0.25), np.float32(1))
    sets = [[0, 0, 0, 0, 0], [0.125, 0.125, 0, -0.25, 0.25], [up, 0, 0, 0, 0], [0, up, 0, 0, 0], [-1e-9, 0, 0, 0, 0], [0, -1e-9, 0, 0, 0],
            [0, 0, 0.25, 0.25, 0.25], [0, 0, -0.25, -0.25, -0.25], [0, 0, 0, -qup, 0], [0, 0, 0, 0, qup], [0, 0, 0.1, 0.11, 0.2],
            [0, 0, 0.21, 0.1, 0.2], [0, 0, 0, 0.1, -0.1], [np.nan, 0, 0, 0, 0], [0, np.inf, 0, 0, 0], [0, 0, np.nan, -0.25, 0.25],
            [0, 0, 0, -np.inf, 0.25], [0, 0, 0, -0.25, np.nan], list(PARAMS), [0.01, 0.001, 0.0123, -0.2, 0.2499]]
    rng = np.random.default_rng(5)
    sets += [list(v) for v in rng.uniform(-0.3, 0.3, (200, 5)) * np.array([0.5, 0.5, 1, 1, 1])]
    sets += [[a, b, f0, lo, hi] for a, b, (lo, f0, hi) in zip(rng.uniform(0, 0.125, 100), rng.uniform(0, 0.125, 100), np.sort(rng.uniform(-0.25, 0.25, (100, 3)), axis=1))]
    q = np.array(sets, np.float32)
    got = ref.derive(build_dir, q)
    assert sum(g[0] for g in got) > 100 and sum(not g[0] for g in got) > 100
    for p, (ok, aw, bw, f0, fmin, fmax) in zip(q, got):
        assert ok == ref.accepted(p), p
        if ok:
            assert (aw, bw, f0, fmin, fmax) == ref.loop_constants(p), p
            assert abs(aw) <= 2.0 ** 29 and abs(bw) <= 2.0 ** 29 and -2 ** 30 <= fmin <= f0 <= fmax <= 2 ** 30

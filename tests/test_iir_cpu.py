"""The IIR bank's ABI, arithmetic and designers, without a GPU: include/hzsdr_iir.h is C99 and declares exactly its nine
entries, the C walkthrough names them all and compiles, the library exports them and _capi.IIR_SIGNATURES binds them
exactly; the bit-exact restatement (tests/host/iir_ref.cpp over the header the kernel evaluates) agrees with the
independent float64 one (tests/iir_ref.py, direct form I) within a bound derived from the case's own coefficients; the
designers by their float64 frequency response; a decay through a pole of 0.5 reaches the denormals and then +0."""
import importlib
import math
import os
import re
import subprocess

import numpy as np
import pytest

import iir_ref as ref
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "hzsdr_iir.h")
WALK = os.path.join(ROOT, "tests", "c", "test_iir_abi.c")
ENTRIES = {"hzsdr_iir_create", "hzsdr_iir_push", "hzsdr_iir_set_sections", "hzsdr_iir_get_state", "hzsdr_iir_set_state",
           "hzsdr_iir_position", "hzsdr_iir_plan", "hzsdr_iir_reset", "hzsdr_iir_free"}
GCC = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include")]


@pytest.fixture(scope="module")
def hz():
    return importlib.import_module("go-sdr_amd")


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("iir_ref"))


def iir_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(hzsdr_[a-z0-9_]+)\s*\(", text)))


# ---- the ABI ---------------------------------------------------------------------------------------

def test_header_is_c99(tmp_path):
    src = tmp_path / "inc.c"
    src.write_text('#include "hzsdr_iir.h"\n'
                   "int main(void) { hzsdr_iir *f = 0; return (f != 0) + HZSDR_IIR_REAL_F32 - HZSDR_IIR_FORM_PER_ROW - HZSDR_IIR_FORM_COMPLEX; }\n")
    subprocess.check_call(GCC + ["-c", str(src), "-o", str(tmp_path / "inc.o")])


def test_header_declares_exactly_the_entries():
    assert len(ENTRIES) == 9 and set(iir_symbols()) == ENTRIES


def test_c_walkthrough_names_every_entry():
    text = open(WALK).read()
    missing = [s for s in iir_symbols() if not re.search(r"\b" + s + r"\s*\(", text)]
    assert missing == []
    assert "iir-abi ok" in text


def test_c_walkthrough_compiles_as_c99(tmp_path):
    subprocess.check_call(GCC + ["-c", WALK, "-o", str(tmp_path / "w.o")])


def test_library_exports_and_ctypes_table(hz):
    capi = importlib.import_module("go-sdr_amd._capi")
    syms = iir_symbols()
    for s in syms:
        assert hasattr(capi.lib, s), f"{s} declared in hzsdr_iir.h but not exported"
    assert sorted(capi.IIR_SIGNATURES) == syms
    others = (set(capi.SIGNATURES) | set(capi.SPECTRUM_SIGNATURES) | set(capi.CHANNELIZER_SIGNATURES) | set(capi.SYNTHESIZER_SIGNATURES)
              | set(capi.RESAMPLER_SIGNATURES) | set(capi.DEMOD_SIGNATURES) | set(capi.TUNER_SIGNATURES) | set(capi.CHANBANK_SIGNATURES)
              | set(capi.COVAR_SIGNATURES))
    assert not set(capi.IIR_SIGNATURES) & others
    for name, (res, args) in capi.IIR_SIGNATURES.items():
        fn = getattr(capi.lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_signatures_have_the_header_arity(hz):
    capi = importlib.import_module("go-sdr_amd._capi")
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    found = re.findall(r"\bint (hzsdr_iir_[a-z_]+)\s*\(([^)]*)\)", text)
    assert {name for name, _ in found} == ENTRIES
    for name, params in found:
        assert len(capi.IIR_SIGNATURES[name][1]) == len(params.split(",")), name


def test_constants_match_header(hz):
    defs = dict(re.findall(r"#define (HZSDR_\w+) (\d+)", open(HEADER).read()))
    assert int(defs["HZSDR_IIR_REAL_F32"]) == hz.IIR_REAL_F32 == ref.REAL_F32 == 32
    # the real kind is none of the four source formats (iq.go:110-126), and no format the library knows
    assert hz.IIR_REAL_F32 not in (hz.FMT_C64, hz.FMT_U8, hz.FMT_I16, hz.FMT_I8) and hz.format_size(hz.IIR_REAL_F32) == 0
    assert int(defs["HZSDR_IIR_FORM_PER_ROW"]) == hz.IIR_FORM_PER_ROW == ref.FORM_PER_ROW == 1
    assert int(defs["HZSDR_IIR_FORM_COMPLEX"]) == hz.IIR_FORM_COMPLEX == ref.FORM_COMPLEX == 2
    assert int(defs["HZSDR_IIR_MAX_SECTIONS"]) == hz.IIR_MAX_SECTIONS == 8
    assert int(defs["HZSDR_IIR_MAX_ROWS"]) == hz.IIR_MAX_ROWS == 8192
    csrc = os.path.join(ROOT, "go-sdr_amd", "csrc")
    assert "kMaxRows = 8192, kLanes = 64" in open(os.path.join(csrc, "hz_rowwave_plan.h")).read()  # (the row-wave banks')
    assert "kMaxSections = 8;" in open(os.path.join(csrc, "hz_iir_plan.h")).read()
    assert hz.IIR_REAL_F32 is importlib.import_module("go-sdr_amd.iir").IIR_REAL_F32


def test_python_layers_are_exported(hz):
    st = importlib.import_module("go-sdr_amd.stream")
    mod = importlib.import_module("go-sdr_amd.iir")
    assert hz.IirBank is mod.IirBank and callable(hz.Context.iir_bank) and callable(st.iir_rows)
    for name in ("push", "set_sections", "state", "set_state", "position", "reset", "plan", "close", "__enter__", "__exit__"):
        assert callable(getattr(hz.IirBank, name)), name
    for name in ("one_pole", "dc_block", "deemphasis", "notch", "lowpass", "highpass", "butterworth"):
        assert getattr(hz, name) is getattr(mod, name), name
    hpp = open(os.path.join(ROOT, "go-sdr_amd", "cxx", "hzsdr.hpp")).read()
    assert "class IirBank" in hpp and '#include "../../include/hzsdr_iir.h"' in hpp
    assert "hzsdr_iir.h" in open(os.path.join(ROOT, "go-sdr_amd", "csrc", "Makefile")).read()


def test_rows_helper_learns_the_real_kind(hz):
    """_rows.rows_input takes float32 rows for IIR_REAL_F32 and what it did for the four formats"""
    rows = importlib.import_module("go-sdr_amd._rows")
    x = np.zeros((3, 40), np.float32)[:, :33]
    ptr, n, pitch = rows.rows_input(x, hz.IIR_REAL_F32, 3, "iir bank")
    assert (ptr, n, pitch) == (x.ctypes.data, 33, 40)
    assert rows.rows_input(np.zeros(7, np.float32), hz.IIR_REAL_F32, 1, "iir bank")[1:] == (7, 7)
    with pytest.raises(ValueError):
        rows.rows_input(np.zeros(7, np.float64), hz.IIR_REAL_F32, 1, "iir bank")
    with pytest.raises(ValueError):
        rows.rows_input(np.zeros(7, np.float32), hz.FMT_C64, 1, "iir bank")
    c = np.zeros((2, 9), np.complex64)
    assert rows.rows_input(c, hz.FMT_C64, 2, "x")[1:] == (9, 9)
    assert rows.rows_input(np.zeros((5, 2), np.uint8), hz.FMT_U8, 1, "x")[1:] == (5, 5)
    assert rows.rows_input(np.zeros((2, 5, 2), np.int16), hz.FMT_I16, 2, "x")[1:] == (5, 5)


# ---- the restatements ------------------------------------------------------------------------------

def white(n, seed, cplx=False):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    if cplx:
        return (x + 1j * rng.uniform(-1.0, 1.0, n).astype(np.float32)).astype(np.complex64)
    return x


def cascades(hz):
    fs = 48_000.0
    return {
        "one_pole": hz.one_pole(0.05),
        "dc_block": hz.dc_block(0.995),
        "deemphasis": hz.deemphasis(75e-6, fs),
        "notch": hz.notch(67.0 * 30, 8.0, fs),
        "lowpass": hz.lowpass(3000.0, 0.9, fs),
        "highpass": hz.highpass(300.0, 0.7071, fs),
        "butter5": hz.butterworth(5, 5000.0, fs),
        "butter16hp": hz.butterworth(16, 2000.0, fs, highpass=True),
        "dc+notch": np.concatenate([hz.dc_block(0.99), hz.notch(1000.0, 30.0, fs)]),
    }


def test_restatements_agree(hz, build_dir):
    """The exact float32 outputs of the program against the float64 direct-form-I recursion, real and complex rows,
    S = 1, 2, 3 and 8, within sum_s 5 (2^-24 max|node_s| + 2^-150) ||1 / A_s||_1 prod_{t > s} ||H_t||_1 -- no fixed
    tolerance: the l1 gains are computed numerically from the case's own coefficients."""
    cases, names = [], []
    for k, (name, sec) in enumerate(cascades(hz).items()):
        assert sec.dtype == np.float32 and sec.ndim == 2 and sec.shape[1] == 5
        for cplx in (False, True):
            cases.append((sec, white(1200 + 7 * k, 100 + k, cplx)))
            names.append(f"{name} S={sec.shape[0]} {'c64' if cplx else 'f32'}")
    assert {c[0].shape[0] for c in cases} >= {1, 2, 3, 8}
    for name, (sec, x), (got, state) in zip(names, cases, ref.exact(build_dir, cases)):
        assert got.dtype == x.dtype and got.shape == x.shape and state.shape[:3] == (1, sec.shape[0], 2)
        want, bnd = ref.float64(sec, x), ref.bound(sec, x)
        d = got.astype(want.dtype) - want
        err = max(np.abs(d.real).max(), np.abs(d.imag).max())
        print(f"{name}: max err {err:.3e}, bound {bnd:.3e}, max |y| {np.abs(want).max():.3e}")
        assert np.abs(want).max() > 1e-3, "the case filters everything away"
        assert err <= bnd, f"{name}: {err:.3e} > {bnd:.3e}"
        # (a product of l1 gains is loose for a 16th-order cascade, 3e-2 there; it must still say something)
        assert bnd <= 0.05 * np.abs(want).max(), f"{name}: the bound {bnd:.3e} says nothing beside max |y|"


def test_a_complex_row_is_two_real_rows(hz, build_dir):
    sec = cascades(hz)["butter5"]
    x = white(500, 9, True)
    (c, zc), (re, zr), (im, zi) = ref.exact(build_dir, [(sec, x), (sec, x.real.copy()), (sec, x.imag.copy())])
    assert np.array_equal(c.real.view(np.uint32), re.view(np.uint32)) and np.array_equal(c.imag.view(np.uint32), im.view(np.uint32))
    assert np.array_equal(zc[..., 0], zr) and np.array_equal(zc[..., 1], zi)


def test_retuning_in_the_restatement(hz, build_dir):
    """a cascade exchanged at sample k: the head is the first cascade's run, and the whole is not the first cascade's"""
    fs, k = 48_000.0, 333
    a, b = hz.notch(1000.0, 5.0, fs), hz.notch(1500.0, 5.0, fs)
    x = white(900, 4)
    (sw, _), (plain, _) = ref.exact(build_dir, [([(0, a), (k, b)], x), (a, x)])
    assert np.array_equal(sw[:k].view(np.uint32), plain[:k].view(np.uint32)) and not np.array_equal(sw[k:], plain[k:])
    # no click: the state carries over, the first retuned output is near the unretuned one
    assert abs(float(sw[k]) - float(plain[k])) < 0.05


def test_decay_reaches_denormals_then_zero(build_dir):
    """An impulse through a pole of 0.5: 2^-n exactly, denormal from n = 127, 2^-149 at n = 149, +0 from n = 150 on."""
    ((y, z),) = ref.exact(build_dir, [(ref.decay_section(), ref.decay_row(200))])
    want = np.array([math.ldexp(1.0, -n) if n < 150 else 0.0 for n in range(200)], np.float32)
    assert np.array_equal(y.view(np.uint32), want.view(np.uint32))
    u = y.view(np.uint32)
    assert ((u[127:150] & 0x7f800000) == 0).all() and (u[127:150] != 0).all(), "the tail is not denormal"
    assert u[149] == 1 and not u[150:].any(), "the decay does not end in +0"
    assert not z.view(np.uint32).any()


# ---- the designers ---------------------------------------------------------------------------------

def gain(sec, f, fs):
    return np.abs(importlib.import_module("go-sdr_amd.iir").response(sec, f, fs))


def test_deemphasis(hz):
    """The bilinear transform maps the digital frequency f to the analogue fa = fs / pi tan(pi f / fs): the response at
    f IS the analogue one at fa.  So at fc = 1 / (2 pi tau) the gain is -3.01 dB less the warping fa / fc computed
    here, and it is -3.01 dB exactly at fs / pi atan(pi fc / fs)."""
    for tau, fs in ((75e-6, 48_000.0), (50e-6, 48_000.0), (75e-6, 240_000.0), (75e-6, 12_000.0)):
        sec = hz.deemphasis(tau, fs)
        assert sec.shape == (1, 5) and sec.dtype == np.float32
        fc = 1.0 / (2.0 * math.pi * tau)
        fa = fs / math.pi * math.tan(math.pi * fc / fs)
        warped = 1.0 / math.sqrt(1.0 + (fa / fc) ** 2)
        got = float(gain(sec, fc, fs))
        db, warp_db = 20.0 * math.log10(got), 20.0 * math.log10(warped) - 20.0 * math.log10(math.sqrt(0.5))
        print(f"tau={tau} fs={fs}: {db:.4f} dB at fc = {fc:.1f} Hz (warping {warp_db:.4f} dB)")
        assert abs(got - warped) <= 1e-6
        assert abs(db + 3.0103) <= abs(warp_db) + 1e-4
        f3 = fs / math.pi * math.atan(math.pi * fc / fs)
        assert abs(float(gain(sec, f3, fs)) ** 2 - 0.5) <= 1e-6
        assert abs(float(gain(sec, 0.0, fs)) - 1.0) <= 1e-6 and float(gain(sec, fs / 2, fs)) <= 1e-6


def test_notch(hz):
    for f0, q, fs in ((67.0, 4.0, 8000.0), (1000.0, 30.0, 48_000.0), (10_000.0, 2.0, 48_000.0)):
        sec = hz.notch(f0, q, fs)
        b, a1, a2 = sec[0, :3].astype(np.float64), float(sec[0, 3]), float(sec[0, 4])
        z1 = np.exp(-2j * np.pi * f0 / fs)
        # the zero sits at f0 up to the float32 rounding of the three numerator coefficients, seen through 1 / |A(f0)|
        tol = 3 * 2.0 ** -24 * np.abs(b).max() / abs(1.0 + a1 * z1 + a2 * z1 * z1)
        got = float(gain(sec, f0, fs))
        print(f"notch f0={f0} q={q}: |H(f0)| = {got:.3e} (tolerance {tol:.3e})")
        assert got <= tol and tol < 1e-3  # (below -60 dB for the narrowest of the three)
        # unit gain at DC and at Nyquist, up to the rounding of all six coefficients seen through 1 / |A| there (at DC
        # both polynomials of a low notch are small differences of their coefficients)
        for f, zz in ((0.0, 1.0), (fs / 2, -1.0)):
            unit = 2 * 2.0 ** -24 * (np.abs(b).sum() + 1.0 + abs(a1) + abs(a2)) / abs(1.0 + a1 * zz + a2)
            assert abs(float(gain(sec, f, fs)) - 1.0) <= unit < 1e-3
        # -3 dB at f0 (1 +- 1 / (2 q)), to first order in 1 / q: well inside [0.5, 0.9] there
        assert 0.5 < float(gain(sec, f0 * (1 + 0.5 / q), fs)) < 0.9


@pytest.mark.parametrize("highpass", [False, True])
@pytest.mark.parametrize("order", [1, 2, 3, 4, 5, 8, 16])
def test_butterworth(hz, order, highpass):
    fs, fc = 48_000.0, 3000.0
    sec = hz.butterworth(order, fc, fs, highpass=highpass)
    assert sec.shape == ((order + 1) // 2, 5) and sec.dtype == np.float32
    assert abs(float(gain(sec, fc, fs)) ** 2 - 0.5) <= 2e-5 * order, "not -3.01 dB at fc"
    f = np.linspace(0.0, fs / 2, 2001)
    g = gain(sec, f, fs)
    step = np.diff(g) if highpass else -np.diff(g)
    assert (step >= -1e-6).all(), "not monotone"
    assert abs(g[-1 if highpass else 0] - 1.0) <= 1e-5 * order and g[0 if highpass else -1] <= 1e-5
    # maximally flat: |H|^2 = 1 / (1 + (tan(pi f / fs) / tan(pi fc / fs))^(2 order)), the closed form of the bilinear design
    w = np.tan(np.pi * f[1:-1] / fs) / math.tan(math.pi * fc / fs)
    closed = 1.0 / np.sqrt(1.0 + (1.0 / w if highpass else w) ** (2 * order))
    assert np.abs(g[1:-1] - closed).max() <= 2e-5 * order
    try:
        from scipy import signal
    except ImportError:
        return
    sos = signal.butter(order, fc, btype="highpass" if highpass else "lowpass", fs=fs, output="sos")
    _, h = signal.sosfreqz(sos, worN=f, fs=fs)
    assert np.abs(g - np.abs(h)).max() <= 2e-5 * order


def test_rbj_lowpass_highpass(hz):
    fs, fc = 48_000.0, 2500.0
    for q in (0.5, 0.7071, 3.0):
        lp, hp = hz.lowpass(fc, q, fs), hz.highpass(fc, q, fs)
        # the cookbook forms: the gain at fc is q, DC / Nyquist gains are 1 and 0
        assert abs(float(gain(lp, fc, fs)) - q) <= 1e-5 * max(1.0, q) and abs(float(gain(hp, fc, fs)) - q) <= 1e-5 * max(1.0, q)
        assert abs(float(gain(lp, 0.0, fs)) - 1.0) <= 1e-5 and float(gain(lp, fs / 2, fs)) <= 1e-6
        assert abs(float(gain(hp, fs / 2, fs)) - 1.0) <= 1e-5 and float(gain(hp, 0.0, fs)) <= 1e-6


def test_dc_block_and_one_pole(hz):
    for r in (0.0, 0.9, 0.999):
        sec = hz.dc_block(r)
        assert float(gain(sec, 0.0, 1.0)) == 0.0, "the zero is not at DC"
        assert abs(float(gain(sec, 0.5, 1.0)) - 2.0 / (1.0 + float(np.float32(r)))) <= 1e-6
    for alpha in (1.0, 0.5, 0.01):
        sec = hz.one_pole(alpha)
        assert abs(float(gain(sec, 0.0, 1.0)) - 1.0) <= 1e-6
        assert sec[0, 0] == np.float32(alpha) and sec[0, 3] == np.float32(-(1.0 - alpha)) and not sec[0, [1, 2, 4]].any()


def test_designers_refuse_nonsense(hz):
    for f, args in ((hz.one_pole, (0.0,)), (hz.one_pole, (1.5,)), (hz.dc_block, (1.0,)), (hz.dc_block, (-0.1,)), (hz.deemphasis, (0.0, 48e3)),
                    (hz.notch, (30e3, 1.0, 48e3)), (hz.notch, (1e3, 0.0, 48e3)), (hz.lowpass, (0.0, 1.0, 48e3)), (hz.highpass, (1e3, -1.0, 48e3)),
                    (hz.butterworth, (0, 1e3, 48e3)), (hz.butterworth, (17, 1e3, 48e3)), (hz.butterworth, (4, 24e3, 48e3))):
        with pytest.raises(ValueError):
            f(*args)

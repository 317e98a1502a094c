"""The polyphase resampler's ABI and host-side helpers, without a GPU: include/hzsdr_resampler.h is C99 and declares
exactly its eight entries, the C walkthrough names them all, the library exports them and _capi.RESAMPLER_SIGNATURES
binds them exactly; the float64 restatements of the definition (tests/resampler_ref.py) agree with each other and with
scipy.signal.upfirdn; resampler_taps' properties; the count identities."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import resampler_ref as ref
from conftest import ROOT
from util import rand_c64

HEADER = os.path.join(ROOT, "include", "hzsdr_resampler.h")
WALK = os.path.join(ROOT, "tests", "c", "test_resampler_abi.c")
ENTRIES = {"hzsdr_resampler_create", "hzsdr_resampler_push", "hzsdr_resampler_flush", "hzsdr_resampler_outputs_for",
           "hzsdr_resampler_pending", "hzsdr_resampler_plan", "hzsdr_resampler_reset", "hzsdr_resampler_free"}
GCC = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include")]
# (U, D, L, N)
SHAPES = [(3, 2, 24, 101), (2, 3, 50, 77), (160, 147, 1920, 300), (1, 8, 128, 1000), (8, 1, 64, 40), (7, 5, 3, 41), (5, 5, 20, 33),
          (1, 1024, 256, 5000), (1024, 1, 2048, 9), (2, 5, 33, 1), (7, 1, 5, 2)]


@pytest.fixture(scope="module")
def hz():
    return importlib.import_module("go-sdr_amd")


def resampler_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(hzsdr_[a-z0-9_]+)\s*\(", text)))


def test_header_is_c99(tmp_path):
    src = tmp_path / "inc.c"
    src.write_text('#include "hzsdr_resampler.h"\n'
                   "int main(void) { hzsdr_resampler *r = 0; return (r != 0) + HZSDR_RESAMPLER_FORM_DIRECT - HZSDR_RESAMPLER_FORM_TAPS_GLOBAL; }\n")
    subprocess.check_call(GCC + ["-c", str(src), "-o", str(tmp_path / "inc.o")])


def test_header_declares_exactly_the_entries():
    assert len(ENTRIES) == 8 and set(resampler_symbols()) == ENTRIES


def test_c_walkthrough_names_every_entry():
    text = open(WALK).read()
    missing = [s for s in resampler_symbols() if not re.search(r"\b" + s + r"\s*\(", text)]
    assert missing == []
    assert "resampler-abi ok" in text


def test_c_walkthrough_compiles_as_c99(tmp_path):
    subprocess.check_call(GCC + ["-c", WALK, "-o", str(tmp_path / "w.o")])


def test_library_exports_and_ctypes_table(hz):
    capi = importlib.import_module("go-sdr_amd._capi")
    syms = resampler_symbols()
    for s in syms:
        assert hasattr(capi.lib, s), f"{s} declared in hzsdr_resampler.h but not exported"
    assert sorted(capi.RESAMPLER_SIGNATURES) == syms
    others = set(capi.SIGNATURES) | set(capi.SPECTRUM_SIGNATURES) | set(capi.CHANNELIZER_SIGNATURES) | set(capi.SYNTHESIZER_SIGNATURES)
    assert not set(capi.RESAMPLER_SIGNATURES) & others
    for name, (res, args) in capi.RESAMPLER_SIGNATURES.items():
        fn = getattr(capi.lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_signatures_have_the_header_arity(hz):
    capi = importlib.import_module("go-sdr_amd._capi")
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    found = re.findall(r"\bint (hzsdr_resampler_[a-z_]+)\s*\(([^)]*)\)", text)
    assert {name for name, _ in found} == ENTRIES
    for name, params in found:
        assert len(capi.RESAMPLER_SIGNATURES[name][1]) == len(params.split(",")), name


def test_constants_match_header(hz):
    defs = dict(re.findall(r"#define (HZSDR_\w+) (\d+)", open(HEADER).read()))
    assert int(defs["HZSDR_RESAMPLER_FORM_DIRECT"]) == hz.RESAMPLER_FORM_DIRECT == 1
    assert int(defs["HZSDR_RESAMPLER_FORM_TAPS_GLOBAL"]) == hz.RESAMPLER_FORM_TAPS_GLOBAL == 2
    assert int(defs["HZSDR_RESAMPLER_FORM_TAPS_UNIFORM"]) == hz.RESAMPLER_FORM_TAPS_UNIFORM == 4
    assert int(defs["HZSDR_RESAMPLER_FORM_WINDOW_PADDED"]) == hz.RESAMPLER_FORM_WINDOW_PADDED == 8
    assert hz.RESAMPLER_FORM_WINDOW_PADDED is importlib.import_module("go-sdr_amd.resampler").RESAMPLER_FORM_WINDOW_PADDED


def test_python_layers_are_exported(hz):
    st = importlib.import_module("go-sdr_amd.stream")
    assert hz.Resampler is importlib.import_module("go-sdr_amd.resampler").Resampler
    assert callable(hz.resampler_taps) and callable(hz.Context.resampler) and callable(st.resampler_samples)
    assert issubclass(st.ResampleReader, st.Reader)
    for name in ("push", "flush", "pending", "outputs_for", "plan", "reset", "close", "__enter__", "__exit__"):
        assert callable(getattr(hz.Resampler, name)), name
    r = hz.Resampler.__new__(hz.Resampler)
    r.up, r.down = 160, 147
    assert r.sample_rate(44_100) == 48_000.0


# ---- the restatements ----------------------------------------------------------------------------

@pytest.mark.parametrize("up,down,ntaps,n", SHAPES)
def test_restatements_agree(up, down, ntaps, n):
    h = np.random.default_rng(ntaps).standard_normal(ntaps)
    x = rand_c64(up * 7 + down, n).astype(np.complex128)
    a, b = ref.upfirdn_direct(h, x, up, down), ref.upfirdn_poly(h, x, up, down)
    assert a.shape == b.shape == (ref.total_outputs(n, ntaps, up, down),)
    err = np.abs(a - b).max() / max(np.abs(a).max(), 1e-300)
    print(f"U={up} D={down} L={ntaps} N={n}: direct / polyphase {err:.3e}")
    assert err <= 1e-10
    try:
        from scipy.signal import upfirdn
    except ImportError:
        return  # (only this assertion needs scipy)
    c = upfirdn(h, x, up, down)
    assert c.shape == a.shape, "upfirdn's length"
    assert np.abs(a - c).max() <= 1e-10 * np.abs(c).max() and np.abs(b - c).max() <= 1e-10 * np.abs(c).max()


def test_an_empty_stream_has_no_outputs():
    assert ref.upfirdn_poly(np.ones(5), np.zeros(0), 3, 2).shape == (0,) and ref.upfirdn_direct(np.ones(5), np.zeros(0), 3, 2).shape == (0,)
    assert ref.total_outputs(0, 5, 3, 2) == 0 and ref.outputs_after(0, 3, 2) == 0


def test_bound_values():
    assert ref.bound(1) == pytest.approx(1.8e-7) and ref.bound(64) == pytest.approx(3.96e-6)


# ---- resampler_taps ------------------------------------------------------------------------------

@pytest.mark.parametrize("up,down", [(1, 4), (3, 2), (2, 3), (160, 147), (147, 160), (2, 5), (8, 1), (1, 1), (24, 25), (4, 1), (1024, 1)])
@pytest.mark.parametrize("tpp", [8, 16])
def test_resampler_taps(hz, up, down, tpp):
    h = hz.resampler_taps(up, down, tpp)
    assert h.dtype == np.float32 and h.shape == (tpp * up,)
    assert np.array_equal(h, h[::-1]), "symmetric"
    assert abs(float(h.astype(np.float64).sum()) - up) <= 1e-6 * up
    phases = h.astype(np.float64).reshape(tpp, up).sum(axis=0)
    worst = np.abs(phases - 1.0).max()
    print(f"U={up} D={down} taps_per_phase={tpp}: |phase sum - 1| <= {worst:.2e}")
    assert worst <= 5e-4


def test_resampler_taps_arguments(hz):
    for bad in ((0, 1, 16), (1, 0, 16), (1, 1, 0)):
        with pytest.raises(ValueError):
            hz.resampler_taps(*bad)
    assert hz.resampler_taps(3, 2).shape == (48,)


# ---- counts --------------------------------------------------------------------------------------

@pytest.mark.parametrize("up,down", [(3, 2), (2, 3), (160, 147), (1, 8), (1024, 1), (1, 1024), (5, 5), (7, 5)])
def test_count_identities(up, down):
    """M(N) is monotone, and for every split N = a + b the two pushes' counts sum to M(N): the count of a push is
    M(a + b) - M(a), whatever came before."""
    m = [ref.outputs_after(n, up, down) for n in range(0, 400)]
    assert m[0] == 0 and all(b >= a for a, b in zip(m, m[1:]))
    assert all(x == -(-n * up // down) for n, x in enumerate(m))
    for n in (1, 2, 7, 146, 147, 148, 399):
        for a in range(n + 1):
            first, second = m[a] - m[0], m[n] - m[a]
            assert first + second == m[n] and second >= 0
    for ntaps in (1, up, up + 1, 16 * up):
        for n in (1, 5, 300):
            assert ref.stream_outputs(n, ntaps, up, down) >= ref.total_outputs(n, ntaps, up, down) > 0
            if ntaps >= up:
                assert ref.stream_outputs(n, ntaps, up, down) == ref.total_outputs(n, ntaps, up, down)

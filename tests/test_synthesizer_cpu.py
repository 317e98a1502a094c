"""The polyphase synthesis bank's ABI and host-side helpers, without a GPU: include/hzsdr_synthesizer.h is C99, its C
walkthrough names every entry, the library exports them and _capi.SYNTHESIZER_SIGNATURES binds them exactly; the
weighted-overlap-add prototype's property; and the float64 restatements of the definition (tests/synthesizer_ref.py)
agree with each other, are the adjoint of the channelizer's (tests/channelizer_ref.py) and invert it."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import channelizer_ref as cref
import synthesizer_ref as ref
from conftest import ROOT
from util import rand_c64

HEADER = os.path.join(ROOT, "include", "hzsdr_synthesizer.h")
WALK = os.path.join(ROOT, "tests", "c", "test_synthesizer_abi.c")
ENTRIES = {"hzsdr_synthesizer_create", "hzsdr_synthesizer_push", "hzsdr_synthesizer_flush", "hzsdr_synthesizer_pending",
           "hzsdr_synthesizer_group_frames", "hzsdr_synthesizer_reset", "hzsdr_synthesizer_free"}
GCC = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include")]


@pytest.fixture(scope="module")
def hz():
    return importlib.import_module("go-sdr_amd")


def synthesizer_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(hzsdr_[a-z0-9_]+)\s*\(", text)))


def test_header_is_c99(tmp_path):
    src = tmp_path / "inc.c"
    src.write_text('#include "hzsdr_synthesizer.h"\n'
                   "int main(void) { hzsdr_synthesizer *s = 0; return (s != 0) + HZSDR_CHANNELIZER_CHANNEL_MAJOR - HZSDR_ORDER_NEGATIVE_FIRST; }\n")
    subprocess.check_call(GCC + ["-c", str(src), "-o", str(tmp_path / "inc.o")])


def test_header_declares_exactly_the_entries():
    assert len(ENTRIES) == 7 and set(synthesizer_symbols()) == ENTRIES


def test_c_walkthrough_names_every_entry():
    text = open(WALK).read()
    missing = [s for s in synthesizer_symbols() if not re.search(r"\b" + s + r"\s*\(", text)]
    assert missing == []
    assert "synthesizer-abi ok" in text


def test_c_walkthrough_compiles_as_c99(tmp_path):
    subprocess.check_call(GCC + ["-c", WALK, "-o", str(tmp_path / "w.o")])


def test_library_exports_and_ctypes_table(hz):
    capi = importlib.import_module("go-sdr_amd._capi")
    syms = synthesizer_symbols()
    for s in syms:
        assert hasattr(capi.lib, s), f"{s} declared in hzsdr_synthesizer.h but not exported"
    assert sorted(capi.SYNTHESIZER_SIGNATURES) == syms
    assert not set(capi.SYNTHESIZER_SIGNATURES) & (set(capi.SIGNATURES) | set(capi.SPECTRUM_SIGNATURES) | set(capi.CHANNELIZER_SIGNATURES))
    for name, (res, args) in capi.SYNTHESIZER_SIGNATURES.items():
        fn = getattr(capi.lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_signatures_have_the_header_arity(hz):
    capi = importlib.import_module("go-sdr_amd._capi")
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    found = re.findall(r"\bint (hzsdr_synthesizer_[a-z_]+)\s*\(([^)]*)\)", text)
    assert {name for name, _ in found} == ENTRIES
    for name, params in found:
        assert len(capi.SYNTHESIZER_SIGNATURES[name][1]) == len(params.split(",")), name


def test_constants_match_header(hz):
    """The synthesizer's layouts and orders are the channelizer's: its header defines none of its own and includes
    the one that does."""
    text = open(HEADER).read()
    assert re.findall(r"#define (HZSDR_\w+) (\d+)", text) == []
    assert '#include "hzsdr_channelizer.h"' in text
    cdefs = dict(re.findall(r"#define (HZSDR_\w+) (\d+)", open(os.path.join(ROOT, "include", "hzsdr_channelizer.h")).read()))
    assert int(cdefs["HZSDR_CHANNELIZER_FRAME_MAJOR"]) == hz.CHANNELIZER_FRAME_MAJOR == 0
    assert int(cdefs["HZSDR_CHANNELIZER_CHANNEL_MAJOR"]) == hz.CHANNELIZER_CHANNEL_MAJOR == 1
    sdefs = dict(re.findall(r"#define (HZSDR_\w+) (\d+)", open(os.path.join(ROOT, "include", "hzsdr_spectrum.h")).read()))
    assert int(sdefs["HZSDR_ORDER_ZERO_FIRST"]) == hz.ZERO_FIRST
    assert int(sdefs["HZSDR_ORDER_NEGATIVE_FIRST"]) == hz.NEGATIVE_FIRST


def test_python_layers_are_exported(hz):
    st = importlib.import_module("go-sdr_amd.stream")
    assert hz.Synthesizer is importlib.import_module("go-sdr_amd.synthesizer").Synthesizer
    assert callable(hz.wola_taps) and callable(hz.Context.synthesizer) and callable(st.synthesizer_samples)
    s = hz.Synthesizer.__new__(hz.Synthesizer)
    s.hop = 256
    assert s.sample_rate(80_000) == 20_480_000.0


# ---- the weighted-overlap-add prototype ----------------------------------------------------------

@pytest.mark.parametrize("m", [256, 1024, 8192])
def test_wola_taps_overlap_to_one(hz, m):
    g = hz.wola_taps(m)
    assert g.dtype == np.float32 and g.shape == (m,) and g[0] == 0.0 and g[m // 2] == 1.0
    c = ref.overlap_gain(g, m // 2, 4 * m)[m // 2:3 * m]  # (the steady region: two frames cover every position)
    err = np.abs(c - 1.0).max()
    print(f"M={m}: |sum_j g^2[t - jD] - 1| <= {err:.3e}")
    assert err <= 2e-7


# ---- the restatements ----------------------------------------------------------------------------

def frames_c128(seed, f, m):
    return rand_c64(seed, f * m).astype(np.complex128).reshape(f, m)


@pytest.mark.parametrize("m,p,d,f", [(256, 2, 100, 7), (256, 1, 128, 5), (512, 3, 512, 4)])
def test_restatements_agree(hz, m, p, d, f):
    g = hz.channelizer_taps(m, p)
    Y = frames_c128(m + p + d, f, m)
    b = ref.synth_ola(Y, g, m, d)
    assert b.shape == ((f - 1) * d + p * m,)
    a = ref.synth_direct(Y, g, m, d, np.arange(b.shape[0]))
    err = np.linalg.norm(a - b) / np.linalg.norm(b)
    print(f"M={m} P={p} D={d} F={f}: direct / overlap-add relative L2 {err:.3e}")
    assert err <= 1e-10


@pytest.mark.parametrize("m,p,d,f", [(256, 4, 192, 9), (512, 3, 100, 12), (256, 8, 256, 6), (256, 2, 1, 300)])
def test_adjoint_of_the_channelizer(hz, m, p, d, f):
    """<Y, A x> = <A* Y, x> for the channelizer A (channelizer_ref.channels_fold) and the synthesis bank A*."""
    g = hz.channelizer_taps(m, p)
    n = ref.samples_of(f, p * m, d)
    x = rand_c64(3 * m + d, n).astype(np.complex128)
    Y = frames_c128(5 * m + f, f, m)
    ax = cref.channels_fold(x, g, m, d)
    assert ax.shape == (f, m)
    lhs = np.vdot(Y, ax)
    rhs = np.vdot(ref.synth_ola(Y, g, m, d), x)
    print(f"M={m} P={p} D={d} F={f}: |<Y,Ax> - <A*Y,x>| / |<Y,Ax>| = {abs(lhs - rhs) / abs(lhs):.3e}")
    assert abs(lhs - rhs) <= 1e-10 * abs(lhs)


@pytest.mark.parametrize("m", [256, 1024])
def test_wola_round_trip(hz, m):
    """Analysis then synthesis with wola_taps at D = M / 2 returns M c[t] x[t], c = sum_j g^2[t - jD] of the rounded
    taps: with L <= M no aliasing term exists."""
    d, f = m // 2, 20
    g = hz.wola_taps(m)
    n = ref.samples_of(f, m, d)
    x = rand_c64(m + 9, n).astype(np.complex128)
    back = ref.synth_ola(cref.channels_fold(x, g, m, d), g, m, d)
    c = ref.overlap_gain(g, d, n)
    lo, hi = m - d, n - (m - d)
    got = back[lo:hi] / (m * c[lo:hi])
    err = np.linalg.norm(got - x[lo:hi]) / np.linalg.norm(x[lo:hi])
    print(f"M={m}: round trip relative L2 {err:.3e}")
    assert err <= 1e-6


def test_bound_values():
    assert ref.bound(256, 1) == pytest.approx(3e-7 * 8 + 6e-8 * 3)
    assert ref.bound(8192, 8) == pytest.approx(3e-7 * 13 + 6e-8 * 10)
    assert ref.terms(1024, 1024) == 1 and ref.terms(2 * 256, 100) == 6 and ref.terms(512, 1) == 512

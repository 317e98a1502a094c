"""The tuner bank's ABI, arithmetic and host-side helpers, without a GPU: include/hzsdr_tuner.h is C99 and declares
exactly its ten entries, the library exports them and _capi.TUNER_SIGNATURES binds them exactly; tuner_word; the
bit-exact restatement (tests/host/tuner_ref.cpp, over the header the kernel evaluates) stays within the bound derived in
tests/tuner_ref.py of the independent float64 restatement over every shape of the GPU tests -- the bound holds for the
contract alone, before a GPU is involved; the program's step-1 taps and tables against float64."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import tuner_ref as ref
from conftest import ROOT
from util import rand_c64, rand_u8

HEADER = os.path.join(ROOT, "include", "hzsdr_tuner.h")
ENTRIES = {"hzsdr_tuner_create", "hzsdr_tuner_push", "hzsdr_tuner_flush", "hzsdr_tuner_outputs_for", "hzsdr_tuner_pending",
           "hzsdr_tuner_plan", "hzsdr_tuner_set_words", "hzsdr_tuner_readout", "hzsdr_tuner_reset", "hzsdr_tuner_free"}
GCC = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include")]


@pytest.fixture(scope="module")
def hz():
    return importlib.import_module("go-sdr_amd")


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("tuner_ref"))


def tuner_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(hzsdr_[a-z0-9_]+)\s*\(", text)))


def test_header_is_c99(tmp_path):
    src = tmp_path / "inc.c"
    src.write_text('#include "hzsdr_tuner.h"\n'
                   "int main(void) { hzsdr_tuner *t = 0; return (t != 0) + HZSDR_TUNER_FORM_CHUNKED - HZSDR_TUNER_READ_TAPS; }\n")
    subprocess.check_call(GCC + ["-c", str(src), "-o", str(tmp_path / "inc.o")])


def test_header_declares_exactly_the_entries():
    assert len(ENTRIES) == 10 and set(tuner_symbols()) == ENTRIES


def test_library_exports_and_ctypes_table(hz):
    capi = importlib.import_module("go-sdr_amd._capi")
    syms = tuner_symbols()
    for s in syms:
        assert hasattr(capi.lib, s), f"{s} declared in hzsdr_tuner.h but not exported"
    assert sorted(capi.TUNER_SIGNATURES) == syms
    others = (set(capi.SIGNATURES) | set(capi.SPECTRUM_SIGNATURES) | set(capi.CHANNELIZER_SIGNATURES) | set(capi.SYNTHESIZER_SIGNATURES)
              | set(capi.RESAMPLER_SIGNATURES) | set(capi.DEMOD_SIGNATURES))
    assert not set(capi.TUNER_SIGNATURES) & others
    for name, (res, args) in capi.TUNER_SIGNATURES.items():
        fn = getattr(capi.lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_signatures_have_the_header_arity(hz):
    capi = importlib.import_module("go-sdr_amd._capi")
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    found = re.findall(r"\bint (hzsdr_tuner_[a-z_]+)\s*\(([^)]*)\)", text)
    assert {name for name, _ in found} == ENTRIES
    for name, params in found:
        assert len(capi.TUNER_SIGNATURES[name][1]) == len(params.split(",")), name


def test_constants_match_header(hz):
    defs = dict(re.findall(r"#define (HZSDR_\w+) (\d+)", open(HEADER).read()))
    assert int(defs["HZSDR_TUNER_FORM_CHUNKED"]) == hz.TUNER_FORM_CHUNKED == 1
    assert int(defs["HZSDR_TUNER_FORM_TRANSPOSED"]) == hz.TUNER_FORM_TRANSPOSED == 2
    assert [int(defs["HZSDR_TUNER_READ_" + n]) for n in ("TAPS", "T2", "T1", "T0")] == [hz.TUNER_READ_TAPS, hz.TUNER_READ_T2, hz.TUNER_READ_T1,
                                                                                         hz.TUNER_READ_T0] == [1, 2, 3, 4]


def test_python_layers_are_exported(hz):
    st = importlib.import_module("go-sdr_amd.stream")
    assert hz.TunerBank is importlib.import_module("go-sdr_amd.tuner").TunerBank
    assert callable(hz.tuner_word) and callable(hz.Context.tuner_bank) and callable(st.tuner_rows)
    for name in ("push", "flush", "retune", "outputs_for", "pending", "plan", "readout", "reset", "sample_rate", "close", "__enter__", "__exit__"):
        assert callable(getattr(hz.TunerBank, name)), name
    b = hz.TunerBank.__new__(hz.TunerBank)
    b.down = 40
    assert b.sample_rate(2_400_000) == 60_000.0


def test_tuner_word(hz):
    fs = 2_400_000
    assert hz.tuner_word(0, fs) == 0 and hz.tuner_word(fs / 2, fs) == 1 << 31 and hz.tuner_word(-fs / 2, fs) == 1 << 31
    assert hz.tuner_word(fs / 4, fs) == 1 << 30 and hz.tuner_word(-fs / 4, fs) == 3 << 30
    assert hz.tuner_word(fs, fs) == 0 and hz.tuner_word(fs + fs / 8, fs) == 1 << 29 and hz.tuner_word(-3 * fs - fs / 8, fs) == 7 << 29
    # the smallest negative frequency is the largest word, and half a step rounds to the nearest
    assert hz.tuner_word(-fs / 2 ** 32, fs) == (1 << 32) - 1 and hz.tuner_word(-1e-9, fs) == 0
    # round trip: the word's frequency, fed back, gives the word; a frequency comes back within half a step
    for w in (1, 12345, (1 << 31) - 1, (1 << 31) + 1, (1 << 32) - 1, 0xdeadbeef):
        assert hz.tuner_word(w * fs / 2 ** 32, fs) == w
        f = w * fs / 2 ** 32 if w < 1 << 31 else (w - (1 << 32)) * fs / 2 ** 32
        assert hz.tuner_word(f, fs) == w
    for f in (851.0125e6 - 850e6, -1_090_000.0, 137.62e6 - 137.5e6):
        w = hz.tuner_word(f, fs)
        back = (w if w < 1 << 31 else w - (1 << 32)) * fs / 2 ** 32
        assert abs(back - f) <= fs / 2 ** 33
    for bad in (0, -1, float("nan")):
        with pytest.raises(ValueError):
            hz.tuner_word(1.0, bad)


# ---- the restatements ------------------------------------------------------------------------------

def converted_u8(x):
    """hzsdr_convert's u8 -> complex64 by the CPU oracle"""
    import oracle as orc
    out = np.zeros(x.shape[0], np.complex64)
    orc.convert(out, x)
    return out


def stream_length(k, q, down):
    """about three tiles of the smallest tile (32 outputs) and an odd remainder: what the GPU tests push, at least"""
    return 3 * 32 * down + 37


@pytest.fixture(scope="module")
def program(build_dir):
    """every shape through the host program with its own step 1, white complex64 and converted u8 samples, computed
    once: [((K, Q, D), words, h, x, y, G, tables)]"""
    cases = []
    for k, q, down in ref.SHAPES:
        n = stream_length(k, q, down)
        for x in (rand_c64(q * 7 + down, n), converted_u8(rand_u8(q + down, n))):
            cases.append((ref.words_for(k, seed=q), down, ref.taps_of(q), x, None))
    return [((len(c[0]), len(c[2]), c[1]), c[0], c[2], c[3]) + r for c, r in zip(cases, ref.exact(build_dir, cases))]


def test_program_is_within_the_bound_of_float64(program):
    for (k, q, down), words, h, x, y, _, _ in program:
        want = ref.tune(words, h, x, down)
        assert y.dtype == np.complex64 and y.shape == want.shape == (k, ref.total_outputs(len(x), q, down))
        err, bnd = np.abs(y.astype(np.complex128) - want), ref.bound(h, x)
        row, m = np.unravel_index(int(np.argmax(err)), err.shape)
        print(f"K={k} Q={q} D={down} N={len(x)}: max err {err.max():.3e} at tuner {row} (word {int(words[row]):#x}), m = {m}; bound {bnd:.3e}")
        assert err.max() <= bnd, f"K={k} Q={q} D={down}: tuner {row} output {m}: {err[row, m]:.3e} > {bnd:.3e}"
        assert np.abs(want).max() > 100 * bnd or q == 1, "the signal is not above the bound: the check shows nothing"


def ulps32(got, want):
    """|got - want| in units of the float32 ulp of `want` (float64), component arrays"""
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    return np.abs(got.astype(np.float64) - want) / ulp


def test_step_one_taps(program):
    """G of the program against h[q] exp(+2 pi i ((w q) mod 2^32) / 2^32) in float64: within one float32 ulp per
    component, exactly (as values) at w = 0 and w = 2^31; the padding tap is +0."""
    seen = set()
    for (k, q, down), words, h, x, _, g, _ in program:
        for row, w in enumerate(int(v) for v in words):
            want = ref.modulated_taps(w, h)
            assert g[row].shape == want.shape
            assert ulps32(g[row].real, want.real).max() <= 1.0 and ulps32(g[row].imag, want.imag).max() <= 1.0, (k, q, w)
            if w in (0, 1 << 31):
                assert np.array_equal(g[row].real, want.real.astype(np.float32)) and np.array_equal(g[row].imag, want.imag.astype(np.float32))
                assert not g[row].imag.any(), "a word on the real axis has real taps"
                seen.add(w)
            if w == 0:
                assert np.array_equal(g[row].real[:q], h)
            if w == 1 << 31:
                assert np.array_equal(g[row].real[:q], h * np.where(np.arange(q) % 2, -1, 1).astype(np.float32))
            if q % 2:
                assert g[row].view(np.uint32)[-2:].tolist() == [0, 0]
    assert seen == {0, 1 << 31}


def test_tables(program):
    """entry 0 of every table is exactly 1 + 0i (+0), every entry within one ulp of float64, T2 exact on the axes"""
    t = program[0][6]
    assert all(np.array_equal(p[6].view(np.uint32), t.view(np.uint32)) for p in program)
    t2, t1, t0 = t[:ref.N_T2], t[ref.N_T2:ref.N_T2 + ref.N_T1], t[ref.N_T2 + ref.N_T1:]
    for got, want in zip((t2, t1, t0), ref.tables()):
        assert got.shape == want.shape
        assert got[:1].view(np.uint32).tolist() == [0x3f800000, 0]
        assert ulps32(got.real, want.real).max() <= 1.0 and ulps32(got.imag, want.imag).max() <= 1.0
    assert t2[512] == -1j and t2[1024] == -1 and t2[1536] == 1j

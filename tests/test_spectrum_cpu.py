"""The fused power spectrum's ABI and host-side helpers, without a GPU: include/hzsdr_spectrum.h is C99, its C
walkthrough names every entry, the library exports them and _capi.SPECTRUM_SIGNATURES binds them exactly; the
FrequencySlice helpers reproduce fft/result_test.go (tests/golden/fft_result_kats.json)."""
import importlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "hzsdr_spectrum.h")


@pytest.fixture(scope="module")
def hz():
    return importlib.import_module("go-sdr_amd")


@pytest.fixture(scope="module")
def sp():
    return importlib.import_module("go-sdr_amd.spectrum")


@pytest.fixture(scope="module")
def fkats():
    with open(os.path.join(ROOT, "tests", "golden", "fft_result_kats.json")) as f:
        return json.load(f)


def spectrum_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(hzsdr_[a-z0-9_]+)\s*\(", text)))


def test_header_is_c99(tmp_path):
    src = tmp_path / "inc.c"
    src.write_text('#include "hzsdr_spectrum.h"\nint main(void) { return HZSDR_ORDER_NEGATIVE_FIRST - 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "inc.o")])


def test_header_declares_the_entries():
    syms = spectrum_symbols()
    assert {"hzsdr_spectrum_create", "hzsdr_spectrum_push", "hzsdr_spectrum_rows_for", "hzsdr_spectrum_pending",
            "hzsdr_spectrum_options", "hzsdr_spectrum_last_form", "hzsdr_spectrum_reset",
            "hzsdr_spectrum_free"} == set(syms)


def test_c_walkthrough_names_every_entry():
    text = open(os.path.join(ROOT, "tests", "c", "test_spectrum_abi.c")).read()
    missing = [s for s in spectrum_symbols() if not re.search(r"\b" + s + r"\s*\(", text)]
    assert missing == []


def test_c_walkthrough_compiles_as_c99(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-c", os.path.join(ROOT, "tests", "c", "test_spectrum_abi.c"), "-o", str(tmp_path / "w.o")])


def test_library_exports_and_ctypes_table(hz):
    capi = importlib.import_module("go-sdr_amd._capi")
    syms = spectrum_symbols()
    for s in syms:
        assert hasattr(capi.lib, s), f"{s} declared in hzsdr_spectrum.h but not exported"
    assert sorted(capi.SPECTRUM_SIGNATURES) == syms
    # the new table stays apart from hzsdr.h's
    assert not set(capi.SPECTRUM_SIGNATURES) & set(capi.SIGNATURES)


def test_constants_match_header(hz):
    text = open(HEADER).read()
    defs = dict(re.findall(r"#define (HZSDR_\w+) (\d+)", text))
    assert int(defs["HZSDR_ORDER_ZERO_FIRST"]) == hz.ZERO_FIRST == 0
    assert int(defs["HZSDR_ORDER_NEGATIVE_FIRST"]) == hz.NEGATIVE_FIRST == 1
    assert int(defs["HZSDR_SPECTRUM_FORM_ROW_WALK"]) == hz.SPECTRUM_FORM_ROW_WALK
    assert int(defs["HZSDR_SPECTRUM_FORM_FRAME_PARALLEL"]) == hz.SPECTRUM_FORM_FRAME_PARALLEL


# ---- FrequencySlice helpers: fft/result_test.go ------------------------------------------------

def complex_test_array(n):
    """complexTestArray (fft/result_test.go): bin i holds its own signed frequency index."""
    half = n // 2
    return np.concatenate([np.arange(half), np.arange(half) - half]).astype(np.float32)


def test_bin_by_freq_out_of_range(sp, fkats):
    for c in fkats["bin_by_freq_out_of_range"]:
        with pytest.raises(sp.ErrFrequencyOutOfSamplingRange):
            sp.bin_by_freq(c["bins"], c["sample_rate"], c["order"], c["freq"])


def test_bins_by_range_nyquist(sp, fkats):
    for c in fkats["bins_by_range_count"]:
        bins = sp.bins_by_range(c["bins"], c["sample_rate"], c["order"], c["range"])
        assert len(bins) == c["count"] and len(set(bins)) == c["distinct"]


def test_bins_by_range(sp, fkats):
    for c in fkats["bins_by_range"]:
        assert sp.bins_by_range(c["bins"], c["sample_rate"], c["order"], c["range"]) == c["want"], c


def test_freq_by_bin_round_trip(sp, fkats):
    for c in fkats["freq_by_bin_round_trip"]:
        f = sp.freq_by_bin(c["bins"], c["sample_rate"], c["order"], c["bin"])
        assert f == c["freq"], c
        assert sp.bin_by_freq(c["bins"], c["sample_rate"], c["order"], f) == c["bin"], c


def test_bin_by_freq_on_test_array(sp, fkats):
    for c in fkats["bin_by_freq_test_array"]:
        a = complex_test_array(c["bins"])
        if c["shifted"]:
            sp.shift(a)
        assert a[sp.bin_by_freq(c["bins"], c["sample_rate"], c["order"], c["freq"])] == c["value"], c


def test_shift(sp, fkats):
    c = fkats["shift_test_array"]
    a = complex_test_array(c["bins"])
    for i, v in c["before"]:
        assert a[i] == v
    sp.shift(a)
    for i, v in c["after"]:
        assert a[i] == v
    sp.shift(a)
    for i, v in c["before"]:
        assert a[i] == v


def test_helper_edges(sp):
    # BinBandwidth is a float32 quotient (fft/result.go:120-123): 20 MHz / 3 bins is not the float64 quotient
    assert sp.bin_bandwidth(3, 20_000_000) == float(np.float32(20_000_000) / np.float32(3))
    assert sp.bin_bandwidth(3, 20_000_000) != 20_000_000 / 3
    assert sp.nyquist(2048) == 1024.0
    # the asymmetric edges of BinByFreq: +nyquist is in range, -nyquist is not
    assert sp.bin_by_freq(2048, 2048, sp.ZeroFirst, 1024) == 1024
    with pytest.raises(sp.ErrFrequencyOutOfSamplingRange):
        sp.bin_by_freq(2048, 2048, sp.ZeroFirst, -1024)
    # truncation toward zero on both sides
    assert sp.bin_by_freq(2048, 2048, sp.ZeroFirst, -0.5) == 2048
    assert sp.bin_by_freq(2048, 2048, sp.NegativeFirst, -1.5) == 1023
    # FreqByBin accepts bin == len (fft/result.go:183) and refuses beyond
    assert sp.freq_by_bin(2048, 2048, sp.ZeroFirst, 2048) == 0.0
    with pytest.raises(sp.ErrFrequencyOutOfSamplingRange):
        sp.freq_by_bin(2048, 2048, sp.ZeroFirst, 2049)
    with pytest.raises(sp.ErrFrequencyOutOfSamplingRange):
        sp.bins_by_range(2048, 2048, sp.ZeroFirst, (0, 1025))


def test_scales(sp):
    w = sp.hann(1024)
    assert sp.spectrum_scale("power", 1024, 16, w) == float(np.float32(1.0 / (16 * float(w.astype(np.float64).sum()) ** 2)))
    d = 1.0 / (16 * 2e6 * float((w.astype(np.float64) ** 2).sum()))
    assert sp.spectrum_scale("density", 1024, 16, w, 2e6) == float(np.float32(d))
    assert sp.spectrum_scale("power", 256, 1) == float(np.float32(1.0 / 256 ** 2))
    with pytest.raises(ValueError):
        sp.spectrum_scale("density", 1024, 16, w)

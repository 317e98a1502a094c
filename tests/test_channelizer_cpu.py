"""The polyphase channelizer's ABI and host-side helpers, without a GPU: include/hzsdr_channelizer.h is C99, its C
walkthrough names every entry, the library exports them and _capi.CHANNELIZER_SIGNATURES binds them exactly; the
prototype designer's properties; and the two float64 restatements of the definition (tests/channelizer_ref.py)
agree with each other."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import channelizer_ref as ref
from conftest import ROOT
from util import rand_c64

HEADER = os.path.join(ROOT, "include", "hzsdr_channelizer.h")
WALK = os.path.join(ROOT, "tests", "c", "test_channelizer_abi.c")
ENTRIES = {"hzsdr_channelizer_create", "hzsdr_channelizer_push", "hzsdr_channelizer_frames_for",
           "hzsdr_channelizer_pending", "hzsdr_channelizer_reset", "hzsdr_channelizer_free"}
GCC = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include")]


@pytest.fixture(scope="module")
def hz():
    return importlib.import_module("go-sdr_amd")


def channelizer_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(hzsdr_[a-z0-9_]+)\s*\(", text)))


def test_header_is_c99(tmp_path):
    src = tmp_path / "inc.c"
    src.write_text('#include "hzsdr_channelizer.h"\n'
                   "int main(void) { return HZSDR_CHANNELIZER_CHANNEL_MAJOR - HZSDR_ORDER_NEGATIVE_FIRST; }\n")
    subprocess.check_call(GCC + ["-c", str(src), "-o", str(tmp_path / "inc.o")])


def test_header_declares_exactly_the_entries():
    assert set(channelizer_symbols()) == ENTRIES


def test_c_walkthrough_names_every_entry():
    text = open(WALK).read()
    missing = [s for s in channelizer_symbols() if not re.search(r"\b" + s + r"\s*\(", text)]
    assert missing == []


def test_c_walkthrough_compiles_as_c99(tmp_path):
    subprocess.check_call(GCC + ["-c", WALK, "-o", str(tmp_path / "w.o")])


def test_library_exports_and_ctypes_table(hz):
    capi = importlib.import_module("go-sdr_amd._capi")
    syms = channelizer_symbols()
    for s in syms:
        assert hasattr(capi.lib, s), f"{s} declared in hzsdr_channelizer.h but not exported"
    assert sorted(capi.CHANNELIZER_SIGNATURES) == syms
    assert not set(capi.CHANNELIZER_SIGNATURES) & (set(capi.SIGNATURES) | set(capi.SPECTRUM_SIGNATURES))
    for name, (res, args) in capi.CHANNELIZER_SIGNATURES.items():
        fn = getattr(capi.lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_signatures_have_the_header_arity(hz):
    capi = importlib.import_module("go-sdr_amd._capi")
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, params in re.findall(r"\bint (hzsdr_channelizer_[a-z_]+)\s*\(([^)]*)\)", text):
        assert len(capi.CHANNELIZER_SIGNATURES[name][1]) == len(params.split(",")), name


def test_constants_match_header(hz):
    defs = dict(re.findall(r"#define (HZSDR_\w+) (\d+)", open(HEADER).read()))
    assert int(defs["HZSDR_CHANNELIZER_FRAME_MAJOR"]) == hz.CHANNELIZER_FRAME_MAJOR == 0
    assert int(defs["HZSDR_CHANNELIZER_CHANNEL_MAJOR"]) == hz.CHANNELIZER_CHANNEL_MAJOR == 1
    sdefs = dict(re.findall(r"#define (HZSDR_\w+) (\d+)", open(os.path.join(ROOT, "include", "hzsdr_spectrum.h")).read()))
    assert int(sdefs["HZSDR_ORDER_ZERO_FIRST"]) == hz.ZERO_FIRST
    assert int(sdefs["HZSDR_ORDER_NEGATIVE_FIRST"]) == hz.NEGATIVE_FIRST


# ---- the prototype designer ---------------------------------------------------------------------

@pytest.mark.parametrize("m,p", [(256, 1), (256, 8), (1024, 4), (8192, 3), (512, 32)])
def test_channelizer_taps(hz, m, p):
    g = hz.channelizer_taps(m, p)
    assert g.dtype == np.float32 and g.shape == (m * p,)
    assert np.array_equal(g, g[::-1]), "the prototype is symmetric"
    # DC gain 1: the float64 sum of the rounded taps is within the rounding of the taps (half an ulp each, of their
    # own size) of 1
    s = float(g.astype(np.float64).sum())
    assert abs(s - 1.0) <= 2.0 ** -24 * float(np.abs(g).astype(np.float64).sum())
    assert g.max() == g[m * p // 2] == g[m * p // 2 - 1], "the peak is in the middle"


@pytest.mark.parametrize("p", [4, 8])
def test_channelizer_taps_first_null_near_channel_spacing(hz, p):
    """|G(f)| of the prototype: 1 at DC, -6 dB at the cutoff fs / (2M), and the first null where the Kaiser window's
    main lobe ends beyond the cutoff: (1/2 + sqrt(pi^2 + beta^2) / (pi P)) fs / M, i.e. 1.18 fs / M at P = 4 and
    0.84 fs / M at P = 8 for beta = 8; everything beyond 1.5 fs / M is stop band."""
    m, beta = 256, 8.0
    g = hz.channelizer_taps(m, p, beta).astype(np.float64)
    over = 64                                     # frequency grid: fs / (over * L)
    G = np.abs(np.fft.fft(g, over * m * p))
    step = 1.0 / (over * p)                      # grid step in units of fs / M
    assert abs(G[0] - 1.0) < 1e-6
    assert 0.45 < G[int(round(0.5 / step))] < 0.55
    k = 1
    while not (G[k] < G[k - 1] and G[k] <= G[k + 1] and G[k] < 1e-2):  # (not a ripple of the pass band)
        k += 1
    want = 0.5 + np.sqrt(np.pi ** 2 + beta ** 2) / (np.pi * p)
    assert abs(k * step - want) <= 0.05, (k * step, want)
    assert 0.5 < k * step < 1.25
    assert G[int(1.5 / step):len(G) // 2].max() < 1e-3, "stop band"


def test_channel_helpers(hz):
    ch = hz.Channelizer.__new__(hz.Channelizer)
    ch.channels, ch.hop = 1024, 256
    ch.order = hz.ZERO_FIRST
    fs = 20_480_000
    assert ch.channel_rate(fs) == fs / 256
    assert ch.channel_center(0, fs) == 0.0
    assert ch.channel_center(1, fs) == 20_000.0
    assert ch.channel_center(511, fs) == 511 * 20_000.0
    assert ch.channel_center(512, fs) == -fs / 2
    assert ch.channel_center(1023, fs) == -20_000.0
    ch.order = hz.NEGATIVE_FIRST
    assert ch.channel_center(0, fs) == -fs / 2
    assert ch.channel_center(512, fs) == 0.0
    assert ch.channel_center(1023, fs) == 511 * 20_000.0
    with pytest.raises(IndexError):
        ch.channel_center(1024, fs)


# ---- the two restatements -----------------------------------------------------------------------

@pytest.mark.parametrize("m,p,d", [(256, 4, 256), (256, 8, 192), (512, 3, 100), (256, 16, 1)])
def test_restatements_agree(hz, m, p, d):
    frames = 5
    L = m * p
    c = rand_c64(m + p + d, (frames - 1) * d + L + d // 2)
    g = hz.channelizer_taps(m, p)
    a = ref.channels_direct(c, g, m, d)
    b = ref.channels_fold(c, g, m, d)
    assert a.shape == b.shape == (frames, m)
    err = np.linalg.norm(a - b, axis=1) / np.linalg.norm(a, axis=1)
    assert err.max() <= 1e-10, err.max()


def test_bound_values():
    assert ref.bound(256, 1) == pytest.approx(3e-7 * 8 + 6e-8 * 3)
    assert ref.bound(8192, 8) == pytest.approx(3e-7 * 13 + 6e-8 * 10)

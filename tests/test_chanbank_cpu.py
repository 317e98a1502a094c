"""The channel bank's ABI, arithmetic and host-side helpers, without a GPU: include/hzsdr_chanbank.h is C99 and declares
exactly its eight entries, the library exports them and _capi.CHANBANK_SIGNATURES binds them exactly; the constants;
channel_center for odd and even M in both orders; the DFT table of every M against an independent float64 value; the
bit-exact restatement (tests/host/chanbank_ref.cpp: the contract evaluated directly and a host transcription of the
kernel's indexing, which the program holds against each other bit for bit) within the bound derived in
tests/chanbank_ref.py of the float64 restatement over every shape and format of the GPU tests, whole and cut streams --
the bound holds for the contract alone, before a GPU is involved."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import chanbank_ref as ref
from conftest import ROOT
from util import rand_c64, rand_i8, rand_i16, rand_u8

HEADER = os.path.join(ROOT, "include", "hzsdr_chanbank.h")
ENTRIES = {"hzsdr_chanbank_create", "hzsdr_chanbank_push", "hzsdr_chanbank_frames_for", "hzsdr_chanbank_pending", "hzsdr_chanbank_plan",
           "hzsdr_chanbank_readout", "hzsdr_chanbank_reset", "hzsdr_chanbank_free"}
GCC = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include")]
RAND = {"c64": rand_c64, "u8": rand_u8, "i8": rand_i8, "i16": rand_i16}


@pytest.fixture(scope="module")
def hz():
    return importlib.import_module("go-sdr_amd")


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("chanbank_ref"))


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def chanbank_symbols():
    return sorted(set(re.findall(r"\b(hzsdr_[a-z0-9_]+)\s*\(", header_text())))


def test_header_is_c99(tmp_path):
    src = tmp_path / "inc.c"
    src.write_text('#include "hzsdr_chanbank.h"\n'
                   "int main(void) { hzsdr_chanbank *c = 0; return (c != 0) + HZSDR_CHANBANK_FORM_A_LDS - HZSDR_CHANBANK_READ_DFT\n"
                   "  + HZSDR_CHANNELIZER_FRAME_MAJOR + HZSDR_ORDER_ZERO_FIRST; }\n")
    subprocess.check_call(GCC + ["-c", str(src), "-o", str(tmp_path / "inc.o")])


def test_header_declares_exactly_the_entries():
    assert len(ENTRIES) == 8 and set(chanbank_symbols()) == ENTRIES
    # the order and layout constants are the channelizer's, not redefined
    assert not re.findall(r"#define\s+HZSDR_(ORDER|CHANNELIZER)_", open(HEADER).read())


def test_library_exports_and_ctypes_table(hz):
    capi = importlib.import_module("go-sdr_amd._capi")
    syms = chanbank_symbols()
    for s in syms:
        assert hasattr(capi.lib, s), f"{s} declared in hzsdr_chanbank.h but not exported"
    assert sorted(capi.CHANBANK_SIGNATURES) == syms
    others = (set(capi.SIGNATURES) | set(capi.SPECTRUM_SIGNATURES) | set(capi.CHANNELIZER_SIGNATURES) | set(capi.SYNTHESIZER_SIGNATURES)
              | set(capi.RESAMPLER_SIGNATURES) | set(capi.DEMOD_SIGNATURES) | set(capi.TUNER_SIGNATURES))
    assert not set(capi.CHANBANK_SIGNATURES) & others
    for name, (res, args) in capi.CHANBANK_SIGNATURES.items():
        fn = getattr(capi.lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_signatures_have_the_header_arity(hz):
    capi = importlib.import_module("go-sdr_amd._capi")
    found = re.findall(r"\bint (hzsdr_chanbank_[a-z_]+)\s*\(([^)]*)\)", header_text())
    assert {name for name, _ in found} == ENTRIES
    for name, params in found:
        assert len(capi.CHANBANK_SIGNATURES[name][1]) == len(params.split(",")), name
    # the entries the channelizer shares have the channelizer's signatures
    for name in ("create", "push", "frames_for", "pending", "reset", "free"):
        assert capi.CHANBANK_SIGNATURES["hzsdr_chanbank_" + name] == capi.CHANNELIZER_SIGNATURES["hzsdr_channelizer_" + name], name


def test_constants_match_header(hz):
    defs = dict(re.findall(r"#define (HZSDR_\w+) (\d+)", open(HEADER).read()))
    assert int(defs["HZSDR_CHANBANK_FORM_A_LDS"]) == hz.CHANBANK_FORM_A_LDS == 1
    assert [int(defs["HZSDR_CHANBANK_READ_" + n]) for n in ("DFT", "TAPS")] == [hz.CHANBANK_READ_DFT, hz.CHANBANK_READ_TAPS] == [1, 2]


def test_python_layers_are_exported(hz):
    st = importlib.import_module("go-sdr_amd.stream")
    cb = importlib.import_module("go-sdr_amd.chanbank")
    assert hz.ChannelBank is cb.ChannelBank and cb.channelizer_taps is hz.channelizer_taps
    assert callable(hz.Context.channel_bank) and callable(st.channel_bank_frames)
    for name in ("push", "frames_for", "pending", "plan", "readout", "reset", "channel_rate", "channel_center", "close", "__enter__", "__exit__"):
        assert callable(getattr(hz.ChannelBank, name)), name
    g = hz.channelizer_taps(100, 8)
    assert g.shape == (800,) and g.dtype == np.float32 and abs(float(g.astype(np.float64).sum()) - 1.0) < 1e-6


def bank_of(hz, m, order, hop=None):
    b = hz.ChannelBank.__new__(hz.ChannelBank)
    b.channels, b.order, b.hop = m, order, m if hop is None else hop
    return b


@pytest.mark.parametrize("m", [2, 7, 8, 25, 100, 255])
def test_channel_center(hz, m):
    """position pos(k) holds channel k, whose centre is k fs / M folded to [-fs/2, fs/2): odd M has no channel at
    -fs/2, NegativeFirst starts at -floor(M / 2) fs / M and ascends (numpy's fftshift of fftfreq)"""
    fs = 2_400_000.0
    want = np.fft.fftfreq(m, 1.0 / fs)
    zero, neg = bank_of(hz, m, hz.ZERO_FIRST), bank_of(hz, m, hz.NEGATIVE_FIRST)
    assert np.allclose([zero.channel_center(k, fs) for k in range(m)], want, rtol=1e-15, atol=0)
    assert np.allclose([neg.channel_center(k, fs) for k in range(m)], np.fft.fftshift(want), rtol=1e-15, atol=0)
    for k in range(m):
        assert neg.channel_center(ref.pos(k, m, True), fs) == zero.channel_center(k, fs)
    centers = [neg.channel_center(k, fs) for k in range(m)]
    assert centers == sorted(centers) and centers[0] == -(m // 2) * fs / m and centers[m // 2] == 0.0
    for bad in (-1, m):
        with pytest.raises(IndexError):
            neg.channel_center(bad, fs)
    assert bank_of(hz, m, hz.ZERO_FIRST, hop=max(1, m // 2)).channel_rate(fs) == fs / max(1, m // 2)


# ---- the restatements ------------------------------------------------------------------------------

def stream(fmt, m, p, d, frames):
    n = m * p + (frames - 1) * d + d // 2
    return ref.converted(fmt, RAND[fmt](1000 * m + 10 * p + d, n))


@pytest.fixture(scope="module")
def program(build_dir, orc):
    """every shape and format through the host program with its own table, whole and cut (at 1, inside a frame, at a
    frame edge, at a tile edge, with an empty push), computed once: [(M, P, D, fmt, g, x, y, table)];
    the program itself fails where its two evaluations differ in a bit"""
    cases, keys = [], []
    for s, (m, p, d) in enumerate(ref.SHAPES):
        g = ref.taps_of(m, p)
        for i, fmt in enumerate(ref.FORMATS):
            x = stream(fmt, m, p, d, 2 * ref.tile_frames(m) + 5)
            ntaps = m * p
            cuts = sorted({1, ntaps + 3 * d + max(1, d // 2), ntaps + 3 * d, ntaps + (ref.tile_frames(m) - 1) * d})
            # (every format both ways over the list: the formats cut in one shape are the whole ones of the next)
            cases.append((m, d, g, x, [] if (s + i) % 2 == 0 else cuts + [cuts[-1]], None))
            keys.append((m, p, d, fmt, g, x))
    return [k + r for k, r in zip(keys, ref.exact(build_dir, cases))]


def test_program_is_within_the_bound_of_float64(program):
    assert len(program) == 4 * len(ref.SHAPES) and {p[3] for p in program} == set(ref.FORMATS)
    worst = 0.0
    for m, p, d, fmt, g, x, y, _ in program:
        want = ref.fold_dft(g, x, m, d)
        assert y.dtype == np.complex64 and y.shape == want.shape == (2 * ref.tile_frames(m) + 5, m)
        err, bnd = np.abs(y.astype(np.complex128) - want), ref.bound(g, x, m)
        j, k = np.unravel_index(int(np.argmax(err)), err.shape)
        worst = max(worst, float(err.max()) / bnd)
        assert err.max() <= bnd, f"M={m} P={p} D={d} {fmt}: frame {j} channel {k}: {err[j, k]:.3e} > {bnd:.3e}"
        assert np.abs(want).max() > 100 * bnd, "the signal is not above the bound: the check shows nothing"
    print(f"worst error / bound over {len(program)} cases: {worst:.3f}")


def test_fold_and_dft_is_the_definition():
    """the float64 fold + DFT against the definition term by term, on the shapes small enough for it"""
    for m, p, d in [s for s in ref.SHAPES if s[0] * s[1] <= 96]:
        g, x = ref.taps_of(m, p), rand_c64(m + p + d, m * p + 6 * d + d // 2)
        a, b = ref.definition(g, x, m, d), ref.fold_dft(g, x, m, d)
        assert a.shape == b.shape == (7, m)
        assert np.abs(a - b).max() <= 1e-13 * float(np.abs(g).sum()) * 2.0


def test_tables_of_every_m(build_dir):
    """W of every M, as the planner makes it (through the host program fed nothing) and as the program's own copy makes
    it: equal bit for bit; within 2^-24 of an independent float64 value; exact on the axes; column 0 exactly 1 + 0i;
    the padding column +0"""
    exe = ref.build_exact(build_dir)
    plan_exe = os.path.join(build_dir, "chanbank_tables")
    src = os.path.join(build_dir, "tables.cpp")
    with open(src, "w") as f:
        f.write('#include <cstdio>\n#include "hz_chanbank_plan.h"\n'
                "int main() { for (unsigned m = 2; m <= 255; m++) { auto w = hz::cp::chanbank_tables(m); fwrite(w.data(), 8, w.size(), stdout); } }\n")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"), src, "-o", plan_exe])
    raw = subprocess.run([plan_exe], stdout=subprocess.PIPE, check=True).stdout
    own = ref.exact(build_dir, [(m, 1, np.ones(m, np.float32), np.zeros(0, np.complex64), [], None) for m in range(2, 256)])
    assert os.path.exists(exe)
    off = 0
    for m, (_, tab) in zip(range(2, 256), own):
        mp = (m + 1) // 2 * 2
        w = np.frombuffer(raw, np.complex64, m * mp, off).reshape(m, mp)
        off += 8 * m * mp
        assert w.tobytes() == tab.tobytes(), f"M={m}: the planner's table and the program's own differ"
        want = ref.table(m)
        assert np.abs(w[:, :m].real.astype(np.float64) - want.real).max() <= 2.0 ** -24, m
        assert np.abs(w[:, :m].imag.astype(np.float64) - want.imag).max() <= 2.0 ** -24, m
        assert np.ascontiguousarray(w[:, 0]).view(np.uint32).reshape(m, 2).tolist() == [[0x3f800000, 0]] * m, m
        assert w[0].view(np.uint32).reshape(mp, 2)[:m].tolist() == [[0x3f800000, 0]] * m, m
        if mp > m:
            assert not np.ascontiguousarray(w[:, m]).view(np.uint32).any(), m
        n = np.outer(np.arange(m), np.arange(m)) % m
        for cond, value in ((4 * n == m, -1j), (2 * n == m, -1.0), (4 * n == 3 * m, 1j), (n == 0, 1.0)):
            hit = w[:, :m][cond]
            assert (hit == np.complex64(value)).all(), (m, value)
            assert not np.signbit(hit.real[hit.real == 0]).any() and not np.signbit(hit.imag[hit.imag == 0]).any(), (m, value)
    assert off == len(raw)

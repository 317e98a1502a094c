"""The demapper bank (include/hzsdr_demap.h) without a GPU: the ABI's header, exports and bindings; the validation at
every bound's edge and one step outside; the host program tests/host/demap_ref.cpp (the bits the device must produce)
against the numpy restatement of tests/demap_ref.py -- whole-array steps -- for every kind, every m from 1 to 8, perm,
flip, holes and per-row gains; and anchors that do not lean on either restatement: noise-free symbols of the package's
constellations come back as the sent bits, the sign is the nearest point's bit (found in float64) wherever the two
minima differ, special values leave as the header says.  Nothing has a tolerance."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import demap_ref as ref
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "hzsdr_demap.h")
ENTRIES = {"hzsdr_demap_create", "hzsdr_demap_run", "hzsdr_demap_sizes", "hzsdr_demap_plan", "hzsdr_demap_free"}
GCC = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include")]


@pytest.fixture(scope="module")
def hz():
    return importlib.import_module("go-sdr_amd")


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("demap_ref"))


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


# ---- the ABI ---------------------------------------------------------------------------------------

def test_header_is_c99(tmp_path):
    src = tmp_path / "inc.c"
    src.write_text('#include "hzsdr_demap.h"\n'
                   "int main(void) { hzsdr_demap *d = 0; return (d != 0) + HZSDR_DEMAP_MAX_ROWS - HZSDR_DEMAP_MAX_BITS - HZSDR_DEMAP_MAX_SYMBOLS"
                   " - HZSDR_DEMAP_MAX_LLRS - HZSDR_DEMAP_MAX_OUT - HZSDR_DEMAP_MAX_FRAMES - HZSDR_DEMAP_C64 - HZSDR_DEMAP_REAL_F32 - HZSDR_DEMAP_LLR_F32"
                   " - HZSDR_DEMAP_FORM_GROUPED - HZSDR_DEMAP_FORM_PERM - HZSDR_DEMAP_FORM_TREE + (HZSDR_DEMAP_ERASED != 0u); }\n")
    subprocess.check_call(GCC + ["-c", str(src), "-o", str(tmp_path / "inc.o")])


def test_header_declares_exactly_the_entries():
    assert set(re.findall(r"\b(hzsdr_demap_[a-z0-9_]+)\s*\(", header_text())) == ENTRIES and len(ENTRIES) == 5


def test_library_exports_and_ctypes_table(hz):
    capi = importlib.import_module("go-sdr_amd._capi")
    for s in ENTRIES:
        assert hasattr(capi.lib, s), f"{s} declared in hzsdr_demap.h but not exported"
    assert set(capi.DEMAP_SIGNATURES) == ENTRIES
    for name, (res, args) in capi.DEMAP_SIGNATURES.items():
        fn = getattr(capi.lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    found = re.findall(r"\bint (hzsdr_demap_[a-z_]+)\s*\(([^)]*)\)", header_text())
    assert {name for name, _ in found} == ENTRIES
    kinds = {"unsigned": C.c_uint, "int": C.c_int, "size_t": C.c_size_t, "float": C.c_float}
    pointers = {"const float *points": C.c_float, "const float *gains": C.c_float, "const uint32_t *perm": C.c_uint32, "const uint8_t *flip": C.c_uint8,
                "size_t *": C.c_size_t, "int *form": C.c_int}
    for name, params in found:
        args = capi.DEMAP_SIGNATURES[name][1]
        decl = [" ".join(p.split()) for p in params.split(",")]
        assert len(args) == len(decl), name
        for a, d in zip(args, decl):  # argument for argument: a pointer for a pointer, the scalar types by width and sign
            if "*" in d:
                assert a is C.c_void_p or hasattr(a, "_type_") and not isinstance(a._type_, str), (name, d)
                for text, ctype in pointers.items():
                    if text in d:
                        assert a._type_ is ctype, (name, d)
            else:
                assert a is kinds[d.split()[0]], (name, d)


def test_constants_and_python_layers(hz):
    defs = dict(re.findall(r"#define (HZSDR_\w+) (\w+)", open(HEADER).read()))
    inc = lambda name: open(os.path.join(ROOT, "include", name)).read()
    assert int(defs["HZSDR_DEMAP_MAX_ROWS"]) == hz.DEMAP_MAX_ROWS == ref.MAX_ROWS == 8192
    assert int(defs["HZSDR_DEMAP_MAX_BITS"]) == hz.DEMAP_MAX_BITS == ref.MAX_BITS == 8
    assert int(defs["HZSDR_DEMAP_MAX_SYMBOLS"]) == hz.DEMAP_MAX_SYMBOLS == ref.MAX_SYMBOLS == 8192
    assert int(defs["HZSDR_DEMAP_MAX_LLRS"]) == hz.DEMAP_MAX_LLRS == ref.MAX_LLRS == 16384
    assert int(defs["HZSDR_DEMAP_MAX_OUT"]) == hz.DEMAP_MAX_OUT == ref.MAX_OUT == hz.LDPC_MAX_BITS == hz.VITERBI_MAX_BITS == 8192
    assert int(defs["HZSDR_DEMAP_MAX_FRAMES"]) == hz.DEMAP_MAX_FRAMES == ref.MAX_FRAMES == 1 << 22
    assert int(defs["HZSDR_DEMAP_ERASED"].rstrip("u"), 16) == hz.DEMAP_ERASED == ref.ERASED == 0xFFFFFFFF
    assert int(defs["HZSDR_DEMAP_C64"]) == hz.DEMAP_C64 == ref.C64 == hz.FMT_C64 == int(re.search(r"#define HZSDR_FMT_C64 (\d+)", inc("hzsdr.h")).group(1))
    assert int(defs["HZSDR_DEMAP_REAL_F32"]) == hz.DEMAP_REAL_F32 == ref.REAL_F32 == hz.SYMSYNC_REAL_F32
    assert int(defs["HZSDR_DEMAP_LLR_F32"]) == hz.DEMAP_LLR_F32 == ref.LLR_F32 == 33
    assert int(defs["HZSDR_DEMAP_FORM_GROUPED"]) == hz.DEMAP_FORM_GROUPED == ref.FORM_GROUPED == 1
    assert int(defs["HZSDR_DEMAP_FORM_PERM"]) == hz.DEMAP_FORM_PERM == ref.FORM_PERM == 2
    assert int(defs["HZSDR_DEMAP_FORM_TREE"]) == hz.DEMAP_FORM_TREE == ref.FORM_TREE == 4
    plan = open(os.path.join(ROOT, "go-sdr_amd", "csrc", "hz_demap_plan.h")).read()
    assert int(re.search(r"#define HZ_DEMAP_TREE_FROM (\d+)", plan).group(1)) == ref.TREE_FROM
    st = importlib.import_module("go-sdr_amd.stream")
    mod = importlib.import_module("go-sdr_amd.demap")
    for name in ("Demapper", "psk_points", "qam_points", "pam_points", "map_bits", "block_interleaver", "demap_gain", "pack_flip"):
        assert getattr(hz, name) is getattr(mod, name), name
    assert callable(hz.Context.demapper)
    import inspect
    for fn in (st.decoded_frames, st.corrected_frames, st.ldpc_frames):
        assert inspect.signature(fn).parameters["demap"].default is None
    for name in ("run", "ragged", "sizes", "plan", "close", "__enter__", "__exit__"):
        assert callable(getattr(hz.Demapper, name)), name
    hpp = open(os.path.join(ROOT, "go-sdr_amd", "cxx", "hzsdr.hpp")).read()
    assert "class Demapper" in hpp and '#include "../../include/hzsdr_demap.h"' in hpp
    make = open(os.path.join(ROOT, "go-sdr_amd", "csrc", "Makefile")).read()
    assert "hzsdr_demap.h" in make and "hz_demap" not in make.split("MFMA_UNITS =")[1].splitlines()[0]
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "hzsdr_demap.h" in open(os.path.join(ROOT, doc)).read(), doc
    header = " ".join(open(HEADER).read().replace(" * ", " ").split())
    for left in ("log-sum", "ombining repeated positions", "not multiples of 90 degrees", "ifferential modes", "separable fast path", "hanging the gain after create"):
        assert left in header, left
    assert "hzsdr_demap.h" in inc("hzsdr_softframe.h") and "hzsdr_demap.h" in inc("hzsdr_ldpc.h")


# ---- the helpers -----------------------------------------------------------------------------------

def test_constellations_and_helpers(hz):
    """unit mean power, Gray neighbours (nearest neighbours differ in one bit), the label's halves per axis, map_bits
    against a loop, block_interleaver against a written-out matrix, pack_flip and demap_gain"""
    for pts in [hz.qam_points(m) for m in (2, 4, 6, 8)] + [hz.psk_points(m) for m in (1, 2, 3, 4)] + [hz.pam_points(m) for m in (1, 2, 3)]:
        M = len(pts)
        assert abs(np.mean(np.abs(pts.astype(np.complex128)) ** 2) - 1) < 1e-6 and len(set(pts.tolist())) == M
        d = np.abs(pts[:, None].astype(np.complex128) - pts[None, :])
        np.fill_diagonal(d, np.inf)
        for p in range(M):
            for q in np.flatnonzero(d[p] < d[p].min() * 1.001):
                assert bin(p ^ int(q)).count("1") == 1, (M, p, q)
    q16 = hz.qam_points(4)
    assert all(q16[p].real == q16[p | 3].real and q16[p].imag == q16[p | 12].imag for p in range(16))
    assert np.allclose(hz.psk_points(2)[[0, 1, 3, 2]] * np.sqrt(2), [1 + 1j, -1 + 1j, -1 - 1j, 1 - 1j])  # Gray around the circle
    assert np.allclose(hz.pam_points(2)[[0, 1, 3, 2]] * np.sqrt(5), [-3, -1, 1, 3])
    assert np.allclose(hz.qam_points(2) * np.sqrt(2), [-1 - 1j, -1 + 1j, 1 - 1j, 1 + 1j])  # bit 1 is the positive side, per axis
    bits = ref.random_bits(24, 3)
    pts = hz.psk_points(3)
    want = [pts[int("".join(map(str, bits[3 * s:3 * s + 3])), 2)] for s in range(8)]
    assert np.array_equal(hz.map_bits(pts, bits), want) and hz.map_bits(pts, bits.reshape(2, 12)).shape == (2, 4)
    sent = np.arange(12).reshape(3, 4).T.reshape(-1)  # written in 3 rows of 4, sent column by column
    assert np.array_equal(sent[hz.block_interleaver(3, 4)], np.arange(12))
    assert hz.pack_flip([1, 0, 0, 0, 0, 0, 0, 1, 1]).tolist() == [0x81, 0x80] and hz.demap_gain(0.5) == 2.0
    with pytest.raises(ValueError):
        hz.qam_points(3)


# ---- the validation --------------------------------------------------------------------------------

def test_restated_validation(hz, build_dir):
    """Every bound accepted at its edge and refused one step outside: csrc/hz_demap_plan.h against the rules restated in
    Python.  (The sanitizers watch the same refusals in tests/test_demap_plan.py.)"""
    q4, p2 = hz.qam_points(2), hz.pam_points(1)
    sets = []

    def add(want, kind, points, S, n_gains=None, **kw):
        q = ref.Config(kind, points, S, **kw)
        assert n_gains is not None or ref.accepted(q) == want, (kind, S, kw)
        sets.append(((q, n_gains), want))

    add(True, ref.C64, q4, 8)
    for kind in (0, 2, 31, 34, 64):
        add(False, kind, q4, 8)
    for m, want in ((1, True), (8, True)):
        add(want, ref.C64, hz.psk_points(m), 8)
        add(want, ref.REAL_F32, hz.pam_points(m), 8)
    add(False, ref.C64, np.zeros(512, np.complex64), 8)  # m = 9
    add(False, ref.C64, np.zeros(1, np.complex64), 8)    # m = 0
    add(False, ref.C64, q4, 8, m=3)                       # the scalar disagrees with the array
    add(False, ref.C64, None, 8, m=2)                     # null points
    add(True, ref.LLR_F32, None, 8)
    add(False, ref.LLR_F32, None, 8, m=2, N=16)
    add(False, ref.LLR_F32, p2, 8)
    for bad in (np.inf, -np.inf, np.nan):
        pts = q4.copy()
        pts[2] = complex(0.5, bad)
        add(False, ref.C64, pts, 8)
        add(False, ref.REAL_F32, np.array([1.0, bad], np.float32), 8)
    for S, m, want in ((1, 2, True), (0, 2, False), (8192, 2, True), (8193, 1, False), (2048, 8, True), (2049, 8, False), (5461, 3, True), (5462, 3, False)):
        perm = np.zeros(7, np.int64)
        add(want, ref.C64, hz.psk_points(m), S, perm=perm)
    for N, want in ((1, True), (8192, True), (8193, False)):
        add(want, ref.C64, q4, 8, perm=np.arange(N) % 16)
    add(False, ref.C64, q4, 8, perm=np.zeros(0, np.int64))
    add(False, ref.C64, q4, 8, N=15)                      # no perm and N != S m
    add(False, ref.C64, q4, 8192)                         # no perm: N = 16384 is above the decoders' limit
    for entry, want in ((15, True), (16, False), (17, False), (0xFFFFFFFE, False), (0x80000000, False), (ref.ERASED, True)):
        perm = np.arange(16)
        perm[5] = entry
        add(want, ref.C64, q4, 8, perm=perm)
    for gains, rows, want in (([1.0], 3, True), ([1.0, 2.0, 3.0], 3, True), ([1.0, 2.0], 3, False), ([0.0], 1, False), ([-1.0], 1, False), ([np.inf], 1, False),
                              ([np.nan], 1, False), ([1e-45], 1, True), ([3.4e38], 1, True), ([1.0, 0.0, 1.0], 3, False)):
        add(want, ref.C64, q4, 8, gains=gains, rows=rows)
    add(False, ref.C64, q4, 8, n_gains=0)
    add(False, ref.C64, q4, 8, n_gains=2)
    add(True, ref.C64, q4, 8, rows=8192)
    add(False, ref.C64, q4, 8, rows=8193)
    add(False, ref.C64, q4, 8, rows=0)
    got = ref.check(build_dir, [s for s, _ in sets])
    for ((q, n_gains), want), ok in zip(sets, got):
        assert ok == want, (q.kind, q.m, q.S, q.N, q.rows, q.gains, n_gains, None if q.perm is None else q.perm[:8])
    assert sum(got) > 15 and sum(not g for g in got) > 30


# ---- the program against the restatement -----------------------------------------------------------------

def constellation(hz, kind, m):
    """a constellation of 2^m points for the kind: the package's where it has one, else a seeded irregular one"""
    if kind == ref.LLR_F32:
        return None
    if kind == ref.REAL_F32:
        return hz.pam_points(m)
    if m % 2 == 0:
        return hz.qam_points(m)
    if m <= 3:
        return hz.psk_points(m)
    g = ref.gaussian(100 + m, 2 << m)  # (APSK-like: no structure the kernel could lean on)
    return (g[:1 << m] + 1j * g[1 << m:]).astype(np.complex64)


@pytest.mark.parametrize("kind,m", [(ref.C64, m) for m in range(1, 9)] + [(ref.REAL_F32, m) for m in range(1, 9)] + [(ref.LLR_F32, 1)])
def test_program_against_whole_array_steps(hz, build_dir, kind, m):
    """noisy symbols with special values among them, under no perm, a perm with holes and repeats, a flip, and per-row
    gains, counts that leave slots out: the program's bits are numpy's"""
    pts = constellation(hz, kind, m)
    S, R, cap = 37, 3, 2
    L = S * m
    probe = ref.Config(kind, pts, S)
    if kind == ref.LLR_F32:
        sym = ref.gaussian(7, R * cap * S).reshape(R, cap, S).astype(np.float32)
    else:
        sym = ref.noisy_symbols(probe, np.stack([ref.random_bits(L, 50 + f) for f in range(R * cap)]).reshape(R, cap, L), 0.3, 11 * m)
    frames = ref.as_floats(probe, sym).copy()
    frames[0, 1, [0, 5, 9, 12, 13]] = np.nan, np.inf, -np.inf, -0.0, 3e19
    perm = (np.arange(L + 9) * 7 + 3) % L
    perm[[2, 11, L + 8]] = ref.ERASED
    perm[4] = perm[3]
    flip = ref.random_bits(len(perm), 77)
    counts = np.array([2, 0, 5], np.uint32)
    cases = [(ref.Config(kind, pts, S, rows=R, gains=[0.75]), frames, None),
             (ref.Config(kind, pts, S, rows=R, gains=[0.5, 2.0, 3.25], perm=perm, flip=flip), frames, counts),
             (ref.Config(kind, pts, S, rows=R, gains=[1.5], flip=ref.random_bits(L, 78)), frames, counts)]
    for (q, fr, cnt), got in zip(cases, ref.exact(build_dir, cases)):
        assert ref.accepted(q)
        want = ref.run(q, fr, cnt)
        assert np.array_equal(got, want), (kind, m, np.argwhere(got != want)[:4])
        assert cnt is None or not got[1].any()
    assert (got[0, 1] == ref.NAN_BITS).sum() >= 1


# ---- independent anchors ---------------------------------------------------------------------------------

def anchors(hz):
    return [("qam16", ref.C64, hz.qam_points(4)), ("qam64", ref.C64, hz.qam_points(6)), ("qam256", ref.C64, hz.qam_points(8)),
            ("qpsk", ref.C64, hz.psk_points(2)), ("8psk", ref.C64, hz.psk_points(3)), ("pam4", ref.REAL_F32, hz.pam_points(2))]


def test_noise_free_symbols_return_the_sent_bits(hz, build_dir):
    """every point of qam_points(4, 6, 8), psk_points(2, 3) and pam_points(2) sent through map_bits: the signs of the
    program's output are the sent bits, all of them"""
    cases, sent = [], []
    for _, kind, pts in anchors(hz):
        m = len(pts).bit_length() - 1
        S = 2 << m  # every label twice, in a seeded order
        labels = np.argsort(ref.splitmix64(m, S)) % (1 << m)
        bits = ((labels[:, None] >> (m - 1 - np.arange(m))) & 1).astype(np.uint8).reshape(-1)
        q = ref.Config(kind, pts, S)
        cases.append((q, ref.as_floats(q, hz.map_bits(pts, bits))[None, None], None))
        sent.append(bits)
    for (q, _, _), bits, got in zip(cases, sent, ref.exact(build_dir, cases)):
        assert np.array_equal((got[0, 0] >> 31) == 0, bits == 1) and not (got == ref.NAN_BITS).any(), q.m


@pytest.mark.parametrize("sigma", [0.0, 0.1])
def test_the_sign_is_the_nearest_points_bit(hz, build_dir, sigma):
    """unit-power 16/64/256-QAM, 8PSK and QPSK, 4096 random symbols each, noise-free and at sigma = 0.1 per component.
    The nearest point is found here in float64.  Wherever d0 != d1 the sign is the nearest point's bit; the (symbol,
    bit) pairs with d0 = d1 are at most 1 % (the restatement's own share on these inputs is 0)."""
    cases, near = [], []
    for name, kind, pts in anchors(hz)[:5]:
        m = len(pts).bit_length() - 1
        q = ref.Config(kind, pts, 512)  # 8 frames of 512 symbols
        sym = ref.noisy_symbols(q, ref.random_bits(4096 * m, 9 + m).reshape(8, 512 * m), sigma, 31 + m)
        cases.append((q, ref.as_floats(q, sym)[None], None))
        near.append(ref.nearest_bits(q, sym.astype(np.complex128)).reshape(-1))
    for (q, frames, _), bits, got in zip(cases, near, ref.exact(build_dir, cases)):
        _, (d0, d1) = ref.values(q, frames[0], 1.0)
        tie = (d0 == d1).reshape(-1)
        assert tie.mean() <= 0.01 and tie.sum() == 0, (q.m, tie.sum())
        sign = (got[0].reshape(-1) >> 31) == 0
        assert np.array_equal(sign[~tie], bits[~tie] == 1), (q.m, sigma)


def test_special_values(hz, build_dir):
    """NaN in either component erases the symbol's m values; +-inf and 3e19 overflow every distance to inf and inf - inf
    leaves as 0x7FC00000; -0 is 0; inputs of 1e-40 under a small gain keep their denormals; a hole and a flip over an
    erasure leave 0x7FC00000"""
    pts = hz.qam_points(4)
    x = np.zeros((1, 1, 16), np.float32)  # 8 symbols
    x[0, 0, :] = [np.nan, 0.3, 0.3, np.nan, np.inf, 0.1, 0.1, -np.inf, 3e19, 0.0, -0.0, -0.0, 0.0, 0.0, 0.3, -0.3]
    perm = np.concatenate([np.arange(32), [ref.ERASED, 0, 1]])
    flip = np.ones(35, np.uint8)
    plain, flipped = ref.exact(build_dir, [(ref.Config(ref.C64, pts, 8), x, None), (ref.Config(ref.C64, pts, 8, perm=perm, flip=flip), x, None)])
    v = plain[0, 0].reshape(8, 4)
    assert (v[:5] == ref.NAN_BITS).all() and not (v[5:] == ref.NAN_BITS).any()
    assert np.array_equal(v[5], v[6])  # -0 is 0
    assert np.array_equal(v[7] >> 31 == 0, ref.nearest_bits(ref.Config(ref.C64, pts, 8), np.complex128(0.3 - 0.3j)) == 1)
    w = flipped[0, 0]
    assert (w[:20] == ref.NAN_BITS).all() and w[32] == ref.NAN_BITS and w[33] == ref.NAN_BITS and np.array_equal(w[20:32], plain[0, 0, 20:] ^ 0x80000000)
    # the canonical NaN whatever NaN comes in
    odd = np.zeros((1, 1, 4), np.float32)
    odd[0, 0] = f32([0xFFC00001, 0x7F800001, 0x7FC00000, 0xFFFFFFFF])
    (got,) = ref.exact(build_dir, [(ref.Config(ref.LLR_F32, None, 4, flip=[1, 0, 1, 0]), odd, None)])
    assert (got == ref.NAN_BITS).all()
    # LLR: +-inf, -0 and the flip on the bit pattern
    vals = np.array([[[np.inf, -np.inf, -0.0, 0.0, 2.0, -3.0]]], np.float32)
    (got,) = ref.exact(build_dir, [(ref.Config(ref.LLR_F32, None, 6, flip=[0, 0, 0, 1, 1, 1], gains=[0.5]), vals, None)])
    assert got[0, 0].tolist() == [0x7F800000, 0xFF800000, 0x80000000, 0x80000000, 0xBF800000, 0x3FC00000]
    # denormals: values of 1e-40 under the gain 1 / 2, and distances and differences of some 1e-40 against points at +-1e-20
    tiny = np.array([1e-40, -1e-40], np.float32)
    q = ref.Config(ref.LLR_F32, None, 2, gains=[0.5])
    (got,) = ref.exact(build_dir, [(q, tiny[None, None], None)])
    assert np.array_equal(got[0, 0], (tiny * np.float32(0.5)).view(np.uint32)) and (got[0, 0] & 0x7F800000 == 0).all() and (got[0, 0] & 0x7FFFFF != 0).all()
    big = ref.Config(ref.REAL_F32, np.array([-1e-20, 1e-20], np.float32), 2, gains=[0.5])
    xs = np.array([[[1e-21, -3e-21]]], np.float32)
    (got,) = ref.exact(build_dir, [(big, xs, None)])
    assert np.array_equal(got, ref.run(big, xs)) and (got & 0x7F800000 == 0).all() and (got & 0x7FFFFF != 0).all()  # denormal values, kept
    assert (got[0, 0] >> 31).tolist() == [0, 1]


# ---- refusals through the library ----------------------------------------------------------------------

def test_call_refusals(build_dir):
    """hz_demap_plan.h's check of a call, the one hzsdr_demap_run makes before it launches or writes: cap = 0, rows * cap
    above 2^22, a short in_stride (invalid) and a short out_stride (destination too small) with rows > 1 and neither with
    one row, null in or out, and every way the two ranges can overlap -- by a float, in place, one inside the other's
    row gaps -- beside ranges that touch"""
    OK, INV, SMALL = ref.CALL_OK, ref.CALL_INVALID, ref.CALL_DST_TOO_SMALL
    S, m, cap = 10, 4, 3          # C64: W = 20, N = 40
    W, N = 2 * S, S * m
    A = 1 << 20
    out_at = lambda floats: A + 4 * floats
    sets = [((ref.C64, m, S, A, A + (1 << 16), cap * W, cap * N, cap, 3), OK),
            ((ref.C64, m, S, A, A + (1 << 16), cap * W, cap * N, 0, 3), INV),
            ((ref.C64, m, S, A, 1 << 40, 1 << 30, 1 << 30, ref.MAX_FRAMES // 3, 3), OK),
            ((ref.C64, m, S, A, 1 << 40, 1 << 30, 1 << 30, ref.MAX_FRAMES // 3 + 1, 3), INV),
            ((ref.C64, m, S, A, A + (1 << 16), cap * W - 1, cap * N, cap, 3), INV),
            ((ref.C64, m, S, A, A + (1 << 16), cap * W, cap * N - 1, cap, 3), SMALL),
            ((ref.C64, m, S, A, A + (1 << 16), 0, 0, cap, 1), OK),           # one row: the strides are not read
            ((ref.C64, m, S, 0, A, cap * W, cap * N, cap, 3), INV),
            ((ref.C64, m, S, A, 0, cap * W, cap * N, cap, 3), INV),
            ((ref.C64, m, S, A, A, cap * W, cap * N, cap, 1), INV),          # in place
            ((ref.C64, m, S, A, out_at(cap * W), 0, 0, cap, 1), OK),         # out begins where in ends
            ((ref.C64, m, S, A, out_at(cap * W - 1), 0, 0, cap, 1), INV),    # ... one float sooner
            ((ref.C64, m, S, out_at(cap * N), A, 0, 0, cap, 1), OK),         # in begins where out ends
            ((ref.C64, m, S, out_at(cap * N - 1), A, 0, 0, cap, 1), INV),
            ((ref.C64, m, S, A, out_at(cap * W), 1000, 1000, cap, 2), INV),  # out's rows inside in's row gaps: the ranges overlap
            ((ref.C64, m, S, A, out_at(1000 + cap * W), 1000, 1000, cap, 2), OK),
            ((ref.C64, m, S, A, A + (1 << 16), 1 << 41, cap * N, cap, 2), INV),
            ((ref.LLR_F32, 1, S, A, out_at(cap * S), 0, 0, cap, 1), OK),
            ((ref.REAL_F32, 2, S, A, out_at(cap * S - 1), 0, 0, cap, 1), INV)]
    got = ref.calls(build_dir, [s for s, _ in sets])
    assert got == [w for _, w in sets], [(i, g, w) for i, (g, (_, w)) in enumerate(zip(got, sets)) if g != w]


def test_create_refusals_without_a_device(hz):
    """a null context and null handles are refused (every other create refusal: test_restated_validation against the
    header the library itself compiles; tests/test_gpu_demap.py sends them through the library)"""
    lib = importlib.import_module("go-sdr_amd._capi").lib
    out = C.c_void_p()
    fp = C.POINTER(C.c_float)
    g = np.ones(1, np.float32)
    assert lib.hzsdr_demap_create(None, ref.LLR_F32, 1, None, 8, None, 8, None, g.ctypes.data_as(fp), 1, 1, C.byref(out)) == hz.ErrInvalidArgument.status
    inval = hz.ErrInvalidArgument.status
    assert lib.hzsdr_demap_run(None, g.ctypes.data, 8, None, 1, g.ctypes.data, 8) == inval
    assert lib.hzsdr_demap_sizes(None, None, None, None, None) == inval and lib.hzsdr_demap_plan(None, None, None, None, None) == inval
    assert lib.hzsdr_demap_free(None) == inval

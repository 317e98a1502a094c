"""The LDPC decoder bank (include/hzsdr_ldpc.h) without a GPU: the ABI's header, exports and bindings; the validation at
every bound's edge and one step outside, forged arrays included; the host program tests/host/ldpc_ref.cpp (the bytes the
device must produce) against the numpy restatement of tests/ldpc_ref.py -- whole-array steps -- for both inputs, both
normalisations and offsets, a head, D < n and frames of NaN, infinities, -0 and erasures; and anchors that do not lean
on either restatement: every frame marked ok is a codeword by a dense H x over GF(2), a clean codeword leaves with
iters = 0 and its own data, the Hamming (7, 4) matrix over all 2^7 hard inputs, the constructors against dense algebra,
and planted codewords under noise that the program recovers.  Nothing has a tolerance."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import ldpc_ref as ref
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "hzsdr_ldpc.h")
ENTRIES = {"hzsdr_ldpc_create", "hzsdr_ldpc_decode", "hzsdr_ldpc_sizes", "hzsdr_ldpc_plan", "hzsdr_ldpc_free"}
GCC = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include")]
PLANTED = dict(n=512, seed=1, sigma=0.7, scale=16.0, a=12, beta=0, frames=64, noise_seed=99)  # tests/test_gpu_ldpc.py plants the same


@pytest.fixture(scope="module")
def hz():
    return importlib.import_module("go-sdr_amd")


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("ldpc_ref"))


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


# ---- the ABI ---------------------------------------------------------------------------------------

def test_header_is_c99(tmp_path):
    src = tmp_path / "inc.c"
    src.write_text('#include "hzsdr_ldpc.h"\n'
                   "int main(void) { hzsdr_ldpc *l = 0; return (l != 0) + HZSDR_LDPC_MAX_ROWS - HZSDR_LDPC_MAX_CHECKS - HZSDR_LDPC_MAX_VARIABLES"
                   " - HZSDR_LDPC_MAX_EDGES - HZSDR_LDPC_MAX_DEGREE - HZSDR_LDPC_MAX_BITS - HZSDR_LDPC_MAX_ITERS - HZSDR_LDPC_MAX_FRAMES - HZSDR_LDPC_BITS"
                   " - HZSDR_LDPC_SOFT_F32 - HZSDR_LDPC_FORM_TABLES_LDS - HZSDR_LDPC_FORM_TABLES_CACHE + HZSDR_FRAMESYNC_MAX_PAYLOAD; }\n")
    subprocess.check_call(GCC + ["-c", str(src), "-o", str(tmp_path / "inc.o")])


def test_header_declares_exactly_the_entries():
    assert set(re.findall(r"\b(hzsdr_ldpc_[a-z0-9_]+)\s*\(", header_text())) == ENTRIES and len(ENTRIES) == 5


def test_library_exports_and_ctypes_table(hz):
    capi = importlib.import_module("go-sdr_amd._capi")
    for s in ENTRIES:
        assert hasattr(capi.lib, s), f"{s} declared in hzsdr_ldpc.h but not exported"
    assert set(capi.LDPC_SIGNATURES) == ENTRIES
    for name, (res, args) in capi.LDPC_SIGNATURES.items():
        fn = getattr(capi.lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    found = re.findall(r"\bint (hzsdr_ldpc_[a-z_]+)\s*\(([^)]*)\)", header_text())
    assert {name for name, _ in found} == ENTRIES
    kinds = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "unsigned": C.c_uint, "int": C.c_int, "size_t": C.c_size_t, "float": C.c_float}
    for name, params in found:
        args = capi.LDPC_SIGNATURES[name][1]
        decl = [" ".join(p.split()) for p in params.split(",")]
        assert len(args) == len(decl), name
        for a, d in zip(args, decl):  # argument for argument: a pointer for a pointer, the scalar types by width and sign
            if "*" in d:
                assert a is C.c_void_p or hasattr(a, "_type_") and not isinstance(a._type_, str), (name, d)
                if "size_t *" in d:
                    assert a._type_ is C.c_size_t, (name, d)
                if "const uint32_t *row_ptr" in d or "const uint32_t *col" in d:
                    assert a._type_ is C.c_uint32, (name, d)
            else:
                assert a is kinds[d.split()[0]], (name, d)


def test_constants_and_python_layers(hz):
    defs = dict(re.findall(r"#define (HZSDR_\w+) (\d+)", open(HEADER).read()))
    fs = dict(re.findall(r"#define (HZSDR_\w+) (\d+)", open(os.path.join(ROOT, "include", "hzsdr_framesync.h")).read()))
    assert int(defs["HZSDR_LDPC_MAX_ROWS"]) == hz.LDPC_MAX_ROWS == ref.MAX_ROWS == 8192
    assert int(defs["HZSDR_LDPC_MAX_CHECKS"]) == hz.LDPC_MAX_CHECKS == ref.MAX_CHECKS == 16384
    assert int(defs["HZSDR_LDPC_MAX_VARIABLES"]) == hz.LDPC_MAX_VARIABLES == ref.MAX_VARIABLES == 16384
    assert int(defs["HZSDR_LDPC_MAX_EDGES"]) == hz.LDPC_MAX_EDGES == ref.MAX_EDGES == 65536
    assert int(defs["HZSDR_LDPC_MAX_DEGREE"]) == hz.LDPC_MAX_DEGREE == ref.MAX_DEGREE == 64
    assert int(defs["HZSDR_LDPC_MAX_BITS"]) == hz.LDPC_MAX_BITS == ref.MAX_BITS == int(fs["HZSDR_FRAMESYNC_MAX_PAYLOAD"]) == 8192
    assert int(defs["HZSDR_LDPC_MAX_ITERS"]) == hz.LDPC_MAX_ITERS == ref.MAX_ITERS == 255
    assert int(defs["HZSDR_LDPC_MAX_FRAMES"]) == hz.LDPC_MAX_FRAMES == ref.MAX_FRAMES == 1 << 22
    assert int(defs["HZSDR_LDPC_BITS"]) == hz.LDPC_BITS == ref.BITS == 1
    assert int(defs["HZSDR_LDPC_SOFT_F32"]) == hz.LDPC_SOFT_F32 == ref.SOFT_F32 == hz.VITERBI_SOFT_F32 == 32
    assert int(defs["HZSDR_LDPC_FORM_TABLES_LDS"]) == hz.LDPC_FORM_TABLES_LDS == ref.FORM_TABLES_LDS == 1
    assert int(defs["HZSDR_LDPC_FORM_TABLES_CACHE"]) == hz.LDPC_FORM_TABLES_CACHE == ref.FORM_TABLES_CACHE == 2
    st = importlib.import_module("go-sdr_amd.stream")
    mod = importlib.import_module("go-sdr_amd.ldpc")
    assert hz.LdpcDecoder is mod.LdpcDecoder and hz.qc_code is mod.qc_code and hz.regular_code is mod.regular_code
    assert hz.ldpc_systematic is mod.ldpc_systematic and hz.ldpc_encode is mod.ldpc_encode and hz.LdpcCode is mod.LdpcCode
    assert callable(hz.Context.ldpc) and callable(st.ldpc_frames) and callable(st.decoded_frames) and callable(st.corrected_frames)
    for name in ("decode", "ragged", "sizes", "plan", "close", "__enter__", "__exit__"):
        assert callable(getattr(hz.LdpcDecoder, name)), name
    hpp = open(os.path.join(ROOT, "go-sdr_amd", "cxx", "hzsdr.hpp")).read()
    assert "class Ldpc" in hpp and '#include "../../include/hzsdr_ldpc.h"' in hpp
    make = open(os.path.join(ROOT, "go-sdr_amd", "csrc", "Makefile")).read()
    assert "hzsdr_ldpc.h" in make and "hz_ldpc" not in make.split("MFMA_UNITS =")[1].splitlines()[0]
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "hzsdr_ldpc.h" in open(os.path.join(ROOT, doc)).read(), doc
    header = open(HEADER).read()
    for left in ("layered schedules", "non-binary codes", "shortening by known", "rate matching", "outer BCH code", "soft outputs"):
        assert left in " ".join(header.replace(" * ", " ").split()), left


# ---- the validation --------------------------------------------------------------------------------

def small(hz):
    return hz.regular_code(24, 3, 6, seed=2)


def test_restated_validation(hz, build_dir):
    """Every bound accepted at its edge and refused one step outside, and forged arrays: csrc/hz_ldpc_plan.h against the
    rules restated in Python.  (The sanitizers watch the same refusals in tests/test_ldpc_plan.py.)"""
    code = small(hz)
    n, rp, col = code.n, code.row_ptr.astype(np.int64), code.col.astype(np.int64)
    sets = []

    def add(want, rp_=rp, col_=col, n_=n, m=None, E=None, **kw):
        q = ref.Config(n_, rp_, col_, **kw)
        assert ref.accepted(q) == want or m is not None or E is not None, (kw, want)
        sets.append(((q, m, E), want))

    add(True)
    for kw, want in ((dict(N=1), True), (dict(N=0), False), (dict(N=24), True), (dict(N=25), False), (dict(head=1), True), (dict(head=1, N=24), False),
                     (dict(head=23, N=1), True), (dict(head=24, N=1), False), (dict(D=1), True), (dict(D=0), False), (dict(D=24), True), (dict(D=25), False),
                     (dict(max_iters=1), True), (dict(max_iters=0), False), (dict(max_iters=255), True), (dict(max_iters=256), False),
                     (dict(a=1), True), (dict(a=0), False), (dict(a=16), True), (dict(a=17), False), (dict(beta=126), True), (dict(beta=127), False),
                     (dict(scale=1e-30), True), (dict(scale=0.0), False), (dict(scale=-1.0), False), (dict(scale=np.inf), False), (dict(scale=np.nan), False),
                     (dict(kind=ref.BITS, level=1), True), (dict(kind=ref.BITS, level=0), False), (dict(kind=ref.BITS, level=127), True),
                     (dict(kind=ref.BITS, level=128), False), (dict(kind=ref.BITS, scale=0.0), True), (dict(level=0), True), (dict(kind=2), False),
                     (dict(kind=0), False)):
        add(want, **kw)
    # forged row pointers
    for k, v in ((0, 1), (3, rp[2] - 1), (3, rp[2]), (3, rp[2] + 1), (5, 0xFFFFFFFF), (len(rp) - 1, len(col) + 1), (len(rp) - 1, len(col) - 1)):
        bad = rp.copy()
        bad[k] = v
        add(False, rp_=bad)
    add(False, rp_=rp[:-1])   # one check fewer than the edges need
    add(False, m=len(rp) - 2)  # the scalar disagrees with the array
    add(False, E=len(col) - 1)
    # forged columns
    for k, v in ((4, n), (4, 0xFFFFFFFF), (7, col[6]), (1, col[0] - 1 if col[0] else col[2])):
        bad = col.copy()
        bad[k] = v
        add(False, col_=bad)
    add(False, n_=n + 1)  # a variable of degree 0
    # degrees: checks of 2, 64 and 65; variables of 64 and 65
    two = np.array([[0, 1], [1, 2], [0, 2]])
    add(True, rp_=np.arange(4) * 2, col_=two.reshape(-1), n_=3)
    add(True, rp_=np.array([0, 64, 128]), col_=np.arange(128), n_=128)
    add(False, rp_=np.array([0, 65, 130]), col_=np.arange(130), n_=130)
    for deg, want in ((64, True), (65, False)):
        cols = np.array([[0, 1 + 2 * k, 2 + 2 * k] for k in range(deg)]).reshape(-1)
        add(want, rp_=np.arange(deg + 1) * 3, col_=cols, n_=2 * deg + 1)
    # the bounds of m, n and E
    big = hz.regular_code(16384, 4, 8, seed=3)
    add(True, rp_=big.row_ptr, col_=big.col, n_=16384, N=8192, head=8192)
    add(False, rp_=big.row_ptr, col_=big.col, n_=16384, N=8193, head=0)
    add(True, rp_=np.arange(16385) * 2, col_=np.stack([np.arange(16384) % 8192, 8192 + np.arange(16384) % 8192], 1).reshape(-1), n_=16384, N=100)
    add(False, rp_=np.arange(16386) * 2, col_=np.stack([np.arange(16385) % 8192, 8192 + np.arange(16385) % 8192], 1).reshape(-1), n_=16384, N=100)
    add(False, rp_=np.arange(13109) * 5, col_=(np.arange(13108)[:, None] + np.arange(5)[None] * 3000).reshape(-1) % 16385, n_=16385, N=100)
    c5 = np.sort((np.arange(13108)[:, None] * 5 + np.arange(5)[None] * 3277) % 16384, axis=1)
    add(False, rp_=np.arange(13109) * 5, col_=c5.reshape(-1), n_=16384, N=100)  # E = 65540
    got = ref.check(build_dir, [s for s, _ in sets])
    for ((q, m, E), want), ok in zip(sets, got):
        assert ok == want, (q.n, q.m, q.E, m, E, q.N, q.head, q.D, q.kind, q.scale, q.level, q.max_iters, q.a, q.beta)
    assert sum(got) > 15 and sum(not g for g in got) > 30


# ---- the program against the restatement -----------------------------------------------------------------

def noisy(hz, code, F, sigma, seed):
    """(soft frames (F, n), data bits (F, k)) of planted codewords under noise"""
    data = np.stack([ref.random_bits(code.k, seed * 1000 + f) for f in range(F)])
    return ref.bpsk(hz.ldpc_encode(code, data), sigma, seed), data


CASES = [dict(a=16, beta=0), dict(a=12, beta=0), dict(a=16, beta=1), dict(a=12, beta=1), dict(a=9, beta=3), dict(a=1, beta=0)]


@pytest.mark.parametrize("k", range(len(CASES)))
@pytest.mark.parametrize("kind", [ref.BITS, ref.SOFT_F32])
def test_program_against_whole_array_steps(hz, build_dir, k, kind):
    """noisy planted codewords at a noise where some frames converge, some take many iterations and some never do:
    bytes and info equal; a head in front, a punctured tail behind, D < n, counts that leave slots out"""
    code, _ = hz.ldpc_systematic(hz.regular_code(96, 3, 6, seed=10 + k))
    x, _ = noisy(hz, code, 6, 0.85, 40 + k)
    head, N = (5, 80) if k % 2 else (0, 96)
    q = ref.Config.of(code, kind=kind, head=head, N=N, D=(code.k, 33, 96)[k % 3], scale=11.0, level=(1, 9, 127)[k % 3], max_iters=(30, 3)[k // 3 % 2], **CASES[k])
    vals = x[:, head:head + N]
    frames = (ref.hard_frames(vals) if kind == ref.BITS else vals).reshape(3, 2, -1)
    counts = np.array([2, 0, 5], np.uint32)
    ((data, info),) = ref.exact(build_dir, [(q, frames, counts)])
    assert not data[1].any() and not info[1].any()
    for r in (0, 2):
        for f in range(2):
            wd, wi, _ = ref.decode(q, frames[r, f])
            assert np.array_equal(data[r, f], wd) and int(info[r, f]) == wi, (vars(q), r, f)
    u, it, ok = ref.split(info[[0, 2]])
    assert ((u == 0) == (ok == 1)).all() and (it <= q.max_iters).all()


def test_special_values_and_erasures(hz, build_dir):
    """frames of NaN, +-infinity, -0 and zeros: an all-erasure frame has no odd check and leaves with iters = 0 and all
    bits 0; all +infinity is the all-ones word, a codeword of a code whose checks all have even degree; the quantiser's
    edges; NaNs and infinities inside a noisy frame: the program and numpy agree"""
    code, _ = hz.ldpc_systematic(hz.regular_code(96, 3, 6, seed=4))
    q = ref.Config.of(code, scale=1.0, max_iters=25, a=12)
    frames = np.zeros((1, 6, 96), np.float32)
    frames[0, 1], frames[0, 2], frames[0, 3], frames[0, 4] = np.nan, -0.0, np.inf, -np.inf
    frames[0, 5] = ref.bpsk(hz.ldpc_encode(code, ref.random_bits(code.k, 5)), 0.8, 6) * 20
    frames[0, 5, [3, 17, 40, 41]] = np.nan, -0.0, np.inf, -np.inf
    ((data, info),) = ref.exact(build_dir, [(q, frames, None)])
    for f in (0, 1, 2, 4):
        assert not data[0, f].any() and int(info[0, f]) == 1 << 31, f
    assert (data[0, 3] == 0xFF).all() and int(info[0, 3]) == 1 << 31
    for f in range(6):
        wd, wi, _ = ref.decode(q, frames[0, f])
        assert np.array_equal(data[0, f], wd) and int(info[0, f]) == wi, f
    assert ref.quantise(np.array([np.inf, -np.inf, np.nan, -0.0, 0.5, 1.5, 2.5, -0.5, -1.5, 126.6, 1e30], np.float32), 1.0).tolist() == \
        [127, -127, 0, 0, 0, 2, 2, 0, -2, 127, 127]


# ---- independent anchors ---------------------------------------------------------------------------------

def test_ok_frames_are_codewords_and_clean_ones_leave_at_once(hz, build_dir):
    """D = n: every frame the program marks ok satisfies a dense H x = 0 over GF(2) and every other one does not, with u
    its number of odd checks; a clean codeword, soft or hard, leaves with iters = 0 and its own bits"""
    code, _ = hz.ldpc_systematic(hz.regular_code(192, 3, 6, seed=8))
    H = code.dense().astype(np.int64)
    x, data = noisy(hz, code, 40, 0.85, 3)
    q = ref.Config.of(code, scale=10.0, max_iters=12, a=12)
    ((out, info),) = ref.exact(build_dir, [(q, x[None], None)])
    u, it, ok = ref.split(info[0])
    for f in range(40):
        word = np.unpackbits(out[0, f])[:code.n].astype(np.int64)
        odd = int(((H @ word) & 1).sum())
        assert odd == u[f] and (odd == 0) == bool(ok[f]), f
    assert 5 < ok.sum() < 40 and it.max() == 12 and it.min() >= 1
    cw = hz.ldpc_encode(code, data)
    assert not ((cw.astype(np.int64) @ H.T) & 1).any()
    clean = (cw.astype(np.float32) * 2 - 1) * np.float32(0.3)
    qh = ref.Config.of(code, kind=ref.BITS, level=5, max_iters=12)
    (so, si), (ho, hi) = ref.exact(build_dir, [(q, clean[None], None), (qh, np.packbits(cw, axis=1)[None], None)])
    for f in range(40):
        assert np.array_equal(so[0, f], np.packbits(cw[f])) and np.array_equal(ho[0, f], np.packbits(cw[f])), f
    assert (si == 1 << 31).all() and (hi == 1 << 31).all()


def test_hamming_7_4_over_every_hard_input(build_dir):
    """all 2^7 hard inputs under the (7, 4) matrix: every frame marked ok is one of the 16 codewords, and each of the 16
    comes back unchanged with iters = 0"""
    H = ref.HAMMING74.astype(np.int64)
    q = ref.Config(*ref.dense_code(H), kind=ref.BITS, level=4, max_iters=10, a=16)
    words = ((np.arange(128)[:, None] >> np.arange(6, -1, -1)) & 1).astype(np.uint8)
    is_cw = ~((words.astype(np.int64) @ H.T) & 1).any(axis=1)
    assert is_cw.sum() == 16
    ((out, info),) = ref.exact(build_dir, [(q, np.packbits(words, axis=1)[None], None)])
    u, it, ok = ref.split(info[0])
    got = np.unpackbits(out[0], axis=1)[:, :7]
    for w in range(128):
        if ok[w]:
            assert not ((got[w].astype(np.int64) @ H.T) & 1).any(), w
        if is_cw[w]:
            assert ok[w] and it[w] == 0 and np.array_equal(got[w], words[w]), w
        else:
            assert it[w] >= 1, w
        wd, wi, _ = ref.decode(q, np.packbits(words[w]))
        assert np.array_equal(out[0, w], wd) and int(info[0, w]) == wi, w
    assert ok.sum() > 16  # some single errors are corrected


def test_planted_codewords_come_back(hz, build_dir):
    """the (3, 6) code of n = 512 that regular_code makes, a = 12, beta = 0, scale 16, BPSK at sigma = 0.7: the program
    recovers all 64 planted codewords (tests/test_gpu_ldpc.py holds the device to the same bytes); n = 96 at sigma = 0.6
    recovers 100 of 100"""
    p = PLANTED
    for n, sigma, F in ((p["n"], p["sigma"], p["frames"]), (96, 0.6, 100)):
        code, _ = hz.ldpc_systematic(hz.regular_code(n, 3, 6, seed=p["seed"]))
        data = np.stack([ref.random_bits(code.k, 7 + i) for i in range(F)])
        x = ref.bpsk(hz.ldpc_encode(code, data), sigma, p["noise_seed"])
        q = ref.Config.of(code, D=code.k, scale=p["scale"], max_iters=50, a=p["a"], beta=p["beta"])
        ((out, info),) = ref.exact(build_dir, [(q, x[None], None)])
        u, it, ok = ref.split(info[0])
        assert ok.all() and np.array_equal(out[0], np.packbits(data, axis=1)) and it.max() > 2, n
        hard = np.unpackbits(ref.hard_frames(x), axis=1)[:, :code.k]
        assert (hard != data).any(axis=1).sum() > F // 2  # (most frames arrive with errors in their data bits)


# ---- the constructors ------------------------------------------------------------------------------------

def test_systematic_and_encode(hz):
    """ldpc_systematic then ldpc_encode give H x = 0 with the data in front -- under the ORIGINAL matrix too, through
    the permutation -- for a full-rank code, a regular code, one whose variables all have even degree (rank-deficient:
    its checks sum to zero) and a matrix with repeated rows"""
    rng = np.random.default_rng(5)
    Hfull = np.concatenate([(rng.random((10, 20)) < 0.3).astype(np.uint8), np.eye(10, dtype=np.uint8)], axis=1)
    Hfull[:, :2] = 1  # (no empty row or column)
    Hrep = np.concatenate([Hfull[:6], Hfull[:3], Hfull[6:]])
    for code in (hz.LdpcCode.from_dense(Hfull), hz.regular_code(96, 3, 6, seed=1), hz.regular_code(96, 4, 8, seed=1), hz.LdpcCode.from_dense(Hrep), hz.LdpcCode.from_dense(ref.HAMMING74)):
        H = code.dense().astype(np.int64)
        sys_code, perm = hz.ldpc_systematic(code)
        assert sorted(perm.tolist()) == list(range(code.n)) and sys_code.m == code.m and sys_code.E == code.E
        assert np.array_equal(sys_code.dense(), code.dense()[:, perm])
        k = sys_code.k
        assert k >= code.n - code.m and k == code.n - gf2_rank(H)
        data = (rng.random((9, k)) < 0.5).astype(np.uint8)
        x = hz.ldpc_encode(sys_code, data)
        assert x.shape == (9, code.n) and np.array_equal(x[:, :k], data)
        assert not ((x.astype(np.int64) @ sys_code.dense().astype(np.int64).T) & 1).any()
        assert not sys_code.syndrome(x).any()
        back = np.zeros_like(x)
        back[:, perm] = x
        assert not ((back.astype(np.int64) @ H.T) & 1).any()
    assert hz.ldpc_systematic(hz.regular_code(96, 4, 8, seed=1))[0].k > 48  # rank-deficient: more free variables than n - m
    assert hz.ldpc_systematic(hz.LdpcCode.from_dense(Hrep))[0].k == 20
    with pytest.raises(ValueError):
        hz.ldpc_encode(hz.regular_code(96, 3, 6), np.zeros(48, np.uint8))


def gf2_rank(H):
    A = (np.asarray(H) & 1).astype(np.uint8).copy()
    r = 0
    for c in range(A.shape[1]):
        hit = np.nonzero(A[r:, c])[0]
        if not len(hit):
            continue
        A[[r, r + hit[0]]] = A[[r + hit[0], r]]
        for i in np.nonzero(A[:, c])[0]:
            if i != r:
                A[i] ^= A[r]
        r += 1
        if r == A.shape[0]:
            break
    return r


def test_qc_code_against_a_dense_expansion(hz):
    """the base table written out block by block: shift s is the identity with row i's one in column (i + s) mod Z"""
    shifts = [[0, -1, 3, 1, 0, -1], [2, 4, -1, 0, 0, 0], [-1, 1, 2, -1, 4, 0]]
    Z = 5
    H = np.zeros((3 * Z, 6 * Z), np.uint8)
    for bi, row in enumerate(shifts):
        for bj, s in enumerate(row):
            for i in range(Z):
                if s >= 0:
                    H[bi * Z + i, bj * Z + (i + s) % Z] = 1
    code = hz.qc_code(shifts, Z)
    assert (code.n, code.m, code.E) == (30, 15, int(H.sum())) and np.array_equal(code.dense(), H)
    assert all(np.all(np.diff(code.col[a:b].astype(np.int64)) > 0) for a, b in zip(code.row_ptr[:-1], code.row_ptr[1:]))
    assert ref.accepted(ref.Config.of(code))
    assert np.array_equal(hz.qc_code([[0, 0]], 1).dense(), [[1, 1]]) and np.array_equal(hz.qc_code([[1]], 3).dense(), np.roll(np.eye(3, dtype=np.uint8), 1, axis=1))
    with pytest.raises(ValueError):
        hz.qc_code([[0, -2]], 4)


def test_regular_code_is_regular_and_reproducible(hz):
    for n, dv, dc in ((96, 3, 6), (512, 3, 6), (128, 2, 4), (256, 8, 16), (2048, 3, 6)):
        code = hz.regular_code(n, dv, dc, seed=7)
        H = code.dense()
        assert H.shape == (n * dv // dc, n) and (H.sum(axis=1) == dc).all() and (H.sum(axis=0) == dv).all() and code.E == n * dv
        assert ref.accepted(ref.Config.of(code, N=min(n, 8192)))
        again = hz.regular_code(n, dv, dc, seed=7)
        assert np.array_equal(again.col, code.col) and not np.array_equal(hz.regular_code(n, dv, dc, seed=8).col, code.col)
    with pytest.raises(ValueError):
        hz.regular_code(100, 3, 7)

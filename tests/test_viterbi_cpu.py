"""The Viterbi decoder bank (include/hzsdr_viterbi.h) without a GPU: the ABI's header, exports and bindings; the
validation at every bound's edge and one step outside; the host program tests/host/viterbi_ref.cpp (the bytes the device
must produce) against the numpy restatement of tests/viterbi_ref.py -- whole-array add-compare-select -- and against its
exhaustive decoder for D <= 12, which scores all 2^D data words by the metric's definition alone; the encoder; error
correction that the code's free distance proves; the CRC register against known answers.  Nothing has a tolerance."""
import binascii
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import viterbi_ref as ref
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "hzsdr_viterbi.h")
ENTRIES = {"hzsdr_viterbi_create", "hzsdr_viterbi_decode", "hzsdr_viterbi_sizes", "hzsdr_viterbi_plan", "hzsdr_viterbi_free"}
GCC = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include")]
CCITT = (16, 0x1021, 0xFFFF, 0)


@pytest.fixture(scope="module")
def hz():
    return importlib.import_module("go-sdr_amd")


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("viterbi_ref"))


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


# ---- the ABI ---------------------------------------------------------------------------------------

def test_header_is_c99(tmp_path):
    src = tmp_path / "inc.c"
    src.write_text('#include "hzsdr_viterbi.h"\n'
                   "int main(void) { hzsdr_viterbi *v = 0; return (v != 0) + HZSDR_VITERBI_MAX_ROWS - HZSDR_VITERBI_MAX_K - HZSDR_VITERBI_MIN_K"
                   " - HZSDR_VITERBI_MAX_RATE - HZSDR_VITERBI_MAX_PATTERN - HZSDR_VITERBI_MAX_BITS - HZSDR_VITERBI_MAX_FRAMES - HZSDR_VITERBI_BITS"
                   " - HZSDR_VITERBI_SOFT_F32 - HZSDR_VITERBI_TAIL - HZSDR_VITERBI_TRUNCATED - HZSDR_VITERBI_FORM_LDS - HZSDR_VITERBI_FORM_SCRATCH"
                   " + HZSDR_FRAMESYNC_MAX_PAYLOAD; }\n")
    subprocess.check_call(GCC + ["-c", str(src), "-o", str(tmp_path / "inc.o")])


def test_header_declares_exactly_the_entries():
    assert set(re.findall(r"\b(hzsdr_viterbi_[a-z0-9_]+)\s*\(", header_text())) == ENTRIES and len(ENTRIES) == 5


def test_library_exports_and_ctypes_table(hz):
    capi = importlib.import_module("go-sdr_amd._capi")
    for s in ENTRIES:
        assert hasattr(capi.lib, s), f"{s} declared in hzsdr_viterbi.h but not exported"
    assert set(capi.VITERBI_SIGNATURES) == ENTRIES
    for name, (res, args) in capi.VITERBI_SIGNATURES.items():
        fn = getattr(capi.lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    found = re.findall(r"\bint (hzsdr_viterbi_[a-z_]+)\s*\(([^)]*)\)", header_text())
    assert {name for name, _ in found} == ENTRIES
    kinds = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "unsigned": C.c_uint, "int": C.c_int, "size_t": C.c_size_t, "float": C.c_float}
    for name, params in found:
        args = capi.VITERBI_SIGNATURES[name][1]
        decl = [" ".join(p.split()) for p in params.split(",")]
        assert len(args) == len(decl), name
        for a, d in zip(args, decl):  # argument for argument: a pointer for a pointer, the scalar types by width and sign
            if "*" in d:
                assert a is C.c_void_p or hasattr(a, "_type_") and not isinstance(a._type_, str), (name, d)
                if "size_t *" in d:
                    assert a._type_ is C.c_size_t, (name, d)
            else:
                assert a is kinds[d.split()[0]], (name, d)


def test_constants_and_python_layers(hz):
    defs = dict(re.findall(r"#define (HZSDR_\w+) (\d+)", open(HEADER).read()))
    fs = dict(re.findall(r"#define (HZSDR_\w+) (\d+)", open(os.path.join(ROOT, "include", "hzsdr_framesync.h")).read()))
    assert int(defs["HZSDR_VITERBI_MAX_ROWS"]) == hz.VITERBI_MAX_ROWS == ref.MAX_ROWS == 8192
    assert int(defs["HZSDR_VITERBI_MIN_K"]) == hz.VITERBI_MIN_K == ref.MIN_K == 3
    assert int(defs["HZSDR_VITERBI_MAX_K"]) == hz.VITERBI_MAX_K == ref.MAX_K == 9
    assert int(defs["HZSDR_VITERBI_MAX_RATE"]) == hz.VITERBI_MAX_RATE == ref.MAX_RATE == 4
    assert int(defs["HZSDR_VITERBI_MAX_PATTERN"]) == hz.VITERBI_MAX_PATTERN == ref.MAX_PATTERN == 64
    assert int(defs["HZSDR_VITERBI_MAX_BITS"]) == hz.VITERBI_MAX_BITS == ref.MAX_BITS == int(fs["HZSDR_FRAMESYNC_MAX_PAYLOAD"]) == 8192
    assert int(defs["HZSDR_VITERBI_MAX_FRAMES"]) == hz.VITERBI_MAX_FRAMES == ref.MAX_FRAMES == 1 << 22
    assert int(defs["HZSDR_VITERBI_BITS"]) == hz.VITERBI_BITS == ref.BITS == 1
    assert int(defs["HZSDR_VITERBI_SOFT_F32"]) == hz.VITERBI_SOFT_F32 == ref.SOFT_F32 == 32
    assert int(defs["HZSDR_VITERBI_TAIL"]) == hz.VITERBI_TAIL == ref.TAIL == 0
    assert int(defs["HZSDR_VITERBI_TRUNCATED"]) == hz.VITERBI_TRUNCATED == ref.TRUNCATED == 1
    assert int(defs["HZSDR_VITERBI_FORM_LDS"]) == hz.VITERBI_FORM_LDS == ref.FORM_LDS == 1
    assert int(defs["HZSDR_VITERBI_FORM_SCRATCH"]) == hz.VITERBI_FORM_SCRATCH == ref.FORM_SCRATCH == 2
    st = importlib.import_module("go-sdr_amd.stream")
    mod = importlib.import_module("go-sdr_amd.viterbi")
    assert hz.ViterbiDecoder is mod.ViterbiDecoder and hz.conv_encode is mod.conv_encode and hz.puncture_pattern is mod.puncture_pattern
    assert hz.crc_register is mod.crc_register and hz.CCSDS_K7 == (7, (0o171, 0o133), 0b10)
    assert callable(hz.Context.viterbi) and callable(st.decoded_frames)
    for name in ("decode", "ragged", "sizes", "plan", "close", "__enter__", "__exit__"):
        assert callable(getattr(hz.ViterbiDecoder, name)), name
    hpp = open(os.path.join(ROOT, "go-sdr_amd", "cxx", "hzsdr.hpp")).read()
    assert "class Viterbi" in hpp and '#include "../../include/hzsdr_viterbi.h"' in hpp
    make = open(os.path.join(ROOT, "go-sdr_amd", "csrc", "Makefile")).read()
    assert "hzsdr_viterbi.h" in make and "hz_viterbi" not in make.split("MFMA_UNITS =")[1].splitlines()[0]
    # the sentences that left decoding and CRCs to others point to the bank
    for path in (os.path.join(ROOT, "include", "hzsdr_framesync.h"), os.path.join(ROOT, "go-sdr_amd", "framesync.py")):
        assert "hzsdr_viterbi.h" in open(path).read(), path
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "hzsdr_viterbi.h" in open(os.path.join(ROOT, doc)).read(), doc
    for name in ("tail-biting", "soft outputs", "Go binding"):
        assert name in open(os.path.join(ROOT, "DESIGN.md")).read(), name


def test_patterns_and_the_encoder(hz):
    for rate, (pat, bits) in ref.PATTERNS.items():
        assert hz.puncture_pattern(rate) == (pat, bits), rate
        num, den = (int(v) for v in rate.split("/"))
        assert bits == 2 * num and bin(pat).count("1") == den  # num input bits give den transmitted ones
    with pytest.raises(ValueError):
        hz.puncture_pattern("4/5")
    K, gens, inv = hz.CCSDS_K7
    for q in (ref.Config(D=40, inv=inv), ref.Config(D=41, pattern=ref.PATTERNS["3/4"], term=ref.TRUNCATED), ref.Config(K=9, gens=(0o557, 0o663, 0o711), D=33),
              ref.Config(K=3, gens=(5, 7), D=9, pattern=ref.PATTERN64), ref.Config(K=5, gens=(0o23, 0o35, 0o27, 0o33), D=17, inv=0b1010)):
        bits = ref.random_bits(q.D, q.K * 7 + q.D)
        got = hz.conv_encode(bits, q.K, q.gens, q.inv, (q.pattern, q.Lp), q.term)
        assert got.dtype == np.uint8 and len(got) == q.N and np.array_equal(got, ref.encode(q, bits)), vars(q)
    # the impulse response of the K = 7 code is its generators, bit by bit, the second inverted for CCSDS
    one = hz.conv_encode([1], K, gens, inv, None, hz.VITERBI_TAIL).reshape(7, 2)
    assert int("".join(map(str, one[:, 0])), 2) == 0o171 and int("".join(map(str, one[:, 1] ^ 1)), 2) == 0o133
    assert np.array_equal(hz.conv_encode(bits, K, gens, 0, "3/4"), hz.conv_encode(bits, K, gens, 0, ref.PATTERNS["3/4"]))


def test_crc_register_known_answers(hz):
    msg = b"123456789"
    bits = np.unpackbits(np.frombuffer(msg, np.uint8))
    assert hz.crc_register(bits, 16, 0x1021, 0xFFFF, 0) == binascii.crc_hqx(msg, 0xFFFF) == 0x29B1
    assert hz.crc_register(bits, 32, 0x04C11DB7, 0xFFFFFFFF, 0) == 0x0376E6E7  # CRC-32/MPEG-2
    assert hz.crc_register(bits, 8, 0x07) == 0xF4 and hz.crc_register(bits, 24, 0x864CFB, 0xB704CE, 0) == 0x21CF02  # CRC-8, CRC-24/OPENPGP
    for seed in range(4):
        data = bytes(ref.splitmix64(seed, 40).astype(np.uint8))
        b = np.unpackbits(np.frombuffer(data, np.uint8))
        assert hz.crc_register(b, 16, 0x1021, 0xFFFF, 0) == binascii.crc_hqx(data, 0xFFFF)
        q = ref.Config(D=len(b) + 16, crc=CCITT)
        assert ref.crc_ok(q, ref.with_crc(q, b)) == 1 and ref.crc_ok(q, ref.with_crc(q, b) ^ np.eye(1, q.D, 5, dtype=np.uint8)[0]) == 0


# ---- the validation --------------------------------------------------------------------------------

def cfg(**kw):
    return ref.Config(**kw)


P34 = ref.PATTERNS["3/4"]
EDGES = [
    (cfg(), True),
    (cfg(K=3, gens=(5, 7)), True), (cfg(K=2, gens=(1, 3)), False), (cfg(K=9, gens=(0o561, 0o753)), True), (cfg(K=10, gens=(0o561, 0o753)), False),
    (cfg(gens=(0o171,)), False), (cfg(gens=(0o171, 0o133, 0o165)), True), (cfg(gens=(0o171, 0o133, 0o165, 0o117)), True),
    (cfg(gens=(0o171, 0o133, 0o165, 0o117, 0o155)), False),
    (cfg(gens=(0, 0o133)), False), (cfg(gens=(1, 0o133)), True), (cfg(gens=(0o177, 0o133)), True), (cfg(gens=(0o200, 0o133)), False),
    (cfg(inv=0b11), True), (cfg(inv=0b100), False), (cfg(gens=(0o171, 0o133, 0o165), inv=0b100), True),
    (cfg(pattern=(0b11, 2)), True), (cfg(pattern=(0b1, 1)), False), (cfg(pattern=(0b111, 3)), False), (cfg(pattern=(0b10, 2)), True),
    (cfg(pattern=(0b1100, 4)), False), (cfg(pattern=(0b1001, 4)), True), (cfg(pattern=(0b10000, 4)), False),
    (cfg(pattern=ref.PATTERN64), True), (cfg(pattern=(2 ** 64 - 1, 64)), True), (cfg(pattern=(2 ** 66 - 1, 66)), False),
    (cfg(gens=(0o171, 0o133, 0o165), pattern=(2 ** 63 - 1, 63)), True), (cfg(gens=(0o171, 0o133, 0o165), pattern=(2 ** 64 - 1, 64)), False),
    (cfg(gens=(0o171, 0o133, 0o165), pattern=(0b100011, 6)), True), (cfg(gens=(0o171, 0o133, 0o165), pattern=(0b111000, 6)), False),
    (cfg(term=ref.TRUNCATED), True), (cfg(term=2), False),
    (cfg(D=1), True), (cfg(D=0), False), (cfg(D=4090), True), (cfg(D=4091), False),  # N = 2 T = 8192, 8194
    (cfg(D=8186, pattern=(0b10, 2)), True), (cfg(D=8187, pattern=(0b10, 2)), False),  # T = 8192, 8193
    (cfg(D=8192, term=ref.TRUNCATED, pattern=(0b10, 2)), True), (cfg(D=8193, term=ref.TRUNCATED, pattern=(0b10, 2)), False),
    (cfg(D=6138, pattern=P34), True), (cfg(D=6139, pattern=P34), False),  # N = 8192, 8194 of T = 6144, 6145
    (cfg(kind=ref.SOFT_F32, scale=1e-30), True), (cfg(kind=ref.SOFT_F32, scale=0.0), False), (cfg(kind=ref.SOFT_F32, scale=-1.0), False),
    (cfg(kind=ref.SOFT_F32, scale=np.inf), False), (cfg(kind=ref.SOFT_F32, scale=np.nan), False), (cfg(kind=ref.SOFT_F32, scale=3.4028234e38), True),
    (cfg(kind=2), False), (cfg(kind=0), False),
    (cfg(crc=CCITT), True), (cfg(crc=(12, 0x80F, 0, 0)), False), (cfg(crc=(40, 1, 0, 0)), False), (cfg(D=16, crc=CCITT), False), (cfg(D=17, crc=CCITT), True),
    (cfg(crc=(8, 0xFF, 0xFF, 0xFF)), True), (cfg(crc=(8, 0x100, 0, 0)), False), (cfg(crc=(8, 7, 0x100, 0)), False), (cfg(crc=(8, 7, 0, 0x100)), False),
    (cfg(crc=(24, 0xFFFFFF, 0, 0)), True), (cfg(crc=(24, 0x1000000, 0, 0)), False), (cfg(crc=(32, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)), True),
    (cfg(D=32, crc=(32, 0x04C11DB7, 0, 0)), False), (cfg(D=33, crc=(32, 0x04C11DB7, 0, 0)), True), (cfg(crc=(0, 1, 0, 0)), False),
]


def test_restated_validation(build_dir):
    """Every bound accepted at its edge and refused one step outside: csrc/hz_viterbi_plan.h against the rules restated in
    Python, and the sizes N and T it derives.  (Rows and cap are refused by the entries themselves: tests/test_gpu_viterbi.py.)"""
    got = ref.check(build_dir, [q for q, _ in EDGES])
    for (q, want), (ok, N, T) in zip(EDGES, got):
        assert ref.accepted(q) == want, vars(q)
        assert ok == want, vars(q)
        if ok:
            assert (N, T) == (q.N, q.T), vars(q)
    assert sum(g[0] for g in got) > 20 and sum(not g[0] for g in got) > 20


# ---- the program against the restatements ------------------------------------------------------------------

CODES = [
    dict(K=7, gens=ref.K7, inv=0b10), dict(K=3, gens=(5, 7)), dict(K=4, gens=(0o15, 0o17, 0o13)), dict(K=5, gens=(0o23, 0o35)),
    dict(K=6, gens=(0o53, 0o75)), dict(K=8, gens=(0o247, 0o371)), dict(K=9, gens=(0o557, 0o663, 0o711)), dict(K=9, gens=(0o463, 0o535, 0o733, 0o745), inv=0b0101),
    dict(K=7, gens=ref.K7, pattern=ref.PATTERNS["2/3"]), dict(K=7, gens=ref.K7, pattern=ref.PATTERNS["7/8"]), dict(K=5, gens=(0o23, 0o35), pattern=ref.PATTERN64),
    dict(K=7, gens=(0o171, 0o133, 0o165), pattern=(0b110101, 6)),
]


def noisy_block(q, R, cap, seed, flips):
    """a clean block whose frames get `flips` random positions hurt each: hard bits inverted, soft values turned into a
    weak value of the wrong sign -- so that the decoders have competing paths to choose between"""
    frames, data = ref.clean_block(q, R, cap, seed)
    for r in range(R):
        for f in range(cap):
            where = (ref.splitmix64(seed * 977 + r * cap + f, flips) % np.uint64(q.N)).astype(int)
            if q.kind == ref.BITS:
                bits = np.unpackbits(frames[r, f])
                bits[where] ^= 1
                frames[r, f] = np.packbits(bits)
            else:
                frames[r, f, where] *= np.float32(-0.4)
    return frames, data


@pytest.mark.parametrize("k", range(len(CODES)))
@pytest.mark.parametrize("kind", [ref.BITS, ref.SOFT_F32])
def test_program_against_whole_array_acs(build_dir, k, kind):
    """random frames with so many errors that decisions, ties and the CRC verdict all vary: bytes and info equal, for
    both terminations, with counts that leave slots out"""
    for term, D in ((ref.TAIL, 45), (ref.TRUNCATED, 67)):
        q = cfg(D=D, term=term, kind=kind, scale=0.5, crc=CCITT if k % 2 else None, **CODES[k])
        frames, _ = noisy_block(q, 3, 2, 40 * k + term, flips=max(2, q.N // 9))
        counts = np.array([2, 0, 5], np.uint32)
        ((data, info),) = ref.exact(build_dir, [(q, frames, counts)])
        assert not data[1].any() and not info[1].any()
        for r in (0, 2):
            for f in range(2):
                wd, wi = ref.decode(q, frames[r, f])
                assert np.array_equal(data[r, f], wd) and int(info[r, f]) == wi, (vars(q), r, f)
        assert len({int(v) & 0x7FFFFFFF for v in info[[0, 2]].reshape(-1)}) > 1


@pytest.mark.parametrize("kind", [ref.BITS, ref.SOFT_F32])
def test_program_against_the_exhaustive_decoder(build_dir, kind):
    """D <= 12, TAIL: the metric always equals the minimum over all 2^D data words, and the bits equal the argmin
    wherever it is unique; ties are met (hard bits make many) and at least as many unique minima"""
    unique = tied = 0
    cases = []
    for k, code in enumerate(CODES):
        for D in (1, 2, 5, 8, 12):
            q = cfg(D=D, kind=kind, scale=0.25, **code)
            frames, _ = noisy_block(q, 1, 3, 900 + 13 * k + D, flips=max(1, q.N // 5))
            cases.append((q, frames, None))
    for (q, frames, _), (data, info) in zip(cases, ref.exact(build_dir, cases)):
        for f in range(3):
            best, words = ref.exhaustive(q, frames[0, f])
            assert int(info[0, f]) == best, (vars(q), f)
            got = np.unpackbits(data[0, f])[:q.D]
            assert any(np.array_equal(got, w) for w in words), (vars(q), f)
            unique += len(words) == 1
            tied += len(words) > 1
    assert unique > 50 and (tied > 10 or kind == ref.SOFT_F32)


@pytest.mark.parametrize("kind", [ref.BITS, ref.SOFT_F32])
def test_encode_then_decode_is_the_data_with_metric_zero(build_dir, hz, kind):
    cases, sent = [], []
    for k, code in enumerate(CODES):
        for term in (ref.TAIL, ref.TRUNCATED):
            q = cfg(D=100 + k, term=term, kind=kind, scale=2.0, crc=(32, 0x04C11DB7, 0xFFFFFFFF, 0), **code)
            data = ref.with_crc(q, ref.random_bits(q.D - 32, k))
            code_bits = hz.conv_encode(data, q.K, q.gens, q.inv, (q.pattern, q.Lp), q.term)
            cases.append((q, ref.frame_of(q, code_bits, k)[None, None], None))
            sent.append(data)
    for (q, _, _), want, (data, info) in zip(cases, sent, ref.exact(build_dir, cases)):
        if q.term == ref.TRUNCATED and q.Lp > q.n:
            # a truncated, punctured frame's last bits may be undetermined: the metric is 0 all the same
            assert int(info[0, 0]) & 0x7FFFFFFF == 0, vars(q)
            continue
        assert np.array_equal(data[0, 0], np.packbits(want)) and int(info[0, 0]) == 1 << 31, vars(q)


def test_provable_error_correction(build_dir):
    """K = 7 (0o171, 0o133) has free distance 10: with TAIL and any <= 4 flipped hard bits the sent word is strictly
    nearest, so the decoded bits are the sent ones and the metric is the number of flips -- random flip sets of 0 ... 4"""
    q = cfg(D=78, inv=0b10, crc=CCITT)
    R, cap = 10, 4
    frames, data = ref.clean_block(q, R, cap, 5)
    flips = np.zeros((R, cap), int)
    for r in range(R):
        for f in range(cap):
            flips[r, f] = (r * cap + f) % 5
            where = np.unique((ref.splitmix64(r * 64 + f, 16) % np.uint64(q.N)).astype(int))[:flips[r, f]]
            assert len(where) == flips[r, f]
            bits = np.unpackbits(frames[r, f])
            bits[where] ^= 1
            frames[r, f] = np.packbits(bits)
    ((got, info),) = ref.exact(build_dir, [(q, frames, None)])
    for r in range(R):
        for f in range(cap):
            assert np.array_equal(got[r, f], np.packbits(data[r, f])), (r, f)
            assert int(info[r, f]) == flips[r, f] | (1 << 31), (r, f)


def test_ties_erasures_and_special_values(build_dir):
    """an all-erasure frame decodes to the tie rule's answer: every decision 0, so TAIL walks back along zeros and
    TRUNCATED takes state 0 -- all data bits 0 with metric 0; -0 is an erasure, infinities saturate, a NaN costs nothing"""
    for term in (ref.TAIL, ref.TRUNCATED):
        q = cfg(D=30, term=term, kind=ref.SOFT_F32, scale=1.0)
        frames = np.zeros((1, 3, q.N), np.float32)
        frames[0, 1] = np.nan
        frames[0, 2] = -0.0
        ((data, info),) = ref.exact(build_dir, [(q, frames, None)])
        assert not data.any() and not info.any()
    assert ref.quantise(np.array([np.inf, -np.inf, np.nan, -0.0, 0.5, 1.5, 2.5, -0.5, -1.5, 126.6, 1e30], np.float32), 1.0).tolist() == \
        [127, -127, 0, 0, 0, 2, 2, 0, -2, 127, 127]
    q = cfg(D=24, kind=ref.SOFT_F32, scale=1.0)
    bits = ref.random_bits(24, 3)
    x = ref.frame_of(q, ref.encode(q, bits), 1)
    x[5], x[9], x[20] = np.nan, -0.0, np.inf if x[20] > 0 else -np.inf
    x[30] = -np.inf if x[30] > 0 else np.inf  # one saturated error: the clean path pays 127 for it
    ((data, info),) = ref.exact(build_dir, [(q, x[None, None], None)])
    assert np.array_equal(data[0, 0], np.packbits(bits)) and int(info[0, 0]) == 127
    wd, wi = ref.decode(q, x)
    assert np.array_equal(data[0, 0], wd) and int(info[0, 0]) == wi

"""The frame sync bank (include/hzsdr_framesync.h) without a GPU: the ABI's header, exports and bindings; the validation
at every bound's edge and one step outside; the host program tests/host/framesync_ref.cpp (the bytes the device must
produce) against the numpy brute force of tests/framesync_ref.py, which evaluates the definition position by position
over the whole stream with no ring, no tiles and no state -- on random rows with planted frames, on every cut of a
300-symbol row into two pushes, and on exact read-outs."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import framesync_ref as ref
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "hzsdr_framesync.h")
ENTRIES = {"hzsdr_framesync_create", "hzsdr_framesync_push", "hzsdr_framesync_get_state", "hzsdr_framesync_set_state", "hzsdr_framesync_positions",
           "hzsdr_framesync_plan", "hzsdr_framesync_reset", "hzsdr_framesync_free"}
GCC = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include")]
WORD32 = 0x1ACFFC1D


@pytest.fixture(scope="module")
def hz():
    return importlib.import_module("go-sdr_amd")


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("framesync_ref"))


def header_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(hzsdr_framesync_[a-z0-9_]+)\s*\(", text)))


# ---- the ABI ---------------------------------------------------------------------------------------

def test_header_is_c99(tmp_path):
    src = tmp_path / "inc.c"
    src.write_text('#include "hzsdr_framesync.h"\n'
                   "int main(void) { hzsdr_framesync *f = 0; return (f != 0) + HZSDR_FRAMESYNC_MAX_ROWS - HZSDR_FRAMESYNC_MAX_WORD"
                   " - HZSDR_FRAMESYNC_MAX_PAYLOAD - HZSDR_FRAMESYNC_MAX_HYPOTHESES - HZSDR_FRAMESYNC_FORM_COMPLEX - HZSDR_FRAMESYNC_FORM_DIBIT"
                   " - HZSDR_FRAMESYNC_FORM_DIFF + HZSDR_SYMSYNC_REAL_F32; }\n")
    subprocess.check_call(GCC + ["-c", str(src), "-o", str(tmp_path / "inc.o")])


def test_header_declares_exactly_the_entries():
    assert len(ENTRIES) == 8 and set(header_symbols()) == ENTRIES


def test_library_exports_and_ctypes_table(hz):
    capi = importlib.import_module("go-sdr_amd._capi")
    syms = header_symbols()
    for s in syms:
        assert hasattr(capi.lib, s), f"{s} declared in hzsdr_framesync.h but not exported"
    assert sorted(capi.FRAMESYNC_SIGNATURES) == syms
    for name, (res, args) in capi.FRAMESYNC_SIGNATURES.items():
        fn = getattr(capi.lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    found = re.findall(r"\bint (hzsdr_framesync_[a-z_]+)\s*\(([^)]*)\)", text)
    assert {name for name, _ in found} == ENTRIES
    import ctypes as C
    kinds = {"uint64_t": C.c_uint64, "unsigned": C.c_uint, "int": C.c_int, "size_t": C.c_size_t}
    for name, params in found:
        args = capi.FRAMESYNC_SIGNATURES[name][1]
        decl = [" ".join(p.split()) for p in params.split(",")]
        assert len(args) == len(decl), name
        for a, d in zip(args, decl):  # argument for argument: a pointer for a pointer, the scalar types by width and sign
            if "*" in d:
                assert a is C.c_void_p or hasattr(a, "_type_") and not isinstance(a._type_, str), (name, d)
                if "size_t *" in d:
                    assert a._type_ is C.c_size_t, (name, d)
                if "uint64_t *" in d and a is not C.c_void_p:
                    assert a._type_ is C.c_uint64, (name, d)
            else:
                assert a is kinds[d.split()[0]], (name, d)


def test_constants_and_python_layers(hz):
    defs = dict(re.findall(r"#define (HZSDR_\w+) (\d+)", open(HEADER).read()))
    assert int(defs["HZSDR_FRAMESYNC_MAX_ROWS"]) == hz.FRAMESYNC_MAX_ROWS == ref.MAX_ROWS == 8192
    assert int(defs["HZSDR_FRAMESYNC_MAX_WORD"]) == hz.FRAMESYNC_MAX_WORD == ref.MAX_WORD == 64
    assert int(defs["HZSDR_FRAMESYNC_MAX_PAYLOAD"]) == hz.FRAMESYNC_MAX_PAYLOAD == ref.MAX_PAYLOAD == 8192
    assert int(defs["HZSDR_FRAMESYNC_MAX_HYPOTHESES"]) == hz.FRAMESYNC_MAX_HYPOTHESES == ref.MAX_HYP == 4
    assert int(defs["HZSDR_FRAMESYNC_FORM_COMPLEX"]) == hz.FRAMESYNC_FORM_COMPLEX == ref.FORM_COMPLEX == 1
    assert int(defs["HZSDR_FRAMESYNC_FORM_DIBIT"]) == hz.FRAMESYNC_FORM_DIBIT == ref.FORM_DIBIT == 2
    assert int(defs["HZSDR_FRAMESYNC_FORM_DIFF"]) == hz.FRAMESYNC_FORM_DIFF == ref.FORM_DIFF == 4
    assert hz.SYMSYNC_REAL_F32 == ref.REAL_F32 and hz.FMT_C64 == ref.C64
    st = importlib.import_module("go-sdr_amd.stream")
    mod = importlib.import_module("go-sdr_amd.framesync")
    assert hz.FrameSync is mod.FrameSync and hz.sync_hypotheses is mod.sync_hypotheses and hz.pack_bits is mod.pack_bits and hz.unpack_bits is mod.unpack_bits
    assert callable(hz.Context.frame_sync) and callable(st.frame_rows)
    for name in ("push", "ragged", "state", "set_state", "positions", "reset", "plan", "close", "__enter__", "__exit__"):
        assert callable(getattr(hz.FrameSync, name)), name
    hpp = open(os.path.join(ROOT, "go-sdr_amd", "cxx", "hzsdr.hpp")).read()
    assert "class FrameSync" in hpp and '#include "../../include/hzsdr_framesync.h"' in hpp
    make = open(os.path.join(ROOT, "go-sdr_amd", "csrc", "Makefile")).read()
    assert "hzsdr_framesync.h" in make and "hz_framesync" not in make.split("MFMA_UNITS =")[1].splitlines()[0]
    # the sentences that left the decisions to others point to the bank
    for path in (os.path.join(ROOT, "include", "hzsdr_symsync.h"), os.path.join(ROOT, "go-sdr_amd", "symsync.py")):
        assert "hzsdr_framesync.h" in open(path).read(), path
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "hzsdr_framesync.h" in open(os.path.join(ROOT, doc)).read(), doc


def test_pack_unpack_and_hypotheses(hz):
    bits = ref.random_bits(13, 4)
    packed = hz.pack_bits(bits)
    assert packed.dtype == np.uint8 and packed.shape == (2,) and np.array_equal(hz.unpack_bits(packed, 13), bits)
    assert packed[0] >> 7 == bits[0] and (packed[1] & 0x07) == 0 and (packed[1] >> 3) & 1 == bits[12]
    assert hz.sync_hypotheses(0x2D, 6) == ([0x2D], [0])
    assert hz.sync_hypotheses(0x2D, 6, 1, "invert") == ([0x2D, 0x12], [0, 1])
    words, maps = hz.sync_hypotheses(WORD32, 32, 2, "rotate")
    assert maps == [0, 1, 2, 3] and words[0] == WORD32 and words[2] == WORD32 ^ 0xFFFFFFFF and len(set(words)) == 4
    # words[q] is what the word looks like received as x i^q; map q of it is the word again
    sent = ref.word_bits(WORD32, 32)
    q2 = ref.Config(32, words, 32, B=2, cplx=True, maps=maps)
    for q in range(4):
        x = ref.soft(sent, 1, q2, rotate=q)
        got = (ref.floats_of(x, q2) >> np.uint32(31)) ^ np.uint32(1)
        assert np.array_equal(got, ref.word_bits(words[q], 32)), q
        assert np.array_equal(ref.map_bits(got, q, 2), sent), q
    for bad in ((0x2D, 6, 1, "rotate"), (0x2D, 6, 2, "invert"), (0x2D, 5, 2, "none"), (1 << 6, 6, 1, "none"), (0, 65, 1, "none")):
        with pytest.raises(ValueError):
            hz.sync_hypotheses(*bad)


# ---- the validation --------------------------------------------------------------------------------

def cfg(**kw):
    base = dict(W=32, words=[WORD32], P=168, B=1, cplx=False, mask=None, thr=2, maps=None, diff=0, holdoff=None)
    base.update(kw)
    return ref.Config(**base)


EDGES = [
    (cfg(), True),
    (cfg(W=1, words=[1], thr=0), True), (cfg(W=64, words=[2 ** 64 - 1]), True), (cfg(W=0, words=[0], mask=1, thr=0), False),
    (cfg(W=65, words=[0], mask=1, thr=0), False),
    (cfg(P=1), True), (cfg(P=8192), True), (cfg(P=0), False), (cfg(P=8200), False), (cfg(P=8193), False),
    (cfg(B=2, cplx=True), True), (cfg(B=2, cplx=True, W=31, words=[1]), False), (cfg(B=2, cplx=True, P=167), False),
    (cfg(B=2, cplx=True, W=2, words=[1], thr=0, P=2), True), (cfg(B=2, cplx=True, W=1, words=[1], thr=0), False), (cfg(B=2, cplx=True, P=1), False),
    (cfg(B=2, cplx=False), False), (cfg(B=1, cplx=True), True), (cfg(B=0), False), (cfg(B=3, cplx=True, W=33, P=168), False),
    (cfg(words=[]), False), (cfg(words=[1, 2, 3, 4]), True), (cfg(words=[1, 2, 3, 4, 5]), False),
    (cfg(mask=0xFF, thr=7), True), (cfg(mask=0xFF, thr=8), False), (cfg(thr=31), True), (cfg(thr=32), False),
    (cfg(mask=0, thr=0), False), (cfg(mask=1 << 32, thr=0), False), (cfg(mask=(1 << 33) - 1), False), (cfg(mask=1 << 31, thr=0), True),
    (cfg(W=64, words=[0], mask=1 << 63, thr=0), True),
    (cfg(diff=1), True), (cfg(diff=2), True), (cfg(diff=3), False), (cfg(diff=1, B=2, cplx=True), False), (cfg(diff=2, B=1, cplx=True), True),
    (cfg(holdoff=1), True), (cfg(holdoff=0), False), (cfg(holdoff=2 ** 31), True), (cfg(holdoff=2 ** 31 + 1), False),
    (cfg(words=[1 << 32]), False), (cfg(words=[1, 2], maps=[0, 1]), True), (cfg(words=[1, 2], maps=[0, 2]), False),
    (cfg(B=2, cplx=True, words=[1, 2], maps=[3, 2]), True), (cfg(B=2, cplx=True, words=[1, 2], maps=[0, 4]), False),
]


def test_restated_validation(build_dir):
    """Every bound accepted at its edge and refused one step outside: csrc/hz_framesync_plan.h against the rules
    restated in Python.  (Rows, 0 and 8193, are refused by hzsdr_framesync_create itself: tests/test_gpu_framesync.py.)"""
    got = ref.check(build_dir, [q for q, _ in EDGES])
    for (q, want), ok in zip(EDGES, got):
        assert ref.accepted(q) == want, vars(q)
        assert ok == want, vars(q)
    assert sum(got) > 15 and sum(not g for g in got) > 15


# ---- the program against the brute force ----------------------------------------------------------------

def planted_row(q, n_bits, seed, plants, hyp=0, errors=0):
    """random bits with the word of hypothesis `hyp` and a random payload planted at each bit of `plants` -> (bits, payloads)"""
    bits = ref.random_bits(n_bits, seed)
    payloads = []
    for k, at in enumerate(plants):
        pay = ref.random_bits(q.P, seed * 131 + k)
        ref.plant(bits, at, q.words[hyp], q.W, pay)
        for e in range(errors):
            bits[at + (7 * e + 3) % q.W] ^= 1
        payloads.append(pay)
    return bits, payloads


CONFIGS = [
    cfg(),
    cfg(W=7, words=[0x5A], P=13, thr=0, holdoff=5),
    cfg(W=8, words=[0xA7, 0x58], maps=[0, 1], P=8, thr=0, holdoff=1),
    cfg(W=24, words=[0xFAF320], P=64, thr=1, mask=0xFFFF0F),
    cfg(W=63, words=[0x2AAAAAAA12345678], P=1, thr=3),
    cfg(W=64, words=[0xF0F0AA5512345678], P=65, cplx=True),
    cfg(W=1, words=[1], P=8, thr=0, holdoff=3),
    cfg(W=32, words=ref.rotated_words(WORD32, 32), maps=[0, 1, 2, 3], P=168, B=2, cplx=True, thr=2),
    cfg(W=16, words=[0xEB90], P=40, diff=1, thr=0),
    cfg(W=16, words=[0x7E7E], P=24, diff=2, thr=1),
]


@pytest.mark.parametrize("k", range(len(CONFIGS)))
def test_program_against_brute_force(build_dir, k):
    """random rows with planted frames, three rows and three pushes of unequal counts: frames, positions, info, counts
    and state, exactly; the planted frames outside each other's hold-off are among them"""
    q = CONFIGS[k]
    sym = 700
    n_bits = sym * q.B
    plants = [2 * q.B * 20, 2 * q.B * 20 + q.W + q.P + 2 * q.B, n_bits - q.W - q.P - 4 * q.B]
    rows, pays = [], []
    for r in range(3):
        bits, p = planted_row(q, n_bits, 100 * k + r, plants, hyp=r % len(q.words), errors=q.thr if r == 1 else 0)
        rows.append(ref.soft(ref.encode_diff(bits, q.diff), 7 * k + r, q))
        pays.append(p)
    x = np.stack(rows)
    cuts = [(0, 257), (257, 300), (300, sym)]
    # row 0 consumes every symbol (a count above n is clamped); row 1 none and row 2 a part of the second push
    counts = [np.array([257, 257, 257], np.uint32), np.array([50, 0, 20], np.uint32), None]
    pushes = [(x[:, a:b], c) if c is not None else x[:, a:b] for (a, b), c in zip(cuts, counts)]
    (got,) = ref.exact(build_dir, [(q, pushes, 8)])
    found = ref.same_as_brute(q, pushes, 8, got)
    assert found >= 1
    # row 0 consumes every symbol: its planted frames are found where they were planted, with their payloads
    per, _ = got
    seen = {int(p): bytes(f) for fr, ps, inf, cnt in per for f, p in zip(fr[0, :min(int(cnt[0]), 8)], ps[0, :min(int(cnt[0]), 8)])}
    if bin(q.mask).count("1") - 2 * q.thr >= 14:
        # a long word: no false candidate holds a plant off (the plants lie outside each other's hold-off)
        for at, pay in zip(plants, pays[0]):
            assert seen[(at + q.W) // q.B] == bytes(np.packbits(pay)), at
    else:
        # a short word matches the random bits too, and a false candidate in front may hold a plant off: at least as
        # many frames as were planted, and the brute force has agreed on each
        assert sum(int(cnt[0]) for _, _, _, cnt in per) >= len(plants)


def test_every_cut_of_a_row_into_two_pushes(build_dir):
    """a 300-symbol row with two planted frames, cut at every symbol 0 ... 300: the frames of the two pushes together,
    and the state behind them, are those of the one push; each frame is emitted by the push that delivers its last bit"""
    for q in (cfg(W=16, words=[0xEB90], P=40, thr=1, holdoff=20), cfg(W=8, words=[0x1B, 0xB1, 0xE4, 0x4E], maps=[0, 1, 2, 3], P=24, B=2, cplx=True, thr=0),
              cfg(W=16, words=[0xEB90], P=40, diff=2, thr=0)):
        n_bits = 300 * q.B
        bits, pays = planted_row(q, n_bits, 77, [31 * q.B, 150 * q.B + 2 * q.B])
        x = ref.soft(ref.encode_diff(bits, q.diff), 5, q)
        cases = [(q, [x], 16)] + [(q, [x[:c], x[c:]], 16) for c in range(0, 301)]
        got = ref.exact(build_dir, cases)
        (whole,), state = got[0]
        want_frames = [(int(p), bytes(f)) for f, p in zip(whole[0][0, :int(whole[3][0])], whole[1][0])]
        assert len(want_frames) >= 2 and ref.same_as_brute(q, [x], 16, got[0]) >= 2
        for c, (per, st) in zip(range(0, 301), got[1:]):
            frames = [(int(p), bytes(f), k) for k, (fr, ps, inf, cnt) in enumerate(per) for f, p in zip(fr[0, :int(cnt[0])], ps[0])]
            assert [(p, f) for p, f, _ in frames] == want_frames, c
            for p, _, k in frames:  # the payload's last symbol is p + P / B - 1: in the first push iff it lies before the cut
                assert k == (0 if p + q.P // q.B <= c else 1), (c, p)
            for a, b in zip(st, state):
                assert np.array_equal(a, b), c
        if q.diff == 0 and q.B == 1:
            ref.same_as_brute(q, [x[:123], x[123:]], 16, got[1 + 123])


def test_exact_readouts(build_dir, hz):
    """a single planted word with a payload that reads back as the bytes written: position, distance, hypothesis, and the
    pad bits zero; an inverted row under the second hypothesis; an all-zero word against an empty history"""
    text = b"frame sync: 21 bytes."
    pay = hz.unpack_bits(np.frombuffer(text, np.uint8), 168)
    q = cfg(words=[WORD32, WORD32 ^ 0xFFFFFFFF], maps=[0, 1])
    bits = np.zeros(400, np.uint8)
    bits[0::3] = 1
    ref.plant(bits, 100, WORD32, 32, pay)
    for inv in (0, 1):
        x = ref.soft(bits ^ inv, 9, q)
        ((per, state),) = ref.exact(build_dir, [(q, [x], 2)])
        fr, ps, inf, cnt = per[0]
        assert cnt[0] == 1 and ps[0, 0] == 132 and inf[0, 0] == (inv << 8) and bytes(fr[0, 0]) == text
        assert state[0][0] == 400 and state[1][0] == 132 + 200
    q13 = cfg(W=7, words=[0x5A], P=13, thr=0)
    bits = np.zeros(60, np.uint8)
    ref.plant(bits, 20, 0x5A, 7, np.ones(13, np.uint8))
    ((per, _),) = ref.exact(build_dir, [(q13, [ref.soft(bits, 2, q13)], 2)])
    assert per[0][3][0] == 1 and bytes(per[0][0][0, 0]) == b"\xff\xf8" and per[0][1][0, 0] == 27
    # bits before position 0 do not exist: an all-zero word is not found in the empty history, only where it was sent
    qz = cfg(W=8, words=[0], P=8, thr=0, holdoff=1)
    bits = np.ones(40, np.uint8)
    bits[16:24] = 0
    ((per, _),) = ref.exact(build_dir, [(qz, [ref.soft(bits, 3, qz)], 8)])
    assert per[0][3][0] == 1 and per[0][1][0, 0] == 24 and bytes(per[0][0][0, 0]) == b"\xff"
    # -0, NaNs of both signs and infinities decide by their sign bit
    odd = np.array([0.0, -0.0, np.nan, -np.nan, np.inf, -np.inf, 1e-45, -1e-45], np.float32)
    odd[3] = np.frombuffer(np.uint32(0xFFC00001).tobytes(), np.float32)[0]
    q8 = cfg(W=8, words=[0b10101010], P=8, thr=0)
    x = np.concatenate([odd, odd]).astype(np.float32)
    ((per, _),) = ref.exact(build_dir, [(q8, [x], 2)])
    assert per[0][3][0] == 1 and per[0][1][0, 0] == 8 and per[0][0][0, 0, 0] == 0b10101010

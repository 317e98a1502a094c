"""The HDLC deframer bank (include/hzsdr_hdlc.h) without a GPU: the ABI's header, exports and bindings; the validation
at every bound's edge and one step outside; the encoder and the two FCS known answers; the host program
tests/host/hdlc_ref.cpp (the bytes the device must produce) against the numpy restatement of tests/hdlc_ref.py on noise
rows and on encoded streams in ragged pushes; both against the textbook bit-serial decoder on error-free streams; every
single-bit error of an encoded frame; and planted faults in the restatement, each of which the assertions notice."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import hdlc_ref as ref
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "hzsdr_hdlc.h")
ENTRIES = {"hzsdr_hdlc_create", "hzsdr_hdlc_push", "hzsdr_hdlc_get_state", "hzsdr_hdlc_set_state", "hzsdr_hdlc_positions", "hzsdr_hdlc_plan",
           "hzsdr_hdlc_reset", "hzsdr_hdlc_free"}
GCC = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include")]
FLAG = [0, 1, 1, 1, 1, 1, 1, 0]


@pytest.fixture(scope="module")
def hz():
    return importlib.import_module("go-sdr_amd")


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("hdlc_ref"))


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


# ---- the ABI ---------------------------------------------------------------------------------------

def test_header_is_c99(tmp_path):
    src = tmp_path / "inc.c"
    src.write_text('#include "hzsdr_hdlc.h"\n'
                   "int main(void) { hzsdr_hdlc *f = 0; return (f != 0) + HZSDR_HDLC_MAX_ROWS - HZSDR_HDLC_MAX_BYTES - HZSDR_HDLC_EVENT_ABORT"
                   " - HZSDR_HDLC_EVENT_FLAG - HZSDR_HDLC_FORM_COMPLEX - HZSDR_HDLC_FORM_DIFF - HZSDR_HDLC_FORM_FCS16 - HZSDR_HDLC_FORM_FCS32"
                   " - HZSDR_HDLC_FORM_MSB_FIRST - HZSDR_HDLC_FORM_KEEP_BAD + HZSDR_SYMSYNC_REAL_F32; }\n")
    subprocess.check_call(GCC + ["-c", str(src), "-o", str(tmp_path / "inc.o")])


def test_header_library_and_ctypes_table(hz):
    import ctypes as C
    capi = importlib.import_module("go-sdr_amd._capi")
    text = header_text()
    assert set(re.findall(r"\b(hzsdr_hdlc_[a-z0-9_]+)\s*\(", text)) == ENTRIES == set(capi.HDLC_SIGNATURES)
    found = re.findall(r"\bint (hzsdr_hdlc_[a-z_]+)\s*\(([^)]*)\)", text)
    assert {name for name, _ in found} == ENTRIES
    kinds = {"uint64_t": C.c_uint64, "unsigned": C.c_uint, "int": C.c_int, "size_t": C.c_size_t}
    for name, params in found:
        fn = getattr(capi.lib, name)
        res, args = capi.HDLC_SIGNATURES[name]
        assert fn.restype is res and list(fn.argtypes) == list(args), name
        decl = [" ".join(p.split()) for p in params.split(",")]
        assert len(args) == len(decl), name
        for a, d in zip(args, decl):
            if "*" in d:
                assert a is C.c_void_p or hasattr(a, "_type_") and not isinstance(a._type_, str), (name, d)
                if "size_t *" in d:
                    assert a._type_ is C.c_size_t, (name, d)
                if "uint64_t *" in d and a is not C.c_void_p:
                    assert a._type_ is C.c_uint64, (name, d)
                if "uint8_t *" in d and a is not C.c_void_p:
                    assert a._type_ is C.c_uint8, (name, d)
            else:
                assert a is kinds[d.split()[0]], (name, d)
    push = dict(found)["hzsdr_hdlc_push"].replace("hzsdr_hdlc *f", "X")
    fs = re.search(r"\bint hzsdr_framesync_push\s*\(([^)]*)\)", open(os.path.join(ROOT, "include", "hzsdr_framesync.h")).read()).group(1)
    assert " ".join(push.split()) == " ".join(fs.replace("hzsdr_framesync *f", "X").split())  # the frame sync bank's argument list


def test_constants_and_python_layers(hz):
    defs = dict(re.findall(r"#define (HZSDR_\w+) (\d+)", open(HEADER).read()))
    assert int(defs["HZSDR_HDLC_MAX_ROWS"]) == hz.HDLC_MAX_ROWS == ref.MAX_ROWS == 8192
    assert int(defs["HZSDR_HDLC_MAX_BYTES"]) == hz.HDLC_MAX_BYTES == ref.MAX_BYTES == 1024
    assert int(defs["HZSDR_HDLC_EVENT_ABORT"]) == hz.HDLC_EVENT_ABORT == ref.EVENT_ABORT == 0
    assert int(defs["HZSDR_HDLC_EVENT_FLAG"]) == hz.HDLC_EVENT_FLAG == ref.EVENT_FLAG == 1
    for name in ("COMPLEX", "DIFF", "FCS16", "FCS32", "MSB_FIRST", "KEEP_BAD"):
        assert int(defs["HZSDR_HDLC_FORM_" + name]) == getattr(hz, "HDLC_FORM_" + name) == getattr(ref, "FORM_" + name), name
    assert hz.HDLC_FORM_COMPLEX == hz.FRAMESYNC_FORM_COMPLEX and hz.HDLC_FORM_DIFF == hz.FRAMESYNC_FORM_DIFF
    st = importlib.import_module("go-sdr_amd.stream")
    mod = importlib.import_module("go-sdr_amd.hdlc")
    assert hz.Hdlc is mod.Hdlc and hz.hdlc_encode is mod.hdlc_encode and hz.hdlc_fcs16 is mod.hdlc_fcs16 and hz.hdlc_fcs32 is mod.hdlc_fcs32
    assert callable(hz.Context.hdlc) and callable(st.hdlc_frames)
    for name in ("push", "ragged", "state", "set_state", "positions", "reset", "plan", "close", "__enter__", "__exit__"):
        assert callable(getattr(hz.Hdlc, name)), name
    hpp = open(os.path.join(ROOT, "go-sdr_amd", "cxx", "hzsdr.hpp")).read()
    assert "class Hdlc" in hpp and '#include "../../include/hzsdr_hdlc.h"' in hpp
    make = open(os.path.join(ROOT, "go-sdr_amd", "csrc", "Makefile")).read()
    assert "hzsdr_hdlc.h" in make and "hz_hdlc" not in make.split("MFMA_UNITS =")[1].splitlines()[0]
    # the sentences that left bit unstuffing to others point to the bank
    for path in (os.path.join(ROOT, "include", "hzsdr_framesync.h"), os.path.join(ROOT, "go-sdr_amd", "framesync.py")):
        assert "hzsdr_hdlc.h" in open(path).read(), path
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "hzsdr_hdlc.h" in open(os.path.join(ROOT, doc)).read(), doc


# ---- the validation --------------------------------------------------------------------------------

def test_validation_at_every_edge(build_dir):
    C = ref.Config
    good = [C(fcs=0, min_bytes=1, max_bytes=1), C(fcs=16, min_bytes=3, max_bytes=3), C(fcs=32, min_bytes=5, max_bytes=1024), C(diff=2, msb_first=1, keep_bad=1),
            C(fcs=0, min_bytes=1024, max_bytes=1024), C(diff=1, cplx=True)]
    bad = [C(fcs=0, min_bytes=0), C(fcs=16, min_bytes=2), C(fcs=32, min_bytes=4), C(max_bytes=1025), C(min_bytes=65, max_bytes=64), C(diff=3), C(fcs=8),
           C(fcs=24), C(msb_first=2), C(keep_bad=2), C(diff=-1), C(fcs=-16), C(max_bytes=0, min_bytes=0, fcs=0)]
    got = ref.accepted_by_program(build_dir, good + bad)
    assert got == [True] * len(good) + [False] * len(bad)
    assert [q.accepted() for q in good + bad] == got


# ---- the encoder and the FCS ------------------------------------------------------------------------

def test_fcs_known_answers_and_the_encoder(hz):
    assert hz.hdlc_fcs16(b"123456789") == 0x906E and hz.hdlc_fcs32(b"123456789") == 0xCBF43926
    assert ref.crc_bytes(b"123456789", 16) == 0x906E and ref.crc_bytes(b"123456789", 32) == 0xCBF43926
    # the register over a frame with its FCS ends at the residue
    for fcs in (16, 32):
        assert ref.fcs_register(ref.frame_bits(b"123456789", fcs), fcs) == ref.GOOD[fcs]
    d = hz.hdlc_encode([b"\xff\x01"], fcs=0)
    assert d.dtype == np.uint8 and d.tolist() == FLAG + [1, 1, 1, 1, 1, 0, 1, 1, 1] + [1, 0, 0, 0, 0, 0, 0, 0] + FLAG
    assert hz.hdlc_encode([b"\x01"], fcs=0, msb_first=True).tolist() == FLAG + [0] * 7 + [1] + FLAG
    assert hz.hdlc_encode([], flags=3, shared_zero=True).tolist() == [0, 1, 1, 1, 1, 1, 1] * 3 + [0]
    body = ref.stuffed(ref.frame_bits(b"\x7e\xff\x7e", 16)).tolist()
    assert hz.hdlc_encode([b"\x7e\xff\x7e"], fcs=16, flags=2).tolist() == FLAG * 2 + body + FLAG * 2
    b = hz.hdlc_encode([b"abc", b"\xff" * 7], fcs=32)
    for diff in (0, 1, 2):
        d = hz.hdlc_encode([b"abc", b"\xff" * 7], fcs=32, diff=diff)
        assert np.array_equal(ref.decided_bits(ref.floats_of(ref.soft(d, 3)), diff)[0], b) and np.array_equal(d, ref.line(b, diff))
        assert np.array_equal(d, hz.hdlc_line(b, diff))
    for kw in (dict(fcs=8), dict(flags=0), dict(diff=3)):
        with pytest.raises(ValueError):
            hz.hdlc_encode([b"x"], **kw)


# ---- streams ----------------------------------------------------------------------------------------

def traffic(hz, q, seed, payloads, shared=False, flags=1, aborts=(), mark=0):
    """the bits of a stream: leading noise-free idle, then every payload as a frame between flags; behind the frames whose
    index is in `aborts` a frame is begun and aborted; `mark` 1s of mark idle between frames"""
    parts = [np.zeros(seed % 5, np.uint8)]
    for k, p in enumerate(payloads):
        parts.append(hz.hdlc_encode([p], fcs=q.fcs, flags=flags, shared_zero=shared, msb_first=bool(q.msb_first)))
        if k in aborts:
            parts.append(np.array(FLAG + ref.stuffed(ref.random_bits(37, seed + k)).tolist() + [0] + [1] * (7 + k % 3), np.uint8))
        if mark:
            parts.append(np.ones(mark, np.uint8))
    parts.append(np.zeros(3, np.uint8))
    return np.concatenate(parts)


def payload_set(q, seed):
    n = q.fcs // 8
    return [ref.random_bytes(q.min_bytes - n, seed) if q.min_bytes > n else b"\x55", ref.random_bytes(q.max_bytes - n, seed + 1), b"\xff" * (q.max_bytes - n),
            b"\x00" * min(9, q.max_bytes - n), ref.random_bytes(min(11, q.max_bytes - n), seed + 2), b"\xff" * min(8, q.max_bytes - n)]


def expected(q, payloads):
    out = []
    for p in payloads:
        data = np.packbits(ref.frame_bits(p, q.fcs, bool(q.msb_first)), bitorder="big" if q.msb_first else "little").tobytes()
        if q.min_bytes <= len(data) <= q.max_bytes:
            out.append(data)
    return out


@pytest.mark.parametrize("diff", [0, 1, 2])
@pytest.mark.parametrize("fcs", [0, 16, 32])
def test_error_free_streams_three_ways(hz, build_dir, diff, fcs):
    """the program, the restatement and the textbook decoder on encoded streams: idle flags, shared zeros, aborts, mark
    idle, frames of min_bytes and max_bytes, all-ones and all-zero payloads, the three diff modes"""
    q = ref.Config(diff=diff, fcs=fcs, min_bytes=fcs // 8 + 2, max_bytes=40)
    for shared, flags, aborts, mark in ((False, 1, (), 0), (True, 3, (1, 4), 0), (False, 2, (0,), 9), (True, 1, (2,), 23)):
        payloads = payload_set(q, 10 * fcs + diff)
        b = traffic(hz, q, 7 + mark, payloads, shared, flags, aborts, mark)
        x = ref.soft(ref.line(b, diff), fcs + diff)
        pushes = [x[:101], x[101:101], x[101:700], x[700:]]
        ((per, st),) = ref.exact(build_dir, [(q, pushes, 16)])
        assert ref.agree(q, pushes, 16, per, st, 1) is None
        got = ref.stored(per, 0)
        assert got == ref.textbook(b, q)
        assert [g[0] for g in got] == expected(q, payloads) and all(g[2] == 1 for g in got)
        if mark == 0 and not shared and flags == 1:  # a closing and an opening flag between: the next frame starts behind both
            assert got[1][1] == got[0][1] + len(ref.stuffed(ref.frame_bits(payloads[0], fcs))) + 16
    # most significant bit first: the same frames, the bits of every byte the other way round
    qm = ref.Config(diff=diff, fcs=fcs, min_bytes=fcs // 8 + 2, max_bytes=40, msb_first=1)
    payloads = payload_set(qm, 5)
    x = ref.soft(ref.line(traffic(hz, qm, 3, payloads), diff), 9)
    ((per, st),) = ref.exact(build_dir, [(qm, [x], 16)])
    assert ref.agree(qm, [x], 16, per, st, 1) is None and [g[0] for g in ref.stored(per, 0)] == expected(qm, payloads)
    assert all(g[0][:len(p)] == p for g, p in zip(ref.stored(per, 0), payloads))


def test_noise_and_ragged_rows_program_against_restatement(hz, build_dir):
    """random signs (an event every 128 bits) and encoded traffic over several rows with ragged counts, n = 0 pushes and
    rows whose count is 0, real and complex rows"""
    R, n = 5, 4096
    for q in (ref.Config(fcs=0, min_bytes=1, max_bytes=64), ref.Config(fcs=0, min_bytes=2, max_bytes=5, diff=2, msb_first=1),
              ref.Config(fcs=16, keep_bad=1, max_bytes=32, cplx=True)):
        rows = [ref.soft(ref.random_bits(n, 100 + r), r, q.cplx) for r in range(R - 1)]
        b = traffic(hz, q, 11, payload_set(q, 2) * 3, True, 2, (1,), 3)
        rows.append(ref.soft(np.resize(ref.line(b, q.diff), n), 99, q.cplx))
        x = np.stack(rows)
        pushes, at = [], 0
        for k, width in enumerate((1000, 0, 63, 1, 2000, 1032)):
            cnt = np.array([width, width // 2, 0 if k % 2 else width, width + 5, width], np.uint32)
            pushes.append((np.ascontiguousarray(x[:, at:at + width]), cnt))
            at += width
        ((per, st),) = ref.exact(build_dir, [(q, pushes, 40)])
        assert ref.agree(q, pushes, 40, per, st, R) is None
        total = sum(int(p[3].sum()) for p in per)
        assert total >= 10, total  # (not two empty lists)
        assert st[0].tolist() == [sum(min(int(c[r]), p.shape[1]) for p, c in pushes) for r in range(R)]
    # cap: counted beyond, stored up to it
    q = ref.Config(fcs=0, min_bytes=1, max_bytes=64)
    x = ref.soft(traffic(hz, q, 5, payload_set(q, 8)), 5)
    ((all_, _), (one, _), (none, _)) = ref.exact(build_dir, [(q, [x], 64), (q, [x], 1), (q, [x], 0)])
    assert int(all_[0][3][0]) == int(one[0][3][0]) == int(none[0][3][0]) > 3
    assert ref.stored(one, 0) == ref.stored(all_, 0)[:1] and none[0][0].size == 0


def test_every_cut_and_the_state_round_trip(hz, build_dir):
    """one frame cut at every position into two pushes; the state behind the first push put into a new run"""
    q = ref.Config(fcs=16, max_bytes=12, diff=2)
    b = traffic(hz, q, 2, [b"\xffcut me\xff", b"\x00\x01"], False, 2)
    x = ref.soft(ref.line(b, 2), 4)
    ((whole, wst),) = ref.exact(build_dir, [(q, [x], 4)])
    want = ref.stored(whole, 0)
    assert [w[0][:-2] for w in want] == [b"\xffcut me\xff", b"\x00\x01"]
    res = ref.exact(build_dir, [(q, [x[:k], x[k:]], 4) for k in range(len(x) + 1)])
    for k, (per, st) in enumerate(res):
        assert ref.stored(per, 0) == want, k
        assert all(np.array_equal(a, c) for a, c in zip(st, wst)), k
        assert ref.agree(q, [x[:k], x[k:]], 4, per, st, 1) is None
    for k in (0, 17, 60, 61, 100):
        ((first, mid),) = ref.exact(build_dir, [(q, [x[:k]], 4)])
        ((second, end),) = ref.exact(build_dir, [(q, [x[k:]], 4, mid)])
        assert ref.stored(first, 0) + ref.stored(second, 0) == want and all(np.array_equal(a, c) for a, c in zip(end, wst)), k


def test_every_single_bit_error(hz, build_dir):
    """every bit of an encoded frame flipped in turn: nothing is emitted with keep_bad = 0; with keep_bad = 1 what is
    still well-formed comes out marked bad (a flipped bit can destroy a flag, create an event or change u)"""
    for fcs, payload in ((16, b"\xf8single bit\x1f"), (32, b"\xff\xff\x00abc")):
        q0, q1 = ref.Config(fcs=fcs, max_bytes=24), ref.Config(fcs=fcs, max_bytes=24, keep_bad=1)
        b = np.concatenate([np.zeros(4, np.uint8), hz.hdlc_encode([payload], fcs=fcs, flags=2), np.zeros(4, np.uint8)])
        body = range(4 + 16, len(b) - 4 - 16)
        cases0, cases1 = [], []
        for i in body:
            e = b.copy()
            e[i] ^= 1
            x = ref.soft(e, i)
            cases0.append((q0, [x], 4))
            cases1.append((q1, [x], 4))
        r0, r1 = ref.exact(build_dir, cases0), ref.exact(build_dir, cases1)
        ((clean, _),) = ref.exact(build_dir, [(q0, [ref.soft(b, 1)], 4)])
        assert [g[0][:-fcs // 8] for g in ref.stored(clean, 0)] == [payload]
        marked = 0
        for (per0, _), (per1, st1), c1 in zip(r0, r1, cases1):
            assert int(per0[0][3][0]) == 0 and ref.stored(per0, 0) == []
            assert ref.agree(q1, c1[1], 4, per1, st1, 1) is None
            got = ref.stored(per1, 0)
            assert all(g[2] == 0 for g in got)
            marked += len(got) > 0
        assert marked > len(body) // 2, (marked, len(body))  # (a flip that keeps u a whole number of bytes: most of them)


# ---- planted faults ---------------------------------------------------------------------------------

def fault_streams(hz):
    """[(config, bits)]: one stream per fault that the restatement can carry"""
    q = ref.Config(fcs=16, max_bytes=40)
    q0 = ref.Config(fcs=0, min_bytes=1, max_bytes=8)
    ones = hz.hdlc_encode([b"\xff" * 20], fcs=16)  # five 1s that straddle bit 64 of the span
    span = ref.stuffed(ref.frame_bits(b"\xff" * 20, 16))
    assert span[59:66].tolist() == [0, 1, 1, 1, 1, 1, 0]
    shared = hz.hdlc_encode([b"shared zero"], fcs=16, flags=2, shared_zero=True)
    aborted = np.array(FLAG + [0] * 9 + [1] * 7 + [0] * 9 + FLAG, np.uint8)  # without the abort: 25 bits, one of them stuffed, three bytes
    return [(q, ones), (q, shared), (q0, aborted), (q, hz.hdlc_encode([b"residue"], fcs=16))]


def check_restatement(hz, build_dir, fault):
    """the assertions of this file on the fault streams -> the list of the streams on which they fail"""
    failed = []
    for k, (q, b) in enumerate(fault_streams(hz)):
        x = ref.soft(b, k)
        ((per, st),) = ref.exact(build_dir, [(q, [x[:50], x[50:]], 4)])
        if ref.agree(q, [x[:50], x[50:]], 4, per, st, 1, fault) is not None:
            failed.append(k)
    return failed


def test_planted_faults_are_noticed(hz, build_dir):
    assert check_restatement(hz, build_dir, None) == []
    ((per, _),) = ref.exact(build_dir, [(fault_streams(hz)[2][0], [ref.soft(fault_streams(hz)[2][1], 0)], 4)])
    assert int(per[0][3][0]) == 0  # the abort discards the frame
    for k, fault in enumerate(("boundary", "shared", "abort", "residue")):
        assert k in check_restatement(hz, build_dir, fault), fault

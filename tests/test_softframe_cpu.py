"""The soft frame bank (include/hzsdr_softframe.h) without a GPU: the host program tests/host/softframe_ref.cpp (push by
push over csrc/hz_softframe_plan.h, the history carried as the bank carries it) against the numpy restatement of
tests/softframe_ref.py (whole streams, no pushes, no history), bit for bit; the NaN fill and the status of forged
positions and hypotheses; and the header's equivalence: the sign of every emitted float is the bit that
tests/framesync_ref.py packs at the same place of the same frame, under all six maps.  The frames are found by the frame
sync bank's own host program in the same pushes."""
import os

import numpy as np
import pytest

import framesync_ref as fsr
import softframe_ref as ref
from conftest import ROOT
from util import splitmix64

BUILD = os.path.join(ROOT, "build")
FORMS = [("real", 40), ("re", 24), ("dibit", 48), ("dibit", 2), ("real", 1)]


def random_cuts(n, seed, small):
    """piece sizes that sum to at most n: random, with 0 and 1 among them; small: all below `small`"""
    z, out, at, k = splitmix64(seed, 4096), [], 0, 0
    while at < n:
        s = int(z[k] % np.uint64(small)) if k % 5 else (k // 5) % 2
        out.append(s)
        at += s
        k += 1
    return out


def run(fq, x, sizes, cap, in_counts=None, state=None):
    q = ref.of_framesync(fq)
    pieces = ref.cut(x, sizes)
    pushes, hard = ref.with_frames(BUILD, fq, pieces, cap, in_counts)
    case = (q, pushes, cap) if state is None else (q, pushes, cap, state)
    ((per, state),) = ref.exact(BUILD, [case])
    return q, pushes, hard, per, state


def check_all(fq, x, sizes, cap, R, expect_frames):
    q, pushes, hard, per, (pos, hist) = run(fq, x, sizes, cap)
    seen = ref.same_as_whole_stream(q, pushes, cap, per, R)
    assert seen == expect_frames, (seen, expect_frames)
    for (_, _, got, _, _), fr, (y, status) in zip(pushes, hard, per):
        for r in range(R):
            m = min(int(got[r]), cap)
            assert (status[r, :m] == ref.SERVED).all() and (status[r, m:] == ref.SENT).all() and (y[r, m:] == ref.SENT).all()
            assert ref.signs_are_the_packed_bits(y[r, :m], fr[r, :m], q.P)
    for r in range(R):
        stream = ref.row_stream(q, pushes, r, R)
        assert int(pos[r]) * q.B == len(stream)
        want = np.zeros(q.HF, np.uint32)
        take = min(q.HF, len(stream))
        if take:
            want[q.HF - take:] = stream[len(stream) - take:]
        assert np.array_equal(hist[r], want), r
    return per


@pytest.mark.parametrize("form,P", FORMS)
def test_program_equals_the_whole_stream_restatement_on_random_cuts(form, P):
    """three rows under different hypotheses, NaNs with payloads, zeros and infinities in the payloads, random cuts with
    pushes of 0 and 1 symbols; every frame is served, equals the slice of the whole stream, and its signs are the
    hard frame's bits; the state is the stream's tail"""
    fq = ref.sync_config(P, form)
    R, nframes = 3, 5
    x = ref.make_rows(fq, R, nframes, 9, 11, special=True)
    for seed, small in ((1, 2 * (32 + P)), (2, 40)):
        check_all(fq, x, random_cuts(x.shape[1], seed, small), 3, R, R * nframes)
    check_all(fq, x, [], 8, R, R * nframes)  # the stream whole


def test_pushes_shorter_than_the_history():
    """pushes of a third of a payload: a payload spans four pushes and more, the carry reads what it must not have
    overwritten"""
    for form, P in (("real", 60), ("dibit", 60)):
        fq = ref.sync_config(P, form)
        x = ref.make_rows(fq, 2, 3, 5, 21, special=True)
        Ps = P // fq.B
        check_all(fq, x, [Ps // 3] * (x.shape[1] // (Ps // 3)), 2, 2, 6)
        check_all(fq, x, [1] * x.shape[1], 1, 2, 6)


def test_all_six_maps_give_the_packed_bits():
    """B = 1 maps 0, 1 and B = 2 maps 0 ... 3, each met by a row received under that hypothesis"""
    met = set()
    for form in ("real", "dibit"):
        fq = ref.sync_config(32, form)
        H = len(fq.words)
        x = ref.make_rows(fq, H, 2, 4, 5)
        q, pushes, hard, per, _ = run(fq, x, [50, 31], 4)
        for (_, _, got, _, info), fr, (y, status) in zip(pushes, hard, per):
            for r in range(H):
                for f in range(int(got[r])):
                    h = (int(info[r, f]) >> 8) & 0xFF
                    assert h == r and ref.signs_are_the_packed_bits(y[r, f], fr[r, f], q.P)
                    met.add((fq.B, fq.maps[h]))
    assert met == {(1, 0), (1, 1), (2, 0), (2, 1), (2, 2), (2, 3)}


def test_rows_with_counts_of_their_own():
    """in_counts: rows consume different parts of a push, one nothing at all"""
    fq = ref.sync_config(20, "re")
    R = 3
    x = ref.make_rows(fq, R, 4, 6, 31)
    n = x.shape[1]
    a, b = n // 3, n // 2
    # row 0 takes everything in two pushes, row 1 lags behind and catches up, row 2 takes nothing in the first push
    pieces = [x[:, :a], None, None]
    counts = [np.array([a, a // 2, 0], np.uint32)]
    second = np.ones((R, b), x.dtype)
    second[0, :b] = x[0, a:a + b]
    second[1, :b] = x[1, a // 2:a // 2 + b]
    second[2, :b] = x[2, :b]
    pieces[1], pieces[2] = second, np.ones((R, 0), x.dtype)
    counts += [np.array([b, b, b], np.uint32), None]
    q = ref.of_framesync(fq)
    pushes, hard = ref.with_frames(BUILD, fq, pieces, 4, counts)
    ((per, (pos, hist)),) = ref.exact(BUILD, [(q, pushes, 4)])
    assert ref.same_as_whole_stream(q, pushes, 4, per, R) > 0
    assert pos.tolist() == [a + b, a // 2 + b, b]


def test_forged_positions_and_hypotheses():
    """a position just before the window, just behind it, at its two edges, near 2^64, and h = H: the quiet NaN and the status"""
    fq = ref.sync_config(16, "real")
    q = ref.of_framesync(fq)
    Ps, Kh = q.Ps, q.Ps - 1
    x = ref.make_stream(fq, 3, 4, 3)
    n = len(x)
    a = n // 2
    cap = 8
    p0, p1 = a, n
    forged = [(p0 - Kh - 1, 0, ref.OUTSIDE), (p0 - Kh, 0, ref.SERVED), (p1 - Ps, 1, ref.SERVED), (p1 - Ps + 1, 0, ref.OUTSIDE), (2 ** 64 - 1, 0, ref.OUTSIDE),
              (2 ** 64 - Kh, 1, ref.OUTSIDE), (p0, 2, ref.NO_HYPOTHESIS), (p0, 255, ref.NO_HYPOTHESIS)]
    pos = np.array([[s for s, _, _ in forged]], np.uint64)
    info = np.array([[h << 8 for _, h, _ in forged]], np.uint32)
    none = (np.zeros(1, np.uint32), np.zeros((1, cap), np.uint64), np.zeros((1, cap), np.uint32))
    pushes = [(x[:a], None, *none), (x[a:], None, np.array([cap + 3], np.uint32), pos, info)]
    ((per, _),) = ref.exact(BUILD, [(q, pushes, cap)])
    y, status = per[1]
    assert status[0].tolist() == [st for _, _, st in forged]
    stream = fsr.floats_of(x, q)
    for f, (s, h, st) in enumerate(forged):
        if st == ref.SERVED:
            assert np.array_equal(y[0, f], ref.frame(q, stream, s, h))
        else:
            assert (y[0, f] == ref.QNAN).all()
    # the first push: p0 = 0 < Kh, so position 0 is inside whatever Kh is, and nothing ending behind p1 is
    pos0 = np.array([[0, a - Ps, a - Ps + 1] + [0] * (cap - 3)], np.uint64)
    pushes = [(x[:a], None, np.array([3], np.uint32), pos0, np.zeros((1, cap), np.uint32))]
    ((per, _),) = ref.exact(BUILD, [(q, pushes, cap)])
    assert per[0][1][0, :3].tolist() == [ref.SERVED, ref.SERVED, ref.OUTSIDE] and (per[0][1][0, 3:] == ref.SENT).all()


def test_a_state_moved_into_a_fresh_bank():
    fq = ref.sync_config(32, "dibit")
    x = ref.make_rows(fq, 2, 4, 3, 41, special=True)
    n = x.shape[1]
    q, pushes, _, whole, end = run(fq, x, [n // 3, n // 3], 4)
    _, _, _, first, mid = run(fq, x[:, :n // 3], [], 4)
    ((rest, end2),) = ref.exact(BUILD, [(q, pushes[1:], 4, mid)])
    for (a, sa), (b, sb) in zip(whole[1:], rest):
        assert np.array_equal(a, b) and np.array_equal(sa, sb)
    assert np.array_equal(end[0], end2[0]) and np.array_equal(end[1], end2[1])


def test_the_layers_agree_with_the_header():
    """every entry the header declares is in the ctypes table, argument for argument by pointer and width; the constants;
    the Python, C++ and build layers name the bank; the remarks that left soft outputs to others point to the header"""
    import ctypes as C
    import importlib
    import re
    hz = importlib.import_module("go-sdr_amd")
    capi = importlib.import_module("go-sdr_amd._capi")
    text = open(os.path.join(ROOT, "include", "hzsdr_softframe.h")).read()
    found = re.findall(r"\bint (hzsdr_softframe_[a-z_]+)\s*\(([^)]*)\)", text)
    assert {name for name, _ in found} == set(capi.SOFTFRAME_SIGNATURES) and len(found) == 8
    kinds = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "unsigned": C.c_uint, "int": C.c_int, "size_t": C.c_size_t, "float": C.c_float}
    for name, params in found:
        res, args = capi.SOFTFRAME_SIGNATURES[name]
        fn = getattr(capi.lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
        decl = [" ".join(p.split()) for p in params.split(",")]
        assert len(args) == len(decl), name
        for a, d in zip(args, decl):
            if "*" in d:
                assert a is C.c_void_p or hasattr(a, "_type_") and not isinstance(a._type_, str), (name, d)
            else:
                assert a is kinds[d.split()[0]], (name, d)
    defs = dict(re.findall(r"#define (HZSDR_\w+) \(?(\d+)", text))
    assert int(defs["HZSDR_SOFTFRAME_MAX_ROWS"]) == hz.SOFTFRAME_MAX_ROWS == 8192 and int(defs["HZSDR_SOFTFRAME_MAX_PAYLOAD"]) == hz.SOFTFRAME_MAX_PAYLOAD == 8192
    assert int(defs["HZSDR_SOFTFRAME_MAX_HYPOTHESES"]) == hz.SOFTFRAME_MAX_HYPOTHESES == 4 and hz.SOFTFRAME_MAX_SLOTS == 1 << 22
    assert "#define HZSDR_SOFTFRAME_MAX_SLOTS (1u << 22)" in text
    assert int(defs["HZSDR_SOFTFRAME_SERVED"]) == hz.SOFTFRAME_SERVED == ref.SERVED == 0
    assert int(defs["HZSDR_SOFTFRAME_OUTSIDE"]) == hz.SOFTFRAME_OUTSIDE == ref.OUTSIDE == 1
    assert int(defs["HZSDR_SOFTFRAME_NO_HYPOTHESIS"]) == hz.SOFTFRAME_NO_HYPOTHESIS == ref.NO_HYPOTHESIS == 2
    assert int(defs["HZSDR_SOFTFRAME_FORM_COMPLEX"]) == hz.SOFTFRAME_FORM_COMPLEX == ref.FORM_COMPLEX == 1
    assert int(defs["HZSDR_SOFTFRAME_FORM_DIBIT"]) == hz.SOFTFRAME_FORM_DIBIT == ref.FORM_DIBIT == 2
    st = importlib.import_module("go-sdr_amd.stream")
    assert hz.SoftFrames is importlib.import_module("go-sdr_amd.softframe").SoftFrames and callable(hz.Context.soft_frames)
    for name in ("push", "ragged", "state", "set_state", "reset", "plan", "positions", "close", "__enter__", "__exit__"):
        assert callable(getattr(hz.SoftFrames, name)), name
    import inspect
    for fn in (st.decoded_frames, st.corrected_frames):
        assert inspect.signature(fn).parameters["soft"].default is None
    hpp = open(os.path.join(ROOT, "go-sdr_amd", "cxx", "hzsdr.hpp")).read()
    assert "class SoftFrames" in hpp and '#include "../../include/hzsdr_softframe.h"' in hpp
    make = open(os.path.join(ROOT, "go-sdr_amd", "csrc", "Makefile")).read()
    assert "hzsdr_softframe.h" in make and "hz_softframe" not in make.split("MFMA_UNITS =")[1].splitlines()[0]
    for path in ("include/hzsdr_framesync.h", "include/hzsdr_viterbi.h", "go-sdr_amd/framesync.py", "go-sdr_amd/viterbi.py",
                 "README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "hzsdr_softframe.h" in open(os.path.join(ROOT, path)).read(), path
    assert "diff" in text and "no soft counterpart" in text.lower().replace("\n * ", " ")


def test_the_validation_is_the_headers():
    sets = [ref.Config(P, B, cplx, maps) for P in (0, 1, 2, 3, 8192, 8193) for B in (0, 1, 2, 3) for cplx in (False, True)
            for maps in ((0,), (1,), (2,), (3,), (4,), (0, 1, 0, 1), (0, 0, 0, 0, 0), ())]
    got = ref.check(BUILD, sets)
    want = [ref.accepted(q) for q in sets]
    assert got == want and any(want) and not all(want)

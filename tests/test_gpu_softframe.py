"""The soft frame bank (include/hzsdr_softframe.h) on the GPU against the host program tests/host/softframe_ref.cpp, which
tests/test_softframe_cpu.py holds to the numpy restatement: floats (as bit patterns) and status are compared EXACTLY, the
destinations are full of sentinels, and every word that is not a stored frame's -- the slots behind a row's count, the
row padding -- is checked.  The frames are found by a real FrameSync in the same pushes, with a clean sync word and thr 0;
the served frames are also held to the whole-stream restatement and their signs to the FrameSync's packed bits, so that
two wrong answers cannot agree."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import framesync_ref as fsr
import softframe_ref as ref
import viterbi_ref as vr
from conftest import ROOT
from util import splitmix64

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BUILD = os.path.join(ROOT, "build")
SENT = ref.SENT


@pytest.fixture(scope="module")
def hz():
    return importlib.import_module("go-sdr_amd")


@pytest.fixture(scope="module")
def ctx(hz):
    c = hz.Context(0, hz.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


@pytest.fixture(scope="module")
def hctx(hz):
    c = hz.Context(0, hz.MEM_HOST)
    yield c
    c.close()


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def banks(c, fq, R):
    args, kw = fq.create_args()
    fs = c.frame_sync(fq.kind, *args, rows=R, **kw)
    return fs, c.soft_frames(fs)


def as_bits(a):
    """host array -> its unsigned bit patterns"""
    a = host(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def run_pushes(c, fq, pieces, cap, device, in_counts=None, pads=(0, 0), state=None, sf_state=None):
    """The pieces through a new FrameSync and the SoftFrames beside it, every push's input inside a wider buffer (row
    pitch n + pads[0]) and its floats inside a wider destination full of sentinels (row pitch cap * P + pads[1]).
    -> (pushes as softframe_ref.exact takes them, hard frames per push, [(wide floats, status)] per push as bit
    patterns, final state); the padding is checked here."""
    q = ref.of_framesync(fq)
    R = 1 if pieces[0].ndim == 1 else pieces[0].shape[0]
    ic = in_counts or [None] * len(pieces)
    pushes, hard, got_all = [], [], []
    fs, sf = banks(c, fq, R)
    with fs, sf:
        if state is not None:
            fs.set_state(*state)
        if sf_state is not None:
            sf.set_state(*sf_state)
        for x, cnt in zip(pieces, ic):
            x2 = np.asarray(x).reshape(R, -1)
            n = x2.shape[1]
            wide_in = np.full((R, n + pads[0]), 3, x2.dtype)
            wide_in[:, :n] = x2
            wide_out = np.full((R, cap * q.P + pads[1]), SENT, np.uint32).view(np.float32)
            status = np.full((R, cap), SENT, np.uint32)
            cin = None if cnt is None else np.asarray(cnt, np.uint32)
            if device:
                wide_in, wide_out, status = dev(wide_in), dev(wide_out), dev(status.view(np.int32))
                cin = None if cin is None else dev(cin.view(np.int32))
            xin = wide_in[:, :n] if R > 1 else wide_in[0, :n]
            if device:
                view = torch.as_strided(wide_out, (R, cap, q.P), (wide_out.shape[1], q.P, 1))
            else:
                view = np.lib.stride_tricks.as_strided(wide_out, (R, cap, q.P), (wide_out.strides[0], 4 * q.P, 4))
            frames, pos, info, got = fs.push(xin, cin, cap)
            sf.push(xin, cin, pos, info, got, cap, out=(view, status))
            if device:
                torch.cuda.synchronize()
            gw = as_bits(wide_out)
            assert (gw[:, cap * q.P:] == SENT).all(), "the row padding was written"
            pushes.append((x2 if R > 1 else x2[0], cnt, as_bits(got).copy(), as_bits(pos).copy(), as_bits(info).copy()))
            hard.append(host(frames).copy())
            got_all.append((gw[:, :cap * q.P].reshape(R, cap, q.P).copy(), as_bits(status).copy()))
        assert np.array_equal(sf.positions(), fs.positions())
        end = sf.state()
    return q, pushes, hard, got_all, end


def check_against_program(q, pushes, hard, got, end, cap, expect_frames=None, state=None):
    R = got[0][0].shape[0]
    case = (q, pushes, cap) if state is None else (q, pushes, cap, state)
    ((per, (wpos, whist)),) = ref.exact(BUILD, [case])
    for k, ((y, st), (wy, wst)) in enumerate(zip(got, per)):
        assert np.array_equal(st, wst), (k, st, wst)
        assert np.array_equal(y, wy), k
    assert np.array_equal(end[0], wpos) and np.array_equal(end[1].view(np.uint32), whist)
    if state is None:
        seen = ref.same_as_whole_stream(q, pushes, cap, got, R)
        if expect_frames is not None:
            assert seen == expect_frames, (seen, expect_frames)
    for (_, _, cnt, _, _), fr, (y, st) in zip(pushes, hard, got):
        for r in range(R):
            m = min(int(cnt[r]), cap)
            assert (st[r, :m] == ref.SERVED).all()
            assert ref.signs_are_the_packed_bits(y[r, :m], fr[r, :m], q.P)
    return per


# ---- 1. forms and sizes ---------------------------------------------------------------------------------------

def plan_sizes(B):
    step = ref.THREADS * B
    return [B, step - B, step, step + B]


@pytest.mark.parametrize("form", ["real", "re", "dibit"])
def test_forms_and_sizes_at_the_plans_edges(hz, ctx, form):
    """P = B (no history), P one below, at and one above the floats a workgroup moves per step (from plan()), under every
    map of the form: rows received under each hypothesis; the stream whole and in pieces around a payload's symbols"""
    B = 2 if form == "dibit" else 1
    for P in plan_sizes(B):
        fq = ref.sync_config(P, form)
        H = len(fq.words)
        fs, sf = banks(ctx, fq, H)
        with fs, sf:
            step, hf, fm = sf.plan()
        assert step == ref.THREADS * B and P in (B, step - B, step, step + B) and hf == P - B
        assert fm == (ref.FORM_COMPLEX if fq.cplx else 0) | (ref.FORM_DIBIT if B == 2 else 0)
        x = ref.make_rows(fq, H, 3, 5, 100 + P, special=True)
        Ps = P // B
        for sizes in ([], [Ps + 40, Ps - 1, Ps, Ps + 1] if Ps > 1 else [33, 0, 1, 1, 2]):
            q, pushes, hard, got, end = run_pushes(ctx, fq, ref.cut(x, sizes), 3, True, pads=(3, 6))
            check_against_program(q, pushes, hard, got, end, 3, expect_frames=3 * H)
            hyps = {(int(i) >> 8) & 0xFF for p in pushes for r in range(H) for i in p[4][r, :min(int(p[2][r]), 3)]}
            assert hyps == set(range(H))


@pytest.mark.parametrize("form", ["real", "dibit"])
def test_the_largest_payload(ctx, form):
    fq = ref.sync_config(8192, form)
    x = ref.make_rows(fq, 2, 2, 3, 7, special=True)
    n = x.shape[1]
    q, pushes, hard, got, end = run_pushes(ctx, fq, ref.cut(x, [n // 3, n // 3]), 2, True, pads=(1, 1))
    check_against_program(q, pushes, hard, got, end, 2, expect_frames=4)


# ---- 2. cuts ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["real", "dibit"])
def test_cuts(ctx, form):
    """one stream whole, then cut so that a frame ends on a push's last symbol, one starts exactly at p0 - Kh, one spans
    four pushes, and the rest goes by in pieces of 1, 7, Ps - 1, Ps and Ps + 1 symbols with n = 0 pushes between"""
    B = 2 if form == "dibit" else 1
    Ps = 24
    fq = ref.sync_config(Ps * B, form)
    Kh, lead, gap, nframes = Ps - 1, 9, 5, 12
    per = (32 + fq.P) // B + gap
    x = ref.make_stream(fq, nframes, gap, 77, turn=1, special=True, lead=lead)
    n = len(x)
    s = [lead + f * per + 32 // B for f in range(nframes)]
    edges = [s[0] + Ps, s[1] + Kh, s[2] + 5, s[2] + 11, s[2] + 17, s[2] + 30]
    at, k = edges[-1], 0
    tail = [1, 1, 1, 7, Ps - 1, Ps, Ps + 1]
    while at < n:
        at += tail[k % len(tail)]
        edges.append(min(at, n))
        k += 1
    sizes, prev = [], 0
    for e in edges:
        sizes += [e - prev, 0]
        prev = e
    q, pushes, hard, got, end = run_pushes(ctx, fq, ref.cut(x, []), nframes, True)
    whole = check_against_program(q, pushes, hard, got, end, nframes, expect_frames=nframes)
    assert pushes[0][3][0].tolist() == s
    q, pushes, hard, got, end2 = run_pushes(ctx, fq, ref.cut(x, sizes), 2, True)
    check_against_program(q, pushes, hard, got, end2, 2, expect_frames=nframes)
    assert np.array_equal(end[0], end2[0]) and np.array_equal(end[1].view(np.uint32), end2[1].view(np.uint32))
    # the same frames, whatever the cut
    served = [y[0, f] for (_, _, cnt, _, _), (y, _) in zip(pushes, got) for f in range(int(cnt[0]))]
    assert len(served) == nframes and all(np.array_equal(a, b) for a, b in zip(served, whole[0][0][0]))
    # and the cut met the three edges
    p0, met = 0, set()
    for (xp, _, cnt, pos, _) in pushes:
        p1 = p0 + len(xp)
        for f in range(int(cnt[0])):
            sf_ = int(pos[0, f])
            met |= {"ends on the last symbol"} if sf_ + Ps == p1 else set()
            met |= {"starts at p0 - Kh"} if sf_ + Kh == p0 else set()
        p0 = p1
    bounds = np.cumsum([len(p[0]) for p in pushes if len(p[0])])
    assert np.searchsorted(bounds, s[2] + Ps - 1, side="right") - np.searchsorted(bounds, s[2], side="right") == 3  # four pushes
    assert met == {"ends on the last symbol", "starts at p0 - Kh"}


# ---- 3. rows, pitches, counts, memory spaces --------------------------------------------------------------------

@pytest.fixture(scope="module")
def row_cases():
    """R -> (fq, pieces, in_counts, cap): rows under every hypothesis, their frames at different places; in the second
    push the rows consume different counts, row 1 nothing at all"""
    out = {}
    for R in (1, 3, 65):
        fq = ref.sync_config(40, "dibit")
        x = ref.make_rows(fq, R, 6, 4, 300 + R, special=True)
        n = x.shape[1]
        a, b = n // 4, n // 2
        c2 = np.array([b - (r % 5) if r != 1 else 0 for r in range(R)], np.uint32)
        second = np.ones((R, b), x.dtype)
        third = np.ones((R, n), x.dtype)
        for r in range(R):
            second[r, :c2[r]] = x[r, a:a + c2[r]]
            rest = x[r, a + c2[r]:]
            third[r, :len(rest)] = rest
        pieces = [x[:, :a], second, third] if R > 1 else [x[0, :a], second[0], third[0]]
        out[R] = (fq, pieces, [None, c2, None])
    return out


@pytest.mark.parametrize("R", [1, 3, 65])
@pytest.mark.parametrize("space", ["device", "host"])
def test_rows_pitches_counts_and_spaces(ctx, hctx, row_cases, space, R):
    """an input pitch above n, an output pitch above cap * P (odd: the float-by-float gather; even: the pair gather), rows
    with counts of their own; cap below a row's count: the stored frames are right and nothing else is touched"""
    fq, pieces, counts = row_cases[R]
    c, device = (ctx, True) if space == "device" else (hctx, False)
    results = []
    for cap, pads in ((4, (5, 7)), (4, (0, 0)), (1, (2, 4))):
        q, pushes, hard, got, end = run_pushes(c, fq, pieces, cap, device, counts, pads)
        check_against_program(q, pushes, hard, got, end, cap)
        results.append((got, end))
        assert any(int(p[2].max()) > 1 for p in pushes)  # (cap = 1 loses frames)
        for (_, _, cnt, _, _), (y, st) in zip(pushes, got):
            for r in range(R):
                m = min(int(cnt[r]), cap)
                assert (y[r, m:] == SENT).all() and (st[r, m:] == SENT).all()
    (a, ea), (b, eb), (one, _) = results
    for (ya, sa), (yb, sb), (y1, _) in zip(a, b, one):
        assert np.array_equal(ya, yb) and np.array_equal(sa, sb)
        assert np.array_equal(np.where(y1 == SENT, ya[:, :1], y1), ya[:, :1])  # (the first frame of a push, whatever cap is)
    assert np.array_equal(ea[1].view(np.uint32), eb[1].view(np.uint32))


def test_device_and_host_spaces_give_equal_bits(ctx, hctx, row_cases):
    fq, pieces, counts = row_cases[3]
    a = run_pushes(ctx, fq, pieces, 4, True, counts, (3, 1))
    b = run_pushes(hctx, fq, pieces, 4, False, counts, (3, 1))
    for (ya, sa), (yb, sb) in zip(a[3], b[3]):
        assert np.array_equal(ya, yb) and np.array_equal(sa, sb)
    assert np.array_equal(a[4][0], b[4][0]) and np.array_equal(a[4][1].view(np.uint32), b[4][1].view(np.uint32))


# ---- 4. state -------------------------------------------------------------------------------------------------------

def test_state_round_trip_and_reset(ctx):
    fq = ref.sync_config(48, "re")
    R = 3
    x = ref.make_rows(fq, R, 5, 3, 55, special=True)
    n = x.shape[1]
    pieces = ref.cut(x, [n // 3, n // 4])
    q, pushes, hard, got, end = run_pushes(ctx, fq, pieces, 4, True)
    check_against_program(q, pushes, hard, got, end, 4, expect_frames=R * 5)
    # the state behind the first push, moved into fresh banks
    fs, sf = banks(ctx, fq, R)
    with fs, sf:
        xd = dev(pieces[0])
        fr = fs.push(xd, None, 4)
        sf.push(xd, None, fr[1], fr[2], fr[3], 4)
        mid_fs, mid = fs.state(), sf.state()
        assert mid[0].tolist() == [n // 3] * R and mid[1].shape == (R, q.HF)
        assert np.array_equal(mid[1].view(np.uint32), fsr.floats_of(pieces[0], q).reshape(R, -1)[:, -q.HF:])  # (NaN payloads included)
        sf.reset()
        zero = sf.state()
        assert not zero[0].any() and not zero[1].view(np.uint32).any()
        with pytest.raises(Exception):
            sf.set_state(mid[0][:2], mid[1][:2])
    q, pushes2, hard2, got2, end2 = run_pushes(ctx, fq, pieces[1:], 4, True, state=mid_fs, sf_state=mid)
    check_against_program(q, pushes2, hard2, got2, end2, 4, state=mid)
    for (ya, sa), (yb, sb) in zip(got[1:], got2):
        assert np.array_equal(ya, yb) and np.array_equal(sa, sb)
    assert np.array_equal(end[0], end2[0]) and np.array_equal(end[1].view(np.uint32), end2[1].view(np.uint32))


# ---- 5. forged inputs ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["real", "dibit"])
def test_forged_positions_and_hypotheses(ctx, form):
    """a position before the window, one past it and h = 4 give NaN frames and status 1, 1, 2; positions near 2^64 and a
    forged count likewise; the neighbouring frames stay right"""
    B = 2 if form == "dibit" else 1
    fq = ref.sync_config(64 * B, form)
    q = ref.of_framesync(fq)
    R, cap = 2, 8
    x = ref.make_rows(fq, R, 3, 6, 91, special=True)
    n = x.shape[1]
    a = n // 2
    fs, sf = banks(ctx, fq, R)
    with fs, sf:
        xa, xb = dev(x[:, :a]), dev(x[:, a:])
        fr = fs.push(xa, None, cap)
        sf.push(xa, None, fr[1], fr[2], fr[3], cap)
        frames, pos, info, got = fs.push(xb, None, cap)
        torch.cuda.synchronize()
        pos, info, got = as_bits(pos).copy(), as_bits(info).copy(), as_bits(got).copy()
        real = [int(g) for g in got]
        assert min(real) >= 1
        p0, p1, Ps, Kh = a, n, q.Ps, q.Ps - 1
        forged = [(p0 - Kh - 1, 0), (p1 - Ps + 1, 0), (p0, 4), (2 ** 64 - 1, 0), (2 ** 64 - Kh, 0), (p0 - Kh, 0), (p1 - Ps, 0)]
        want_status = [1, 1, 2, 1, 1, 0, 0]
        for r in range(R):  # behind the row's real frames, which stay
            for j, (s, h) in enumerate(forged[:cap - real[r]]):
                pos[r, real[r] + j], info[r, real[r] + j] = s, h << 8
        got[:] = 0xFFFFFFF0  # (a forged count: clamped to cap)
        out = torch.full((R, cap, q.P), float("inf"), dtype=torch.float32, device="cuda")
        status = torch.full((R, cap), 9, dtype=torch.int32, device="cuda")
        sf.push(xb, None, dev(pos.view(np.int64)), dev(info.view(np.int32)), dev(got.view(np.int32)), cap, out=(out, status))
        torch.cuda.synchronize()
    y, st = as_bits(out), as_bits(status)
    push_b = (x[:, a:], None, got, pos, info)
    state = (np.full(R, a, np.uint64), fsr.floats_of(x[:, :a], q).reshape(R, -1)[:, -q.HF:])
    ((per, _),) = ref.exact(BUILD, [(q, [push_b], cap, state)])
    assert np.array_equal(y, per[0][0]) and np.array_equal(st, per[0][1])
    for r in range(R):
        stream = fsr.floats_of(x[r], q)
        k = cap - real[r]
        assert st[r].tolist() == [0] * real[r] + want_status[:k]
        for f in range(cap):
            if st[r, f] == 0:
                assert np.array_equal(y[r, f], ref.frame(q, stream, pos[r, f], (int(info[r, f]) >> 8) & 0xFF))
            else:
                assert (y[r, f] == ref.QNAN).all()
        assert ref.signs_are_the_packed_bits(y[r, :real[r]], host(frames)[r, :real[r]], q.P)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", [1, 3])
def test_refused_calls_leave_outputs_and_state(hz, ctx, R):
    lib = importlib.import_module("go-sdr_amd._capi").lib
    fq = ref.sync_config(32, "real")
    q = ref.of_framesync(fq)
    cap, P = 2, q.P
    x = ref.make_rows(fq, R, 1, 3, 5)
    n = x.shape[1]
    xd = dev(x)
    out = torch.full((R, cap * P), 7.0, dtype=torch.float32, device="cuda")
    status = torch.full((R, cap), 7, dtype=torch.int32, device="cuda")
    pos, info, got = torch.zeros((R, cap), dtype=torch.int64, device="cuda"), torch.zeros((R, cap), dtype=torch.int32, device="cuda"), \
        torch.ones(R, dtype=torch.int32, device="cuda")
    fs, sf = banks(ctx, fq, R)
    with fs, sf:
        sf.push(xd if R > 1 else xd[0], None, pos[:, :0], info[:, :0], got, 0)  # cap = 0: the history only
        before = sf.state()
        assert before[0].tolist() == [n] * R
        call = lambda *a: ctx._ck(lib.hzsdr_softframe_push(sf._h, *a))
        good = (xd.data_ptr(), n, n, None, pos.data_ptr(), info.data_ptr(), got.data_ptr(), cap, out.data_ptr(), cap * P, status.data_ptr())
        names = ("i", "n", "istride", "ic", "pos", "info", "got", "cap", "o", "ostride", "st")

        def but(**kw):
            return tuple(kw.get(k, g) for k, g in zip(names, good))
        if R > 1:
            with pytest.raises(hz.ErrDstTooSmall):
                call(*but(ostride=cap * P - 1))
            with pytest.raises(hz.ErrInvalidArgument):
                call(*but(istride=n - 1))
        for bad in (but(i=None), but(pos=None), but(info=None), but(got=None), but(o=None), but(st=None), but(cap=hz.SOFTFRAME_MAX_SLOTS // R + 1),
                    but(n=2 ** 31 - 15, istride=2 ** 31 - 15)):
            with pytest.raises(hz.ErrInvalidArgument):
                call(*bad)
        assert lib.hzsdr_softframe_push(None, *good) == hz.ErrInvalidArgument.status
        torch.cuda.synchronize()
        after = sf.state()
        assert (out == 7.0).all() and (status == 7).all()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1].view(np.uint32), after[1].view(np.uint32))
        with pytest.raises(ValueError):
            sf.push(xd if R > 1 else xd[0], None, pos, info, got, cap, out=(out.view(R, cap, P)[:, :, :P - 1], status))
        with pytest.raises(ValueError):
            sf.push(xd if R > 1 else xd[0], None, pos.int(), info, got, cap)
        call(*but(n=0, i=None, istride=0))  # n = 0: nothing ends in the push; the state stays
        torch.cuda.synchronize()
        assert (as_bits(out).reshape(R, cap, P)[:, 0] == ref.QNAN).all() and (as_bits(out).reshape(R, cap, P)[:, 1] == as_bits(np.float32([7.0]))[0]).all()
        assert as_bits(status).tolist() == [[1, 7]] * R
        assert np.array_equal(sf.state()[1].view(np.uint32), before[1].view(np.uint32)) and sf.positions().tolist() == [n] * R


def test_create_errors(hz, ctx):
    lib = importlib.import_module("go-sdr_amd._capi").lib
    out = C.c_void_p()

    def create(kind=hz.SYMSYNC_REAL_F32, B=1, P=8, maps=(0,), rows=1, H=None):
        m = (C.c_uint * max(len(maps), 1))(*maps)
        return lib.hzsdr_softframe_create(ctx._h, kind, B, P, len(maps) if H is None else H, m, rows, C.byref(out))

    inval = hz.ErrInvalidArgument.status
    assert create(kind=hz.FMT_U8) == hz.ErrSampleFormatUnknown.status
    for bad in (dict(rows=0), dict(rows=hz.SOFTFRAME_MAX_ROWS + 1), dict(B=2), dict(B=0), dict(kind=hz.FMT_C64, B=3, P=9), dict(P=0), dict(P=8193),
                dict(kind=hz.FMT_C64, B=2, P=7), dict(H=0), dict(maps=(0, 0, 0, 0, 0)), dict(maps=(2,)), dict(kind=hz.FMT_C64, B=2, maps=(0, 4)),
                dict(kind=hz.FMT_C64, maps=(0, 2))):
        assert create(**bad) == inval, bad
    sets = [ref.Config(P, B, cplx, maps) for P, B, cplx, maps in ((0, 1, False, (0,)), (8, 2, False, (0,)), (8, 2, True, (4,)), (8, 1, True, (2,)), (8193, 1, False, (0,)))]
    assert ref.check(BUILD, sets) == [False] * len(sets)
    for good in (dict(P=1), dict(P=8192, rows=hz.SOFTFRAME_MAX_ROWS), dict(kind=hz.FMT_C64, B=2, P=8192, maps=(3, 2, 1, 0)), dict(kind=hz.FMT_C64, P=5, maps=(1, 0))):
        assert create(**good) == 0 and lib.hzsdr_softframe_free(out) == 0, good
    with ctx.frame_sync(hz.SYMSYNC_REAL_F32, 8, [0xA5], [0], 16, diff=1) as fs, pytest.raises(ValueError):
        ctx.soft_frames(fs)
    with pytest.raises(hz.ErrInvalidArgument):
        hz.SoftFrames(ctx, hz.SYMSYNC_REAL_F32, 8, [0], rows=0)


# ---- 7. the chain and the coding gain -------------------------------------------------------------------------------

SIGMA, FRAMES, ROWS = 0.8, 64, 4
CRC16 = (16, 0x1021, 0xFFFF, 0)


def gaussian(seed, n, sigma):
    """noise of standard deviation sigma: a scaled sum of four uniforms out of util.splitmix64"""
    u = (splitmix64(seed, 4 * n) >> np.uint64(11)).astype(np.float64) / float(1 << 53)
    return (u.reshape(n, 4).sum(axis=1) - 2.0) * np.sqrt(3.0) * sigma


@pytest.fixture(scope="module")
def noisy():
    """64 coded frames (K = 7, rate 1/2, D = 78 with a CRC-16) of unit amplitude behind a clean 32-bit word in ROWS rows,
    noise of sigma 0.8 on the payloads only, and what the reference decoders make of every frame, hard and soft"""
    qh = vr.Config(D=78, crc=CRC16, kind=vr.BITS)
    qs = vr.Config(D=78, crc=CRC16, kind=vr.SOFT_F32, scale=32.0)
    N, per_row = qh.N, FRAMES // ROWS
    assert N == 168
    fq = fsr.Config(32, [ref.WORD32], N)
    lead, gap = 11, 6
    per = 32 + N + gap
    x = np.ones((ROWS, lead + per_row * per + 5), np.float32)
    sent, floats = [], []
    for r in range(ROWS):
        for f in range(per_row):
            k = r * per_row + f
            data = vr.with_crc(qh, vr.random_bits(78 - 16, 9000 + k))
            code = vr.encode(qh, data).astype(np.float64) * 2 - 1
            rx = (code + gaussian(500 + k, N, SIGMA)).astype(np.float32)
            at = lead + f * per
            x[r, at:at + 32] = fsr.word_bits(ref.WORD32, 32).astype(np.float32) * 2 - 1
            x[r, at + 32:at + 32 + N] = rx
            sent.append(data)
            floats.append(rx)
    hard = [vr.decode(qh, np.packbits((f.view(np.uint32) >> np.uint32(31)) ^ np.uint32(1))) for f in floats]
    soft = [vr.decode(qs, f) for f in floats]
    return fq, qh, qs, x, floats, hard, soft, per_row


def chain(hz, ctx, noisy, use_soft):
    st = importlib.import_module("go-sdr_amd.stream")
    fq, qh, qs, x, floats, hard, soft, per_row = noisy
    qv = qs if use_soft else qh
    args, kw = qv.create_args()
    n = x.shape[1]
    xd = dev(x)
    pieces = [xd[:, :n // 3], xd[:, n // 3:n // 2 + 7], xd[:, n // 2 + 7:]]
    fs, sf = banks(ctx, fq, ROWS)
    with fs, sf, ctx.viterbi(*args, rows=ROWS, **kw) as vd:
        parts = list(st.decoded_frames(pieces, fs, vd, cap=per_row, soft=sf if use_soft else None))
    out = []
    for r in range(ROWS):
        row = [(d, int(p), int(m), bool(ok)) for part in parts for d, p, m, ok in zip(part[r][0], part[r][1], part[r][3], part[r][4])]
        assert len(row) == per_row, (r, len(row))
        out += row
    return out


def test_the_chain_equals_the_reference_decoder_of_the_reference_soft_frames(hz, ctx, noisy):
    """stream.decoded_frames(..., soft=...) in a DEVICE context: data, metric and CRC verdict of every frame are
    viterbi_ref.decode's of the whole-stream restatement's soft frame"""
    fq, qh, qs, x, floats, hard, soft, per_row = noisy
    q = ref.of_framesync(fq)
    got = chain(hz, ctx, noisy, True)
    for k, (d, p, m, ok) in enumerate(got):
        r = k // per_row
        frame = ref.frame(q, fsr.floats_of(x[r], q), p, 0)
        assert np.array_equal(frame, floats[k].view(np.uint32)), k
        wd, winfo = soft[k]
        assert np.array_equal(d, wd) and m == winfo & 0x7FFFFFFF and ok == bool(winfo >> 31), k


def test_the_coding_gain(hz, ctx, noisy):
    """CRC-ok frames through the hard chain and through the soft chain: each count is the reference decoder's, and the
    soft chain recovers at least 16 frames of 64 more"""
    fq, qh, qs, x, floats, hard, soft, per_row = noisy
    want_hard, want_soft = sum(i >> 31 for _, i in hard), sum(i >> 31 for _, i in soft)
    got_hard = sum(ok for _, _, _, ok in chain(hz, ctx, noisy, False))
    got_soft = sum(ok for _, _, _, ok in chain(hz, ctx, noisy, True))
    print("CRC-ok frames of", FRAMES, "hard:", got_hard, "(reference", want_hard, ") soft:", got_soft, "(reference", want_soft, ")")
    assert got_hard == want_hard and got_soft == want_soft
    assert got_soft >= got_hard + 16


def test_mismatched_banks_are_refused_before_anything_runs(hz, ctx, noisy):
    st = importlib.import_module("go-sdr_amd.stream")
    fq, qh, qs = noisy[:3]
    fs, sf = banks(ctx, fq, ROWS)
    (sa, skw), (ha, hkw) = qs.create_args(), qh.create_args()
    with fs, sf, ctx.viterbi(*sa, rows=ROWS, **skw) as vs, ctx.viterbi(*ha, rows=ROWS, **hkw) as vh:
        other_rows, other_p = ctx.soft_frames(fs), hz.SoftFrames(ctx, fq.kind, fq.P - 2, fq.maps, rows=ROWS)
        other_rows.rows = ROWS + 1
        other_kind = hz.SoftFrames(ctx, hz.FMT_C64, fq.P, fq.maps, rows=ROWS)
        for bad_soft, vd in ((other_rows, vs), (other_p, vs), (other_kind, vs), (sf, vh)):
            with pytest.raises(ValueError):
                list(st.decoded_frames([], fs, vd, soft=bad_soft))
        with ctx.viterbi(vr.SOFT_F32, 7, vr.K7, 70, rows=ROWS) as short, pytest.raises(ValueError):
            list(st.decoded_frames([], fs, short, soft=sf))
        for b in (other_rows, other_p, other_kind):
            b.close()
        assert list(st.decoded_frames([], fs, vs, soft=sf)) == []


# ---- 8. the other layers --------------------------------------------------------------------------------------------

def _run(exe):
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "go-sdr_amd") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    return subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)


def test_c_softframe_walkthrough(hz):
    """tests/c/test_softframe_abi.c compiled by gcc as C99 and run against libhzsdr_hip.so."""
    exe = os.path.join(BUILD, "test_softframe_abi")
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "test_softframe_abi.c"), "-L" + os.path.join(ROOT, "go-sdr_amd"),
                           "-lhzsdr_hip", "-lm", "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    p = _run(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "softframe-abi ok" in p.stdout


def test_cxx_softframe(hz):
    """tests/cxx/test_softframe.cpp (hzsdr::stream::SoftFrames) built with g++ -Werror and run."""
    exe = os.path.join(BUILD, "test_softframe_cxx")
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + ROOT, os.path.join(ROOT, "tests", "cxx", "test_softframe.cpp"),
                           "-L" + os.path.join(ROOT, "go-sdr_amd"), "-lhzsdr_hip", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    p = _run(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "softframe-cxx ok" in p.stdout

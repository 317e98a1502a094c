"""The AGC bank (include/hzsdr_agc.h) on the GPU, every comparison of outputs, track and state BIT FOR BIT against
tests/host/agc_ref.cpp (the host program over the header the kernel evaluates): rows around the rows-per-wave edges and
samples around the tile edge, both kinds, pitches above the need on the input, the output and the track with sentinels
behind every row's n-th column, both memory spaces; every rows-per-wave the planner has; every template form (kind x
shared / per-row parameters x with / without track); in place; cuts with and without the state carried into a new
object; shared against per-row parameters; new parameters between pushes, reset; a NaN and an infinity kept to their
sample, a NaN gain healed; refusals; the demodulator's and the tuner bank's blocks straight in; the chain tuner -> AGC ->
carrier -> symbol timing at amplitudes 0.05 and 8; the C and C++ layers; a Reader."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import agc_ref as ref
import carrier_ref
import symsync_ref
import tuner_ref
from conftest import ROOT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BUILD = os.path.join(ROOT, "build")
SENTINEL = 0x7F7F7F7F  # (3.39e38: no output and no track value of these tests)
T = 256
# ref, attack, decay, floor, g0, gmin, gmax: white rows of components in [-1, 1) take every branch but the gmax clamp
# under the loud set and that one under the quiet set (tests/test_agc_cpu.py counts them)
PARAMS = ref.LOUD
KINDS = (False, True)  # complex rows?


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


def bits(a):
    return np.ascontiguousarray(host(a)).view(np.uint32)


def kind_of(hz, cplx):
    return hz.FMT_C64 if cplx else hz.AGC_REAL_F32


def rows_of(r, n, seed, cplx):
    return ref.white((n,) if r == 1 else (r, n), seed, cplx)


def per_row_params(r, seed=0):
    """r sets of their own: the loud and the quiet set in turn, rates, gate, start and range differing from row to row"""
    k = (np.arange(r) + seed) % 7
    p = np.where(((np.arange(r) + seed) % 2 == 0)[:, None], ref.LOUD, ref.QUIET).astype(np.float64)
    p[:, 0] *= 1.0 + 0.05 * k
    p[:, 1] *= 1.0 - 0.1 * k
    p[:, 2] *= 1.0 - 0.05 * k
    p[:, 3] += 0.01 * k
    p[:, 4] = 1.0 + 0.1 * (k - 3)
    p[:, 5] -= 0.02 * k
    p[:, 6] += 0.1 * k
    return p.astype(np.float32)


def sentinels(shape, dtype, device):
    words = np.full(shape + ((2,) if dtype == np.complex64 else ()), SENTINEL, np.uint32)
    buf = words.view(dtype).reshape(shape)
    return dev(buf) if device else buf


def pitched(x, pad, device):
    """x (R, n) inside a wider buffer of pitch n + pad (R > 1) -> the view of the rows"""
    if x.ndim == 1:
        return dev(x) if device else x.copy()
    wide = np.zeros((x.shape[0], x.shape[1] + pad), x.dtype)
    wide[:, :x.shape[1]] = x
    wide = dev(wide) if device else wide
    return wide[:, :x.shape[1]]


def run(bank, x, device, track=True, pads=(3, 5, 7)):
    """one push of the rows x (numpy) with pitches above the need on all three sides, into destinations full of
    sentinels -> (the whole output as uint32 words (R, width, 1 or 2), the whole track as words (R, width) or None)"""
    r, n = (1, x.shape[0]) if x.ndim == 1 else x.shape
    w = 2 if np.iscomplexobj(x) else 1
    shape = lambda pad: (n + pad,) if r == 1 else (r, n + pad)
    out = sentinels(shape(pads[1]), x.dtype.type, device)
    tr = sentinels(shape(pads[2]), np.float32, device) if track else None
    got = bank.push(pitched(x, pads[0], device), out=out, track=tr)
    if device:
        torch.cuda.synchronize()
    y = got[0] if track else got
    assert y.shape[-1] == n and (not track or got[1].shape[-1] == n)
    return bits(out).reshape(r, n + pads[1], w), bits(tr).reshape(r, n + pads[2]) if track else None


def check(words, twords, want, what, skip=None):
    """the push's destinations against the program's (y, track, state): equal bits in the first n columns of every row,
    the sentinel in every column behind them.  skip: (row, column) whose output is compared by the caller."""
    y, tr = want[0], want[1]
    n = y.shape[1]
    wy = bits(y).reshape(y.shape[0], n, -1)
    diff = (words[:, :n] != wy).any(axis=2)
    if skip is not None:
        diff[skip] = False
    bad = np.flatnonzero(diff.any(axis=1))
    assert bad.size == 0, f"{what}: outputs differ in {bad.size} rows, the first {int(bad[0])} at column {int(np.flatnonzero(diff[bad[0]])[0])}"
    assert (words[:, n:] == SENTINEL).all(), f"{what}: an output column behind the samples was touched"
    if twords is not None:
        bad = np.flatnonzero((twords[:, :n] != bits(tr)).any(axis=1))
        assert bad.size == 0, f"{what}: the track differs in {bad.size} rows, the first {int(bad[0])}"
        assert (twords[:, n:] == SENTINEL).all(), f"{what}: a track column behind the samples was touched"


def same_state(z, want):
    return np.array_equal(bits(z), bits(want))


# ---- 1. exact streams ------------------------------------------------------------------------------

@pytest.mark.parametrize("space", ["device", "host"])
@pytest.mark.parametrize("cplx", KINDS)
def test_streams_exact(hz, ctx, hctx, space, cplx):
    """R in {1, 3, 64, 1024, 1025, 8192} x n in {1, 255, 256, 257, 773}, white rows, the loud and the quiet set in
    turn, pitches above the need on the input, the output and the track."""
    c = ctx if space == "device" else hctx
    shapes = [(r, n) for r in (1, 3, 64, 1024, 1025, 8192) for n in (1, T - 1, T, T + 1, 3 * T + 5)]
    cases = [((ref.LOUD, ref.QUIET)[k % 2], rows_of(r, n, 1000 * r + n, cplx)) for k, (r, n) in enumerate(shapes)]
    for (p, x), want in zip(cases, ref.exact(BUILD, cases)):
        r = 1 if x.ndim == 1 else x.shape[0]
        with c.agc(kind_of(hz, cplx), p, rows=r) as f:
            g, t, form = f.plan()
            assert g == (r + 1023) // 1024 and t == T and form == (hz.AGC_FORM_COMPLEX if cplx else 0)
            words, twords = run(f, x, space == "device")
            z, pos = f.state()
        what = f"R={r} n={x.shape[-1]} complex {cplx} {space}"
        check(words, twords, want, what)
        assert pos == x.shape[-1] and same_state(z, want[2]), f"{what}: the state differs"


@pytest.mark.parametrize("cplx", KINDS)
def test_every_rows_per_wave(hz, ctx, cplx):
    """The rows-per-wave values 2 ... 8: the smallest bank of each, an odd one whose last wave is short, and the largest;
    T + 1 samples, per-row parameters that differ row by row and mix the loud and the quiet set."""
    seen = set()
    sizes = [1024 * (k - 1) + 1 for k in range(2, 9)] + [5000, hz.AGC_MAX_ROWS - 1, hz.AGC_MAX_ROWS]
    cases = [(per_row_params(r, k), rows_of(r, T + 1, r, cplx)) for k, r in enumerate(sizes)]
    for (p, x), want in zip(cases, ref.exact(BUILD, cases)):
        with ctx.agc(kind_of(hz, cplx), p, rows=x.shape[0], per_row=True) as f:
            seen.add(f.plan()[0])
            words, twords = run(f, x, True)
            z, _ = f.state()
        check(words, twords, want, f"R={x.shape[0]} complex {cplx}")
        assert same_state(z, want[2])
    assert seen == set(range(2, 9)), f"rows per wave seen: {sorted(seen)}"


# ---- 2. every template form, shared against per-row parameters ------------------------------------------

@pytest.mark.parametrize("r", [3, 1025])
@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("per_row", [False, True])
@pytest.mark.parametrize("cplx", KINDS)
def test_every_form(hz, ctx, cplx, per_row, track, r):
    """kind x shared / per-row parameters x with / without track, one row per wave and two; a modulated row at a low
    level beside white ones; per-row parameters of equal values give the shared form's bits, and the outputs and the
    state do not depend on whether the track is asked for."""
    n = 2 * T + 9
    x = rows_of(r, n, 17 * r + cplx, cplx)
    x[0] = ref.noisy_qpsk(n, 0.05, 5) if cplx else ref.noisy_qpsk(n, 0.05, 5).real
    p = per_row_params(r) if per_row else PARAMS
    (want,) = ref.exact(BUILD, [(p, x)])
    with ctx.agc(kind_of(hz, cplx), p, rows=r, per_row=per_row) as f:
        assert f.plan()[2] == (hz.AGC_FORM_PER_ROW if per_row else 0) + (hz.AGC_FORM_COMPLEX if cplx else 0)
        words, twords = run(f, x, True, track=track)
        z, pos = f.state()
    check(words, twords, want, f"complex {cplx} per_row {per_row} track {track} R={r}")
    assert pos == n and same_state(z, want[2])
    if not per_row:
        with ctx.agc(kind_of(hz, cplx), np.broadcast_to(PARAMS, (r, 7)), rows=r, per_row=True) as f:
            words2, twords2 = run(f, x, True, track=track)
            assert np.array_equal(words2, words) and (not track or np.array_equal(twords2, twords)) and same_state(f.state()[0], z)


# ---- 3. in place -----------------------------------------------------------------------------------

@pytest.mark.parametrize("space", ["device", "host"])
@pytest.mark.parametrize("r", [1, 3, 1025])
@pytest.mark.parametrize("cplx", KINDS)
def test_in_place(hz, ctx, hctx, space, r, cplx):
    """out == in, rows of a wider buffer: the out-of-place bits, the columns behind the rows untouched"""
    c, n = (ctx if space == "device" else hctx), 3 * T + 5
    x = rows_of(r, n, 99 + r, cplx)
    (want,) = ref.exact(BUILD, [(PARAMS, x)])
    wide = sentinels((n + 6,) if r == 1 else (r, n + 6), x.dtype.type, False)
    wide[..., :n] = x
    wide = dev(wide) if space == "device" else wide
    view = wide[..., :n]
    kind = kind_of(hz, cplx)
    with c.agc(kind, PARAMS, rows=r) as f, c.agc(kind, PARAMS, rows=r) as g:
        y = f.push(view, out=view)
        apart, tr = g.push(dev(x) if space == "device" else x, track=True)
        if space == "device":
            torch.cuda.synchronize()
        assert (y.data_ptr() == wide.data_ptr()) if space == "device" else (y.ctypes.data == wide.ctypes.data)
        assert same_state(f.state()[0], want[2]) and same_state(g.state()[0], want[2])
    w = 2 if cplx else 1
    check(bits(wide).reshape(r, n + 6, w), None, want, f"in place R={r} {space}")
    assert np.array_equal(bits(apart).reshape(r, n, w), bits(want[0]).reshape(r, n, w)) and np.array_equal(bits(tr).reshape(r, n), bits(want[1]))
    if r > 1 and space == "device":
        lib = importlib.import_module("go-sdr_amd._capi").lib
        with ctx.agc(kind, PARAMS, rows=r) as f, pytest.raises(hz.ErrInvalidArgument):
            d = dev(np.zeros((r, n + 6), x.dtype))
            ctx._ck(lib.hzsdr_agc_push(f._h, d.data_ptr(), n, n + 6, d.data_ptr(), n + 5, None, 0))


# ---- 4. cuts ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("carry", [False, True])
@pytest.mark.parametrize("r", [3, 1025])
@pytest.mark.parametrize("cplx", KINDS)
def test_cuts_bit_identical(hz, ctx, r, carry, cplx):
    """1100 samples as one push against the same stream cut at 1, 255, 256 and 257 samples (and a push of none); with
    `carry`, the state goes through get_state into a NEW object's set_state at every cut."""
    n = 1100
    x = rows_of(r, n, r + n, cplx)
    x[1] = ref.noisy_qpsk(n, 0.3, 8) if cplx else ref.noisy_qpsk(n, 0.3, 8).imag
    ((y, tr, wz),) = ref.exact(BUILD, [(PARAMS, x)])
    dx, kind = dev(x), kind_of(hz, cplx)
    for cut in (1, T - 1, T, T + 1):
        f = ctx.agc(kind, PARAMS, rows=r)
        parts, tracks, done = [], [], 0
        for size in (cut, 0, n - cut):
            s, t = f.push(dx[:, done:done + size], track=True)
            assert s.shape == (r, size) and t.shape == (r, size)
            parts.append(host(s)), tracks.append(host(t))
            done += size
            assert f.position() == done
            if carry:
                z, pos = f.state()
                g = ctx.agc(kind, PARAMS, rows=r)
                g.set_state(z, pos)
                f.close()
                f = g
                assert f.position() == done
        z, pos = f.state()
        f.close()
        assert pos == n and same_state(z, wz), f"cut {cut}"
        assert np.array_equal(bits(np.hstack(parts)), bits(y)) and np.array_equal(bits(np.hstack(tracks)), bits(tr)), f"cut {cut}"


# ---- 5. new parameters, reset ------------------------------------------------------------------------

@pytest.mark.parametrize("per_row", [False, True])
@pytest.mark.parametrize("cplx", KINDS)
def test_set_params_and_reset(hz, ctx, per_row, cplx):
    """set_params between two pushes keeps g (the restatement that exchanges the parameters at that sample, state kept;
    the new range holds BEHIND the next sample); refused parameters change nothing; reset restores g0."""
    r, k, n = 5, T + 3, 2 * T + 11
    a = per_row_params(r) if per_row else PARAMS.copy()
    b = a.copy()
    b[..., 0], b[..., 1], b[..., 5], b[..., 6], b[..., 4] = a[..., 0] * 3.0, a[..., 1] * 0.5, 0.875, 1.125, 1.0
    x = rows_of(r, n, 11, cplx)
    ((y, tr, wz),) = ref.exact(BUILD, [([(0, a), (k, b)], x)])
    (first,) = ref.exact(BUILD, [(a, x[:, :k])])
    with ctx.agc(kind_of(hz, cplx), a, rows=r, per_row=per_row) as f:
        dx = dev(x)
        head, thead = f.push(dx[:, :k], track=True)
        z0, _ = f.state()
        assert same_state(z0, first[2]) and (z0 < 0.875).any()
        bad = b.copy()
        bad[..., 1] = 0.6  # attack above 0.5
        with pytest.raises(hz.ErrInvalidArgument):
            f.set_params(bad)
        with pytest.raises(hz.ErrInvalidArgument):
            f.set_params(b[None] if not per_row else b[0])
        f.set_params(b)
        z1, p1 = f.state()
        assert p1 == k and same_state(z1, z0), "set_params touched the gains"
        tail, ttail = f.push(dx[:, k:], track=True)
        z, pos = f.state()
        assert pos == n and same_state(z, wz)
        assert np.array_equal(bits(np.hstack([host(head), host(tail)])), bits(y)) and np.array_equal(bits(np.hstack([host(thead), host(ttail)])), bits(tr))
        tt = host(ttail)
        assert same_state(tt[:, 0], z0) and tt[:, 1:].min() >= 0.875 and tt[:, 1:].max() <= 1.125
        # reset: position 0, g0 of the parameters in force; with the first parameters, the first stream again
        f.reset()
        z, pos = f.state()
        assert pos == 0 and np.array_equal(z, np.broadcast_to(b, (r, 7))[:, 4])
        f.set_params(a)
        f.reset()
        again = f.push(dx[:, :k])
        assert np.array_equal(bits(again), bits(head)) and same_state(f.state()[0], z0)


# ---- 6. isolation ----------------------------------------------------------------------------------

@pytest.mark.parametrize("cplx", KINDS)
def test_nan_and_infinity_stay_in_their_sample(hz, ctx, cplx):
    """A NaN in one sample of one row and an infinity in one of another, 2047 rows (two per wave): every other row is
    bit-equal, and so is every other sample of the two rows, the track and the state: the gain behind the NaN is that
    of the row with a sample that holds the gain (one under the gate) in its place.  (Which NaN the bad sample's output
    is is not part of the contract.)  Then a NaN gain: its row is NaN, the others are not; set_state heals it."""
    r, n, nan_row, inf_row = 2047, T + 40, 5, 1024
    x = rows_of(r, n, 31, cplx)
    bad, held = x.copy(), x.copy()
    bad[nan_row, 10] = complex(np.nan, 0.25) if cplx else np.nan
    bad[inf_row, T + 3] = complex(0.5, -np.inf) if cplx else -np.inf
    held[nan_row, 10] = 0.0  # (under the loud set's floor of 0.2: s = 0, as for the NaN)
    want, wheld = ref.exact(BUILD, [(PARAMS, bad), (PARAMS, held)])
    kind = kind_of(hz, cplx)
    with ctx.agc(kind, PARAMS, rows=r) as f:
        words, twords = run(f, bad, True)
        z, _ = f.state()
        got = words[:, :n].copy().view(np.float32)
        for row, col in ((nan_row, 10), (inf_row, T + 3)):
            w = np.atleast_1d(want[0][row, col:col + 1].view(np.float32))
            for g, v in zip(got[row, col], w):
                assert (np.isnan(g) and np.isnan(v)) or g == v, f"row {row}: {g} for {v}"
            words[row, col] = bits(want[0][row, col:col + 1])
        assert np.isnan(got[nan_row, 10]).any() and not np.isfinite(got[inf_row, T + 3]).all()
        check(words, twords, want, f"beside a NaN and an infinity, complex {cplx}")
        assert same_state(z, want[2]) and same_state(z[nan_row], wheld[2][nan_row])
        assert np.array_equal(twords[nan_row, :n], bits(wheld[1][nan_row]))
        assert np.isfinite(twords[:, :n].view(np.float32)).all()
        # a NaN gain stays, and stays in its row; set_state heals it
        sick = z.copy()
        sick[nan_row] = np.nan
        f.set_state(sick, n)
        (wsick,) = ref.exact(BUILD, [(PARAMS, x, sick)])
        y, tr = f.push(dev(x), track=True)
        y, tr, z2 = host(y), host(tr), f.state()[0]
        assert np.isnan(y[nan_row].view(np.float32)).all() and np.isnan(tr[nan_row]).all() and np.isnan(z2[nan_row])
        rest = np.arange(r) != nan_row
        assert np.array_equal(bits(y[rest]), bits(wsick[0][rest])) and np.array_equal(bits(tr[rest]), bits(wsick[1][rest])) and same_state(z2[rest], wsick[2][rest])
        f.set_state(z, n)
        (wwell,) = ref.exact(BUILD, [(PARAMS, x, z)])
        y, tr = f.push(dev(x), track=True)
        assert np.array_equal(bits(y), bits(wwell[0])) and np.array_equal(bits(tr), bits(wwell[1])) and same_state(f.state()[0], wwell[2])


# ---- 7. refusals -----------------------------------------------------------------------------------

@pytest.mark.parametrize("r", [1, 3])
def test_refused_pushes_leave_the_state(hz, ctx, r):
    """pitches below n and null pointers are refused before anything runs: the next push continues the stream"""
    lib = importlib.import_module("go-sdr_amd._capi").lib
    n = 300
    x = rows_of(3, 2 * n, 5, True)[:r]
    ((y, tr, wz),) = ref.exact(BUILD, [(PARAMS, x)])
    dx = dev(x)
    with ctx.agc(hz.FMT_C64, PARAMS, rows=r) as f:
        head = f.push(dx[:, :n] if r > 1 else dx[0, :n])
        z0, p0 = f.state()
        out = torch.zeros((r, n), dtype=torch.complex64, device="cuda")
        trk = torch.zeros((r, n), dtype=torch.float32, device="cuda")
        part = dx[:, n:].contiguous()
        push = lambda *a: ctx._ck(lib.hzsdr_agc_push(f._h, *a))
        if r > 1:
            with pytest.raises(hz.ErrDstTooSmall):
                push(part.data_ptr(), n, n, out.data_ptr(), n - 1, None, 0)
            with pytest.raises(hz.ErrDstTooSmall):
                push(part.data_ptr(), n, n, out.data_ptr(), n, trk.data_ptr(), n - 1)
            with pytest.raises(hz.ErrInvalidArgument):
                push(part.data_ptr(), n, n - 1, out.data_ptr(), n, None, 0)
        with pytest.raises(hz.ErrInvalidArgument):
            push(None, n, n, out.data_ptr(), n, None, 0)
        with pytest.raises(hz.ErrInvalidArgument):
            push(part.data_ptr(), n, n, None, n, None, 0)
        assert lib.hzsdr_agc_push(None, part.data_ptr(), n, n, out.data_ptr(), n, None, 0) == hz.ErrInvalidArgument.status
        torch.cuda.synchronize()
        z1, p1 = f.state()
        assert p1 == p0 == n and same_state(z1, z0) and not out.any() and not trk.any()
        push(part.data_ptr(), n, n, out.data_ptr(), n, trk.data_ptr(), n)
        z, pos = f.state()
        assert pos == 2 * n and same_state(z, wz)
        assert np.array_equal(bits(np.hstack([host(head).reshape(r, n), host(out)])), bits(y)) and np.array_equal(bits(trk), bits(tr[:, n:]))
        if r > 1:
            with pytest.raises(hz.ErrDstTooSmall):
                ctx._ck(lib.hzsdr_agc_get_state(f._h, (C.c_float * (r - 1))(), r - 1))
        with pytest.raises(hz.ErrInvalidArgument):
            ctx._ck(lib.hzsdr_agc_set_state(f._h, (C.c_float * (r + 1))(), r + 1, 0))
        assert same_state(f.state()[0], wz)


def test_create_errors(hz, ctx):
    lib = importlib.import_module("go-sdr_amd._capi").lib
    out = C.c_void_p()

    def create(kind, p, per_row=0, rows=1):
        ptr = p.ctypes.data_as(C.POINTER(C.c_float)) if p is not None else None
        return lib.hzsdr_agc_create(ctx._h, kind, ptr, per_row, rows, C.byref(out))

    inval = hz.ErrInvalidArgument.status
    assert create(hz.FMT_C64, PARAMS, 0, 0) == inval and create(hz.FMT_C64, PARAMS, 0, hz.AGC_MAX_ROWS + 1) == inval
    assert create(hz.FMT_C64, None) == inval
    for kind in (-1, 0, hz.FMT_U8, hz.FMT_I16, 31, 33):
        assert create(kind, PARAMS) == hz.ErrSampleFormatUnknown.status, f"kind {kind}"
    up = lambda v: np.nextafter(np.float32(v), np.float32(np.inf))
    down = lambda v: np.nextafter(np.float32(v), np.float32(-np.inf))
    for k, v in ((0, down(2.0 ** -64)), (0, up(2.0 ** 64)), (0, np.nan), (1, up(0.5)), (1, down(0.0)), (1, np.inf), (2, up(0.5)), (2, down(0.0)),
                 (2, np.nan), (3, down(0.0)), (3, np.inf), (4, 0.4), (4, 2.5), (4, np.nan), (5, down(2.0 ** -64)), (5, 1.5), (5, -np.inf),
                 (6, up(2.0 ** 64)), (6, 0.75), (6, np.nan)):
        p = PARAMS.copy()
        p[k] = v
        assert create(hz.FMT_C64, p) == inval, f"parameter {k} = {v}"
    lo, hi = 2.0 ** -64, 2.0 ** 64
    for p in ([lo, 0.5, 0.5, 0, lo, lo, lo], [hi, 0, 0, 3e38, hi, hi, hi], [1, 0, 0, 0, 1, lo, hi]):
        assert create(hz.AGC_REAL_F32, np.array(p, np.float32)) == 0 and lib.hzsdr_agc_free(out) == 0, p
    per = np.broadcast_to(PARAMS, (3, 7)).copy()
    per[2, 1] = 0.6
    assert create(hz.FMT_C64, per, 1, 3) == inval, "a refused parameter of the last row"
    assert create(hz.FMT_C64, PARAMS, 0, hz.AGC_MAX_ROWS) == 0 and lib.hzsdr_agc_free(out) == 0
    with pytest.raises(hz.ErrInvalidArgument):
        ctx.agc(hz.FMT_C64, np.ones((2, 7), np.float32), rows=3, per_row=True)
    with pytest.raises(hz.ErrInvalidArgument):
        ctx.agc(hz.FMT_C64, np.ones((3, 7), np.float32), rows=3)
    with ctx.agc(hz.AGC_REAL_F32, PARAMS) as f, pytest.raises(ValueError):
        f.push(dev(rows_of(1, 8, 1, True)))


# ---- 8. straight in, the chain -----------------------------------------------------------------------

def test_the_demodulator_and_the_tuner_bank_straight_in(hz, ctx):
    """The envelope demodulator's PITCHED float32 block (the same pointer, a pitch above the count) goes into a real
    bank as it is, the tuner bank's complex64 block into a complex one; both against the program over the same block."""
    r, n = 12, 1000
    x = np.stack([ref.noisy_qpsk(n, 0.01 * 3.0 ** i, 60 + i) for i in range(r)])
    p = np.array([1.0, 0.1, 0.01, 1e-4, 1.0, 2.0 ** -12, 2.0 ** 12], np.float32)
    with ctx.demodulator(hz.FMT_C64, hz.DEMOD_ENVELOPE, streams=r) as dm, ctx.agc(hz.AGC_REAL_F32, p, rows=r) as f:
        block = torch.zeros((r, n + 9), dtype=torch.float32, device="cuda")
        d = dm.push(dev(x), out=block)
        assert d.shape[0] == r and d.stride(0) == n + 9 and d.data_ptr() == block.data_ptr()
        y, tr = f.push(d, track=True)
        z = f.state()[0]
    (want,) = ref.exact(BUILD, [(p, host(d))])
    assert np.array_equal(bits(y), bits(want[0])) and np.array_equal(bits(tr), bits(want[1])) and same_state(z, want[2])
    wide, words, h, _ = ref.two_channels(300, (0.002, -0.003), (0.05, 8.0), 40)
    with ctx.tuner_bank(hz.FMT_C64, words, h, 4) as tb, ctx.agc(hz.FMT_C64, p, rows=2) as f:
        block = tb.push(dev(wide))
        y, tr = f.push(block, track=True)
        z = f.state()[0]
    (want,) = ref.exact(BUILD, [(p, host(block))])
    assert block.shape[0] == 2 and np.array_equal(bits(y), bits(want[0])) and np.array_equal(bits(tr), bits(want[1])) and same_state(z, want[2])


def test_the_chain_at_amplitudes_0_05_and_8(hz, ctx):
    """The carrier test's two QPSK channels (0.002 and -0.003 cycles per sample off) at amplitudes 0.05 and 8 out of one
    stream: tuner_bank, then agc_rows -> carrier_rows -> symbol_rows on the device, each block going into the next as
    it is.  The soft symbols are bit-equal to the four host programs chained.  The spread of the fourth power of the
    last quarter's symbols is at most TWICE that of the same channels at unit amplitude without the AGC (the three
    host programs): the gain's ripple adds amplitude noise and the residual level error moves the loop gains, hence the
    margin; without the AGC the two channels do not lock at these amplitudes (the spread goes all round, about six
    times the locked figure), so the assertion separates.
    Measured: with the AGC 0.507 and 0.471 rad, at unit amplitude 0.505 and 0.497 rad; at 0.05 and 8 without the AGC
    3.113 and 1.222 rad."""
    st = importlib.import_module("go-sdr_amd.stream")
    offsets, down, sps = (0.002, -0.003), 4, 5.0
    p = np.array([*carrier_ref.gains(0.01), 0.0, -0.01, 0.01], np.float32)
    sp = np.array([sps, 0.01, *hz.loop_gains(sps)], np.float32)
    ap = np.array([1.0, 0.05, 0.005, 0.0, 1.0, 2.0 ** -10, 2.0 ** 10], np.float32)

    def host_chain(amplitudes, agc):
        x, words, h, _ = ref.two_channels(1500, offsets, amplitudes, 40, sps=5, down=down)
        n = -(-len(x) // down)
        ((tuned, _, _),) = tuner_ref.exact(BUILD, [(words, down, h, x, None)])
        t = tuned[:, :n]
        if agc:
            ((t, _, _),) = ref.exact(BUILD, [(ap, t)])
        ((derot, _, _),) = carrier_ref.exact(BUILD, [(carrier_ref.QPSK, p, t)])
        ((s, cnt, _, _),) = symsync_ref.exact(BUILD, [(sp, derot)])
        return x, words, h, s, cnt

    spread = lambda s, cnt, k: carrier_ref.phase_spread(carrier_ref.QPSK, s[k][3 * int(cnt[k]) // 4:int(cnt[k])])
    x, words, h, want, wcnt = host_chain((0.05, 8.0), True)
    _, _, _, unit, ucnt = host_chain((1.0, 1.0), False)
    _, _, _, loose, lcnt = host_chain((0.05, 8.0), False)
    with ctx.tuner_bank(hz.FMT_C64, words, h, down) as tb, ctx.agc(hz.FMT_C64, ap, rows=2) as ag, \
            ctx.carrier_loop(hz.CARRIER_QPSK, p, rows=2) as cr, ctx.symbol_sync(hz.FMT_C64, sp, rows=2) as ts:
        dx = dev(x)
        cuts = (0, 4 * 700, 4 * 701, len(x))
        blocks = (tb.push(dx[a:b]) for a, b in zip(cuts, cuts[1:]))
        parts = [ts.ragged(s, c) for s, c in st.symbol_rows(st.carrier_rows(st.agc_rows(blocks, ag), cr), ts)]
    got = [np.concatenate([host(part[k]) for part in parts]) for k in range(2)]
    for k in range(2):
        cnt = int(wcnt[k])
        assert len(got[k]) == cnt and np.array_equal(bits(got[k]), bits(want[k, :cnt]))
        with_agc, at_unit, without = spread(got, wcnt, k), spread(unit, ucnt, k), spread(loose, lcnt, k)
        print(f"channel {k}: spread of the fourth power {with_agc:.3f} rad with the AGC, {at_unit:.3f} at unit amplitude, {without:.3f} without the AGC")
        assert with_agc <= 2.0 * at_unit
        assert at_unit < np.pi / 2 and without > 2.0 * at_unit


# ---- 9. the other layers ---------------------------------------------------------------------------

def _run(exe):
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "go-sdr_amd") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    return subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)


def test_c_agc_walkthrough(hz):
    """tests/c/test_agc_abi.c compiled by gcc as C99 and run against libhzsdr_hip.so."""
    exe = os.path.join(BUILD, "test_agc_abi")
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "test_agc_abi.c"), "-L" + os.path.join(ROOT, "go-sdr_amd"),
                           "-lhzsdr_hip", "-lm", "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    p = _run(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "agc-abi ok" in p.stdout


def test_cxx_agc(hz):
    """tests/cxx/test_agc.cpp (hzsdr::stream::Agc of go-sdr_amd/cxx/hzsdr.hpp) built with g++ and run."""
    exe = os.path.join(BUILD, "test_agc_cxx")
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + ROOT, os.path.join(ROOT, "tests", "cxx", "test_agc.cpp"),
                           "-L" + os.path.join(ROOT, "go-sdr_amd"), "-lhzsdr_hip", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    p = _run(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "agc-cxx ok" in p.stdout


def test_agc_rows_over_a_reader(hz, hctx):
    """stream.agc_rows over a BufferReader with short reads is one push of the whole stream; fed with an iterable of
    blocks, it takes them as they are (real blocks too); a Reader of another format, or a real bank, is refused."""
    st = importlib.import_module("go-sdr_amd.stream")
    p = np.array([1.0, 0.1, 0.01, 1e-4, 1.0, 2.0 ** -12, 2.0 ** 12], np.float32)
    x = ref.noisy_qpsk(5000, 0.03, 3, sps=5)
    ((y, _, wz),) = ref.exact(BUILD, [(p, x)])
    with hctx.agc(hz.FMT_C64, p) as f:
        blocks = [np.array(b) for b in st.agc_rows(st.BufferReader(x, 48_000, max_read=777), f, block=1024)]
        assert f.position() == len(x) and same_state(f.state()[0], wz)
    got = np.concatenate(blocks)
    assert len(blocks) > 3 and got.dtype == np.complex64 and np.array_equal(bits(got), bits(y[0]))
    xr = np.ascontiguousarray(x.real)
    ((yr, _, wzr),) = ref.exact(BUILD, [(p, xr)])
    with hctx.agc(hz.AGC_REAL_F32, p) as f:
        got = np.concatenate([np.array(b) for b in st.agc_rows((xr[i:i + 1000] for i in range(0, 5000, 1000)), f)])
        assert got.dtype == np.float32 and np.array_equal(bits(got), bits(yr[0])) and same_state(f.state()[0], wzr)
        with pytest.raises(hz.ErrSampleFormatMismatch):
            list(st.agc_rows(st.BufferReader(x, 48_000), f))
    u8 = np.zeros((64, 2), np.uint8)
    with hctx.agc(hz.FMT_C64, p) as f, pytest.raises(hz.ErrSampleFormatMismatch):
        list(st.agc_rows(st.BufferReader(u8, 48_000), f))

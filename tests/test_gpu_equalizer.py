"""The equalizer bank (include/hzsdr_equalizer.h) on the GPU, every comparison of outputs, track and state BIT FOR BIT
against tests/host/equalizer_ref.cpp (the host program over the header the kernel evaluates): rows around the
rows-per-wave edges and symbols around the tile edge with the tap counts around every lanes-per-row step, both kinds,
pitches above the need on the input, the output and the track with sentinels behind every row's count, both memory
spaces; every template form (kind x shared / per-row parameters x with / without track); ragged counts mixed inside one
wave; in place; cuts, pushes shorter than N - 1 and of 0 included, with and without the state carried into a new
object; shared against per-row parameters; new parameters between pushes, reset; a NaN row beside clean rows of the same
wave; refusals; the convergence case; the chain symbol timing -> equalizer -> frame sync with no host read between the
stages; the C and C++ layers; a Reader.

The rows of a large bank repeat a small set of distinct rows (row r is row r % D of the set, D coprime to the rows per
wave), so that the host program runs D rows and not 8192: the results do not depend on the other rows."""
import ctypes as C
import importlib
import math
import os
import subprocess

import numpy as np
import pytest

import equalizer_ref as ref
import framesync_ref
import symsync_ref
from conftest import ROOT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BUILD = os.path.join(ROOT, "build")
SENTINEL = 0x7F7F7F7F  # (3.39e38: no output and no track value of these tests)
T = 256
D = 35  # distinct rows of a large bank: coprime to every rows-per-wave, a multiple of the 5 counts of the ragged test
KINDS = (False, True)  # complex rows?
TAPS = (1, 3, 8, 9, 32, 33, 64)
f32 = np.float32


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
    return hz.FMT_C64 if cplx else hz.EQUALIZER_REAL_F32


def mode_of(k, cplx):
    return (ref.CMA, ref.DD_BPSK, ref.DD_QPSK)[k % 3] if cplx else (ref.CMA, ref.DD_BPSK)[k % 2]


def params_of(mode, rows=None, seed=0):
    """a step large enough for the taps to move within a tile; per row (rows given): steps and levels of their own"""
    base = np.array([0.05, 0.6 if mode == ref.CMA else 0.5], f32)
    if rows is None:
        return base
    k = (np.arange(rows) + seed) % 7
    return np.stack([base[0] * (1.0 + 0.1 * k), base[1] * (1.0 - 0.03 * k)], axis=1).astype(f32)


def distinct_rows(r, n, seed, cplx):
    """min(r, D) distinct white rows"""
    return ref.white((min(r, D), n), seed, cplx, 0.9)


def tiled(a, r):
    """row k of the result is row k % len(a) of a"""
    return a if len(a) == r else a[np.arange(r) % len(a)]


def sentinels(shape, dtype, device):
    words = np.full(shape + ((2,) if dtype == np.complex64 else ()), SENTINEL, np.uint32)
    buf = words.view(dtype).reshape(shape)
    return dev(buf) if device else buf


def pitched(x, pad, device):
    """x (R, n) inside a wider buffer of pitch n + pad -> the view of the rows"""
    wide = np.zeros((x.shape[0], x.shape[1] + pad), x.dtype)
    wide[:, :x.shape[1]] = x
    wide = dev(wide) if device else wide
    return wide[:, :x.shape[1]]


def run(bank, x, device, counts=None, track=True, pads=(3, 5, 7)):
    """one push of the rows x (numpy (R, n)) with pitches above the need on all three sides, into destinations full of
    sentinels -> (the whole output as uint32 words (R, width, 1 or 2), the whole track as words (R, width) or None)"""
    r, n = x.shape
    w = 2 if np.iscomplexobj(x) else 1
    out = sentinels((r, n + pads[1]), x.dtype.type, device)
    tr = sentinels((r, n + pads[2]), np.float32, device) if track else None
    src = pitched(x, pads[0], device)
    if r == 1:
        src, out, tr = src[0], out[0], (tr[0] if track else None)
    if counts is not None:
        counts = dev(counts.view(np.int32)) if device else counts
    got = bank.push(src, counts, out=out, track=tr)
    if device:
        torch.cuda.synchronize()
    y = got[0] if track else got
    assert y.shape[-1] == n and (not track or got[1].shape[-1] == n)
    return bits(out).reshape(r, n + pads[1], w), bits(tr).reshape(r, n + pads[2]) if track else None


def check(words, twords, want, what, counts=None):
    """the push's destinations against the program's (y, track, state) of the DISTINCT rows: equal bits in the columns
    of every row up to its count, the sentinel in every column behind it"""
    r = words.shape[0]
    y, tr = tiled(want[0], r), tiled(want[1], r)
    n = y.shape[1]
    cnt = np.full(r, n) if counts is None else np.minimum(counts.astype(np.int64), n)
    live = np.arange(words.shape[1])[None, :] < cnt[:, None]
    wy = np.full(words.shape, SENTINEL, np.uint32)
    wy[:, :n][live[:, :n]] = bits(y).reshape(r, n, -1)[live[:, :n]]
    bad = np.flatnonzero((words != wy).any(axis=(1, 2)))
    assert bad.size == 0, f"{what}: outputs differ in {bad.size} rows, the first {int(bad[0])} at column {int(np.flatnonzero((words[bad[0]] != wy[bad[0]]).any(axis=1))[0])}"
    if twords is not None:
        live = np.arange(twords.shape[1])[None, :] < cnt[:, None]
        wt = np.full(twords.shape, SENTINEL, np.uint32)
        wt[:, :n][live[:, :n]] = bits(tr)[live[:, :n]]
        bad = np.flatnonzero((twords != wt).any(axis=1))
        assert bad.size == 0, f"{what}: the track differs in {bad.size} rows, the first {int(bad[0])}"


def same_state(z, want):
    return np.array_equal(bits(z), bits(tiled(want, len(z))))


# ---- 1. exact streams ------------------------------------------------------------------------------

def stream_shapes():
    shapes, k = [], 0
    for r in (1, 2, 1024, 1025, 2049, 8192):
        for slot in range(6):
            taps = TAPS[k % len(TAPS)]
            n = (1, max(taps - 2, 0), T - 1, T, T + 1, 2 * T + 1)[slot]
            k += 1
            if r >= 1024 and n > T + 1:
                continue
            shapes.append((r, n, taps))
    return shapes


@pytest.mark.parametrize("space", ["device", "host"])
@pytest.mark.parametrize("cplx", KINDS)
def test_streams_exact(hz, ctx, hctx, space, cplx):
    """R in {1, 2, 1024, 1025, 2049, 8192} x n in {1, N - 2, 255, 256, 257, 513} (the large R: n <= 257), N cycled over
    {1, 3, 8, 9, 32, 33, 64} and the modes in turn, white rows, pitches above the need on the input, the output and the
    track."""
    c = ctx if space == "device" else hctx
    shapes = stream_shapes()
    assert {s[2] for s in shapes} == set(TAPS) and {(s[0], s[2]) for s in shapes} >= {(8192, 64), (8192, 8), (1, 1), (1, 33)}
    cases = [(mode_of(k, cplx), taps, taps // 2, params_of(mode_of(k, cplx)), distinct_rows(r, n, 1000 * r + n, cplx)) for k, (r, n, taps) in enumerate(shapes)]
    for (r, n, taps), case, want in zip(shapes, cases, ref.exact(BUILD, cases)):
        mode, _, centre, p, x = case
        lanes = ref.pow2_up(taps)
        with c.equalizer(kind_of(hz, cplx), mode, taps, centre, p, rows=r) as f:
            g, t, form = f.plan()
            assert g == min(8, 64 // lanes, (r + 1023) // 1024) and t == T and form == (hz.EQUALIZER_FORM_COMPLEX if cplx else 0)
            what = f"R={r} n={n} taps={taps} mode={mode} complex {cplx} {space}"
            if n:
                words, twords = run(f, tiled(x, r), space == "device")
                check(words, twords, want, what)
            else:
                f.push((dev if space == "device" else np.asarray)(tiled(x, r) if r > 1 else x[0]))
            assert same_state(f.state(), want[2]), f"{what}: the state differs"


# ---- 2. every template form, shared against per-row parameters ------------------------------------------

@pytest.mark.parametrize("r", [3, 2049])
@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("per_row", [False, True])
@pytest.mark.parametrize("cplx", KINDS)
def test_every_form(hz, ctx, cplx, per_row, track, r):
    """kind x shared / per-row parameters x with / without track, one row per wave and three, 11 taps; per-row
    parameters of equal values give the shared form's bits, and the outputs and the state do not depend on whether the
    track is asked for."""
    n, taps, mode = T + 9, 11, ref.DD_QPSK if cplx else ref.CMA
    x = distinct_rows(r, n, 17 * r + cplx, cplx)
    p = params_of(mode, len(x)) if per_row else params_of(mode)
    (want,) = ref.exact(BUILD, [(mode, taps, 5, p, x)])
    with ctx.equalizer(kind_of(hz, cplx), mode, taps, 5, tiled(p, r) if per_row else p, rows=r, per_row=per_row) as f:
        assert f.plan()[2] == (hz.EQUALIZER_FORM_PER_ROW if per_row else 0) + (hz.EQUALIZER_FORM_COMPLEX if cplx else 0)
        words, twords = run(f, tiled(x, r), True, track=track)
        z = f.state()
    check(words, twords, want, f"complex {cplx} per_row {per_row} track {track} R={r}")
    assert same_state(z, want[2])
    if not per_row:
        with ctx.equalizer(kind_of(hz, cplx), mode, taps, 5, np.broadcast_to(p, (r, 2)), rows=r, per_row=True) as f:
            words2, twords2 = run(f, tiled(x, r), True, track=track)
            assert np.array_equal(words2, words) and (not track or np.array_equal(twords2, twords)) and np.array_equal(bits(f.state()), bits(z))


# ---- 3. ragged counts ------------------------------------------------------------------------------

@pytest.mark.parametrize("space", ["device", "host"])
@pytest.mark.parametrize("cplx", KINDS)
def test_ragged_counts_inside_one_wave(hz, ctx, hctx, space, cplx):
    """counts of 0, 1, n - 1, n and n + 5 (clamped) in turn over the rows of banks whose waves own 8, 2 and 1 rows: every
    row consumes its own count, the columns behind it keep the sentinel, the counts are not rewritten"""
    c = ctx if space == "device" else hctx
    n = T + 40
    for r, taps in ((8192, 8), (2049, 32), (5, 64)):
        mode = mode_of(taps, cplx)
        x = distinct_rows(r, n, r + taps, cplx)
        choice = np.array([0, 1, n - 1, n, n + 5], np.uint32)
        counts = choice[np.arange(len(x)) % 5]
        (want,) = ref.exact(BUILD, [(mode, taps, 0, params_of(mode), x, None, counts)])
        with c.equalizer(kind_of(hz, cplx), mode, taps, 0, params_of(mode), rows=r) as f:
            all_counts = np.ascontiguousarray(tiled(counts, r))
            before = all_counts.copy()
            words, twords = run(f, tiled(x, r), space == "device", counts=all_counts)
            check(words, twords, want, f"ragged R={r} taps={taps} complex {cplx} {space}", counts=all_counts)
            assert same_state(f.state(), want[2]) and np.array_equal(all_counts, before)


# ---- 4. in place -----------------------------------------------------------------------------------

@pytest.mark.parametrize("space", ["device", "host"])
@pytest.mark.parametrize("r", [1, 3, 1025])
@pytest.mark.parametrize("cplx", KINDS)
def test_in_place(hz, ctx, hctx, space, r, cplx):
    """out == in, rows of a wider buffer: the out-of-place bits, the columns behind the rows untouched"""
    c, n, taps, mode = (ctx if space == "device" else hctx), 2 * T + 5, 17, ref.CMA
    x = distinct_rows(r, n, 99 + r, cplx)
    (want,) = ref.exact(BUILD, [(mode, taps, 8, params_of(mode), x)])
    wide = sentinels((r, n + 6), x.dtype.type, False)
    wide[:, :n] = tiled(x, r)
    wide = dev(wide) if space == "device" else wide
    view = wide[:, :n] if r > 1 else wide[0, :n]
    with c.equalizer(kind_of(hz, cplx), mode, taps, 8, params_of(mode), rows=r) as f:
        y = f.push(view, out=view)
        if space == "device":
            torch.cuda.synchronize()
        assert (y.data_ptr() == wide.data_ptr()) if space == "device" else (y.ctypes.data == wide.ctypes.data)
        assert same_state(f.state(), want[2])
    check(bits(wide).reshape(r, n + 6, 2 if cplx else 1), None, want, f"in place R={r} {space}")
    if r > 1 and space == "device":
        lib = importlib.import_module("go-sdr_amd._capi").lib
        with ctx.equalizer(kind_of(hz, cplx), mode, taps, 8, params_of(mode), rows=r) as f, pytest.raises(hz.ErrInvalidArgument):
            d = dev(np.zeros((r, n + 6), x.dtype))
            ctx._ck(lib.hzsdr_equalizer_push(f._h, d.data_ptr(), n, n + 6, None, d.data_ptr(), n + 5, None, 0))


# ---- 5. cuts ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("carry", [False, True])
@pytest.mark.parametrize("r,taps", [(3, 33), (1025, 9)])
@pytest.mark.parametrize("cplx", KINDS)
def test_cuts_bit_identical(hz, ctx, r, taps, carry, cplx):
    """700 symbols as one push against the same stream in pushes of 1, 0, N - 2, 3, 255 and the rest, and of 256, 257 and
    the rest; with `carry`, the state goes through state() into a NEW object's set_state at every cut."""
    n, mode = 700, ref.DD_BPSK
    x = distinct_rows(r, n, r + n, cplx)
    ((y, tr, wz),) = ref.exact(BUILD, [(mode, taps, 1, params_of(mode), x)])
    dx, kind = dev(tiled(x, r)), kind_of(hz, cplx)
    for sizes in ((1, 0, taps - 2, 3, T - 1), (T, T + 1)):
        f = ctx.equalizer(kind, mode, taps, 1, params_of(mode), rows=r)
        parts, tracks, done = [], [], 0
        for size in sizes + (n - sum(sizes),):
            s, t = f.push(dx[:, done:done + size], track=True)
            assert s.shape == (r, size) and t.shape == (r, size)
            parts.append(host(s)), tracks.append(host(t))
            done += size
            if carry:
                g = ctx.equalizer(kind, mode, taps, 1, params_of(mode), rows=r)
                g.set_state(f.state())
                f.close()
                f = g
        z = f.state()
        f.close()
        assert same_state(z, wz), f"cuts {sizes}"
        assert np.array_equal(bits(np.hstack(parts)), bits(tiled(y, r))) and np.array_equal(bits(np.hstack(tracks)), bits(tiled(tr, r))), f"cuts {sizes}"


# ---- 6. new parameters, reset, a fixed FIR ---------------------------------------------------------------

@pytest.mark.parametrize("per_row", [False, True])
@pytest.mark.parametrize("cplx", KINDS)
def test_set_params_and_reset(hz, ctx, per_row, cplx):
    """set_params between two pushes keeps the state (the program run in two parts, state carried); refused parameters
    change nothing; reset restores w[c] = 1 and the empty history; mu = 0 with taps of its own is a fixed FIR."""
    r, k, n, taps, mode = 5, T + 3, 2 * T + 11, 8, ref.CMA
    a = params_of(mode, r) if per_row else params_of(mode)
    b = (a * np.array([0.5, 1.25], f32)).astype(f32)
    x = distinct_rows(r, n, 11, cplx)
    ((y1, t1, z1),) = ref.exact(BUILD, [(mode, taps, 3, a, x[:, :k])])
    ((y2, t2, z2),) = ref.exact(BUILD, [(mode, taps, 3, b, x[:, k:], z1)])
    with ctx.equalizer(kind_of(hz, cplx), mode, taps, 3, a, rows=r, per_row=per_row) as f:
        dx = dev(x)
        head, thead = f.push(dx[:, :k], track=True)
        assert same_state(f.state(), z1)
        bad = b.copy()
        bad[..., 0] = np.nextafter(f32(1.0), f32(2.0))
        with pytest.raises(hz.ErrInvalidArgument):
            f.set_params(bad)
        with pytest.raises(hz.ErrInvalidArgument):
            f.set_params(b[None] if not per_row else b[0])
        f.set_params(b)
        assert same_state(f.state(), z1), "set_params touched the state"
        tail, ttail = f.push(dx[:, k:], track=True)
        assert same_state(f.state(), z2)
        assert np.array_equal(bits(head), bits(y1)) and np.array_equal(bits(tail), bits(y2)) and np.array_equal(bits(ttail), bits(t2))
        f.reset()
        assert np.array_equal(bits(f.state()), bits(ref.initial_state(r, taps, 3, cplx)))
        f.set_params(a)
        again = f.push(dx[:, :k])
        assert np.array_equal(bits(again), bits(head)) and same_state(f.state(), z1)
        # a fixed FIR: mu = 0, the taps of the first part
        still = a.copy()
        still[..., 0] = 0.0
        f.set_params(still)
        ((y3, _, z3),) = ref.exact(BUILD, [(mode, taps, 3, still, x[:, k:], z1)])
        fir = f.push(dx[:, k:])
        w = (2 if cplx else 1) * taps
        assert np.array_equal(bits(fir), bits(y3)) and same_state(f.state(), z3) and np.array_equal(bits(z3[:, :w]), bits(z1[:, :w]))
        assert f.taps().shape == (r, taps) and np.array_equal(bits(f.taps()).reshape(r, -1), bits(z1[:, :w]))


# ---- 7. isolation ----------------------------------------------------------------------------------

@pytest.mark.parametrize("cplx", KINDS)
def test_a_nan_row_beside_clean_rows_of_its_wave(hz, ctx, cplx):
    """8192 rows of 8 taps (eight rows to the wave) and 2049 rows of 32 taps (two): a NaN in one symbol of one row and an
    infinity in one of another leave every other row of their waves, and every other wave, bit-identical in outputs,
    track and state; set_state heals the rows."""
    n = T + 40
    for r, taps, nan_row, inf_row in ((8192, 8, 8 * 100 + 3, 8 * 512 + 7), (2049, 32, 2 * 50 + 1, 2 * 600)):
        mode = ref.CMA
        x = distinct_rows(r, n, 31 + taps, cplx)
        (want,) = ref.exact(BUILD, [(mode, taps, taps // 2, params_of(mode), x)])
        full = tiled(x, r).copy()
        full[nan_row, 10] = complex(np.nan, 0.25) if cplx else np.nan
        full[inf_row, T + 3] = complex(0.5, -np.inf) if cplx else -np.inf
        clean = np.ones(r, bool)
        clean[[nan_row, inf_row]] = False
        with ctx.equalizer(kind_of(hz, cplx), mode, taps, taps // 2, params_of(mode), rows=r) as f:
            assert f.plan()[0] == 64 // taps
            words, twords = run(f, full, True)
            z = f.state()
            wy, wt, wz = tiled(want[0], r), tiled(want[1], r), tiled(want[2], r)
            assert np.array_equal(words[clean][:, :n].reshape(clean.sum(), -1), bits(wy[clean]).reshape(clean.sum(), -1)), f"taps {taps}"
            assert np.array_equal(twords[clean][:, :n], bits(wt[clean])) and np.array_equal(bits(z[clean]), bits(wz[clean]))
            assert (words[:, n:] == SENTINEL).all() and (twords[:, n:] == SENTINEL).all()
            # the two rows: equal before the bad symbol, not finite behind it
            assert np.array_equal(words[nan_row, :10].reshape(-1), bits(wy[nan_row, :10]).reshape(-1))
            assert np.array_equal(words[inf_row, :T + 3].reshape(-1), bits(wy[inf_row, :T + 3]).reshape(-1))
            assert np.isnan(words[nan_row, 10:n].view(f32)).all() and not np.isfinite(z[nan_row, :taps]).any() and not np.isfinite(z[inf_row, :taps]).any()
            f.set_state(wz)
            y = f.push(dev(tiled(x, r)))
            ((y2, _, z2),) = ref.exact(BUILD, [(mode, taps, taps // 2, params_of(mode), x, want[2])])
            assert np.array_equal(bits(y), bits(tiled(y2, r))) and same_state(f.state(), z2)


# ---- 8. refusals -----------------------------------------------------------------------------------

@pytest.mark.parametrize("r", [1, 3])
def test_refused_pushes_leave_the_state(hz, ctx, r):
    """pitches below n, unequal strides in place and null pointers are refused before anything runs: the next push
    continues the stream"""
    lib = importlib.import_module("go-sdr_amd._capi").lib
    n, taps, mode = 300, 5, ref.DD_QPSK
    x = distinct_rows(3, 2 * n, 5, True)[:r]
    ((y, tr, wz),) = ref.exact(BUILD, [(mode, taps, 2, params_of(mode), x)])
    dx = dev(x)
    with ctx.equalizer(hz.FMT_C64, mode, taps, 2, params_of(mode), rows=r) as f:
        head = f.push(dx[:, :n] if r > 1 else dx[0, :n])
        z0 = f.state()
        out = torch.zeros((r, n), dtype=torch.complex64, device="cuda")
        trk = torch.zeros((r, n), dtype=torch.float32, device="cuda")
        part = dx[:, n:].contiguous()
        push = lambda *a: ctx._ck(lib.hzsdr_equalizer_push(f._h, *a))
        if r > 1:
            with pytest.raises(hz.ErrDstTooSmall):
                push(part.data_ptr(), n, n, None, out.data_ptr(), n - 1, None, 0)
            with pytest.raises(hz.ErrDstTooSmall):
                push(part.data_ptr(), n, n, None, out.data_ptr(), n, trk.data_ptr(), n - 1)
            with pytest.raises(hz.ErrInvalidArgument):
                push(part.data_ptr(), n, n - 1, None, out.data_ptr(), n, None, 0)
            with pytest.raises(hz.ErrInvalidArgument):
                push(part.data_ptr(), n - 1, n, None, part.data_ptr(), n - 1, None, 0)  # in place, unequal strides
        with pytest.raises(hz.ErrInvalidArgument):
            push(None, n, n, None, out.data_ptr(), n, None, 0)
        with pytest.raises(hz.ErrInvalidArgument):
            push(part.data_ptr(), n, n, None, None, n, None, 0)
        assert lib.hzsdr_equalizer_push(None, part.data_ptr(), n, n, None, out.data_ptr(), n, None, 0) == hz.ErrInvalidArgument.status
        torch.cuda.synchronize()
        assert np.array_equal(bits(f.state()), bits(z0)) and not out.any() and not trk.any()
        push(part.data_ptr(), n, n, None, out.data_ptr(), n, trk.data_ptr(), n)
        assert same_state(f.state(), wz)
        assert np.array_equal(bits(np.hstack([host(head).reshape(r, n), host(out)])), bits(y)) and np.array_equal(bits(trk), bits(tr[:, n:]))
        words = r * (2 * taps - 1) * 2
        with pytest.raises(hz.ErrDstTooSmall):
            ctx._ck(lib.hzsdr_equalizer_get_state(f._h, (C.c_float * (words - 1))(), words - 1))
        for count in (words - 1, words + 1):
            with pytest.raises(hz.ErrInvalidArgument):
                ctx._ck(lib.hzsdr_equalizer_set_state(f._h, (C.c_float * count)(), count))
        with pytest.raises(hz.ErrInvalidArgument):
            f.set_state(np.zeros((r, words // r + 1), f32))
        assert same_state(f.state(), wz)


def test_create_errors(hz, ctx):
    lib = importlib.import_module("go-sdr_amd._capi").lib
    out = C.c_void_p()
    good = np.array([0.01, 1.0], f32)

    def create(kind=hz.FMT_C64, mode=hz.EQUALIZER_CMA, taps=11, centre=5, p=good, per_row=0, rows=1):
        ptr = p.ctypes.data_as(C.POINTER(C.c_float)) if p is not None else None
        return lib.hzsdr_equalizer_create(ctx._h, kind, mode, taps, centre, ptr, per_row, rows, C.byref(out))

    inval = hz.ErrInvalidArgument.status
    assert create(rows=0) == inval and create(rows=hz.EQUALIZER_MAX_ROWS + 1) == inval and create(p=None) == inval
    assert create(taps=0, centre=0) == inval and create(taps=65) == inval and create(centre=11) == inval and create(taps=2 ** 40, centre=0) == inval
    assert create(mode=-1) == inval and create(mode=3) == inval and create(kind=hz.EQUALIZER_REAL_F32, mode=hz.EQUALIZER_DD_QPSK) == inval
    for kind in (-1, 0, hz.FMT_U8, hz.FMT_I16, 31, 33):
        assert create(kind=kind) == hz.ErrSampleFormatUnknown.status, f"kind {kind}"
    up = lambda v: np.nextafter(f32(v), f32(np.inf))
    down = lambda v: np.nextafter(f32(v), f32(-np.inf))
    for k, v in ((0, up(1.0)), (0, down(0.0)), (0, np.nan), (0, np.inf), (1, down(2.0 ** -64)), (1, up(2.0 ** 64)), (1, 0.0), (1, np.nan), (1, -np.inf)):
        p = good.copy()
        p[k] = v
        assert create(p=p) == inval, f"parameter {k} = {v}"
    for p, taps, centre, kind, mode in (([0.0, 2.0 ** -64], 1, 0, hz.EQUALIZER_REAL_F32, hz.EQUALIZER_CMA), ([1.0, 2.0 ** 64], 64, 63, hz.FMT_C64, hz.EQUALIZER_DD_QPSK),
                                        ([0.5, 1.0], 64, 0, hz.EQUALIZER_REAL_F32, hz.EQUALIZER_DD_BPSK)):
        assert create(kind=kind, mode=mode, taps=taps, centre=centre, p=np.array(p, f32)) == 0 and lib.hzsdr_equalizer_free(out) == 0, p
    per = np.broadcast_to(good, (3, 2)).copy()
    per[2, 0] = 1.5
    assert create(p=per, per_row=1, rows=3) == inval, "a refused parameter of the last row"
    assert create(rows=hz.EQUALIZER_MAX_ROWS) == 0 and lib.hzsdr_equalizer_free(out) == 0
    with pytest.raises(hz.ErrInvalidArgument):
        ctx.equalizer(hz.FMT_C64, hz.EQUALIZER_CMA, 11, 5, np.ones((2, 2), f32), rows=3, per_row=True)
    with pytest.raises(hz.ErrInvalidArgument):
        ctx.equalizer(hz.FMT_C64, hz.EQUALIZER_CMA, 11, 5, np.ones((3, 2), f32), rows=3)
    with ctx.equalizer(hz.EQUALIZER_REAL_F32, hz.EQUALIZER_CMA, 11, 5, good) as f, pytest.raises(ValueError):
        f.push(dev(ref.white((8,), 1, True)))


# ---- 9. convergence, the chain ------------------------------------------------------------------------

def test_convergence_on_the_device(hz, ctx):
    """The convergence case of tests/test_equalizer_cpu.py (its docstring has the signal and the figures), seed 0: first
    on the host program, so that a failure there blames the inputs, then on the device, whose outputs are also the
    program's bit for bit."""
    r, a = ref.qpsk_through_channel(6000, 0)
    raw, cma, dd, wmax = ref.converge(lambda *case: ref.exact(BUILD, [case])[0], r, a)
    assert raw > 100 and cma == 0 and dd == 0

    seen = []

    def on_device(mode, taps, centre, params, x, state=None):
        with ctx.equalizer(hz.FMT_C64, mode, taps, centre, params) as f:
            if state is not None:
                f.set_state(state)
            y = host(f.push(dev(x)))[None]
            z = f.state()
        ((wy, _, wz),) = ref.exact(BUILD, [(mode, taps, centre, params, x) + ((state,) if state is not None else ())])
        seen.append(np.array_equal(bits(y), bits(wy)) and np.array_equal(bits(z), bits(wz)))
        return y, None, z
    raw, cma, dd, wmax = ref.converge(on_device, r, a)
    print(f"on the device: wrong decisions of 2000: unequalized {raw}, CMA {cma}, DD {dd}; largest |w| {wmax:.3f}")
    assert raw > 100 and cma == 0 and dd == 0 and seen == [True, True]


WORD32 = 0x1ACFFC1D
CHAIN_ROWS, CHAIN_SYMBOLS, CHAIN_FIRST, CHAIN_EVERY, CHAIN_SPS = 8, 2000, 1000, 110, 5.0


def chain_signal(q):
    """8 rows of 2000 QPSK symbols (b0 on Re, b1 on Im) that carry a frame -- the 32-bit word, 168 payload bits -- every
    110 symbols from symbol 1000 on (the equalizer has the first thousand to open the eye), through the 4-tap channel at
    the symbol rate, then raised-cosine pulses at 5 samples per symbol with noise 34 dB down -> (x (8, n), [[payload]])"""
    rows, sent = [], []
    for r in range(CHAIN_ROWS):
        b = framesync_ref.random_bits(2 * CHAIN_SYMBOLS, 70 + r)
        pays = []
        for k, at in enumerate(range(CHAIN_FIRST, CHAIN_SYMBOLS - (q.W + q.P) // 2 - 1, CHAIN_EVERY)):
            pays.append(framesync_ref.random_bits(q.P, 1000 * (70 + r) + k))
            framesync_ref.plant(b, 2 * at, q.words[0], q.W, pays[-1])
        v = b.astype(np.float64) * 2.0 - 1.0
        a = (v[0::2] + 1j * v[1::2]) / math.sqrt(2.0)
        rows.append(symsync_ref.signal(np.convolve(a, ref.CHANNEL)[:CHAIN_SYMBOLS], CHAIN_SPS, 0.25 * (r % 4), noise_db=-34.0, seed=r))
        sent.append([bytes(np.packbits(p)) for p in pays])
    n = min(len(x) for x in rows)
    return np.stack([x[:n] for x in rows]), sent


def frames_of(per, row):
    """{position: (frame bytes, info)} of everything stored for `row`, over the pushes"""
    out = {}
    for fr, ps, inf, cnt in per:
        for k in range(min(int(cnt[row]), fr.shape[1])):
            out[int(ps[row, k])] = (bytes(fr[row, k]), int(inf[row, k]))
    return out


def test_the_chain_symbol_timing_equalizer_frame_sync(hz, ctx):
    """Symbol timing -> equalizer (CMA, 11 taps) -> frame sync on the device, every block going into the next stage as it
    is (the pitched symbols, the int32 counts), nothing read in between.  On the chained host programs every one of the
    9 frames of every row is found with the equalizer, payload bit for bit, and frames are lost without it (measured:
    none of the 72 survives); the device's frames are the host chain's exactly."""
    st = importlib.import_module("go-sdr_amd.stream")
    words, maps = hz.sync_hypotheses(WORD32, 32, 2, "rotate")
    q = framesync_ref.Config(W=32, words=words, P=168, B=2, cplx=True, thr=2, maps=maps)
    x, sent = chain_signal(q)
    sp = np.array([CHAIN_SPS, 0.01, *hz.loop_gains(CHAIN_SPS)], f32)
    ep = np.array([0.01, 1.0], f32)
    cuts = (0, 4000, 4001, x.shape[1])
    # the host chain, push by push as the device takes them
    sym_state = eq_state = None
    pushes, bare = [], []
    for a, b in zip(cuts, cuts[1:]):
        ((sym, cnt, sym_state, _),) = symsync_ref.exact(BUILD, [(sp, x[:, a:b]) + ((sym_state,) if sym_state is not None else ())])
        ((y, _, eq_state),) = ref.exact(BUILD, [(ref.CMA, 11, 5, ep, sym, eq_state, cnt)])
        pushes.append((y, cnt)), bare.append((sym, cnt))
    ((per, _),) = framesync_ref.exact(BUILD, [(q, pushes, 16)])
    ((per_bare, _),) = framesync_ref.exact(BUILD, [(q, bare, 16)])
    want = [frames_of(per, r) for r in range(CHAIN_ROWS)]
    lost = 0
    for r in range(CHAIN_ROWS):
        assert len(sent[r]) == 9 and {v[0] for v in want[r].values()} >= set(sent[r]), f"row {r}: a frame is lost WITH the equalizer"
        lost += len(set(sent[r]) - {v[0] for v in frames_of(per_bare, r).values()})
    print(f"frames lost without the equalizer: {lost} of {9 * CHAIN_ROWS}")
    assert lost > 0
    args, kw = q.create_args()
    with ctx.symbol_sync(hz.FMT_C64, sp, rows=CHAIN_ROWS) as ts, ctx.equalizer(hz.FMT_C64, hz.EQUALIZER_CMA, 11, 5, ep, rows=CHAIN_ROWS) as eq, \
            ctx.frame_sync(q.kind, *args, rows=CHAIN_ROWS, **kw) as fs:
        dx = dev(x)
        blocks = [dx[:, a:b] for a, b in zip(cuts, cuts[1:])]
        parts = list(st.frame_rows(st.equalized_rows(st.symbol_rows(blocks, ts), eq), fs, cap=16))
        assert same_state(eq.state(), eq_state)
    for r in range(CHAIN_ROWS):
        got = {int(p): (bytes(fr), int(i)) for part in parts for fr, p, i in zip(*part[r])}
        assert got == want[r], r


# ---- 10. the other layers --------------------------------------------------------------------------

def _run(exe):
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "go-sdr_amd") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    return subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)


def test_c_equalizer_walkthrough(hz):
    """tests/c/test_equalizer_abi.c compiled by gcc as C99 and run against libhzsdr_hip.so."""
    exe = os.path.join(BUILD, "test_equalizer_abi")
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "test_equalizer_abi.c"), "-L" + os.path.join(ROOT, "go-sdr_amd"),
                           "-lhzsdr_hip", "-lm", "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    p = _run(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "equalizer-abi ok" in p.stdout


def test_cxx_equalizer(hz):
    """tests/cxx/test_equalizer.cpp (hzsdr::stream::Equalizer of go-sdr_amd/cxx/hzsdr.hpp) built with g++ and run."""
    exe = os.path.join(BUILD, "test_equalizer_cxx")
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + ROOT, os.path.join(ROOT, "tests", "cxx", "test_equalizer.cpp"),
                           "-L" + os.path.join(ROOT, "go-sdr_amd"), "-lhzsdr_hip", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    p = _run(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "equalizer-cxx ok" in p.stdout


def test_equalized_rows_over_a_reader(hz, hctx):
    """stream.equalized_rows over a BufferReader with short reads is one push of the whole stream; fed with an iterable
    of (symbols, counts) pairs or of blocks, it takes them as they are; a Reader of another format, or a real bank, is
    refused."""
    st = importlib.import_module("go-sdr_amd.stream")
    p = np.array([0.01, 1.0], f32)
    x, _ = ref.qpsk_through_channel(3000, 7)
    ((y, _, wz),) = ref.exact(BUILD, [(ref.CMA, 11, 5, p, x)])
    with hctx.equalizer(hz.FMT_C64, hz.EQUALIZER_CMA, 11, 5, p) as f:
        blocks = [np.array(b) for b, c in st.equalized_rows(st.BufferReader(x, 48_000, max_read=777), f, block=1024) if c is None]
        assert same_state(f.state(), wz)
    got = np.concatenate(blocks)
    assert len(blocks) > 3 and got.dtype == np.complex64 and np.array_equal(bits(got), bits(y[0]))
    xr = np.ascontiguousarray(x.real)
    ((yr, _, wzr),) = ref.exact(BUILD, [(ref.CMA, 11, 5, p, xr)])
    with hctx.equalizer(hz.EQUALIZER_REAL_F32, hz.EQUALIZER_CMA, 11, 5, p) as f:
        pairs = list(st.equalized_rows(((xr[i:i + 1000], np.array([1000], np.uint32)) for i in range(0, 3000, 1000)), f))
        got = np.concatenate([np.array(b) for b, _ in pairs])
        assert all(c[0] == 1000 for _, c in pairs) and got.dtype == np.float32 and np.array_equal(bits(got), bits(yr[0])) and same_state(f.state(), wzr)
        with pytest.raises(hz.ErrSampleFormatMismatch):
            list(st.equalized_rows(st.BufferReader(x, 48_000), f))
    u8 = np.zeros((64, 2), np.uint8)
    with hctx.equalizer(hz.FMT_C64, hz.EQUALIZER_CMA, 11, 5, p) as f, pytest.raises(hz.ErrSampleFormatMismatch):
        list(st.equalized_rows(st.BufferReader(u8, 48_000), f))

"""The carrier recovery bank (include/hzsdr_carrier.h) on the GPU, every comparison of outputs, track and state BIT FOR
BIT against tests/host/carrier_ref.cpp (the host program over the header the kernel evaluates): rows around the
rows-per-wave edges and samples around the tile edge, pitches above the need on the input, the output and the track with
sentinels behind every row's n-th column, both memory spaces; every rows-per-wave the planner has; every template form
(detector x shared / per-row parameters x with / without track); in place; cuts with and without the state carried into
a new object; new parameters between pushes, reset; a NaN and an infinity kept to their sample and row; refusals;
acquisition behind the tuner bank and in front of the symbol-timing bank; the C and C++ layers; a Reader."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import carrier_ref as ref
import symsync_ref
import tuner_ref
from conftest import ROOT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BUILD = os.path.join(ROOT, "build")
SENTINEL = 0x7F7F7F7F  # (3.39e38: no output and no track value of these tests)
T = 256
ALPHA, BETA = ref.gains(0.02)
PARAMS = np.array([ALPHA, BETA, 0.001, -0.01, 0.01], np.float32)
MODES = (ref.TONE, ref.BPSK, ref.QPSK)


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


def rows_of(r, n, seed):
    return ref.white((n,) if r == 1 else (r, n), seed)


def per_row_params(r, seed=0):
    """r sets of their own: gains, start and range differ from row to row"""
    k = (np.arange(r) + seed) % 7
    lo, hi = -0.004 - 0.001 * k, 0.003 + 0.002 * k
    return np.stack([ALPHA * (1.0 + 0.1 * k), BETA * (1.0 + 0.2 * k), 0.0005 * (k - 3), lo, hi], axis=1).astype(np.float32)


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
    sentinels -> (the whole output as uint32 words (R, width, 2), the whole track as words (R, width) or None)"""
    r, n = (1, x.shape[0]) if x.ndim == 1 else x.shape
    shape = lambda pad: (n + pad,) if r == 1 else (r, n + pad)
    out = sentinels(shape(pads[1]), np.complex64, device)
    tr = sentinels(shape(pads[2]), np.float32, device) if track else None
    got = bank.push(pitched(x, pads[0], device), out=out, track=tr)
    if device:
        torch.cuda.synchronize()
    y = got[0] if track else got
    assert y.shape[-1] == n and (not track or got[1].shape[-1] == n)
    return bits(out).reshape(r, n + pads[1], 2), bits(tr).reshape(r, n + pads[2]) if track else None


def check(words, twords, want, what, skip=None):
    """the push's destinations against the program's (y, track, state): equal bits in the first n columns of every row,
    the sentinel in every column behind them.  skip: (row, column) whose output is compared by the caller."""
    y, tr = want[0], want[1]
    n = y.shape[1]
    wy = bits(y).reshape(y.shape[0], n, 2)
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


# ---- 1. exact streams ------------------------------------------------------------------------------

@pytest.mark.parametrize("space", ["device", "host"])
def test_streams_exact(hz, ctx, hctx, space):
    """R in {1, 3, 64, 1024, 1025, 8192} x n in {1, 255, 256, 257, 3 * 256 + 5}, white rows (both signs of every
    detector branch; the clip: test_every_rows_per_wave), the detectors in turn, pitches above the need on the input,
    the output and the track."""
    c = ctx if space == "device" else hctx
    shapes = [(r, n) for r in (1, 3, 64, 1024, 1025, 8192) for n in (1, T - 1, T, T + 1, 3 * T + 5)]
    cases = [(MODES[k % 3], PARAMS, rows_of(r, n, 1000 * r + n)) for k, (r, n) in enumerate(shapes)]
    for (mode, _, x), want in zip(cases, ref.exact(BUILD, cases)):
        r = 1 if x.ndim == 1 else x.shape[0]
        with c.carrier_loop(mode, PARAMS, rows=r) as f:
            g, t, form = f.plan()
            assert g == (r + 1023) // 1024 and t == T and form == mode * hz.CARRIER_FORM_MODE
            words, twords = run(f, x, space == "device")
            z, pos = f.state()
        what = f"R={r} n={x.shape[-1]} mode {mode} {space}"
        check(words, twords, want, what)
        assert pos == x.shape[-1] and np.array_equal(z, want[2]), f"{what}: the state differs"


def test_white_rows_reach_every_branch():
    """what the tests above and below rely on: white rows give errors of both signs inside the clip and take both signs of
    both QPSK selections; at twice the amplitude (test_every_rows_per_wave; 1.5 times in test_every_form) every
    detector clips on both sides -- the BPSK error of components below 1 cannot reach the clip"""
    x = rows_of(3, 3 * T + 5, 3773).astype(np.complex128)
    for mode in MODES:
        y, _, _ = ref.float64(mode, PARAMS, x[0])
        e = y.imag if mode == ref.TONE else y.real * y.imag if mode == ref.BPSK else np.copysign(1, y.real) * y.imag - np.copysign(1, y.imag) * y.real
        assert (np.abs(e) < 1).any() and (e > 0).any() and (e < 0).any()
        assert (y.real < 0).any() and (y.real > 0).any() and (y.imag < 0).any() and (y.imag > 0).any()
    big = 2.0 * x[0]  # (twice the amplitude: every detector clips on both sides)
    for mode in MODES:
        y, _, _ = ref.float64(mode, PARAMS, big)
        e = y.imag if mode == ref.TONE else y.real * y.imag if mode == ref.BPSK else np.copysign(1, y.real) * y.imag - np.copysign(1, y.imag) * y.real
        assert (e > 1).any() and (e < -1).any()


def test_every_rows_per_wave(hz, ctx):
    """The rows-per-wave values 2 ... 8: the smallest bank of each, an odd one whose last wave is short, and the largest;
    T + 1 samples of twice the white rows' amplitude (every detector clips), per-row parameters."""
    seen = set()
    sizes = [1024 * (k - 1) + 1 for k in range(2, 9)] + [5000, hz.CARRIER_MAX_ROWS - 1, hz.CARRIER_MAX_ROWS]
    cases = [(MODES[k % 3], per_row_params(r, k), 2.0 * rows_of(r, T + 1, r)) for k, r in enumerate(sizes)]
    for (mode, p, x), want in zip(cases, ref.exact(BUILD, cases)):
        with ctx.carrier_loop(mode, p, rows=x.shape[0], per_row=True) as f:
            seen.add(f.plan()[0])
            words, twords = run(f, x, True)
            z, _ = f.state()
        check(words, twords, want, f"R={x.shape[0]} mode {mode}")
        assert np.array_equal(z, want[2])
    assert seen == set(range(2, 9)), f"rows per wave seen: {sorted(seen)}"


# ---- 2. every template form ------------------------------------------------------------------------

@pytest.mark.parametrize("r", [3, 1025])
@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("per_row", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_every_form(hz, ctx, mode, per_row, track, r):
    """detector x shared / per-row parameters x with / without track, one row per wave and two; modulated rows beside
    white ones; per-row parameters of equal values give the shared form's bits."""
    n = 2 * T + 9
    x = 1.5 * rows_of(r, n, 17 * r + mode)
    x[0] = ref.signal(mode, n, 0.003, 0.7, 5 + mode, noise=0.05)
    p = per_row_params(r) if per_row else PARAMS
    (want,) = ref.exact(BUILD, [(mode, p, x)])
    with ctx.carrier_loop(mode, p, rows=r, per_row=per_row) as f:
        assert f.plan()[2] == (hz.CARRIER_FORM_PER_ROW if per_row else 0) + mode * hz.CARRIER_FORM_MODE
        words, twords = run(f, x, True, track=track)
        z, pos = f.state()
    check(words, twords, want, f"mode {mode} per_row {per_row} track {track} R={r}")
    assert pos == n and np.array_equal(z, want[2])
    if not per_row:
        with ctx.carrier_loop(mode, np.broadcast_to(PARAMS, (r, 5)), rows=r, per_row=True) as f:
            words2, twords2 = run(f, x, True, track=track)
            assert np.array_equal(words2, words) and (not track or np.array_equal(twords2, twords)) and np.array_equal(f.state()[0], z)


# ---- 3. in place -----------------------------------------------------------------------------------

@pytest.mark.parametrize("space", ["device", "host"])
@pytest.mark.parametrize("r", [1, 3, 1025])
def test_in_place(hz, ctx, hctx, space, r):
    """out == in, rows of a wider buffer: the out-of-place bits, the columns behind the rows untouched"""
    c, n = (ctx if space == "device" else hctx), 3 * T + 5
    x = rows_of(r, n, 99 + r)
    (want,) = ref.exact(BUILD, [(ref.QPSK, PARAMS, x)])
    wide = sentinels((n + 6,) if r == 1 else (r, n + 6), np.complex64, False)
    wide[..., :n] = x
    wide = dev(wide) if space == "device" else wide
    view = wide[..., :n]
    with c.carrier_loop(ref.QPSK, PARAMS, rows=r) as f, c.carrier_loop(ref.QPSK, PARAMS, rows=r) as g:
        y = f.push(view, out=view)
        apart, tr = g.push(dev(x) if space == "device" else x, track=True)
        if space == "device":
            torch.cuda.synchronize()
        assert (y.data_ptr() == wide.data_ptr()) if space == "device" else (y.ctypes.data == wide.ctypes.data)
        assert np.array_equal(f.state()[0], want[2]) and np.array_equal(g.state()[0], want[2])
    check(bits(wide).reshape(r, n + 6, 2), None, want, f"in place R={r} {space}")
    assert np.array_equal(bits(apart).reshape(r, n, 2), bits(want[0]).reshape(r, n, 2)) and np.array_equal(bits(tr).reshape(r, n), bits(want[1]))
    if r > 1:
        lib = importlib.import_module("go-sdr_amd._capi").lib
        with ctx.carrier_loop(ref.QPSK, PARAMS, rows=r) as f, pytest.raises(hz.ErrInvalidArgument):
            d = dev(np.zeros((r, n + 6), np.complex64))
            ctx._ck(lib.hzsdr_carrier_push(f._h, d.data_ptr(), n, n + 6, d.data_ptr(), n + 5, None, 0))


# ---- 4. cuts ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("carry", [False, True])
@pytest.mark.parametrize("r", [3, 1025])
def test_cuts_bit_identical(hz, ctx, r, carry):
    """1100 samples as one push against the same stream cut at 1, 255, 256 and 257 samples (and a push of none); with
    `carry`, the state goes through get_state into a NEW object's set_state at every cut."""
    n = 1100
    x = rows_of(r, n, seed=r + n)
    x[1] = ref.signal(ref.BPSK, n, -0.002, 0.3, 8, noise=0.1)
    ((y, tr, wz),) = ref.exact(BUILD, [(ref.BPSK, PARAMS, x)])
    dx = dev(x)
    for cut in (1, T - 1, T, T + 1):
        f = ctx.carrier_loop(ref.BPSK, PARAMS, rows=r)
        parts, tracks, done = [], [], 0
        for size in (cut, 0, n - cut):
            s, t = f.push(dx[:, done:done + size], track=True)
            assert s.shape == (r, size) and t.shape == (r, size)
            parts.append(host(s)), tracks.append(host(t))
            done += size
            assert f.position() == done
            if carry:
                z, pos = f.state()
                g = ctx.carrier_loop(ref.BPSK, PARAMS, rows=r)
                g.set_state(z, pos)
                f.close()
                f = g
                assert f.position() == done
        z, pos = f.state()
        f.close()
        assert pos == n and np.array_equal(z, wz), f"cut {cut}"
        assert np.array_equal(bits(np.hstack(parts)), bits(y)) and np.array_equal(bits(np.hstack(tracks)), bits(tr)), f"cut {cut}"


# ---- 5. new parameters, reset ------------------------------------------------------------------------

@pytest.mark.parametrize("per_row", [False, True])
def test_set_params_and_reset(hz, ctx, per_row):
    """set_params between two pushes keeps theta and F (the restatement that exchanges the parameters at that sample,
    state kept; the new clamp holds from the next sample); refused parameters change nothing; reset restores F0."""
    r, k, n = 5, T + 3, 2 * T + 11
    a = per_row_params(r) if per_row else PARAMS
    b = a.copy()
    b[..., 3], b[..., 4], b[..., 0] = -0.0002, 0.0001, a[..., 0] * 0.5
    b[..., 2] = 0.0
    x = rows_of(r, n, seed=11)
    ((y, tr, wz),) = ref.exact(BUILD, [(ref.TONE, [(0, a), (k, b)], x)])
    (first,) = ref.exact(BUILD, [(ref.TONE, a, x[:, :k])])
    with ctx.carrier_loop(ref.TONE, a, rows=r, per_row=per_row) as f:
        dx = dev(x)
        head, thead = f.push(dx[:, :k], track=True)
        z0, _ = f.state()
        assert np.array_equal(z0, first[2])
        bad = b.copy()
        bad[..., 1] = 0.2  # beta above 0.125
        with pytest.raises(hz.ErrInvalidArgument):
            f.set_params(bad)
        with pytest.raises(hz.ErrInvalidArgument):
            f.set_params(b[None] if not per_row else b[0])
        f.set_params(b)
        z1, p1 = f.state()
        assert p1 == k and np.array_equal(z1, z0), "set_params touched theta or F"
        tail, ttail = f.push(dx[:, k:], track=True)
        z, pos = f.state()
        assert pos == n and np.array_equal(z, wz)
        assert np.array_equal(bits(np.hstack([host(head), host(tail)])), bits(y)) and np.array_equal(bits(np.hstack([host(thead), host(ttail)])), bits(tr))
        # reset: position 0, theta 0, F0 of the parameters in force; with the first parameters, the first stream again
        f.reset()
        z, pos = f.state()
        f0 = np.array([ref.loop_constants(q)[2] for q in np.broadcast_to(b, (r, 5))], np.int32)
        assert pos == 0 and not z[:, 0].any() and np.array_equal(z[:, 1].view(np.int32), f0)
        f.set_params(a)
        f.reset()
        again = f.push(dx[:, :k])
        assert np.array_equal(bits(again), bits(head)) and np.array_equal(f.state()[0], z0)


# ---- 6. isolation ----------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_nan_and_infinity_stay_in_their_sample(hz, ctx, mode):
    """A NaN in one sample of one row and an infinity in one of another, 2047 rows (two per wave): every other row is
    bit-equal, and so is every other sample of the two rows, the track and the state: theta and F behind the NaN are
    those of the row with a zero in its place.  (Which NaN the bad sample's output is is not part of the contract.)"""
    r, n, nan_row, inf_row = 2047, T + 40, 5, 1024
    x = rows_of(r, n, seed=31)
    bad, zero = x.copy(), x.copy()
    bad[nan_row, 10] = complex(np.nan, 0.25)
    bad[inf_row, T + 3] = complex(0.5, -np.inf)
    zero[nan_row, 10] = 0.0
    want, wzero = ref.exact(BUILD, [(mode, PARAMS, bad), (mode, PARAMS, zero)])
    with ctx.carrier_loop(mode, PARAMS, rows=r) as f:
        words, twords = run(f, bad, True)
        z, _ = f.state()
    got = words[:, :n].copy().view(np.float32)
    for row, col in ((nan_row, 10), (inf_row, T + 3)):
        w = want[0][row, col]
        for g, v in ((got[row, col, 0], w.real), (got[row, col, 1], w.imag)):
            assert (np.isnan(g) and np.isnan(v)) or g == v, f"row {row}: {g} for {v}"
        words[row, col] = bits(want[0][row, col:col + 1])
    assert np.isnan(got[nan_row, 10]).all()
    check(words, twords, want, f"beside a NaN and an infinity, mode {mode}")
    assert np.array_equal(z, want[2]) and np.array_equal(z[nan_row], wzero[2][nan_row])
    assert np.array_equal(twords[nan_row, :n], bits(wzero[1][nan_row]))


# ---- 7. refusals -----------------------------------------------------------------------------------

@pytest.mark.parametrize("r", [1, 3])
def test_refused_pushes_leave_the_state(hz, ctx, r):
    """pitches below n and null pointers are refused before anything runs: the next push continues the stream"""
    lib = importlib.import_module("go-sdr_amd._capi").lib
    n = 300
    x = rows_of(3, 2 * n, seed=5)[:r]
    ((y, tr, wz),) = ref.exact(BUILD, [(ref.QPSK, PARAMS, x)])
    dx = dev(x)
    with ctx.carrier_loop(ref.QPSK, PARAMS, rows=r) as f:
        head = f.push(dx[:, :n] if r > 1 else dx[0, :n])
        z0, p0 = f.state()
        out = torch.zeros((r, n), dtype=torch.complex64, device="cuda")
        trk = torch.zeros((r, n), dtype=torch.float32, device="cuda")
        part = dx[:, n:].contiguous()
        push = lambda *a: ctx._ck(lib.hzsdr_carrier_push(f._h, *a))
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
        assert lib.hzsdr_carrier_push(None, part.data_ptr(), n, n, out.data_ptr(), n, None, 0) == hz.ErrInvalidArgument.status
        torch.cuda.synchronize()
        z1, p1 = f.state()
        assert p1 == p0 == n and np.array_equal(z1, z0) and not out.any() and not trk.any()
        push(part.data_ptr(), n, n, out.data_ptr(), n, trk.data_ptr(), n)
        z, pos = f.state()
        assert pos == 2 * n and np.array_equal(z, wz)
        assert np.array_equal(bits(np.hstack([host(head).reshape(r, n), host(out)])), bits(y)) and np.array_equal(bits(trk), bits(tr[:, n:]))
        with pytest.raises(hz.ErrDstTooSmall):
            lib_state = (C.c_uint32 * (2 * r - 1))()
            ctx._ck(lib.hzsdr_carrier_get_state(f._h, lib_state, 2 * r - 1))
        with pytest.raises(hz.ErrInvalidArgument):
            ctx._ck(lib.hzsdr_carrier_set_state(f._h, (C.c_uint32 * (2 * r + 1))(), 2 * r + 1, 0))
        assert np.array_equal(f.state()[0], wz)


def test_create_errors(hz, ctx):
    lib = importlib.import_module("go-sdr_amd._capi").lib
    out = C.c_void_p()

    def create(mode, p, per_row=0, rows=1):
        ptr = p.ctypes.data_as(C.POINTER(C.c_float)) if p is not None else None
        return lib.hzsdr_carrier_create(ctx._h, mode, ptr, per_row, rows, C.byref(out))

    inval = hz.ErrInvalidArgument.status
    assert create(ref.TONE, PARAMS, 0, 0) == inval and create(ref.TONE, PARAMS, 0, hz.CARRIER_MAX_ROWS + 1) == inval
    assert create(ref.TONE, None) == inval
    for mode in (-1, 3, 32, hz.FMT_C64 + 100):
        assert create(mode, PARAMS) == inval, f"mode {mode}"
    up, qup = np.nextafter(np.float32(0.125), np.float32(1)), np.nextafter(np.float32(0.25), np.float32(1))
    for k, v in ((0, up), (0, -1e-9), (0, np.nan), (1, up), (1, -1e-9), (1, np.inf), (2, 0.011), (2, -0.011), (2, np.nan), (3, -qup), (3, 0.002),
                 (3, -np.inf), (4, qup), (4, 0.0005), (4, np.nan)):
        p = PARAMS.copy()
        p[k] = v
        assert create(ref.QPSK, p) == inval, f"parameter {k} = {v}"
    for p in ([0.125, 0.125, 0.25, -0.25, 0.25], [0, 0, -0.25, -0.25, -0.25], [0, 0, 0, 0, 0]):
        assert create(ref.BPSK, np.array(p, np.float32)) == 0 and lib.hzsdr_carrier_free(out) == 0, p
    per = np.broadcast_to(PARAMS, (3, 5)).copy()
    per[2, 1] = 0.2
    assert create(ref.TONE, per, 1, 3) == inval, "a refused parameter of the last row"
    assert create(ref.TONE, PARAMS, 0, hz.CARRIER_MAX_ROWS) == 0 and lib.hzsdr_carrier_free(out) == 0
    with pytest.raises(hz.ErrInvalidArgument):
        ctx.carrier_loop(ref.TONE, np.zeros((2, 5), np.float32), rows=3, per_row=True)
    with pytest.raises(hz.ErrInvalidArgument):
        ctx.carrier_loop(ref.TONE, np.zeros((3, 5), np.float32), rows=3)


# ---- 8. acquisition, the chain ---------------------------------------------------------------------

def test_acquisition_behind_the_tuner_bank(hz, ctx):
    """Two QPSK channels at offsets of their own out of one stream: tuner_bank, then carrier_loop, then symbol_sync on
    the device, each block going into the next as it is.  The soft symbols are bit-equal to the three host programs
    chained; their fourth power keeps to one direction (the last quarter within pi / 2 of its mean: locked), where the
    symbols of the same chain without the loop go all round the circle; the track ends at the offsets."""
    offsets, down, sps = (0.002, -0.003), 4, 5.0
    x, words, h, a = ref.two_channels(1500, offsets, 40, sps=5, down=down)
    n = -(-len(x) // down)
    p = np.array([*ref.gains(0.01), 0.0, -0.01, 0.01], np.float32)
    sp = np.array([sps, 0.01, *hz.loop_gains(sps)], np.float32)
    ((tuned, _, _),) = tuner_ref.exact(BUILD, [(words, down, h, x, None)])
    ((derot, wtrack, wz),) = ref.exact(BUILD, [(ref.QPSK, p, tuned[:, :n])])
    (want, loose) = symsync_ref.exact(BUILD, [(sp, derot), (sp, tuned[:, :n])])
    with ctx.tuner_bank(hz.FMT_C64, words, h, down) as tb, ctx.carrier_loop(ref.QPSK, p, rows=2) as cr, ctx.symbol_sync(hz.FMT_C64, sp, rows=2) as ts:
        block = tb.push(dev(x))
        assert block.shape == (2, n)
        y, track = cr.push(block, track=True)
        got = ts.ragged(*ts.push(y))
        z, _ = cr.state()
    assert np.array_equal(bits(y), bits(derot)) and np.array_equal(bits(track), bits(wtrack)) and np.array_equal(z, wz)
    for k in range(2):
        cnt = int(want[1][k])
        assert len(got[k]) == cnt and np.array_equal(bits(got[k]), bits(want[0][k, :cnt]))
        locked = ref.phase_spread(ref.QPSK, got[k][3 * cnt // 4:])
        spinning = ref.phase_spread(ref.QPSK, loose[0][k, 3 * int(loose[1][k]) // 4:int(loose[1][k])])
        freq = float(host(track)[k, 3 * n // 4:].mean())
        print(f"channel {k}: spread of the fourth power {locked:.3f} rad (without the loop {spinning:.3f}), track {freq:.6f} for {offsets[k]}")
        assert locked < np.pi / 2 and spinning > 3.0 and abs(freq - offsets[k]) < 2e-5


# ---- 9. the other layers ---------------------------------------------------------------------------

def _run(exe):
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "go-sdr_amd") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    return subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)


def test_c_carrier_walkthrough(hz):
    """tests/c/test_carrier_abi.c compiled by gcc as C99 and run against libhzsdr_hip.so."""
    exe = os.path.join(BUILD, "test_carrier_abi")
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "test_carrier_abi.c"), "-L" + os.path.join(ROOT, "go-sdr_amd"),
                           "-lhzsdr_hip", "-lm", "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    p = _run(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "carrier-abi ok" in p.stdout


def test_cxx_carrier(hz):
    """tests/cxx/test_carrier.cpp (hzsdr::stream::CarrierLoop of go-sdr_amd/cxx/hzsdr.hpp) built with g++ and run."""
    exe = os.path.join(BUILD, "test_carrier_cxx")
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + ROOT, os.path.join(ROOT, "tests", "cxx", "test_carrier.cpp"),
                           "-L" + os.path.join(ROOT, "go-sdr_amd"), "-lhzsdr_hip", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    p = _run(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "carrier-cxx ok" in p.stdout


def test_carrier_rows_over_a_reader(hz, hctx):
    """stream.carrier_rows over a BufferReader with short reads is one push of the whole stream; fed with an iterable
    of blocks, it takes them as they are; its blocks go on into symbol_rows."""
    st = importlib.import_module("go-sdr_amd.stream")
    x = ref.signal(ref.QPSK, 5000, 0.003, 0.4, 3, sps=5, noise=0.05)
    ((y, _, wz),) = ref.exact(BUILD, [(ref.QPSK, PARAMS, x)])
    with hctx.carrier_loop(ref.QPSK, PARAMS) as f:
        blocks = [np.array(b) for b in st.carrier_rows(st.BufferReader(x, 48_000, max_read=777), f, block=1024)]
        assert f.position() == len(x) and np.array_equal(f.state()[0], wz)
    got = np.concatenate(blocks)
    assert len(blocks) > 3 and got.dtype == np.complex64 and np.array_equal(bits(got), bits(y[0]))
    sp = np.array([5.0, 0.01, *hz.loop_gains(5.0)], np.float32)
    ((s, wc, _, _),) = symsync_ref.exact(BUILD, [(sp, y[0])])
    with hctx.carrier_loop(ref.QPSK, PARAMS) as f, hctx.symbol_sync(hz.FMT_C64, sp) as ts:
        chain = st.symbol_rows(st.carrier_rows((x[i:i + 1000] for i in range(0, 5000, 1000)), f), ts)
        soft = np.concatenate([ts.ragged(a, c)[0] for a, c in chain])
    assert len(soft) == wc[0] and np.array_equal(bits(soft), bits(s[0, :wc[0]]))
    u8 = np.zeros((64, 2), np.uint8)
    with hctx.carrier_loop(ref.QPSK, PARAMS) as f, pytest.raises(hz.ErrSampleFormatMismatch):
        list(st.carrier_rows(st.BufferReader(u8, 48_000), f))

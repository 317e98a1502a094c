"""The IIR bank (include/hzsdr_iir.h) on the GPU, every comparison BIT FOR BIT against the outputs of
tests/host/iir_ref.cpp (the host program over the header the kernel evaluates): rows around the rows-per-wave edge and
samples around the tile edge, real and complex, every source format, pitches on both sides, both memory spaces; every
rows-per-wave the planner has; cuts with and without the state carried into a new object; shared and per-row cascades;
retuning; in place; the denormal decay; a NaN kept to its row; errors that leave the state alone; behind the demodulator;
the C and C++ layers; a Reader."""
import ctypes as C
import importlib
import math
import os
import subprocess

import numpy as np
import pytest

import iir_ref as ref
from conftest import ROOT
from util import FMT, splitmix64

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BUILD = os.path.join(ROOT, "build")
FS = 48_000.0


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


@pytest.fixture(scope="module")
def plan(hz, ctx):
    """(G, T of float32 / complex64 / int16 rows, T of the byte formats) from hzsdr_iir_plan: G is the rows per wave
    of the largest bank"""
    with ctx.iir_bank(hz.IIR_REAL_F32, hz.one_pole(0.5), rows=hz.IIR_MAX_ROWS) as f:
        g, t, form = f.plan()
        assert form == 0
    with ctx.iir_bank(hz.FMT_U8, hz.one_pole(0.5)) as f:
        g1, t8, form = f.plan()
        assert g1 == 1 and form == hz.IIR_FORM_COMPLEX
    assert 2 <= g <= 64 and t >= 64 and t8 >= 64
    return g, t, t8


def kind_of(hz, name):
    return hz.IIR_REAL_F32 if name == "f32" else FMT[name]


def white(name, shape, seed):
    """white samples of a kind: float32 / complex64 components in [-1, 1), or every byte / int16 value"""
    n = int(np.prod(shape))
    if name in ("f32", "c64"):
        z = splitmix64(seed, n * (2 if name == "c64" else 1))
        f = ((z >> np.uint64(40)).astype(np.float64) / float(1 << 23) - 1.0).astype(np.float32)
        return (f.view(np.complex64) if name == "c64" else f).reshape(shape)
    z = splitmix64(seed, 2 * n)
    if name == "i16":
        return (z >> np.uint64(48)).astype(np.uint16).view(np.int16).reshape(tuple(shape) + (2,))
    b = (z >> np.uint64(56)).astype(np.uint8)
    return (b if name == "u8" else b.view(np.int8)).reshape(tuple(shape) + (2,))


def cascade(hz, s, seed=0):
    """s stable sections of the designers, different from one another"""
    pool = [hz.lowpass(2000.0 + 300.0 * seed, 0.8, FS), hz.dc_block(0.97), hz.notch(5000.0 - 100.0 * seed, 6.0, FS), hz.highpass(400.0, 0.7, FS),
            hz.deemphasis(75e-6, FS), hz.one_pole(0.2 + 0.01 * seed), hz.lowpass(9000.0, 1.5, FS), hz.notch(12_000.0, 3.0, FS)]
    return np.concatenate(pool[:s]).astype(np.float32)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def first_difference(got, want):
    g, w = bits(got).reshape(-1), bits(want).reshape(-1)
    bad = np.flatnonzero(g != w)
    return f"{bad.size} of {w.size} words differ, the first at {int(bad[0])}" if bad.size else "equal"


def pitched(x, pad, device, fill=None):
    """x (R, n[, 2]) inside a wider buffer of pitch n + pad (R > 1) -> the view of the rows"""
    if x.ndim == 1 or (x.ndim == 2 and x.shape[-1] == 2 and x.dtype in (np.uint8, np.int8, np.int16)):
        return dev(x) if device else x.copy()  # one row: no pitch
    wide = np.zeros((x.shape[0], x.shape[1] + pad) + x.shape[2:], x.dtype)
    if fill is not None:
        wide[:] = fill
    wide[:, :x.shape[1]] = x
    wide = dev(wide) if device else wide
    return wide[:, :x.shape[1]]


def nan_out(x, cplx, pad, device):
    """a NaN-filled destination for the rows of x with a pitch of n + pad -> (whole buffer, n)"""
    dt = np.complex64 if cplx else np.float32
    one = x.ndim == 1 or (x.ndim == 2 and x.dtype in (np.uint8, np.int8, np.int16))
    n = x.shape[0] if one else x.shape[1]
    shape = (n + pad,) if one else (x.shape[0], n + pad)
    buf = np.full(shape, np.nan, dt)
    return (dev(buf) if device else buf), n


def run(bank, x, device, pad_in=3, pad_out=5):
    """one push of the rows x (numpy) with pitches above n on both sides; the columns past n stay NaN"""
    xs = pitched(x, pad_in, device)
    out, n = nan_out(x, bank.complex, pad_out, device)
    got = bank.push(xs, out=out)
    if device:
        torch.cuda.synchronize()
        got, out = got.cpu().numpy(), out.cpu().numpy()
    assert got.shape[-1] == n and np.isnan(out[..., n:]).all(), "columns past the samples were touched"
    return np.array(got)


def rows_of(r, n, name, seed):
    return white(name, (n,) if r == 1 else (r, n), seed)


# ---- 1. exact streams ------------------------------------------------------------------------------

@pytest.mark.parametrize("space", ["device", "host"])
@pytest.mark.parametrize("s", [1, 2, 8])
@pytest.mark.parametrize("name", ["f32", "c64"])
def test_streams_exact(hz, ctx, hctx, plan, name, s, space):
    """R in {1, 3, G - 1, G, G + 1, 2 G + 2} x n in {1, T - 1, T, T + 1, 2 T + 5}, pitches above n on both sides."""
    g, t, _ = plan
    c = ctx if space == "device" else hctx
    sec = cascade(hz, s)
    cases = [(sec, rows_of(r, n, name, 1000 * r + n + s)) for r in (1, 3, g - 1, g, g + 1, 2 * g + 2) for n in (1, t - 1, t, t + 1, 2 * t + 5)]
    assert len(cases) == 30
    for (sec, x), (want, zwant) in zip(cases, ref.exact(BUILD, cases)):
        r = 1 if x.ndim == 1 else x.shape[0]
        with c.iir_bank(kind_of(hz, name), sec, rows=r) as f:
            assert f.plan()[1] == t and bool(f.plan()[2] & hz.IIR_FORM_COMPLEX) == (name == "c64")
            got = run(f, x, space == "device")
            z, pos = f.state()
        assert same(got, want), f"R={r} n={x.shape[-1]} S={s} {name} {space}: {first_difference(got, want)}"
        assert pos == x.shape[-1] and same(z, zwant), f"R={r} n={x.shape[-1]}: the state differs"


@pytest.mark.parametrize("name", ["f32", "c64"])
def test_every_rows_per_wave(hz, ctx, plan, name):
    """The rows-per-wave values 2 ... G occur only in large banks: the smallest bank of each, an odd one whose last
    wave is short, and the largest; T + 1 samples."""
    g, t, _ = plan
    seen = set()
    rows = [1024 * (k - 1) + 1 for k in range(2, g + 1)] + [5000, hz.IIR_MAX_ROWS - 1, hz.IIR_MAX_ROWS]
    sec = cascade(hz, 2)
    cases = [(sec, rows_of(r, t + 1, name, r)) for r in rows]
    for (sec, x), (want, zwant) in zip(cases, ref.exact(BUILD, cases)):
        with ctx.iir_bank(kind_of(hz, name), sec, rows=x.shape[0]) as f:
            seen.add(f.plan()[0])
            got = run(f, x, True)
            z, _ = f.state()
        assert same(got, want), f"R={x.shape[0]} {name}: {first_difference(got, want)}"
        assert same(z, zwant)
    assert seen == set(range(2, g + 1)), f"rows per wave seen: {sorted(seen)}"


@pytest.mark.parametrize("name", ["u8", "i8", "i16"])
def test_other_sources_exact(hz, ctx, plan, name):
    """One shape each: 2047 rows (two per wave, the last wave short), 2 T + 5 samples, S = 2; the restatement runs on
    hzsdr_convert's complex64 of the same samples."""
    _, t, t8 = plan
    r, sec = 2047, cascade(hz, 2, seed=3)
    with ctx.iir_bank(FMT[name], sec, rows=r) as f:
        gg, tt, form = f.plan()
        assert gg == 2 and tt == (t if name == "i16" else t8) and form == hz.IIR_FORM_COMPLEX
        n = 2 * tt + 5
        x = white(name, (r, n), seed=77)
        got = run(f, x, True)
    flat = dev(x.reshape(r * n, 2))
    c64 = torch.empty(r * n, dtype=torch.complex64, device="cuda")
    assert ctx.convert(c64, flat) == r * n
    ((want, _),) = ref.exact(BUILD, [(sec, c64.cpu().numpy().reshape(r, n))])
    assert same(got, want), f"{name}: {first_difference(got, want)}"


# ---- 2. cuts ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("carry", [False, True])
@pytest.mark.parametrize("name,r", [("f32", 3), ("c64", 3), ("f32", 2047), ("u8", 3)])
def test_cuts_bit_identical(hz, ctx, plan, name, r, carry):
    """3 T + 7 samples as one push against pushes of 1, T - 1, T + 1 and the rest; with `carry`, the state goes through
    get_state into a NEW object's set_state in the middle."""
    sec = cascade(hz, 3)
    f = ctx.iir_bank(kind_of(hz, name), sec, rows=r)
    t = f.plan()[1]
    n = 3 * t + 7
    x = dev(white(name, (r, n), seed=r + n))
    one = f.push(x).clone()
    f.reset()
    assert f.position() == 0
    parts, done = [], 0
    for k, size in enumerate((1, t - 1, t + 1, n - 2 * t - 1)):
        parts.append(f.push(x[:, done:done + size]))
        done += size
        assert f.position() == done
        if carry and k == 1:
            z, pos = f.state()
            assert pos == t and np.abs(z).max() > 0
            g = ctx.iir_bank(kind_of(hz, name), sec, rows=r)
            g.set_state(z, pos)
            f.close()
            f = g
            assert f.position() == t
    torch.cuda.synchronize()
    assert done == n and same(torch.cat(parts, dim=1), one), first_difference(torch.cat(parts, dim=1), one)
    f.close()


# ---- 3. coefficient forms, retuning ----------------------------------------------------------------

@pytest.mark.parametrize("name", ["f32", "c64"])
def test_coefficient_forms(hz, ctx, plan, name):
    """Per-row cascades of equal values give the shared form's bits; distinct per-row cascades match the restatement
    row by row.  2047 rows: two per wave, so neighbouring lanes hold different coefficients."""
    _, t, _ = plan
    r, n, s = 2047, t + 9, 2
    x = white(name, (r, n), seed=5)
    shared = cascade(hz, s)
    with ctx.iir_bank(kind_of(hz, name), shared, rows=r) as a, ctx.iir_bank(kind_of(hz, name), np.broadcast_to(shared, (r, s, 5)), rows=r) as b:
        assert a.plan()[2] & hz.IIR_FORM_PER_ROW == 0 and b.plan()[2] & hz.IIR_FORM_PER_ROW
        ya, yb = run(a, x, True), run(b, x, True)
    assert same(ya, yb), "equal per-row cascades differ from the shared one"
    rng = np.random.default_rng(3)
    per = np.stack([np.concatenate([hz.lowpass(rng.uniform(500, 20_000), rng.uniform(0.5, 3.0), FS), hz.dc_block(rng.uniform(0.5, 0.999))])
                    for _ in range(r)])
    ((want, zwant),) = ref.exact(BUILD, [(per, x)])
    with ctx.iir_bank(kind_of(hz, name), per, rows=r) as f:
        got = run(f, x, True)
        z, _ = f.state()
    assert same(got, want) and same(z, zwant), first_difference(got, want)
    assert not same(got, ya)


@pytest.mark.parametrize("per_row", [False, True])
def test_retuning(hz, ctx, plan, per_row):
    """set_sections between two pushes: the restatement that exchanges the cascade at that sample, state kept."""
    _, t, _ = plan
    r, k, n = 5, t + 3, 2 * t + 11
    a, b = hz.notch(1000.0, 5.0, FS), hz.notch(1700.0, 5.0, FS)
    if per_row:
        a = np.stack([hz.notch(1000.0 + 50 * i, 5.0, FS) for i in range(r)])
        b = np.stack([hz.notch(1700.0 + 50 * i, 5.0, FS) for i in range(r)])
    x = white("f32", (r, n), seed=11)
    ((want, zwant),) = ref.exact(BUILD, [([(0, a), (k, b)], x)])
    with ctx.iir_bank(hz.IIR_REAL_F32, a, rows=r) as f:
        dx = dev(x)
        head = f.push(dx[:, :k])
        with pytest.raises(hz.ErrInvalidArgument):
            f.set_sections(np.concatenate([b, b], axis=-2))
        bad = b.copy()
        bad[..., 0, 2] = np.inf
        with pytest.raises(hz.ErrInvalidArgument):
            f.set_sections(bad)
        assert f.position() == k
        f.set_sections(b)
        tail = f.push(dx[:, k:])
        torch.cuda.synchronize()
        z, pos = f.state()
    assert pos == n and same(torch.cat([head, tail], dim=1), want) and same(z, zwant)


# ---- 4. in place -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["f32", "c64"])
def test_in_place(hz, ctx, hctx, plan, name):
    _, t, _ = plan
    r, n = 7, 2 * t + 5
    sec = cascade(hz, 2)
    x = white(name, (r, n), seed=21)
    ((want, _), (want1, _)) = ref.exact(BUILD, [(sec, x), (sec, x[0])])
    with ctx.iir_bank(kind_of(hz, name), sec, rows=r) as f:
        wide = pitched(x, 4, True)
        got = f.push(wide, out=wide)
        torch.cuda.synchronize()
        assert got.data_ptr() == wide.data_ptr() and same(wide, want)
    with hctx.iir_bank(kind_of(hz, name), sec, rows=r) as f:
        wide = pitched(x, 4, False)
        f.push(wide, out=wide)
        assert same(wide, want)
    with ctx.iir_bank(kind_of(hz, name), sec) as f:
        one = dev(x[0])
        f.push(one, out=one)
        torch.cuda.synchronize()
        assert same(one, want1)
    # another format, or other strides, in place: refused, nothing consumed
    lib = importlib.import_module("go-sdr_amd._capi").lib
    got = C.c_size_t(3)
    with ctx.iir_bank(hz.FMT_I16, sec, rows=2) as f:
        buf = torch.zeros((2, 64), dtype=torch.complex64, device="cuda")
        rc = lib.hzsdr_iir_push(f._h, buf.data_ptr(), 16, 64, buf.data_ptr(), 64, 64, C.byref(got))
        assert rc == hz.ErrInvalidArgument.status and got.value == 0 and f.position() == 0
    with ctx.iir_bank(hz.FMT_C64, sec, rows=2) as f:
        rc = lib.hzsdr_iir_push(f._h, buf.data_ptr(), 16, 32, buf.data_ptr(), 64, 64, C.byref(got))
        assert rc == hz.ErrInvalidArgument.status and f.position() == 0


# ---- 5. denormals, isolation -----------------------------------------------------------------------

def test_denormal_decay_beside_ordinary_rows(hz, ctx, hctx):
    """An impulse through a pole of 0.5 beside rows of white samples: 2^-n exactly through the denormals, +0 from
    n = 150 on, on the device as in the restatement."""
    n = 200
    x = white("f32", (5, n), seed=8)
    x[2] = ref.decay_row(n)
    ((want, zwant),) = ref.exact(BUILD, [(ref.decay_section(), x)])
    for c, device in ((ctx, True), (hctx, False)):
        with c.iir_bank(hz.IIR_REAL_F32, ref.decay_section(), rows=5) as f:
            got = run(f, x, device)
            z, _ = f.state()
        assert same(got, want) and same(z, zwant), first_difference(got, want)
        u = bits(got[2])
        assert [int(v) for v in u[147:152]] == [4, 2, 1, 0, 0] and ((u[127:150] & 0x7f800000) == 0).all() and not u[150:].any()
        assert got[2, 100] == np.float32(math.ldexp(1.0, -100))


def test_a_nan_stays_in_its_row(hz, ctx, plan):
    """A NaN in one row of 2047 (two rows per wave): every other row keeps its bits; the row stays poisoned over the
    next push, and reset or set_state heals it."""
    _, t, _ = plan
    r, n, bad = 2047, t + 20, 5
    sec = cascade(hz, 2)
    x = white("f32", (r, n), seed=31)
    y = x.copy()
    y[bad, 10] = np.nan
    with ctx.iir_bank(hz.IIR_REAL_F32, sec, rows=r) as f:
        clean = run(f, x, True)
        zc, _ = f.state()
        f.reset()
        got = run(f, y, True)
        others = np.arange(r) != bad
        assert same(got[others], clean[others]), "a NaN changed another row"
        assert same(got[bad, :10], clean[bad, :10]) and np.isnan(got[bad, 10:]).all()
        again = run(f, x, True)
        assert np.isnan(again[bad]).all() and not np.isnan(again[others]).any(), "the row is not poisoned until reset"
        z, pos = f.state()
        assert np.isnan(z[bad]).all() and not np.isnan(z[others]).any() and pos == 2 * n
        f.set_state(zc, n)
        healed = run(f, x, True)
        ((want, _),) = ref.exact(BUILD, [(sec, np.concatenate([x, x], axis=1))])
        assert same(healed, want[:, n:]) and f.position() == 2 * n
        f.reset()
        assert same(run(f, x, True), clean)


# ---- 6. errors and state ---------------------------------------------------------------------------

def test_create_errors(hz, ctx):
    sec = cascade(hz, 2)
    lib = importlib.import_module("go-sdr_amd._capi").lib
    out = C.c_void_p()

    def create(kind, s, n_sections, per_row=0, rows=1):
        p = s.ctypes.data_as(C.POINTER(C.c_float)) if s is not None else None
        return lib.hzsdr_iir_create(ctx._h, kind, p, n_sections, per_row, rows, C.byref(out))

    inval = hz.ErrInvalidArgument.status
    big = cascade(hz, 8)
    nine = np.concatenate([big, sec[:1]])
    assert create(hz.IIR_REAL_F32, sec, 0) == inval, "S = 0"
    assert create(hz.IIR_REAL_F32, nine, 9) == inval, "S = 9"
    assert create(hz.IIR_REAL_F32, sec, 2, 0, 0) == inval, "R = 0"
    assert create(hz.IIR_REAL_F32, sec, 2, 0, hz.IIR_MAX_ROWS + 1) == inval, "R = 8193"
    assert create(hz.IIR_REAL_F32, None, 2) == inval, "null sections"
    assert lib.hzsdr_iir_create(ctx._h, hz.IIR_REAL_F32, sec.ctypes.data_as(C.POINTER(C.c_float)), 2, 0, 1, None) == inval, "null out"
    for badv in (np.nan, np.inf, -np.inf):
        for where in (0, 9):
            s = sec.copy()
            s.reshape(-1)[where] = badv
            assert create(hz.FMT_C64, s, 2) == inval, "a non-finite coefficient"
    per = np.broadcast_to(sec, (3, 2, 5)).copy()
    per[2, 1, 4] = np.nan
    assert create(hz.IIR_REAL_F32, per, 2, 1, 3) == inval, "a non-finite coefficient of the last row"
    for kind in (0, 5, 9, 31, 33, -1):
        assert create(kind, sec, 2) == hz.ErrSampleFormatUnknown.status, f"kind {kind}"
    assert create(hz.IIR_REAL_F32, big, 8, 0, hz.IIR_MAX_ROWS) == 0 and lib.hzsdr_iir_free(out) == 0
    with pytest.raises(hz.ErrInvalidArgument):
        ctx.iir_bank(hz.IIR_REAL_F32, nine)
    with pytest.raises(hz.ErrInvalidArgument):
        ctx.iir_bank(hz.IIR_REAL_F32, np.zeros((2, 2, 5), np.float32), rows=3)


@pytest.mark.parametrize("r", [1, 3])
def test_refused_pushes_leave_the_state(hz, ctx, r):
    lib = importlib.import_module("go-sdr_amd._capi").lib
    sec, n = cascade(hz, 2), 150
    x = white("f32", (r, 2 * n), seed=5)
    ((want, _),) = ref.exact(BUILD, [(sec, x)])
    dx = dev(x)
    out = torch.zeros((r, n), dtype=torch.float32, device="cuda")
    with ctx.iir_bank(hz.IIR_REAL_F32, sec, rows=r) as f:
        head = f.push(dx[:, :n] if r > 1 else dx[0, :n]).clone()
        z0, p0 = f.state()
        got = C.c_size_t(7)
        part = dx[:, n:].contiguous()
        with pytest.raises(hz.ErrDstTooSmall):
            ctx._ck(lib.hzsdr_iir_push(f._h, part.data_ptr(), n, n, out.data_ptr(), n - 1, n, C.byref(got)))
        assert got.value == 0
        if r > 1:
            with pytest.raises(hz.ErrDstTooSmall):
                ctx._ck(lib.hzsdr_iir_push(f._h, part.data_ptr(), n, n, out.data_ptr(), n, n - 1, C.byref(got)))
            with pytest.raises(hz.ErrInvalidArgument):
                ctx._ck(lib.hzsdr_iir_push(f._h, part.data_ptr(), n, n - 1, out.data_ptr(), n, n, C.byref(got)))
        with pytest.raises(hz.ErrInvalidArgument):
            ctx._ck(lib.hzsdr_iir_push(f._h, None, n, n, out.data_ptr(), n, n, C.byref(got)))
        z1, p1 = f.state()
        assert p1 == p0 == n and same(z1, z0) and got.value == 0
        tail = f.push(part if r > 1 else part[0])
        torch.cuda.synchronize()
        whole = torch.cat([head.reshape(r, n), tail.reshape(r, n)], dim=1)
        assert same(whole, want.reshape(r, 2 * n))
        # reset: position 0, a zero state, the first stream again
        f.reset()
        z, p = f.state()
        assert p == 0 and not bits(z).any()
        assert same(f.push(dx[:, :n] if r > 1 else dx[0, :n]), head)
        assert f.push(dx[:, :0] if r > 1 else dx[0, :0]).shape[-1] == 0 and f.position() == n


# ---- 7. behind the demodulator ---------------------------------------------------------------------

def test_the_demodulator_feeds_it(hz, ctx):
    """FM of a frequency-modulated carrier, 12 rows, demodulated into a PITCHED block that goes into the de-emphasis as
    it is (no copy: the same pointer, a pitch above the count).  Bit for bit the restatement of the demodulator's own
    output; and the audio tone comes out scaled by the de-emphasis's |H| at its frequency."""
    r, n, fm, tau = 12, 4000, 3000.0, 75e-6
    k = np.arange(n)
    beta = 0.5 + 0.1 * np.arange(r)[:, None]
    ph = beta * np.sin(2.0 * np.pi * fm * k / FS)[None, :]
    x = (np.cos(ph) + 1j * np.sin(ph)).astype(np.complex64)
    sec = hz.deemphasis(tau, FS)
    with ctx.demodulator(hz.FMT_C64, hz.DEMOD_FM, streams=r) as dm, ctx.iir_bank(hz.IIR_REAL_F32, sec, rows=r) as f:
        block = torch.zeros((r, n + 9), dtype=torch.float32, device="cuda")
        d = dm.push(dev(x), out=block)
        assert d.shape == (r, n) and d.stride(0) == n + 9 and d.data_ptr() == block.data_ptr()
        y = f.push(d)
        torch.cuda.synchronize()
    dn = d.cpu().numpy()
    ((want, _),) = ref.exact(BUILD, [(sec, dn)])
    assert same(y, want), first_difference(y, want)
    h = abs(importlib.import_module("go-sdr_amd.iir").response(sec, fm, FS))
    yn = y.cpu().numpy().astype(np.float64)
    # 100 whole periods of the tone (16 samples each) behind the transient (fs tau = 3.6 samples)
    ratio = np.sqrt((yn[:, -1600:] ** 2).mean(axis=1) / (dn[:, -1600:].astype(np.float64) ** 2).mean(axis=1))
    print("de-emphasis gain at the tone:", ratio, "expected", h)
    assert np.abs(ratio - h).max() <= 1e-4 * h and 0.4 < h < 0.7


# ---- 8. the other layers ---------------------------------------------------------------------------

def _run(exe):
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "go-sdr_amd") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    return subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)


def test_c_iir_walkthrough(hz):
    """tests/c/test_iir_abi.c compiled by gcc as C99 and run against libhzsdr_hip.so."""
    exe = os.path.join(BUILD, "test_iir_abi")
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "test_iir_abi.c"), "-L" + os.path.join(ROOT, "go-sdr_amd"),
                           "-lhzsdr_hip", "-lm", "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    p = _run(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "iir-abi ok" in p.stdout


def test_cxx_iir(hz):
    """tests/cxx/test_iir.cpp (hzsdr::stream::IirBank of go-sdr_amd/cxx/hzsdr.hpp) built with g++ and run."""
    exe = os.path.join(BUILD, "test_iir_cxx")
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + ROOT, os.path.join(ROOT, "tests", "cxx", "test_iir.cpp"),
                           "-L" + os.path.join(ROOT, "go-sdr_amd"), "-lhzsdr_hip", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    p = _run(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "iir-cxx ok" in p.stdout


def test_iir_rows_over_a_reader(hz, hctx):
    """stream.iir_rows over a BufferReader with short reads is one push of the whole stream; fed with
    demodulator_blocks, it filters the demodulator's float32 blocks."""
    st = importlib.import_module("go-sdr_amd.stream")
    x = white("i16", (5000,), seed=3)
    dc = hz.dc_block(0.995)
    with hctx.iir_bank(hz.FMT_I16, dc) as one:
        want = np.array(one.push(x))
    with hctx.iir_bank(hz.FMT_I16, dc) as f:
        blocks = list(st.iir_rows(st.BufferReader(x, 48_000, max_read=777), f, block=1024))
        assert f.position() == 5000
    assert len(blocks) > 3 and all(b.dtype == np.complex64 for b in blocks) and same(np.concatenate(blocks), want)
    with hctx.iir_bank(hz.FMT_U8, dc) as f, pytest.raises(hz.ErrSampleFormatMismatch):
        list(st.iir_rows(st.BufferReader(x, 48_000), f))
    # the demodulator's blocks (the pushes' and the flush's) through the de-emphasis
    de = hz.deemphasis(75e-6, 48_000.0)
    with hctx.demodulator(hz.FMT_I16, hz.DEMOD_FM) as dm:
        audio = np.concatenate([dm.push(x), dm.flush()])
    ((want, _),) = ref.exact(BUILD, [(de, audio)])
    with hctx.demodulator(hz.FMT_I16, hz.DEMOD_FM) as dm, hctx.iir_bank(hz.IIR_REAL_F32, de) as f:
        got = list(st.iir_rows(st.demodulator_blocks(st.BufferReader(x, 48_000, max_read=777), dm, block=1024), f))
    assert len(got) > 3 and all(b.dtype == np.float32 for b in got) and same(np.concatenate(got), want)

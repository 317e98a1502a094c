"""The symbol-timing recovery bank (include/hzsdr_symsync.h) on the GPU, every comparison of symbols, counts and state
BIT FOR BIT against tests/host/symsync_ref.cpp (the host program over the header the kernel evaluates): rows around the
rows-per-wave edges and samples around the tile edge, real and complex, pitches on both sides with sentinels behind
every row's count, both memory spaces; every rows-per-wave the planner has; ragged rows whose counts differ 25-fold and
pass the storer's 64-lane steps; cuts with and without the state carried into a new object; shared and per-row
parameters, new parameters between pushes; a capacity below the bound refused; a NaN kept to its row; acquisition on
the device; behind the demodulator and the IIR bank; the C and C++ layers; a Reader."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import symsync_ref as ref
from conftest import ROOT
from util import splitmix64

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BUILD = os.path.join(ROOT, "build")
SENTINEL = 0x7F7F7F7F  # (3.39e38: no symbol of these tests)
T = 256


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


def kind_of(hz, name):
    return hz.SYMSYNC_REAL_F32 if name == "f32" else hz.FMT_C64


def params_for(hz, sps, limit=0.01):
    return np.array([sps, limit, *hz.loop_gains(sps)], np.float32)


def white(name, shape, seed):
    """white float32 / complex64 samples, components in [-1, 1)"""
    n = int(np.prod(shape))
    z = splitmix64(seed, n * (2 if name == "c64" else 1))
    f = ((z >> np.uint64(40)).astype(np.float64) / float(1 << 23) - 1.0).astype(np.float32)
    return (f.view(np.complex64) if name == "c64" else f).reshape(shape)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def bits(a):
    return np.ascontiguousarray(host(a)).view(np.uint32)


def pitched(x, pad, device):
    """x (R, n) inside a wider buffer of pitch n + pad (R > 1) -> the view of the rows"""
    if x.ndim == 1:
        return dev(x) if device else x.copy()
    wide = np.zeros((x.shape[0], x.shape[1] + pad), x.dtype)
    wide[:, :x.shape[1]] = x
    wide = dev(wide) if device else wide
    return wide[:, :x.shape[1]]


def run(bank, x, device, pad_in=3, pad_out=5):
    """one push of the rows x (numpy) with pitches above the need on both sides, into a destination full of sentinels
    -> (the whole destination as uint32 words (R, width[, 2]), counts as uint32, the bound)"""
    r = 1 if x.ndim == 1 else x.shape[0]
    bound = bank.max_symbols(x.shape[-1])
    dt = np.complex64 if bank.complex else np.float32
    buf = np.full((bound + pad_out,) if r == 1 else (r, bound + pad_out), 0, np.uint64 if bank.complex else np.uint32)
    buf[...] = SENTINEL | (SENTINEL << 32) if bank.complex else SENTINEL
    buf = buf.view(dt)
    buf = dev(buf) if device else buf
    counts = torch.full((r,), -7, dtype=torch.int32, device="cuda") if device else np.full(r, 77, np.uint32)
    got, cnt = bank.push(pitched(x, pad_in, device), out=buf, counts=counts)
    if device:
        torch.cuda.synchronize()
    assert got.shape[-1] == bound and (cnt.data_ptr() == counts.data_ptr() if device else cnt is counts)
    words = bits(buf).reshape(r, bound + pad_out, -1)
    return words, host(cnt).view(np.uint32).copy(), bound


def check(words, counts, want, what):
    """the push's destination against the program's (symbols, counts, ...): equal counts, equal bits up to each row's
    count, the sentinel in every column behind it"""
    y, wc = want[0], want[1]
    assert np.array_equal(counts, wc), f"{what}: counts differ in {np.flatnonzero(counts != wc)[:8]}: {counts[counts != wc][:8]} for {wc[counts != wc][:8]}"
    width = words.shape[1]
    assert wc.max(initial=0) <= width
    wy = np.zeros(words.shape, np.uint32)
    k = min(width, y.shape[1])
    wy[:, :k] = bits(y).reshape(y.shape[0], y.shape[1], -1)[:, :k]
    mask = (np.arange(width)[None, :] < wc[:, None])[:, :, None]
    bad = np.flatnonzero(((words != wy) & mask).any(axis=(1, 2)))
    assert bad.size == 0, f"{what}: symbols differ in {bad.size} rows, the first {int(bad[0])}"
    assert ((words == SENTINEL) | mask).all(), f"{what}: a column behind a row's count was touched"


def rows_of(r, n, name, seed):
    return white(name, (n,) if r == 1 else (r, n), seed)


# ---- 1. exact streams ------------------------------------------------------------------------------

@pytest.mark.parametrize("space", ["device", "host"])
@pytest.mark.parametrize("name", ["f32", "c64"])
def test_streams_exact(hz, ctx, hctx, name, space):
    """R in {1, 3, 64, 1024, 1025, 8192} x n in {1, 255, 256, 257, 3 * 256 + 5}, pitches above the need on both sides."""
    c = ctx if space == "device" else hctx
    p = params_for(hz, 5.0)
    cases = [(p, rows_of(r, n, name, 1000 * r + n)) for r in (1, 3, 64, 1024, 1025, 8192) for n in (1, T - 1, T, T + 1, 3 * T + 5)]
    for (_, x), want in zip(cases, ref.exact(BUILD, cases)):
        r = 1 if x.ndim == 1 else x.shape[0]
        with c.symbol_sync(kind_of(hz, name), p, rows=r) as f:
            g, t, form = f.plan()
            assert g == (r + 1023) // 1024 and t == T and form == (hz.SYMSYNC_FORM_COMPLEX if name == "c64" else 0)
            words, counts, bound = run(f, x, space == "device")
            z, pos = f.state()
        what = f"R={r} n={x.shape[-1]} {name} {space}"
        assert bound == ref.max_symbols(x.shape[-1], p), what
        check(words, counts, want, what)
        assert pos == x.shape[-1] and np.array_equal(bits(z), bits(want[2])), f"{what}: the state differs"


@pytest.mark.parametrize("name", ["f32", "c64"])
def test_every_rows_per_wave(hz, ctx, name):
    """The rows-per-wave values 2 ... 8: the smallest bank of each, an odd one whose last wave is short, and the largest;
    T + 1 samples."""
    seen = set()
    p = params_for(hz, 4.0)
    cases = [(p, rows_of(r, T + 1, name, r)) for r in [1024 * (k - 1) + 1 for k in range(2, 9)] + [5000, hz.SYMSYNC_MAX_ROWS - 1, hz.SYMSYNC_MAX_ROWS]]
    for (_, x), want in zip(cases, ref.exact(BUILD, cases)):
        with ctx.symbol_sync(kind_of(hz, name), p, rows=x.shape[0]) as f:
            seen.add(f.plan()[0])
            words, counts, _ = run(f, x, True)
            z, _ = f.state()
        check(words, counts, want, f"R={x.shape[0]} {name}")
        assert np.array_equal(bits(z), bits(want[2]))
    assert seen == set(range(2, 9)), f"rows per wave seen: {sorted(seen)}"


# ---- 2. ragged rows --------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["f32", "c64"])
def test_ragged_rows(hz, ctx, name):
    """Per-row parameters give neighbouring rows of one wave (2047 rows: two per wave) 2.5, 64 and 2.001 samples per
    symbol: the counts differ about 25-fold, the 2.5 row passes 64 symbols within a tile and the 2.001 row -- the
    densest the definition allows -- reaches 128, the storer's second 64-lane step full."""
    r, n = 2047, 3 * T + 5
    per = np.stack([params_for(hz, 2.5), params_for(hz, 64.0), np.array([2.001, 0, 0, 0], np.float32)] * 683)[:r]
    x = rows_of(r, n, name, 42)
    want, tile0 = ref.exact(BUILD, [(per, x), (per, x[:, :T])])
    assert tile0[1][0] > 64 and tile0[1][1] <= 4 and tile0[1][2] == 128, tile0[1][:3]
    assert 20 <= want[1][0] / want[1][1] <= 30, want[1][:3]
    with ctx.symbol_sync(kind_of(hz, name), per, rows=r) as f:
        assert f.plan()[0] == 2 and f.plan()[2] & hz.SYMSYNC_FORM_PER_ROW
        words, counts, bound = run(f, x, True)
        z, _ = f.state()
    assert bound == ref.max_symbols(n, per) and counts.max() <= bound
    check(words, counts, want, f"ragged {name}")
    assert np.array_equal(bits(z), bits(want[2]))


# ---- 3. cuts ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("carry", [False, True])
@pytest.mark.parametrize("name,r", [("f32", 3), ("c64", 3), ("f32", 1025)])
def test_cuts_bit_identical(hz, ctx, name, r, carry):
    """1100 samples as one push against pushes of 1, 7, 255, 256, 300 and the rest (and one of none); with `carry`, the
    state goes through get_state into a NEW object's set_state in the middle."""
    p, n = params_for(hz, 5.0), 1100
    x = rows_of(r, n, name, seed=r + n)
    ((y, wc, wz, _),) = ref.exact(BUILD, [(p, x)])
    dx = dev(x)
    f = ctx.symbol_sync(kind_of(hz, name), p, rows=r)
    parts, done = [[] for _ in range(r)], 0
    for k, size in enumerate((1, 7, 0, 255, 256, 300, n - 819)):
        s, c = f.push(dx[:, done:done + size])
        assert s.shape == (r, f.max_symbols(size))
        for i, row in enumerate(f.ragged(s, c)):
            parts[i].append(row)
        done += size
        assert f.position() == done
        if carry and k == 3:
            z, pos = f.state()
            g = ctx.symbol_sync(kind_of(hz, name), p, rows=r)
            g.set_state(z, pos)
            f.close()
            f = g
            assert f.position() == done
    z, pos = f.state()
    f.close()
    assert done == n == pos and np.array_equal(bits(z), bits(wz))
    for i in range(r):
        got = np.concatenate(parts[i])
        assert len(got) == wc[i] and np.array_equal(bits(got), bits(y[i, :wc[i]])), f"row {i}"


# ---- 4. parameter forms, new parameters ------------------------------------------------------------

@pytest.mark.parametrize("name", ["f32", "c64"])
def test_parameter_forms(hz, ctx, name):
    """Per-row parameters of equal values give the shared form's bits; 2047 rows, two per wave."""
    r, n = 2047, T + 9
    p = params_for(hz, 6.0)
    x = rows_of(r, n, name, seed=5)
    ((want),) = ref.exact(BUILD, [(p, x)])
    with ctx.symbol_sync(kind_of(hz, name), p, rows=r) as a, ctx.symbol_sync(kind_of(hz, name), np.broadcast_to(p, (r, 4)), rows=r) as b:
        assert a.plan()[2] & hz.SYMSYNC_FORM_PER_ROW == 0 and b.plan()[2] & hz.SYMSYNC_FORM_PER_ROW
        wa, ca, _ = run(a, x, True)
        wb, cb, _ = run(b, x, True)
        za, zb = a.state()[0], b.state()[0]
    check(wa, ca, want, "shared")
    check(wb, cb, want, "per row")
    assert np.array_equal(bits(za), bits(zb)) and np.array_equal(bits(za), bits(want[2]))


@pytest.mark.parametrize("per_row", [False, True])
@pytest.mark.parametrize("name", ["f32", "c64"])
def test_set_params_between_pushes(hz, ctx, name, per_row):
    """set_params between two pushes: the restatement that exchanges the parameters at that sample, state kept; refused
    parameters change nothing.  Five rows: one per wave, so the per-row form of the one-row walk runs for both kinds."""
    r, k, n = 5, T + 3, 2 * T + 11
    a, b = params_for(hz, 5.0), params_for(hz, 5.2, limit=0.05)
    if per_row:
        a = np.stack([params_for(hz, 5.0 + 0.1 * i) for i in range(r)])
        b = np.stack([params_for(hz, 5.3 - 0.1 * i, limit=0.03) for i in range(r)])
    x = white(name, (r, n), seed=11)
    ((y, wc, wz, _),) = ref.exact(BUILD, [([(0, a), (k, b)], x)])
    with ctx.symbol_sync(kind_of(hz, name), a, rows=r) as f:
        assert f.plan()[0] == 1 and bool(f.plan()[2] & hz.SYMSYNC_FORM_PER_ROW) == per_row
        dx = dev(x)
        head = f.ragged(*f.push(dx[:, :k]))
        bad = b.copy()
        bad[..., 2] = 9.0  # hmin - g_mu far below 1
        with pytest.raises(hz.ErrInvalidArgument):
            f.set_params(bad)
        with pytest.raises(hz.ErrInvalidArgument):
            f.set_params(b[None] if not per_row else b[0])
        assert f.position() == k
        f.set_params(b)
        tail = f.ragged(*f.push(dx[:, k:]))
        z, pos = f.state()
    assert pos == n and np.array_equal(bits(z), bits(wz))
    for i in range(r):
        got = np.concatenate([head[i], tail[i]])
        assert len(got) == wc[i] and np.array_equal(bits(got), bits(y[i, :wc[i]])), f"row {i}"


# ---- 5. refusals -----------------------------------------------------------------------------------

@pytest.mark.parametrize("r", [1, 3])
def test_refused_pushes_leave_the_state(hz, ctx, r):
    """A capacity (or, with several rows, an out_stride) one below max_symbols(n) is refused before anything runs: the
    next push continues the stream."""
    lib = importlib.import_module("go-sdr_amd._capi").lib
    p, n = params_for(hz, 5.0), 300
    x = white("f32", (r, 2 * n), seed=5)
    ((y, wc, wz, _),) = ref.exact(BUILD, [(p, x)])
    dx = dev(x)
    with ctx.symbol_sync(hz.SYMSYNC_REAL_F32, p, rows=r) as f:
        bound = f.max_symbols(n)
        assert bound == ref.max_symbols(n, p)
        head = f.ragged(*f.push(dx[:, :n] if r > 1 else dx[0, :n]))
        z0, p0 = f.state()
        out = torch.zeros((r, bound), dtype=torch.float32, device="cuda")
        cnt = torch.full((r,), 9, dtype=torch.int32, device="cuda")
        most = C.c_size_t(7)
        part = dx[:, n:].contiguous()
        with pytest.raises(hz.ErrDstTooSmall):
            ctx._ck(lib.hzsdr_symsync_push(f._h, part.data_ptr(), n, n, out.data_ptr(), bound - 1, bound, cnt.data_ptr(), C.byref(most)))
        assert most.value == 0
        if r > 1:
            with pytest.raises(hz.ErrDstTooSmall):
                ctx._ck(lib.hzsdr_symsync_push(f._h, part.data_ptr(), n, n, out.data_ptr(), bound, bound - 1, cnt.data_ptr(), None))
            with pytest.raises(hz.ErrInvalidArgument):
                ctx._ck(lib.hzsdr_symsync_push(f._h, part.data_ptr(), n, n - 1, out.data_ptr(), bound, bound, cnt.data_ptr(), None))
        with pytest.raises(hz.ErrInvalidArgument):
            ctx._ck(lib.hzsdr_symsync_push(f._h, None, n, n, out.data_ptr(), bound, bound, cnt.data_ptr(), None))
        with pytest.raises(hz.ErrInvalidArgument):
            ctx._ck(lib.hzsdr_symsync_push(f._h, part.data_ptr(), n, n, out.data_ptr(), bound, bound, None, None))
        torch.cuda.synchronize()
        z1, p1 = f.state()
        assert p1 == p0 == n and np.array_equal(bits(z1), bits(z0)) and (cnt == 9).all() and not out.any()
        # the exact capacity is taken, and max_written is the largest count
        ctx._ck(lib.hzsdr_symsync_push(f._h, part.data_ptr(), n, n, out.data_ptr(), bound, bound, cnt.data_ptr(), C.byref(most)))
        tail = f.ragged(out if r > 1 else out[0], cnt)
        z, pos = f.state()
        assert most.value == int(cnt.max()) and pos == 2 * n and np.array_equal(bits(z), bits(wz))
        for i in range(r):
            got = np.concatenate([head[i], tail[i]])
            assert len(got) == wc[i] and np.array_equal(bits(got), bits(y[i, :wc[i]])), f"row {i}"
        # reset: position 0, the initial state, the first stream again
        f.reset()
        z, pos = f.state()
        assert pos == 0 and z[:, 1].tolist() == [2.5] * r and not np.delete(z, 1, axis=1).any()
        again = f.ragged(*f.push(dx[:, :n] if r > 1 else dx[0, :n]))
        assert all(np.array_equal(bits(u), bits(v)) for u, v in zip(again, head))


def test_create_errors(hz, ctx):
    lib = importlib.import_module("go-sdr_amd._capi").lib
    out = C.c_void_p()
    good = params_for(hz, 5.0)

    def create(kind, p, per_row=0, rows=1):
        ptr = p.ctypes.data_as(C.POINTER(C.c_float)) if p is not None else None
        return lib.hzsdr_symsync_create(ctx._h, kind, ptr, per_row, rows, C.byref(out))

    inval = hz.ErrInvalidArgument.status
    assert create(hz.SYMSYNC_REAL_F32, good, 0, 0) == inval and create(hz.SYMSYNC_REAL_F32, good, 0, hz.SYMSYNC_MAX_ROWS + 1) == inval
    assert create(hz.SYMSYNC_REAL_F32, None) == inval
    for k, v in ((0, 2.0), (0, 257.0), (0, np.nan), (1, 0.26), (1, -0.01), (2, -1.0), (2, 1.6), (3, -1.0), (3, np.inf)):
        p = good.copy()
        p[k] = v
        assert create(hz.FMT_C64, p) == inval, f"parameter {k} = {v}"
    per = np.broadcast_to(good, (3, 4)).copy()
    per[2, 0] = 2.0
    assert create(hz.SYMSYNC_REAL_F32, per, 1, 3) == inval, "a refused parameter of the last row"
    for kind in (0, hz.FMT_U8, hz.FMT_I16, hz.FMT_I8, 5, 31, 33, -1):
        assert create(kind, good) == hz.ErrSampleFormatUnknown.status, f"kind {kind}"
    assert create(hz.SYMSYNC_REAL_F32, good, 0, hz.SYMSYNC_MAX_ROWS) == 0 and lib.hzsdr_symsync_free(out) == 0
    with pytest.raises(hz.ErrInvalidArgument):
        ctx.symbol_sync(hz.SYMSYNC_REAL_F32, np.zeros((2, 4), np.float32), rows=3)


# ---- 6. isolation ----------------------------------------------------------------------------------

def test_a_nan_stays_in_its_row(hz, ctx):
    """A NaN in one row of 2047 (two rows per wave): every other row keeps its symbols, counts and state; the row writes
    no more than its capacity; set_state heals it."""
    r, n, bad = 2047, T + 40, 5
    p = params_for(hz, 5.0)
    x = white("f32", (r, 2 * n), seed=31)
    y = x[:, :n].copy()
    y[bad, 10] = np.nan
    clean, both = ref.exact(BUILD, [(p, x[:, :n]), (p, x)])
    others = np.arange(r) != bad
    with ctx.symbol_sync(hz.SYMSYNC_REAL_F32, p, rows=r) as f:
        words, counts, bound = run(f, y, True)
        z, _ = f.state()
        assert counts[bad] <= bound
        counts2, words2 = counts.copy(), words.copy()
        counts2[bad], words2[bad] = clean[1][bad], SENTINEL  # (the row's own bits are not part of the contract)
        words2[bad, :clean[1][bad]] = bits(clean[0][bad, :clean[1][bad]])[:, None]
        check(words2, counts2, clean, "beside a NaN")
        assert np.array_equal(bits(z[others]), bits(clean[2][others])), "a NaN changed another row's state"
        assert (words[bad, counts[bad]:] == SENTINEL).all(), "the row wrote behind its count"
        # healed by the state of the clean run: the second half of the stream as if nothing had been
        f.set_state(clean[2], n)
        words, counts, _ = run(f, x[:, n:], True)
        z, pos = f.state()
    assert pos == 2 * n and np.array_equal(bits(z), bits(both[2]))
    for i in (0, bad, bad + 1, r - 1):
        got = words[i, :counts[i], 0]
        assert clean[1][i] + counts[i] == both[1][i] and np.array_equal(got, bits(both[0][i, clean[1][i]:both[1][i]])), f"row {i}"


# ---- 7. acquisition, the chain ---------------------------------------------------------------------

@pytest.mark.parametrize("sps,ppm,off,cplx", [(5.0, 200.0, 0.37, False), (8.0, 500.0, 0.5, True)])
def test_acquisition_on_the_device(hz, ctx, sps, ppm, off, cplx):
    """One case per kind of the definition's list, beside a row of its negative: the device's symbols are the
    program's, and they are the transmitted ones behind the first 1000."""
    a = ref.symbols(3000, 7 + int(sps * 10), cplx)
    x = ref.signal(a, sps * (1.0 + ppm * 1e-6), off)
    p = params_for(hz, sps)
    rows = np.stack([x, -x])
    ((y, wc, wz, _),) = ref.exact(BUILD, [(p, rows)])
    with ctx.symbol_sync(hz.FMT_C64 if cplx else hz.SYMSYNC_REAL_F32, p, rows=2) as f:
        s, c = f.push(dev(rows))
        got = f.ragged(s, c)
        z, _ = f.state()
    assert np.array_equal(bits(z), bits(wz))
    for i in range(2):
        assert len(got[i]) == wc[i] and np.array_equal(bits(got[i]), bits(y[i, :wc[i]]))
    lag, bad, n = ref.best_lag(got[0][:2980], a, 1000)
    level = np.abs(got[0][1000:2980].real).min()
    rel = abs(float(z[0, 1]) / (sps * (1.0 + ppm * 1e-6) / 2.0) - 1.0)
    print(f"sps {sps}: lag {lag}, {bad} of {n} differ, min level {level:.4f}, h at the end off by {rel:.2e}")
    assert n == 1980 and bad == 0 and level >= (0.6 if cplx else 0.85)


def test_behind_the_demodulator_and_the_iir_bank(hz, ctx):
    """12 rows of binary FSK at 5 samples per symbol: the FM demodulator's PITCHED float32 block goes into the bank as it
    is (the same pointer, a pitch above the count), and after it the IIR bank's block; both against the program over the
    same float32 block.  The symbols behind the smoother are the transmitted ones."""
    r, sps, nsym = 12, 5.0, 700
    a = np.stack([ref.symbols(nsym, 100 + i) for i in range(r)])
    f_dev = np.stack([ref.signal(a[i], sps, 0.1 * i + 0.05)[:3490] for i in range(r)]).astype(np.float64)
    ph = np.cumsum(f_dev, axis=1) * (np.pi / 4.0)
    x = np.exp(1j * ph).astype(np.complex64)
    n = x.shape[1]
    p = params_for(hz, sps)
    smooth = hz.lowpass(8000.0, 0.7071, 48_000.0)
    unit = np.array([4.0 / np.pi], np.float32)  # (radians per sample -> unit symbol amplitude)
    with ctx.demodulator(hz.FMT_C64, hz.DEMOD_FM, unit, streams=r) as dm, ctx.iir_bank(hz.IIR_REAL_F32, smooth, rows=r) as lp, \
            ctx.symbol_sync(hz.SYMSYNC_REAL_F32, p, rows=r) as s1, ctx.symbol_sync(hz.SYMSYNC_REAL_F32, p, rows=r) as s2:
        block = torch.zeros((r, n + 9), dtype=torch.float32, device="cuda")
        d = dm.push(dev(x), out=block)
        assert d.shape == (r, n) and d.stride(0) == n + 9 and d.data_ptr() == block.data_ptr()
        got1 = s1.ragged(*s1.push(d))
        audio = lp.push(d)
        got2 = s2.ragged(*s2.push(audio))
        z1, z2 = s1.state()[0], s2.state()[0]
    w1, w2 = ref.exact(BUILD, [(p, host(d)), (p, host(audio))])
    for got, want, z in ((got1, w1, z1), (got2, w2, z2)):
        assert np.array_equal(bits(z), bits(want[2]))
        for i in range(r):
            assert len(got[i]) == want[1][i] and np.array_equal(bits(got[i]), bits(want[0][i, :want[1][i]])), f"row {i}"
    scale = np.abs(host(d)).max()
    assert 0.9 < scale < 1.6, scale  # (unit symbols; the raised cosine overshoots to 1.49 between them)
    for i in (0, r - 1):
        lag, bad, k = ref.best_lag(got2[i][:650], a[i], 300)
        assert k == 350 and bad == 0, f"row {i}: {bad} of {k} symbols differ at lag {lag}"


# ---- 8. the other layers ---------------------------------------------------------------------------

def _run(exe):
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "go-sdr_amd") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    return subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)


def test_c_symsync_walkthrough(hz):
    """tests/c/test_symsync_abi.c compiled by gcc as C99 and run against libhzsdr_hip.so."""
    exe = os.path.join(BUILD, "test_symsync_abi")
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "test_symsync_abi.c"), "-L" + os.path.join(ROOT, "go-sdr_amd"),
                           "-lhzsdr_hip", "-lm", "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    p = _run(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "symsync-abi ok" in p.stdout


def test_cxx_symsync(hz):
    """tests/cxx/test_symsync.cpp (hzsdr::stream::SymbolSync of go-sdr_amd/cxx/hzsdr.hpp) built with g++ and run."""
    exe = os.path.join(BUILD, "test_symsync_cxx")
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + ROOT, os.path.join(ROOT, "tests", "cxx", "test_symsync.cpp"),
                           "-L" + os.path.join(ROOT, "go-sdr_amd"), "-lhzsdr_hip", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    p = _run(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "symsync-cxx ok" in p.stdout


def test_symbol_rows_over_a_reader(hz, hctx):
    """stream.symbol_rows over a BufferReader with short reads is one push of the whole stream; fed with
    iir_rows(demodulator_blocks(...)), it takes the chain's float32 blocks."""
    st = importlib.import_module("go-sdr_amd.stream")
    a = ref.symbols(1000, 3, True)
    x = ref.signal(a, 5.0, 0.3)
    p = params_for(hz, 5.0)
    ((y, wc, _, _),) = ref.exact(BUILD, [(p, x)])
    with hctx.symbol_sync(hz.FMT_C64, p) as f:
        blocks = [f.ragged(s, c)[0] for s, c in st.symbol_rows(st.BufferReader(x, 48_000, max_read=777), f, block=1024)]
        assert f.position() == len(x)
    got = np.concatenate(blocks)
    assert len(blocks) > 3 and got.dtype == np.complex64 and len(got) == wc[0] and np.array_equal(bits(got), bits(y[0, :wc[0]]))
    with hctx.symbol_sync(hz.SYMSYNC_REAL_F32, p) as f, pytest.raises(hz.ErrSampleFormatMismatch):
        list(st.symbol_rows(st.BufferReader(x, 48_000), f))
    # the demodulator's blocks through a smoother into the bank
    smooth = hz.one_pole(0.7)
    with hctx.demodulator(hz.FMT_C64, hz.DEMOD_FM) as dm, hctx.iir_bank(hz.IIR_REAL_F32, smooth) as lp:
        audio = np.array(lp.push(np.concatenate([dm.push(x), dm.flush()])))
    ((y, wc, _, _),) = ref.exact(BUILD, [(p, audio)])
    with hctx.demodulator(hz.FMT_C64, hz.DEMOD_FM) as dm, hctx.iir_bank(hz.IIR_REAL_F32, smooth) as lp, hctx.symbol_sync(hz.SYMSYNC_REAL_F32, p) as f:
        chain = st.iir_rows(st.demodulator_blocks(st.BufferReader(x, 48_000, max_read=777), dm, block=1024), lp)
        got = np.concatenate([f.ragged(s, c)[0] for s, c in st.symbol_rows(chain, f)])
    assert got.dtype == np.float32 and len(got) == wc[0] and np.array_equal(bits(got), bits(y[0, :wc[0]]))

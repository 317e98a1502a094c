"""The polyphase rational resampler (include/hzsdr_resampler.h) on the GPU: every block of 256 outputs against the
float64 restatement of tests/resampler_ref.py within bound(Q) = 6e-8 (Q + 2), over a list of shapes that takes every
kernel form the planner can choose and its largest LDS request; every table entry read out on its own by impulse
trains, EQUAL to the float64 reference (tests/readout.py); bit for bit across cuts, memory spaces, stream counts,
pitches, sub-slices and runs; behind the GPU channelizer; errors and state; the C and C++ layers."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import readout as ro
import resampler_ref as ref
from conftest import ROOT
from util import FMT, splitmix64

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BLOCK = 256
# (U, D, L) of the accuracy list (tests/readout.py has it, with the planner's tiles, for the CPU tests too)
SHAPES = [s[:3] for s in ro.RESAMPLER_SHAPES[:-1]]
# beside the list: the direct form with the table in memory
EXTRA_SHAPES = [s[:3] for s in ro.RESAMPLER_SHAPES[-1:]]
TILE = {s[:3]: s[3] for s in ro.RESAMPLER_SHAPES}
# the shapes whose blocks are checked for i8 and i16 sources too: T1024 pad (lds at the largest request, uniform), T256
# pad (lds at the largest request, global), both direct forms and one plain shape
ALL_SOURCES = {(2, 5, 50), (1, 4, 64), (170, 845, 5440), (26, 498, 6110), (40, 300, 8000), (1, 1024, 256), (32, 1024, 8192), (3, 2, 24)}
# the 11 combinations resampler_geom can reach: (tile, window padded, table form, direct)
FORMS = {(1024, pad, table, False) for pad in (False, True) for table in ("lds", "global", "uniform")} | {
    (256, True, table, False) for table in ("lds", "global", "uniform")} | {(256, False, table, True) for table in ("lds", "global")}


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


taps_of = ro.kaiser_taps  # a Kaiser-windowed sinc of any length, cutoff 1 / max(U, D), scaled to sum U, float32


def white(fmt, n, seed):
    """n white samples of the format: complex64 components in [-1, 1), or every byte / int16 value"""
    z = splitmix64(seed, 2 * n)
    if fmt == "c64":
        f = ((z >> np.uint64(40)).astype(np.float64) / float(1 << 23) - 1.0).astype(np.float32)
        return f.view(np.complex64).reshape(n)
    if fmt == "i16":
        return (z >> np.uint64(48)).astype(np.uint16).view(np.int16).reshape(n, 2)
    b = (z >> np.uint64(56)).astype(np.uint8)
    return (b if fmt == "u8" else b.view(np.int8)).reshape(n, 2)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits(t):
    t = t.detach().cpu() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return torch.view_as_real(t.contiguous()).contiguous().view(torch.int32)


def same(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and torch.equal(a, b)


def as_c64(ctx, x):
    """hzsdr_convert of device samples to complex64"""
    if x.dtype == torch.complex64:
        return x
    out = torch.empty(x.shape[0], dtype=torch.complex64, device=x.device)
    assert ctx.convert(out, x) == x.shape[0]
    return out


def run(rs, x, cuts=None, flush=True, check=None):
    """push x whole or cut at `cuts`, then flush; the pushes' outputs and the flush's, concatenated.  `check`, when
    given, is called after every push with the samples pushed so far."""
    c64 = "complex64" in str(x.dtype)
    n = x.shape[-1] if c64 else x.shape[-2]
    if cuts is None:
        cuts = [0, n]
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        out.append(rs.push(x[..., a:b] if c64 else x[..., a:b, :]))
        if check:
            check(b)
    if flush:
        out.append(rs.flush())
    if isinstance(out[0], torch.Tensor):
        torch.cuda.synchronize()
        return torch.cat(out, dim=-1)
    return np.concatenate(out, axis=-1)


samples_for = ro.samples_for  # the fewest samples after which `count` outputs have been written


def form_of(hz, tile, form):
    """the planner's report as (tile, window padded, table form, direct)"""
    table = "global" if form & hz.RESAMPLER_FORM_TAPS_GLOBAL else "uniform" if form & hz.RESAMPLER_FORM_TAPS_UNIFORM else "lds"
    return tile, bool(form & hz.RESAMPLER_FORM_WINDOW_PADDED), table, bool(form & hz.RESAMPLER_FORM_DIRECT)


def check_blocks(got, want, q, what):
    """every block of 256 outputs within bound(Q) relative L2; a block whose reference is identically zero is bit-zero"""
    got = np.asarray(got)
    assert got.shape == want.shape, f"{what}: {got.shape[0]} outputs, the reference has {want.shape[0]}"
    worst = 0.0
    for a in range(0, want.shape[0], BLOCK):
        g, w = got[a:a + BLOCK], want[a:a + BLOCK]
        nw = np.linalg.norm(w)
        if nw == 0.0:
            assert not g.view(np.uint32).any(), f"{what}: block {a // BLOCK} of an all-zero reference is not bit-zero"
            continue
        e = np.linalg.norm(g.astype(np.complex128) - w) / nw
        worst = max(worst, e)
        assert e <= ref.bound(q), f"{what}: block {a // BLOCK}: relative L2 {e:.3e} > {ref.bound(q):.3e}"
    return worst


# ---- 1. accuracy against float64 -------------------------------------------------------------------

@pytest.mark.parametrize("up,down,ntaps", SHAPES + EXTRA_SHAPES)
def test_blocks_against_float64(hz, ctx, up, down, ntaps):
    """Streams whose output counts land on T - 1, T, T + 1 and 2 T + 3 (as near as U/D allows; three workgroups),
    c64 and u8 (i8 and i16 too for the shapes of ALL_SOURCES), every block of 256 outputs of pushes and flush against
    upfirdn_poly of the converted samples."""
    h = taps_of(up, down, ntaps)
    q = -(-ntaps // up)
    for fmt in (("c64", "u8", "i8", "i16") if (up, down, ntaps) in ALL_SOURCES else ("c64", "u8")):
        rs = ctx.resampler(FMT[fmt], up, down, h)
        tile, form = rs.plan()
        assert tile == TILE[(up, down, ntaps)]
        worst = 0.0
        for target in (tile - 1, tile, tile + 1, 2 * tile + 3):
            n = samples_for(target, up, down)
            x = dev(white(fmt, n, seed=up * 1009 + down * 31 + n))
            assert rs.outputs_for(n) == ref.outputs_after(n, up, down) >= target
            got = run(rs, x).cpu().numpy()
            assert rs.pending() == (0, 0, 0)
            want = ref.upfirdn_poly(h, as_c64(ctx, x).cpu().numpy(), up, down)
            assert want.shape[0] == ref.total_outputs(n, ntaps, up, down)
            assert got.shape[0] == ref.stream_outputs(n, ntaps, up, down)
            if got.shape[0] > want.shape[0]:  # (L < U: the pushes' last outputs lie past upfirdn's end, all padding taps)
                assert not got[want.shape[0]:].view(np.uint32).any(), "outputs of padding taps alone are not bit-zero"
                got = got[:want.shape[0]]
            worst = max(worst, check_blocks(got, want, q, f"U={up} D={down} L={ntaps} {fmt} n={n}"))
        rs.close()
        print(f"U={up} D={down} L={ntaps} Q={q} {fmt}: T={tile} form={form}: worst block {worst:.3e} (bound {ref.bound(q):.3e})")


def test_the_list_covers_every_form(hz, ctx):
    """Over the accuracy list every combination of tile, window padding, table form and direct that the planner can
    reach occurs, by the planner's own report: a changed threshold cannot quietly leave a form untested.  The i8 and
    i16 shapes cover a padded four-chain, a padded one-chain and both direct forms."""
    forms, combos = {}, {}
    for up, down, ntaps in SHAPES + EXTRA_SHAPES:
        with ctx.resampler(hz.FMT_C64, up, down, taps_of(up, down, ntaps)) as rs:
            tile, form = rs.plan()
        combos[(up, down, ntaps)] = form_of(hz, tile, form)
        if (up, down, ntaps) in SHAPES:
            forms[(up, down, ntaps)] = form
    print(combos)
    assert set(combos.values()) == FORMS and len(FORMS) == 11, sorted(FORMS - set(combos.values()))
    assert {(t, p, d) for t, p, _, d in (combos[s] for s in ALL_SOURCES)} >= {(1024, True, False), (256, True, False), (256, False, True)}
    # the shapes the findings named take the forms they were added for, the largest LDS requests among them
    for shape, combo in {(1, 2, 31): (1024, True, "uniform", False), (1, 4, 64): (1024, True, "uniform", False),
                         (2, 5, 50): (1024, True, "lds", False), (64, 135, 7000): (1024, True, "global", False),
                         (3, 20, 90): (256, True, "lds", False), (40, 300, 8000): (256, True, "global", False),
                         (170, 845, 5440): (1024, True, "lds", False), (26, 498, 6110): (256, True, "lds", False)}.items():
        assert combos[shape] == combo, (shape, combos[shape])
    # (that (26, 498, 6110) is the planner's largest LDS request is asserted where the search runs: tests/test_resampler_plan.py)
    direct = {bool(f & hz.RESAMPLER_FORM_DIRECT) for f in forms.values()}
    tglobal = {bool(f & hz.RESAMPLER_FORM_TAPS_GLOBAL) for f in forms.values()}
    print(forms)
    assert direct == {False, True} and tglobal == {False, True}
    # where U divides D the one row in use is read as scalars: both kinds of in-LDS-or-not shapes are in the list
    uniform = {k: bool(f & hz.RESAMPLER_FORM_TAPS_UNIFORM) for k, f in forms.items()}
    assert uniform[(1, 8, 128)] and uniform[(5, 5, 20)] and not uniform[(3, 2, 24)] and not uniform[(160, 147, 1920)]
    assert any(f == 0 for f in forms.values()), "no shape of the list has window and table in LDS"
    assert forms[(147, 160, 18816)] & hz.RESAMPLER_FORM_TAPS_GLOBAL and forms[(1, 1024, 256)] & hz.RESAMPLER_FORM_DIRECT
    for up, down, ntaps in EXTRA_SHAPES:
        with ctx.resampler(hz.FMT_C64, up, down, taps_of(up, down, ntaps)) as rs:
            assert rs.plan()[1] == hz.RESAMPLER_FORM_DIRECT | hz.RESAMPLER_FORM_TAPS_GLOBAL


# ---- 1b. every table entry on its own ---------------------------------------------------------------

@pytest.mark.parametrize("shape", ro.RESAMPLER_SHAPES, ids=lambda s: "U%d-D%d-L%d" % s[:3])
def test_tap_readout(hz, ctx, shape):
    """Q rows, row r zero but for impulses of power-of-two amplitude at r, r + Q, r + 2 Q, ...: every output is ONE
    exact product h[phi_m + q U] amp, every other term fma(h, +-0, acc), so pushes and flush EQUAL the float64
    reference rounded to complex64 -- no tolerance.  Across the rows every output meets every q: every entry of the
    polyphase table that a stream can read is read (the share is computed from the definition's indices and must be
    100 %).  Cut inside the first Q - 1 samples and at T - 1 outputs, then flushed, so the held tail's values are read
    out too.  c64, i8 and i16 (u8's conversion has no zero); the one shape whose rows would be a gigabyte runs i8
    alone over T + 3 outputs."""
    up, down, ntaps, tile = shape
    q = -(-ntaps // up)
    h = taps_of(up, down, ntaps)
    count = ro.readout_outputs(shape)
    n = samples_for(count, up, down)
    # `exist` counts the entries hp[phi][q] with phi + q U < L whose phase a stream can have: phi a multiple of
    # gcd(U, D).  Where U and D share a factor (as at (5, 5, 20)) no input reaches the other phases, so they are left
    # out of the 100 %; for coprime U and D this is every entry with phi + q U < L.
    read, exist = ro.resampler_coverage(n, ntaps, up, down)
    assert read == exist > 0, f"{read} of {exist} table entries read"
    c0 = max(1, (q - 1) // 2)
    cuts = sorted({0, min(c0, n), min(max(c0, samples_for(tile - 1, up, down)), n), n})
    for fmt in (("i8",) if shape == ro.READOUT_SMALL else ("c64", "i8", "i16")):
        raw = ro.train_rows(fmt, n, q)
        x = dev(raw if q > 1 else raw[0])
        del raw
        if fmt != "c64":  # the values were chosen so that the conversion is an exact power of two
            assert np.array_equal(as_c64(ctx, x[0] if q > 1 else x).cpu().numpy(), ro.train(fmt, n, q, first=0)[1])
        with ctx.resampler(FMT[fmt], up, down, h, streams=q) as rs:
            assert rs.plan()[0] == tile
            got = run(rs, x, cuts).cpu().numpy().reshape(q, -1)
        total = ref.total_outputs(n, ntaps, up, down)
        assert got.shape[1] == ref.stream_outputs(n, ntaps, up, down) >= count
        assert not got[:, total:].any(), "outputs of padding taps alone are not zero"
        for r in range(q):
            want = ref.upfirdn_poly(h, ro.train(fmt, n, q, first=r)[1], up, down)
            if not ro.readout_equal(got[r, :total], want):
                bad = np.flatnonzero(~(got[r, :total] == want.astype(np.complex64)))
                m = int(bad[0])
                raise AssertionError(f"U={up} D={down} L={ntaps} {fmt} row {r}: {bad.size} outputs differ, the first m = {m} "
                                     f"(phi {m * down % up}, i {m * down // up}): {got[r, m]} for {want[m]}")
    print(f"U={up} D={down} L={ntaps} Q={q}: {read} of {exist} table entries read and equal over {q} rows of {got.shape[1]} outputs, cuts {cuts}")


# ---- 2. identity -----------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["u8", "i8", "i16"])
def test_identity_equals_convert(hz, ctx, fmt):
    """U = D = 1, h = [1.0]: bit-equal to hzsdr_convert to complex64."""
    with ctx.resampler(FMT[fmt], 1, 1, np.ones(1, np.float32)) as rs:
        tile, _ = rs.plan()
        x = dev(white(fmt, 2 * tile + 3, seed=17))
        got = rs.push(x)
        assert rs.pending() == (2 * tile + 3, 2 * tile + 3, 0) and rs.flush().shape[0] == 0
        torch.cuda.synchronize()
        assert same(got, as_c64(ctx, x))


# ---- 3. cuts ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("up,down,ntaps", [(3, 2, 24), (160, 147, 1920), (1, 8, 128), (2, 5, 50)])
@pytest.mark.parametrize("fmt", ["c64", "u8"])
def test_cuts_bit_identical(hz, ctx, up, down, ntaps, fmt):
    h = taps_of(up, down, ntaps)
    q = -(-ntaps // up)
    rs = ctx.resampler(FMT[fmt], up, down, h)
    tile, _ = rs.plan()
    n = samples_for(2 * tile + 3, up, down)
    x = dev(white(fmt, n, seed=n + up))
    one = run(rs, x)
    assert one.shape[0] == ref.total_outputs(n, ntaps, up, down)
    # a cut inside the first Q - 1 samples, a push of nothing, a push of one sample, and ragged ones
    c0 = max(1, (q - 1) // 2)
    cuts = [0, c0, c0, c0 + 1, c0 + 2, c0 + 2 + samples_for(tile - 1, up, down), n - 1, n]
    assert cuts == sorted(cuts) and cuts[-2] > cuts[-3]
    empty = []

    def check(done, last=[0]):
        assert rs.pending()[:2] == (done, ref.outputs_after(done, up, down))
        assert rs.pending()[2] == ref.total_outputs(done, ntaps, up, down) - ref.outputs_after(done, up, down)
        assert rs.outputs_for(5) == ref.outputs_after(done + 5, up, down) - ref.outputs_after(done, up, down)
        if done > last[0] and ref.outputs_after(done, up, down) == ref.outputs_after(last[0], up, down):
            empty.append(done)
        last[0] = done

    cut = run(rs, x, cuts, check=check)
    if down > up:
        assert empty, "no push of samples that completes no output among the cuts"
    assert same(cut, one)
    small = x[:300]
    want = run(rs, small)

    def counts(done):
        assert rs.pending()[:2] == (done, ref.outputs_after(done, up, down))

    got = run(rs, small, list(range(301)), check=counts)
    assert same(got, want) and got.shape[0] == ref.total_outputs(300, ntaps, up, down)
    rs.close()


# ---- 4. streams and pitch --------------------------------------------------------------------------

@pytest.mark.parametrize("streams,fmt,up,down,ntaps", [(5, "u8", 3, 2, 24), (256, "c64", 2, 3, 50), (5, "c64", 1, 1024, 256),
                                                      (5, "i16", 2, 5, 50)])
def test_streams_and_pitch(hz, ctx, hctx, streams, fmt, up, down, ntaps):
    """Rows that differ, an input pitch above n, an output pitch above the count: every row bit-equal to a
    single-stream object on that row, guard columns intact; HOST results bit-equal to DEVICE ones."""
    h = taps_of(up, down, ntaps)
    rs = ctx.resampler(FMT[fmt], up, down, h, streams=streams)
    single = ctx.resampler(FMT[fmt], up, down, h)
    tile, _ = rs.plan()
    n = samples_for(tile + 37, up, down)
    n1 = n // 3  # (two pushes: the held tails of the rows are in play)
    pad = 5
    wide = white(fmt, streams * (n + pad), seed=streams + n)
    wide = wide.reshape((streams, n + pad) + wide.shape[1:])
    dwide = dev(wide)
    xs = dwide[:, :n]
    counts = [ref.outputs_after(n1, up, down), ref.outputs_after(n, up, down) - ref.outputs_after(n1, up, down),
              ref.total_outputs(n, ntaps, up, down) - ref.outputs_after(n, up, down)]
    total = sum(counts)
    nan = torch.full((streams, total + 7), float("nan"), dtype=torch.float32, device="cuda")
    out = torch.complex(nan, nan.clone())
    guard = bits(out[:, total:]).clone()
    done = 0
    for part, c in zip((xs[:, :n1], xs[:, n1:], None), counts):
        w = rs.push(part, out=out[:, done:]) if part is not None else rs.flush(out=out[:, done:])
        assert w.shape == (streams, c)
        done += c
    torch.cuda.synchronize()
    assert torch.equal(bits(out[:, total:]), guard), "columns past the outputs written were touched"
    assert not torch.isnan(torch.view_as_real(out[:, :total])).any()
    for s in range(streams):
        want = run(single, xs[s].contiguous(), [0, n1, n])
        assert same(out[s, :total], want), f"row {s} differs from the single-stream run"
    # HOST context, unpinned and pinned destinations, the same pitches
    hrs = hctx.resampler(FMT[fmt], up, down, h, streams=streams)
    pinned = hctx.pinned_samples(hz.FMT_C64, streams * (total + 7)).reshape(streams, total + 7)
    for dst in (np.empty((streams, total + 7), np.complex64), pinned):
        dst[:] = np.complex64(complex(np.nan, np.nan))
        done = 0
        for part, c in zip((wide[:, :n1], wide[:, n1:n], None), counts):
            w = hrs.push(part, out=dst[:, done:]) if part is not None else hrs.flush(out=dst[:, done:])
            assert w.shape == (streams, c)
            done += c
        assert same(dst[:, :total], out[:, :total]) and np.isnan(dst[:, total:]).all()
    for o in (rs, single, hrs):
        o.close()


# ---- 5. sub-slices ---------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,start", [("u8", 1), ("u8", 3), ("i16", 1), ("i16", 3), ("c64", 1)])
def test_sub_slices(hz, ctx, fmt, start):
    """Input starting `start` samples into its buffer, output starting one value into its own: the bits of the
    aligned run, guards on both sides of the output intact."""
    up, down, ntaps = 3, 2, 24
    h = taps_of(up, down, ntaps)
    rs = ctx.resampler(FMT[fmt], up, down, h)
    tile, _ = rs.plan()
    n = samples_for(tile + 5, up, down)
    x = white(fmt, n, seed=start + 40)
    aligned = run(rs, dev(x))
    total = aligned.shape[0]
    buf = dev(np.concatenate([white(fmt, start, seed=1), x, white(fmt, 2, seed=2)]))
    nan = torch.full((total + 3,), float("nan"), dtype=torch.float32, device="cuda")
    out = torch.complex(nan, nan.clone())
    a = rs.push(buf[start:start + n], out=out[1:])
    b = rs.flush(out=out[1 + a.shape[0]:])
    torch.cuda.synchronize()
    assert a.shape[0] + b.shape[0] == total
    assert same(out[1:1 + total], aligned)
    assert torch.isnan(torch.view_as_real(out[:1])).all() and torch.isnan(torch.view_as_real(out[1 + total:])).all()
    rs.close()


# ---- 6. behind the channelizer ---------------------------------------------------------------------

def test_the_channelizer_feeds_it(hz, ctx):
    """The channelizer's channel-major tensor, with its pitch, straight into a 256-stream resampler by 4/1."""
    m, p, hop, up, down, ntaps = 256, 4, 192, 4, 1, 48
    n = p * m + 40 * hop
    ch = ctx.channelizer(hz.FMT_C64, m, hz.channelizer_taps(m, p), hop=hop, layout="channels")
    frames = ch.frames_for(n)
    buf = torch.zeros((m, frames + 9), dtype=torch.complex64, device="cuda")
    rows = ch.push(dev(white("c64", n, seed=77)), out=buf)
    assert rows.shape == (m, frames) and rows.stride(0) == frames + 9
    h = taps_of(up, down, ntaps)
    rs = ctx.resampler(hz.FMT_C64, up, down, h, streams=m)
    single = ctx.resampler(hz.FMT_C64, up, down, h)
    got = run(rs, rows)
    assert got.shape == (m, ref.total_outputs(frames, ntaps, up, down))
    for k in range(m):
        assert same(got[k], run(single, rows[k].contiguous())), f"channel row {k}"
    k = 37
    check_blocks(got[k].cpu().numpy(), ref.upfirdn_poly(h, rows[k].cpu().numpy(), up, down), ntaps // up, f"channel row {k}")
    for o in (ch, rs, single):
        o.close()


# ---- 7. errors and state ---------------------------------------------------------------------------

def test_create_errors(hz, ctx):
    h = taps_of(3, 2, 24)
    for kw in (dict(up=1025), dict(down=1025), dict(up=0), dict(down=0), dict(streams=8193), dict(streams=0)):
        args = dict(up=3, down=2, streams=1)
        args.update(kw)
        with pytest.raises(hz.ErrInvalidArgument):
            ctx.resampler(hz.FMT_C64, args["up"], args["down"], h, streams=args["streams"])
    lib = importlib.import_module("go-sdr_amd._capi").lib
    out = C.c_void_p()

    def create(fmt, up, down, taps, n, streams=1):
        p = taps.ctypes.data_as(C.POINTER(C.c_float)) if taps is not None else None
        return lib.hzsdr_resampler_create(ctx._h, fmt, up, down, p, n, streams, C.byref(out))

    inval = hz.ErrInvalidArgument.status
    assert create(hz.FMT_C64, 0, 2, h, 24) == create(hz.FMT_C64, 3, 1025, h, 24) == create(hz.FMT_C64, 3, 2, h, 24, 8193) == inval
    big = np.ones(65537, np.float32)
    assert create(hz.FMT_C64, 3, 2, None, 24) == inval, "null taps"
    assert create(hz.FMT_C64, 3, 2, h, 0) == inval, "L = 0"
    assert create(hz.FMT_C64, 1024, 2, big, 65537) == inval, "L above 65536"
    assert create(hz.FMT_C64, 1, 2, big, 257) == inval, "Q above 256"
    assert create(hz.FMT_C64, 1, 2, big, 256) == 0 and lib.hzsdr_resampler_free(out) == 0
    for bad in (np.nan, np.inf, -np.inf):
        g = h.copy()
        g[7] = bad
        assert create(hz.FMT_C64, 3, 2, g, 24) == inval, "a non-finite tap"
    with pytest.raises(hz.HzsdrError) as e:
        ctx.resampler(9, 3, 2, h)
    assert type(e.value).__name__ == "ErrSampleFormatUnknown"


def test_in_stride_below_the_push(hz, ctx):
    lib = importlib.import_module("go-sdr_amd._capi").lib
    with ctx.resampler(hz.FMT_C64, 3, 2, taps_of(3, 2, 24), streams=2) as rs:
        x = torch.zeros((2, 10), dtype=torch.complex64, device="cuda")
        out = torch.zeros((2, 32), dtype=torch.complex64, device="cuda")
        got = C.c_size_t(5)
        rc = lib.hzsdr_resampler_push(rs._h, x.data_ptr(), 10, 9, out.data_ptr(), 32, 32, C.byref(got))
        assert rc == hz.ErrInvalidArgument.status and got.value == 0 and rs.pending() == (0, 0, 0)


@pytest.mark.parametrize("streams", [1, 3])
def test_dst_too_small_leaves_state(hz, ctx, streams):
    up, down, ntaps = 3, 2, 24
    h = taps_of(up, down, ntaps)
    lib = importlib.import_module("go-sdr_amd._capi").lib
    x = dev(white("c64", streams * 200, seed=5).reshape(streams, 200))
    x = x[0] if streams == 1 else x
    rs = ctx.resampler(hz.FMT_C64, up, down, h, streams=streams)
    want = run(rs, x, [0, 50, 200])
    first = rs.push(x[..., :50]).clone()
    state = rs.pending()
    count = rs.outputs_for(150)
    out = torch.zeros((streams, count), dtype=torch.complex64, device="cuda")
    got = C.c_size_t(7)
    part = x[..., 50:].contiguous()
    with pytest.raises(hz.ErrDstTooSmall):
        ctx._ck(lib.hzsdr_resampler_push(rs._h, part.data_ptr(), 150, 150, out.data_ptr(), count - 1, count, C.byref(got)))
    assert got.value == 0 and rs.pending() == state
    if streams > 1:
        with pytest.raises(hz.ErrDstTooSmall):
            ctx._ck(lib.hzsdr_resampler_push(rs._h, part.data_ptr(), 150, 150, out.data_ptr(), count, count - 1, C.byref(got)))
        assert rs.pending() == state
    with pytest.raises(hz.ErrDstTooSmall):
        ctx._ck(lib.hzsdr_resampler_flush(rs._h, out.data_ptr(), state[2] - 1, count, C.byref(got)))
    assert rs.pending() == state
    rest = torch.cat([rs.push(part), rs.flush()], dim=-1)
    torch.cuda.synchronize()
    assert same(torch.cat([first, rest], dim=-1), want)
    rs.close()


def test_reset_flush_and_runs(hz, ctx):
    up, down, ntaps = 160, 147, 1920
    h = taps_of(up, down, ntaps)
    x = dev(white("u8", 1500, seed=8))
    rs = ctx.resampler(hz.FMT_U8, up, down, h)
    assert rs.flush().shape[0] == 0 and rs.pending() == (0, 0, 0), "flush on a fresh object writes nothing"
    a = run(rs, x)
    assert rs.pending() == (0, 0, 0)
    b = run(rs, x)  # (flush, then a push: a new stream)
    rs.push(x[:700])
    rs.reset()
    assert rs.pending() == (0, 0, 0)
    c = run(rs, x)
    with ctx.resampler(hz.FMT_U8, up, down, h) as other:
        d = run(other, x)
    assert same(a, b) and same(a, c) and same(a, d)
    rs.close()


# ---- 8. the other layers ---------------------------------------------------------------------------

def _run(exe):
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "go-sdr_amd") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    return subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)


def test_c_resampler_walkthrough(hz):
    """tests/c/test_resampler_abi.c compiled by gcc as C99 and run against libhzsdr_hip.so."""
    exe = os.path.join(ROOT, "build", "test_resampler_abi")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "test_resampler_abi.c"), "-L" + os.path.join(ROOT, "go-sdr_amd"),
                           "-lhzsdr_hip", "-lm", "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    p = _run(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "resampler-abi ok" in p.stdout


def test_cxx_resampler(hz):
    """tests/cxx/test_resampler.cpp (hzsdr::stream::Resampler of go-sdr_amd/cxx/hzsdr.hpp) built with g++ and run."""
    exe = os.path.join(ROOT, "build", "test_resampler_cxx")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + ROOT, os.path.join(ROOT, "tests", "cxx", "test_resampler.cpp"),
                           "-L" + os.path.join(ROOT, "go-sdr_amd"), "-lhzsdr_hip", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    p = _run(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "resampler-cxx ok" in p.stdout


def test_resample_reader(hz, hctx):
    """stream.ResampleReader over a BufferReader with short reads: the pushes' outputs and the flush, i.e. one push
    plus flush, at the rate sample_rate * U / D."""
    st = importlib.import_module("go-sdr_amd.stream")
    up, down = 160, 147
    x = white("i16", 5000, seed=3)
    with hctx.resampler(hz.FMT_I16, up, down) as one:
        want = run(one, x)
    rs = hctx.resampler(hz.FMT_I16, up, down)
    r = st.ResampleReader(st.BufferReader(x, 44_100, max_read=777), rs, block=1024)
    assert r.sample_format() == hz.FMT_C64 and r.sample_rate() == 48_000.0
    got, buf = [], np.zeros(1000, np.complex64)
    while True:
        try:
            k = r.read(buf)
        except st.EOF:
            break
        got.append(buf[:k].copy())
    rs.close()
    assert same(np.concatenate(got), want) and want.shape[0] == ref.total_outputs(5000, 16 * up, up, down)

"""The demodulator bank (include/hzsdr_demod.h) on the GPU: every mode and every kernel shape BIT FOR BIT against the
outputs of tests/host/demod_ref.cpp (the host program over the header the kernel evaluates) and, within the bound
derived in tests/demod_ref.py, against the float64 restatement; the detector inputs that can go wrong; an FM tone;
bit for bit across cuts, memory spaces, stream counts, pitches, sub-slices and runs; behind the GPU channelizer; errors
and state; the C and C++ layers."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import demod_ref as ref
from conftest import ROOT
from util import FMT, splitmix64

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BUILD = os.path.join(ROOT, "build")
MODES = ["fm", "phase", "envelope", "power"]
# (Q, D): the bare detector; odd and even D; Q above the 8-tap trips and not a multiple of them; the four tile sizes
# (1024, 512, 256 and the half tile of 128 outputs, tests/test_demod_plan.py has the planner's thresholds)
SHAPES = [(1, 1), (7, 3), (33, 1), (64, 5), (256, 8), (129, 64), (1024, 64), (1024, 1)]
TILE = {(1, 1): 1024, (7, 3): 1024, (33, 1): 1024, (64, 5): 1024, (256, 8): 1024, (129, 64): 256, (1024, 64): 128, (1024, 1): 1024}


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


def taps_of(q, seed=0):
    """q float32 taps of both signs, sum |h| about 1"""
    h = np.random.default_rng(1000 * q + seed).standard_normal(q)
    return (h / np.abs(h).sum()).astype(np.float32) if q > 1 else np.ones(1, np.float32)


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
    return t.contiguous().view(torch.int32)


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


def run(dm, x, cuts=None, flush=True, check=None):
    """push x whole or cut at `cuts`, then flush; the pushes' outputs and the flush's, concatenated"""
    c64 = "complex64" in str(x.dtype)
    n = x.shape[-1] if c64 else x.shape[-2]
    if cuts is None:
        cuts = [0, n]
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        out.append(dm.push(x[..., a:b] if c64 else x[..., a:b, :]))
        if check:
            check(b)
    if flush:
        out.append(dm.flush())
    if isinstance(out[0], torch.Tensor):
        torch.cuda.synchronize()
        return torch.cat(out, dim=-1)
    return np.concatenate(out, axis=-1)


def first_difference(got, want):
    g, w = np.asarray(got).view(np.uint32), np.asarray(want).view(np.uint32)
    bad = np.flatnonzero(g != w)
    m = int(bad[0])
    return f"{bad.size} of {w.size} outputs differ, the first m = {m}: {np.asarray(got)[m]!r} for {np.asarray(want)[m]!r}"


def check_stream(hz, ctx, mode, q, down, fmt, x, what, float64=True):
    """one whole stream through a fresh object: the counts, the bits of the host program, the float64 bound"""
    h = taps_of(q)
    with ctx.demodulator(FMT[fmt], ref.MODES[mode], h, down) as dm:
        n = x.shape[0]
        assert dm.outputs_for(n) == ref.outputs_after(n, down)
        got = run(dm, x).cpu().numpy()
        assert dm.pending() == (0, 0, 0)
    xc = as_c64(ctx, x).cpu().numpy()
    (want,) = ref.exact(BUILD, [(ref.MODES[mode], down, h, xc)])
    assert got.shape == want.shape == (ref.total_outputs(n, q, down),)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{what}: {first_difference(got, want)}"
    if float64:
        y, mag = ref.demodulate(ref.MODES[mode], h, xc, down)
        err, bnd = np.abs(got.astype(np.float64) - y), ref.bound(ref.MODES[mode], h, mag)
        worst = int(np.argmax(err - bnd))
        print(f"{what}: worst |err| - bound at m = {worst}: {err[worst]:.3e} (bound {bnd[worst]:.3e}); max err {err.max():.3e}")
        assert (err <= bnd).all(), f"{what}: output {worst}: {err[worst]:.3e} > {bnd[worst]:.3e}"


# ---- 1. bit for bit against the host program, and within the bound of float64 ------------------------

@pytest.mark.parametrize("fmt", ["c64", "u8"])
@pytest.mark.parametrize("q,down", SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_streams_exact_and_float64(hz, ctx, mode, q, down, fmt):
    """N = 2 T D + 37 samples, two full tiles and a partial one, pushes and flush."""
    with ctx.demodulator(FMT[fmt], ref.MODES[mode], taps_of(q), down) as dm:
        tile, form = dm.plan()
    assert tile == TILE[(q, down)] and bool(form & hz.DEMOD_FORM_HALF_TILE) == (tile == 128)
    assert bool(form & hz.DEMOD_FORM_TRANSPOSED) == (down > 1)
    n = 2 * tile * down + 37
    x = dev(white(fmt, n, seed=q * 131 + down))
    check_stream(hz, ctx, mode, q, down, fmt, x, f"{mode} Q={q} D={down} {fmt} T={tile} n={n}")


@pytest.mark.parametrize("fmt", ["i8", "i16"])
@pytest.mark.parametrize("q,down", [(1, 1), (64, 5)])
@pytest.mark.parametrize("mode", MODES)
def test_streams_exact_other_sources(hz, ctx, mode, q, down, fmt):
    n = 2 * TILE[(q, down)] * down + 37
    check_stream(hz, ctx, mode, q, down, fmt, dev(white(fmt, n, seed=q + 7)), f"{mode} Q={q} D={down} {fmt} n={n}")


def test_the_list_covers_every_tile(hz, ctx):
    tiles = set()
    for q, down in SHAPES + [(600, 20)]:
        with ctx.demodulator(hz.FMT_C64, hz.DEMOD_FM, taps_of(q), down) as dm:
            tiles.add(dm.plan()[0])
    assert tiles == {1024, 512, 256, 128}


@pytest.mark.parametrize("mode", MODES)
def test_the_two_chain_tile(hz, ctx, mode):
    """(600, 20): the window of 1024 outputs is past the budget, that of 512 is not"""
    q, down = 600, 20
    with ctx.demodulator(hz.FMT_C64, ref.MODES[mode], taps_of(q), down) as dm:
        assert dm.plan()[0] == 512
    n = 2 * 512 * down + 37
    check_stream(hz, ctx, mode, q, down, "c64", dev(white("c64", n, seed=5)), f"{mode} Q={q} D={down} n={n}")


# ---- 2. detector inputs that can go wrong -------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_every_u8_pair(hz, ctx, mode):
    """All 65 536 (I, Q) byte pairs in sequence through the bare detector: every angle and magnitude the format has
    (and, for FM, every pair behind its predecessor in the sequence)."""
    v = np.arange(65536, dtype=np.uint32)
    x = np.stack([v & 0xff, v >> 8], axis=1).astype(np.uint8)
    check_stream(hz, ctx, mode, 1, 1, "u8", dev(x), f"{mode}: every u8 pair")


def special_c64():
    """both axes, +-0, |re| = |im|, denormals, 1e38, a sample after a zero sample.  No two neighbours whose product
    with the conjugate is inf - inf: the bits of a NaN are not part of the contract."""
    tiny, den, big = np.float32(1e-38), np.float32(1e-42), np.float32(1e38)
    one = np.float32(1.0)
    z = [complex(one, 0), complex(0, one), complex(-one, 0), complex(0, -one),            # the axes, in turn
         complex(0.0, 0.0), complex(one, one), complex(-0.0, 0.0), complex(0.5, -0.5),    # zeros, each followed by a sample
         complex(0.0, -0.0), complex(-one, one), complex(-0.0, -0.0), complex(-one, -one),
         complex(one, -0.0), complex(-one, -0.0), complex(-one, 0.0), complex(-0.0, one), complex(-0.0, -one),
         complex(den, 0), complex(0, den), complex(den, den), complex(-den, den), complex(den, -3 * den), complex(one, den),
         complex(den, one), complex(-one, den), complex(-one, -den), complex(tiny, tiny), complex(tiny, -den),
         complex(0.25, 0.25), complex(big, 0), complex(1e-3, 1e-3), complex(0, -big), complex(0.5, 0.25), complex(big, big),
         complex(0.0, 0.0), complex(-big, big), complex(1e-30, -1e-30), complex(big, den), complex(one, 0), complex(den, big),
         complex(0.0, 0.0), complex(0.0, 0.0), complex(3.0, -4.0)]
    a = np.zeros(len(z), np.complex64)
    a.real = [np.float32(v.real) for v in z]
    a.imag = [np.float32(v.imag) for v in z]
    return a


@pytest.mark.parametrize("mode", MODES)
def test_special_c64_inputs(hz, ctx, mode):
    x = special_c64()
    assert ((np.ascontiguousarray(x.real).view(np.uint32) & 0x7f800000) == 0).sum() > 8, "no denormal or zero components"
    xs = np.concatenate([x, x[::-1], x[::2]])
    h = np.ones(1, np.float32)
    with ctx.demodulator(hz.FMT_C64, ref.MODES[mode], h, 1) as dm:
        got = run(dm, dev(xs)).cpu().numpy()
    (want,) = ref.exact(BUILD, [(ref.MODES[mode], 1, h, xs)])
    assert not np.isnan(want).any(), "the list has neighbours that give a NaN"
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{mode}: {first_difference(got, want)}"
    zero = np.flatnonzero((xs.real == 0) & (xs.imag == 0))
    assert zero.size >= 6 and not got.view(np.uint32)[zero].any(), "a zero sample does not give +0"


def test_fm_of_a_tone(hz, ctx):
    """exp(2 pi i f n / fs): every d[n], n >= 1, is 2 pi f / fs within E (the arctangent) + 2^-22 (the angle error of
    the separately rounded product of two float32 unit vectors); with fm_gain in the tap, f / deviation."""
    fs, n = 48_000.0, 5000
    for f in (1000.0, -7300.0, 23_000.0, 0.0):
        ph = 2.0 * np.pi * ((f * np.arange(n)) % fs) / fs
        x = (np.cos(ph) + 1j * np.sin(ph)).astype(np.complex64)
        with ctx.demodulator(hz.FMT_C64, hz.DEMOD_FM) as dm:
            got = run(dm, dev(x)).cpu().numpy().astype(np.float64)
        err = np.abs(got[1:] - 2.0 * np.pi * f / fs).max()
        print(f"f = {f}: max |d - 2 pi f / fs| = {err:.3e} (bound {ref.E + 2.0 ** -22:.3e})")
        assert got.shape == (n,) and err <= ref.E + 2.0 ** -22
    g = np.float32(hz.fm_gain(fs, 5000.0))
    with ctx.demodulator(hz.FMT_C64, hz.DEMOD_FM, np.array([g], np.float32)) as dm:
        ph = 2.0 * np.pi * ((2500.0 * np.arange(n)) % fs) / fs
        got = run(dm, dev((np.cos(ph) + 1j * np.sin(ph)).astype(np.complex64))).cpu().numpy()
    assert np.abs(got[1:] - 0.5).max() <= float(g) * (ref.E + 2.0 ** -22) + 2.0 ** -24


# ---- 3. cuts ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode,q,down,fmt", [("fm", 64, 5, "c64"), ("fm", 33, 1, "u8"), ("envelope", 129, 64, "u8"), ("phase", 7, 3, "c64"),
                                             ("power", 1024, 64, "c64"), ("fm", 1, 1, "u8")])
def test_cuts_bit_identical(hz, ctx, mode, q, down, fmt):
    dm = ctx.demodulator(FMT[fmt], ref.MODES[mode], taps_of(q), down)
    tile, _ = dm.plan()
    n = 2 * tile * down + 37
    x = dev(white(fmt, n, seed=n + q))
    one = run(dm, x)
    assert one.shape[0] == ref.total_outputs(n, q, down)
    edge = tile * down  # the samples after which one tile's outputs are written

    def check(done):
        assert dm.pending() == (done, ref.outputs_after(done, down), ref.total_outputs(done, q, down) - ref.outputs_after(done, down))
        assert dm.outputs_for(5) == ref.outputs_after(done + 5, down) - ref.outputs_after(done, down)

    for cuts in ([0, 1, n], [0, edge - 1, n], [0, edge, n], [0, edge + 1, n], [0, 2 * edge - 1, 2 * edge, 2 * edge + 1, n],
                 [0, 0, 3, 3, edge - down, edge - down, n, n]):
        assert same(run(dm, x, cuts, check=check), one), f"cuts {cuts}"
    # pushes shorter than Q (and than D), the held tail shifted through several of them
    step = max(1, min(q - 1, 7))
    small = x[:max(3 * q, 300)]
    want = run(dm, small)
    got = run(dm, small, list(range(0, small.shape[0], step)) + [small.shape[0]], check=check)
    assert same(got, want) and got.shape[0] == ref.total_outputs(small.shape[0], q, down)
    dm.close()


# ---- 4. streams and pitch --------------------------------------------------------------------------

@pytest.mark.parametrize("streams,fmt,mode,q,down", [(5, "u8", "fm", 64, 5), (256, "c64", "fm", 33, 1), (5, "c64", "envelope", 129, 64),
                                                    (5, "i16", "phase", 7, 3)])
def test_streams_and_pitch(hz, ctx, hctx, streams, fmt, mode, q, down):
    """Rows that differ, an input pitch above n, an output pitch above the count: every row bit-equal to a
    single-stream object on that row, padding columns intact; HOST results bit-equal to DEVICE ones."""
    h = taps_of(q)
    dm = ctx.demodulator(FMT[fmt], ref.MODES[mode], h, down, streams=streams)
    single = ctx.demodulator(FMT[fmt], ref.MODES[mode], h, down)
    tile, _ = dm.plan()
    n = (tile + 37) * down + 1
    n1 = n // 3  # (two pushes: the held tails of the rows are in play)
    pad = 5
    wide = white(fmt, streams * (n + pad), seed=streams + n)
    wide = wide.reshape((streams, n + pad) + wide.shape[1:])
    dwide = dev(wide)
    xs = dwide[:, :n]
    counts = [ref.outputs_after(n1, down), ref.outputs_after(n, down) - ref.outputs_after(n1, down),
              ref.total_outputs(n, q, down) - ref.outputs_after(n, down)]
    total = sum(counts)
    out = torch.full((streams, total + 7), float("nan"), dtype=torch.float32, device="cuda")
    guard = bits(out[:, total:]).clone()
    done = 0
    for part, c in zip((xs[:, :n1], xs[:, n1:], None), counts):
        w = dm.push(part, out=out[:, done:]) if part is not None else dm.flush(out=out[:, done:])
        assert w.shape == (streams, c)
        done += c
    torch.cuda.synchronize()
    assert torch.equal(bits(out[:, total:]), guard), "columns past the outputs written were touched"
    assert not torch.isnan(out[:, :total]).any()
    for s in range(streams):
        want = run(single, xs[s].contiguous(), [0, n1, n])
        assert same(out[s, :total], want), f"row {s} differs from the single-stream run"
    # HOST context, unpinned and pinned destinations, the same pitches
    hdm = hctx.demodulator(FMT[fmt], ref.MODES[mode], h, down, streams=streams)
    pinned = hctx.pinned_samples(hz.FMT_C64, streams * (total + 7)).view(np.float32)[:streams * (total + 7)].reshape(streams, total + 7)
    for dst in (np.empty((streams, total + 7), np.float32), pinned):
        dst[:] = np.float32(np.nan)
        done = 0
        for part, c in zip((wide[:, :n1], wide[:, n1:n], None), counts):
            w = hdm.push(part, out=dst[:, done:]) if part is not None else hdm.flush(out=dst[:, done:])
            assert w.shape == (streams, c)
            done += c
        assert same(dst[:, :total], out[:, :total]) and np.isnan(dst[:, total:]).all()
    for o in (dm, single, hdm):
        o.close()


def test_host_pitched_rows_both_ways(hz, ctx, hctx):
    """3 streams, HOST context, input AND output with a pitch in one call: both from ordinary memory (each takes the 2-D
    copy), then both inside pinned_samples memory (the kernel reads and writes the caller's rows).  Bit for bit the
    DEVICE context's dense result; the output's pitch gap and the values behind its last row intact."""
    streams, fmt, q, down, pad = 3, "c64", 33, 5, 7
    h = taps_of(q)
    dm = ctx.demodulator(FMT[fmt], hz.DEMOD_FM, h, down, streams=streams)
    hdm = hctx.demodulator(FMT[fmt], hz.DEMOD_FM, h, down, streams=streams)
    n = (dm.plan()[0] + 37) * down + 1
    x = white(fmt, streams * n, seed=91).reshape(streams, n)
    want = run(dm, dev(x), [0, n // 3, n])
    total = want.shape[1]
    wi, wo = n + pad, total + pad
    srcs = (np.empty(streams * wi, np.complex64), hctx.pinned_samples(hz.FMT_C64, streams * wi))
    dsts = (np.empty(streams * wo + 8, np.float32), hctx.pinned_samples(hz.FMT_C64, streams * wo + 8).view(np.float32)[:streams * wo + 8])
    for src, dst in zip(srcs, dsts):
        wide = src.reshape(streams, wi)
        wide[:] = np.complex64(complex(5.0, -5.0))
        wide[:, :n] = x
        dst[:] = np.float32(np.nan)
        out = dst[:streams * wo].reshape(streams, wo)
        done = 0
        for part in (wide[:, :n // 3], wide[:, n // 3:n], None):
            w = hdm.push(part, out=out[:, done:]) if part is not None else hdm.flush(out=out[:, done:])
            done += w.shape[1]
        assert done == total and same(out[:, :total], want), "pitched rows differ from the DEVICE context's dense ones"
        assert np.isnan(out[:, total:]).all() and np.isnan(dst[streams * wo:]).all(), "the pitch gap or the values behind the rows were touched"
    dm.close()
    hdm.close()


# ---- 5. sub-slices ---------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,start", [("u8", 1), ("u8", 3), ("i16", 1), ("i16", 3), ("c64", 1)])
def test_sub_slices(hz, ctx, fmt, start):
    """Input starting `start` samples into its buffer (an odd byte offset for the byte formats' pairs), output
    starting one value into its own: the bits of the aligned run, guards on both sides of the output intact."""
    q, down = 64, 5
    dm = ctx.demodulator(FMT[fmt], hz.DEMOD_FM, taps_of(q), down)
    tile, _ = dm.plan()
    n = (tile + 5) * down
    x = white(fmt, n, seed=start + 40)
    aligned = run(dm, dev(x))
    total = aligned.shape[0]
    buf = dev(np.concatenate([white(fmt, start, seed=1), x, white(fmt, 2, seed=2)]))
    out = torch.full((total + 3,), float("nan"), dtype=torch.float32, device="cuda")
    a = dm.push(buf[start:start + n], out=out[1:])
    b = dm.flush(out=out[1 + a.shape[0]:])
    torch.cuda.synchronize()
    assert a.shape[0] + b.shape[0] == total
    assert same(out[1:1 + total], aligned)
    assert torch.isnan(out[:1]).all() and torch.isnan(out[1 + total:]).all()
    dm.close()


# ---- 6. behind the channelizer ---------------------------------------------------------------------

def test_the_channelizer_feeds_it(hz, ctx):
    """The channelizer's channel-major tensor, with its pitch, straight into a 256-stream FM demodulator."""
    m, p, hop, q, down = 256, 4, 192, 33, 2
    n = p * m + 60 * hop
    ch = ctx.channelizer(hz.FMT_C64, m, hz.channelizer_taps(m, p), hop=hop, layout="channels")
    frames = ch.frames_for(n)
    buf = torch.zeros((m, frames + 9), dtype=torch.complex64, device="cuda")
    rows = ch.push(dev(white("c64", n, seed=77)), out=buf)
    assert rows.shape == (m, frames) and rows.stride(0) == frames + 9
    h = taps_of(q)
    dm = ctx.demodulator(hz.FMT_C64, hz.DEMOD_FM, h, down, streams=m)
    single = ctx.demodulator(hz.FMT_C64, hz.DEMOD_FM, h, down)
    got = run(dm, rows)
    assert got.shape == (m, ref.total_outputs(frames, q, down)) and got.dtype == torch.float32
    for k in range(m):
        assert same(got[k], run(single, rows[k].contiguous())), f"channel row {k}"
    for o in (ch, dm, single):
        o.close()


# ---- 7. errors and state ---------------------------------------------------------------------------

def test_create_errors(hz, ctx):
    h = taps_of(24)
    for kw in (dict(mode=0), dict(mode=5), dict(down=65), dict(down=0), dict(streams=8193), dict(streams=0)):
        args = dict(mode=hz.DEMOD_FM, down=2, streams=1)
        args.update(kw)
        with pytest.raises(hz.ErrInvalidArgument):
            ctx.demodulator(hz.FMT_C64, args["mode"], h, args["down"], streams=args["streams"])
    lib = importlib.import_module("go-sdr_amd._capi").lib
    out = C.c_void_p()

    def create(fmt, mode, down, taps, n, streams=1):
        p = taps.ctypes.data_as(C.POINTER(C.c_float)) if taps is not None else None
        return lib.hzsdr_demod_create(ctx._h, fmt, mode, down, p, n, streams, C.byref(out))

    inval = hz.ErrInvalidArgument.status
    assert create(hz.FMT_C64, 0, 2, h, 24) == create(hz.FMT_C64, 5, 2, h, 24) == create(hz.FMT_C64, -1, 2, h, 24) == inval
    assert create(hz.FMT_C64, 1, 0, h, 24) == create(hz.FMT_C64, 1, 65, h, 24) == create(hz.FMT_C64, 1, 2, h, 24, 8193) == inval
    big = np.ones(1025, np.float32)
    assert create(hz.FMT_C64, 1, 2, None, 24) == inval, "null taps"
    assert create(hz.FMT_C64, 1, 2, h, 0) == inval, "Q = 0"
    assert create(hz.FMT_C64, 1, 2, big, 1025) == inval, "Q above 1024"
    assert create(hz.FMT_C64, 4, 64, big, 1024, 8192) == 0 and lib.hzsdr_demod_free(out) == 0
    for bad in (np.nan, np.inf, -np.inf):
        g = h.copy()
        g[7] = bad
        assert create(hz.FMT_C64, 1, 2, g, 24) == inval, "a non-finite tap"
    with pytest.raises(hz.HzsdrError) as e:
        ctx.demodulator(9, hz.DEMOD_FM, h)
    assert type(e.value).__name__ == "ErrSampleFormatUnknown"


def test_in_stride_below_the_push(hz, ctx):
    lib = importlib.import_module("go-sdr_amd._capi").lib
    with ctx.demodulator(hz.FMT_C64, hz.DEMOD_FM, taps_of(24), 2, streams=2) as dm:
        x = torch.zeros((2, 10), dtype=torch.complex64, device="cuda")
        out = torch.zeros((2, 32), dtype=torch.float32, device="cuda")
        got = C.c_size_t(5)
        rc = lib.hzsdr_demod_push(dm._h, x.data_ptr(), 10, 9, out.data_ptr(), 32, 32, C.byref(got))
        assert rc == hz.ErrInvalidArgument.status and got.value == 0 and dm.pending() == (0, 0, 0)


@pytest.mark.parametrize("streams", [1, 3])
def test_dst_too_small_leaves_state(hz, ctx, streams):
    q, down = 24, 2
    h = taps_of(q)
    lib = importlib.import_module("go-sdr_amd._capi").lib
    x = dev(white("c64", streams * 200, seed=5).reshape(streams, 200))
    x = x[0] if streams == 1 else x
    dm = ctx.demodulator(hz.FMT_C64, hz.DEMOD_FM, h, down, streams=streams)
    want = run(dm, x, [0, 51, 200])
    first = dm.push(x[..., :51]).clone()
    state = dm.pending()
    assert state[2] > 1
    count = dm.outputs_for(149)
    out = torch.zeros((streams, count), dtype=torch.float32, device="cuda")
    got = C.c_size_t(7)
    part = x[..., 51:].contiguous()
    with pytest.raises(hz.ErrDstTooSmall):
        ctx._ck(lib.hzsdr_demod_push(dm._h, part.data_ptr(), 149, 149, out.data_ptr(), count - 1, count, C.byref(got)))
    assert got.value == 0 and dm.pending() == state
    if streams > 1:
        with pytest.raises(hz.ErrDstTooSmall):
            ctx._ck(lib.hzsdr_demod_push(dm._h, part.data_ptr(), 149, 149, out.data_ptr(), count, count - 1, C.byref(got)))
        assert dm.pending() == state
    with pytest.raises(hz.ErrDstTooSmall):
        ctx._ck(lib.hzsdr_demod_flush(dm._h, out.data_ptr(), state[2] - 1, count, C.byref(got)))
    assert dm.pending() == state
    rest = torch.cat([dm.push(part), dm.flush()], dim=-1)
    torch.cuda.synchronize()
    assert same(torch.cat([first, rest], dim=-1), want)
    dm.close()


def test_reset_flush_and_runs(hz, ctx):
    q, down = 64, 5
    h = taps_of(q)
    x = dev(white("u8", 1500, seed=8))
    dm = ctx.demodulator(hz.FMT_U8, hz.DEMOD_FM, h, down)
    assert dm.flush().shape[0] == 0 and dm.pending() == (0, 0, 0), "flush on a fresh object writes nothing"
    a = run(dm, x)
    assert dm.pending() == (0, 0, 0)
    b = run(dm, x)  # (flush, then a push: a new stream)
    dm.push(x[:700])
    dm.reset()
    assert dm.pending() == (0, 0, 0)
    c = run(dm, x)
    with ctx.demodulator(hz.FMT_U8, hz.DEMOD_FM, h, down) as other:
        d = run(other, x)
    assert same(a, b) and same(a, c) and same(a, d)
    assert a.shape[0] == ref.total_outputs(1500, q, down)
    dm.close()


# ---- 8. the other layers ---------------------------------------------------------------------------

def _run(exe):
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "go-sdr_amd") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    return subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)


def test_c_demod_walkthrough(hz):
    """tests/c/test_demod_abi.c compiled by gcc as C99 and run against libhzsdr_hip.so."""
    exe = os.path.join(BUILD, "test_demod_abi")
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "test_demod_abi.c"), "-L" + os.path.join(ROOT, "go-sdr_amd"),
                           "-lhzsdr_hip", "-lm", "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    p = _run(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "demod-abi ok" in p.stdout


def test_cxx_demod(hz):
    """tests/cxx/test_demod.cpp (hzsdr::stream::Demodulator of go-sdr_amd/cxx/hzsdr.hpp) built with g++ and run."""
    exe = os.path.join(BUILD, "test_demod_cxx")
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + ROOT, os.path.join(ROOT, "tests", "cxx", "test_demod.cpp"),
                           "-L" + os.path.join(ROOT, "go-sdr_amd"), "-lhzsdr_hip", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    p = _run(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "demod-cxx ok" in p.stdout


def test_demodulator_blocks(hz, hctx):
    """stream.demodulator_blocks over a BufferReader with short reads: the pushes' outputs and the flush last, i.e.
    one push plus flush."""
    st = importlib.import_module("go-sdr_amd.stream")
    q, down = 33, 4
    h = taps_of(q)
    x = white("i16", 5000, seed=3)
    with hctx.demodulator(hz.FMT_I16, hz.DEMOD_FM, h, down) as one:
        want = run(one, x)
        assert one.sample_rate(48_000) == 12_000.0
    dm = hctx.demodulator(hz.FMT_I16, hz.DEMOD_FM, h, down)
    blocks = list(st.demodulator_blocks(st.BufferReader(x, 48_000, max_read=777), dm, block=1024))
    dm.close()
    assert len(blocks) > 3 and all(b.dtype == np.float32 for b in blocks)
    assert blocks[-1].shape[0] == ref.total_outputs(5000, q, down) - ref.outputs_after(5000, down)
    assert same(np.concatenate(blocks), want) and want.shape[0] == ref.total_outputs(5000, q, down)

"""The channel bank (include/hzsdr_chanbank.h) on the GPU: every format, shape, order and layout BIT FOR BIT against the
outputs of tests/host/chanbank_ref.cpp (the host program over the headers the kernel evaluates, fed the table the
library reads out) and, within the bound derived in tests/chanbank_ref.py, against the independent float64
restatement; bit for bit across cuts, placements in the tile, memory spaces, pitches and runs; against the tuner bank;
a tone; in front of the demodulator; errors and state; the C++ layer and the C walkthrough.  Streams are
2 * tile_frames + 5 frames long (tile_frames from plan()), so that the last tile is partly dead."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import chanbank_ref as ref
import tuner_ref
from conftest import ROOT
from util import FMT, splitmix64

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BUILD = os.path.join(ROOT, "build")
ORDERS_LAYOUTS = [(o, lay) for o in ("neg", "zero") for lay in ("frames", "channels")]


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


def as_c64(ctx, x):
    """hzsdr_convert of device samples to complex64, as numpy"""
    if x.dtype == torch.complex64:
        return x.cpu().numpy()
    out = torch.empty(x.shape[0], dtype=torch.complex64, device=x.device)
    assert ctx.convert(out, x) == x.shape[0]
    torch.cuda.synchronize()
    return out.cpu().numpy()


def make(hz, ctx, fmt, m, g, d, order="neg", layout="frames"):
    return ctx.channel_bank(FMT[fmt], m, g, hop=d, order=hz.NEGATIVE_FIRST if order == "neg" else hz.ZERO_FIRST, layout=layout)


def run(bank, x, cuts=()):
    """push x whole or cut at the stream positions `cuts` -> the frames, concatenated, as numpy"""
    edges = [0] + list(cuts) + [x.shape[0]]
    out = [bank.push(x[a:b]) for a, b in zip(edges[:-1], edges[1:])]
    if isinstance(out[0], torch.Tensor):
        torch.cuda.synchronize()
        out = [o.cpu().numpy() for o in out]
    return np.concatenate(out, axis=1 if bank.channel_major else 0)


def canon(hz, bank, y):
    """the bank's output -> (frames, M) with channel k in column k"""
    y = y.T if bank.channel_major else y
    return np.ascontiguousarray(y[:, ref.positions(bank.channels, bank.order == hz.NEGATIVE_FIRST)])


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def first_difference(got, want):
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    bad = np.argwhere(g != w)
    row, col = (int(v) for v in bad[0])
    return f"{bad.shape[0]} of {w.size} components differ, the first in frame {row}, channel {col // 2}: {got[row, col // 2]!r} for {want[row, col // 2]!r}"


def stream_length(bank, frames=None):
    t = bank.plan()[0]
    frames = 2 * t + 5 if frames is None else frames
    return bank.taps.shape[0] + (frames - 1) * bank.hop


def table_of(hz, bank):
    return np.stack([bank.readout(hz.CHANBANK_READ_DFT, k) for k in range(bank.channels)])


# ---- 1. bit for bit against the host program, and within the bound of float64 ---------------------------

@pytest.mark.parametrize("fmt", ref.FORMATS)
def test_bits_and_bound(hz, ctx, fmt, tmp_path):
    cases, got = [], []
    for m, p, d in ref.SHAPES:
        g = ref.taps_of(m, p)
        outs = []
        for order, layout in ORDERS_LAYOUTS:
            with make(hz, ctx, fmt, m, g, d, order, layout) as bank:
                if not outs:
                    t, rows, form = bank.plan()
                    assert t in (32, 64) and rows >= 2 * m and rows % 32 == 0 and form in (0, hz.CHANBANK_FORM_A_LDS)
                    x = dev(white(fmt, stream_length(bank), 1000 * m + 10 * p + d))
                    tab = table_of(hz, bank)
                    assert same(bank.readout(hz.CHANBANK_READ_TAPS), g)
                y = run(bank, x)
                assert y.shape == ((m, 2 * t + 5) if layout == "channels" else (2 * t + 5, m))
                outs.append(canon(hz, bank, y))
        for o, (order, layout) in zip(outs[1:], ORDERS_LAYOUTS[1:]):
            assert same(o, outs[0]), f"M={m} P={p} D={d} {fmt}: order {order}, layout {layout}: " + first_difference(o, outs[0])
        got.append(outs[0])
        cases.append((m, d, g, as_c64(ctx, x), [], tab))
    worst = 0.0
    for (m, d, g, xc, _, tab), y, (want, used) in zip(cases, got, ref.exact(str(tmp_path), cases)):
        assert same(used, tab)
        assert same(y, want), f"M={m} P={len(g) // m} D={d} {fmt}: " + first_difference(y, want)
        f64 = ref.fold_dft(g, xc, m, d)
        err, bnd = float(np.abs(y.astype(np.complex128) - f64).max()), ref.bound(g, xc, m)
        worst = max(worst, err / bnd)
        assert err <= bnd, f"M={m} P={len(g) // m} D={d} {fmt}: max err {err:.3e} > bound {bnd:.3e}"
        assert np.abs(f64).max() > 100 * bnd, "the signal is not above the bound: the check shows nothing"
    print(f"{fmt}: {len(cases)} shapes bit for bit; worst error / bound {worst:.3f}")


# ---- 2, 3. cuts and placement ---------------------------------------------------------------------------

CUT_SHAPES = [(7, 3, 5, "u8"), (16, 32, 1, "i8"), (100, 3, 61, "i16"), (128, 3, 77, "u8"), (255, 1, 255, "c64"), (2, 1, 2, "c64")]


@pytest.mark.parametrize("m,p,d,fmt", CUT_SHAPES)
@pytest.mark.parametrize("layout", ["frames", "channels"])
def test_cuts_and_placement(hz, ctx, m, p, d, fmt, layout):
    g = ref.taps_of(m, p)
    with make(hz, ctx, fmt, m, g, d, "neg", layout) as bank:
        t, ntaps = bank.plan()[0], m * p
        n = stream_length(bank)
        x = dev(white(fmt, n, 77 * m + d))
        whole = run(bank, x)
        assert bank.pending() == (n - (2 * t + 5) * d, 2 * t + 5)
        frame_edge, inside, tile_edge = ntaps + 3 * d, ntaps + 3 * d + max(1, d // 2), ntaps + (t - 1) * d
        plans = {"at 1": [1], "inside a frame": [inside], "at a frame edge": [frame_edge], "at a tile edge": [tile_edge],
                 "all of them": sorted({1, inside, frame_edge, tile_edge}),
                 "with empty pushes between": [0, 1, 1, frame_edge, frame_edge, inside, tile_edge, tile_edge, n],
                 # placement: 1, 7, T - 1 and T + 3 frames complete first, the rest land in other tile columns
                 "after 1 frame": [ntaps], "after 7 frames": [ntaps + 6 * d], "after T - 1 frames": [ntaps + (t - 2) * d],
                 "after T + 3 frames": [ntaps + (t + 2) * d]}
        for what, cuts in plans.items():
            bank.reset()
            assert bank.pending() == (0, 0)
            y = run(bank, x, cuts)
            assert same(y, whole), f"M={m} P={p} D={d} {fmt} {layout}: cut {what}"


# ---- 4. HOST against DEVICE, pitch, untouched columns ---------------------------------------------------

@pytest.mark.parametrize("m,p,d,fmt", [(12, 3, 11, "u8"), (100, 3, 100, "i16"), (255, 3, 154, "c64")])
def test_host_context_and_pitch(hz, ctx, hctx, m, p, d, fmt):
    g = ref.taps_of(m, p)
    with make(hz, ctx, fmt, m, g, d, "neg", "channels") as bank, make(hz, hctx, fmt, m, g, d, "neg", "channels") as hbank:
        n = stream_length(bank)
        raw = white(fmt, n, 5 * m + d)
        frames = bank.frames_for(n)
        dense = run(bank, dev(raw))
        mark = np.complex64(-7.5 + 3.25j)
        # DEVICE, a pitch above the count
        buf = torch.full((m, frames + 9), complex(mark), dtype=torch.complex64, device="cuda")
        bank.reset()
        rows = bank.push(dev(raw), out=buf)
        torch.cuda.synchronize()
        assert rows.shape == (m, frames) and rows.stride(0) == frames + 9
        assert same(rows.cpu().numpy(), dense) and bool((buf[:, frames:] == complex(mark)).all())
        # a wider buffer cut to a pitched view: the columns past the view belong to someone else
        view = torch.full((m, frames + 20), complex(mark), dtype=torch.complex64, device="cuda")[:, 3:frames + 8]
        bank.reset()
        rows = bank.push(dev(raw), out=view)
        torch.cuda.synchronize()
        assert same(rows.cpu().numpy(), dense) and bool((view[:, frames:] == complex(mark)).all())
        # HOST: dense, and pitched rows through the 2-D copy
        assert same(run(hbank, raw), dense)
        hbuf = np.full((m, frames + 4), mark, np.complex64)
        hbank.reset()
        hrows = hbank.push(raw, out=hbuf)
        assert same(hrows, dense) and bool((hbuf[:, frames:] == mark).all())
        # HOST frame-major against DEVICE frame-major
    with make(hz, ctx, fmt, m, g, d, "zero", "frames") as bank, make(hz, hctx, fmt, m, g, d, "zero", "frames") as hbank:
        assert same(run(hbank, raw, [n // 3]), run(bank, dev(raw)))


ZERO_COPY_MAX = 2 << 20  # Stage's kZeroCopyMax: up to this many bytes in total, a HOST call's dense buffers go through the pinned staging area


def test_host_channel_major_routes(hz, ctx, hctx):
    """HOST context, channel-major, M = 12, P = 3, D = 11, u8, every result bit for bit the DEVICE context's dense one:
    a dense destination (stride == frames) under and over the staging limit in total bytes; a pitched destination in
    ordinary memory and inside pinned_samples memory, the pitch gap and the values behind the last row intact; a push
    too short to complete a frame into either, which writes nothing and keeps its samples for the next."""
    m, p, d, fmt = 12, 3, 11, "u8"
    g = ref.taps_of(m, p)
    mark = np.complex64(-7.5 + 3.25j)
    with make(hz, ctx, fmt, m, g, d, "neg", "channels") as bank, make(hz, hctx, fmt, m, g, d, "neg", "channels") as hbank:
        for frames, over in ((None, False), (22000, True)):
            n = stream_length(bank, frames)
            raw = white(fmt, n, 77 + n)
            bank.reset()
            dense = run(bank, dev(raw))
            f = dense.shape[1]
            assert (m * f * 8 > ZERO_COPY_MAX) if over else (m * f * 8 + raw.nbytes + 512 <= ZERO_COPY_MAX)
            hbuf = np.full(m * f + 8, mark, np.complex64)
            hbank.reset()
            rows = hbank.push(raw, out=hbuf[:m * f].reshape(m, f))
            assert rows.shape == (m, f) and rows.strides[0] == 8 * f
            assert same(rows, dense), f"dense rows of {f} frames differ from the DEVICE context's"
            assert bool((hbuf[m * f:] == mark).all()), "values behind the last row were touched"
        # (raw, dense, f: the short stream from here on)
        n = stream_length(bank)
        raw = white(fmt, n, 77 + n)
        bank.reset()
        dense = run(bank, dev(raw))
        f, w, short = dense.shape[1], dense.shape[1] + 9, m * p - 1
        pinned = hctx.pinned_samples(hz.FMT_C64, m * w + 8)
        for flat in (np.empty(m * w + 8, np.complex64), pinned):
            flat[:] = mark
            buf = flat[:m * w].reshape(m, w)
            hbank.reset()
            none = hbank.push(raw[:short], out=buf)
            assert none.shape == (m, 0) and hbank.pending()[0] == short
            assert bool((flat == mark).all()), "a push that completes no frame wrote"
            rows = hbank.push(raw[short:], out=buf)
            assert rows.shape == (m, f) and rows.strides[0] == 8 * w
            assert same(rows, dense), "pitched rows differ from the DEVICE context's dense ones"
            assert bool((buf[:, f:] == mark).all()) and bool((flat[m * w:] == mark).all()), "the pitch gap or the values behind the rows were touched"


# ---- 5. against the tuner bank --------------------------------------------------------------------------

def test_against_the_tuner_bank(hz, ctx):
    """M = 16, D = 1: channel k is the tuner at word k 2^28 with h = g reversed; frame j is output j + L - 1"""
    m, p = 16, 3
    g = ref.taps_of(m, p)
    ntaps = m * p
    with make(hz, ctx, "c64", m, g, 1, "zero", "channels") as bank:
        n = stream_length(bank)
        x = dev(white("c64", n, 31))
        y = run(bank, x)
    words = [k << 28 for k in range(m)]
    with ctx.tuner_bank(hz.FMT_C64, words, g[::-1].copy(), 1) as tb:
        z = tb.push(x)
        torch.cuda.synchronize()
        z = z.cpu().numpy()
    frames = n - ntaps + 1
    assert y.shape == (m, frames) and z.shape == (m, n)
    xc = x.cpu().numpy()
    bnd = ref.bound(g, xc, m) + tuner_ref.bound(g[::-1], xc)
    err = float(np.abs(y.astype(np.complex128) - z[:, ntaps - 1:].astype(np.complex128)).max())
    print(f"channel bank against tuner bank: max difference {err:.3e}, sum of the bounds {bnd:.3e}")
    assert err <= bnd and np.abs(y).max() > 100 * bnd


# ---- 6. a tone ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", ["neg", "zero"])
def test_tone(hz, ctx, order):
    """a tone at channel k0 + 0.1 of M = 100: the peak at pos(k0), the neighbours at the prototype's response"""
    m, p, k0 = 100, 8, 37
    g = hz.channelizer_taps(m, p)
    with make(hz, ctx, "c64", m, g, m, order, "frames") as bank:
        n = stream_length(bank, 9)
        tt = np.arange(n, dtype=np.float64)
        x = np.exp(2j * np.pi * (k0 + 0.1) * tt / m).astype(np.complex64)
        y = run(bank, dev(x))
    pos = ref.positions(m, order == "neg")
    mag = np.abs(y.astype(np.complex128))
    assert (mag.argmax(axis=1) == pos[k0]).all()
    i = np.arange(m * p, dtype=np.float64)
    bnd = ref.bound(g, x, m) + 2.0 ** -24 * float(np.abs(g).sum())  # (and the tone's own rounding to complex64)
    for k in (k0 - 2, k0 - 1, k0, k0 + 1, k0 + 2, (k0 + 50) % m):
        response = abs(np.sum(g.astype(np.float64) * np.exp(2j * np.pi * (k0 + 0.1 - k) * i / m)))
        assert np.abs(mag[:, pos[k]] - response).max() <= bnd, f"channel {k}: {mag[:, pos[k]]} for {response}"
    assert mag[0, pos[k0]] > 0.9 and mag[0, pos[(k0 + 50) % m]] < 1e-3


# ---- 7. feeds the demodulator ---------------------------------------------------------------------------

def test_feeds_the_demodulator(hz, ctx):
    """channel-major rows of M = 12, with their pitch, straight into a 12-stream FM demodulator: the demodulator fed a
    contiguous copy gives the same bits"""
    m, p, d = 12, 8, 6
    with make(hz, ctx, "u8", m, hz.channelizer_taps(m, p), d, "neg", "channels") as bank:
        n = stream_length(bank)
        frames = bank.frames_for(n)
        buf = torch.zeros((m, frames + 9), dtype=torch.complex64, device="cuda")
        rows = bank.push(dev(white("u8", n, 12)), out=buf)
        assert rows.shape == (m, frames) and rows.stride(0) == frames + 9
        lp = tuner_ref.taps_of(16, seed=1)
        with ctx.demodulator(hz.FMT_C64, hz.DEMOD_FM, lp, 2, streams=m) as dm:
            a = torch.cat([dm.push(rows), dm.flush()], dim=-1)
            b = torch.cat([dm.push(rows.contiguous()), dm.flush()], dim=-1)
            torch.cuda.synchronize()
        assert a.shape == b.shape and a.shape[0] == m and a.shape[-1] > 0
        assert same(a.cpu().numpy(), b.cpu().numpy())
        assert float(a.abs().max()) > 0


# ---- 8. errors and state --------------------------------------------------------------------------------

def test_create_errors_and_limits(hz, ctx):
    lib = importlib.import_module("go-sdr_amd._capi").lib
    taps = np.ones(32 * 256, np.float32)
    tp = taps.ctypes.data_as(C.POINTER(C.c_float))

    def create(fmt, m, t, n, hop, order=hz.NEGATIVE_FIRST, layout=hz.CHANNELIZER_FRAME_MAJOR):
        out = C.c_void_p()
        rc = lib.hzsdr_chanbank_create(ctx._h, fmt, m, t, n, hop, order, layout, C.byref(out))
        assert (rc == 0) == bool(out.value)
        if out.value:
            lib.hzsdr_chanbank_free(out)
        return rc

    inval = hz.ErrInvalidArgument.status
    for m in (0, 1, 256, 1000):
        assert create(hz.FMT_C64, m, tp, 4 * max(m, 1), 1) == inval, f"M = {m}"
    assert create(hz.FMT_C64, 12, tp, 0, 12) == create(hz.FMT_C64, 12, tp, 30, 12) == create(hz.FMT_C64, 12, tp, 33 * 12, 12) == inval, "taps"
    assert create(hz.FMT_C64, 12, tp, 24, 0) == create(hz.FMT_C64, 12, tp, 24, 13) == inval, "hop"
    assert create(hz.FMT_C64, 12, tp, 24, 12, order=5) == create(hz.FMT_C64, 12, tp, 24, 12, layout=2) == inval, "order, layout"
    assert create(hz.FMT_C64, 12, None, 24, 12) == inval, "null taps"
    assert lib.hzsdr_chanbank_create(ctx._h, hz.FMT_C64, 12, tp, 24, 12, hz.NEGATIVE_FIRST, 0, None) == inval, "null result"
    assert create(9, 12, tp, 24, 12) == hz.ErrSampleFormatUnknown.status
    # the limits themselves
    for fmt in (hz.FMT_C64, hz.FMT_U8, hz.FMT_I8, hz.FMT_I16):
        assert create(fmt, 2, tp, 2, 1) == create(fmt, 2, tp, 64, 2) == create(fmt, 255, tp, 32 * 255, 255) == create(fmt, 255, tp, 255, 1) == 0
    with pytest.raises(hz.ErrInvalidArgument):
        ctx.channel_bank(hz.FMT_C64, 256, taps[:512])
    with pytest.raises(ValueError):
        ctx.channel_bank(hz.FMT_C64, 12, taps[:24], layout="rows")
    with ctx.channel_bank(hz.FMT_C64, 7, taps[:21]) as bank:
        assert bank.hop == 7 and bank.order == hz.NEGATIVE_FIRST and not bank.channel_major
        buf = np.zeros(64, np.complex64)
        assert lib.hzsdr_chanbank_readout(bank._h, 0, 0, buf.ctypes.data, 64) == lib.hzsdr_chanbank_readout(bank._h, 3, 0, buf.ctypes.data, 64) == inval
        assert lib.hzsdr_chanbank_readout(bank._h, hz.CHANBANK_READ_DFT, 7, buf.ctypes.data, 64) == inval, "no such row"
        assert lib.hzsdr_chanbank_readout(bank._h, hz.CHANBANK_READ_DFT, 0, None, 64) == inval
        assert lib.hzsdr_chanbank_readout(bank._h, hz.CHANBANK_READ_DFT, 0, buf.ctypes.data, 7) == hz.ErrDstTooSmall.status
        assert lib.hzsdr_chanbank_readout(bank._h, hz.CHANBANK_READ_TAPS, 0, buf.ctypes.data, 20) == hz.ErrDstTooSmall.status
        assert lib.hzsdr_chanbank_readout(bank._h, hz.CHANBANK_READ_DFT, 6, buf.ctypes.data, 8) == 0
        assert bank.readout(hz.CHANBANK_READ_DFT, 0).view(np.uint32).reshape(-1, 2).tolist() == [[0x3f800000, 0]] * 7 + [[0, 0]]
        assert lib.hzsdr_chanbank_push(bank._h, None, 5, None, 0, 0, None) == inval, "null input"
        assert lib.hzsdr_chanbank_plan(None, None, None, None) == inval and lib.hzsdr_chanbank_plan(bank._h, None, None, None) == 0


@pytest.mark.parametrize("layout", ["frames", "channels"])
def test_dst_too_small_reset_and_runs(hz, ctx, layout):
    lib = importlib.import_module("go-sdr_amd._capi").lib
    m, p, d = 17, 3, 11
    g = ref.taps_of(m, p)
    with make(hz, ctx, "i16", m, g, d, "neg", layout) as bank:
        n = stream_length(bank)
        x = dev(white("i16", n, 171))
        whole = run(bank, x)
        bank.reset()
        assert same(run(bank, x), whole), "run to run"
        bank.reset()
        head = bank.push(x[:m * p + 4 * d + 3])
        torch.cuda.synchronize()
        state = bank.pending()
        assert state == (m * p + 4 * d + 3 - 5 * d, 5)
        part = x[m * p + 4 * d + 3:].contiguous()
        count = bank.frames_for(part.shape[0])
        assert count == whole.shape[1 if layout == "channels" else 0] - 5
        out = torch.zeros((m, count) if layout == "channels" else (count, m), dtype=torch.complex64, device="cuda")
        got = C.c_size_t(7)
        with pytest.raises(hz.ErrDstTooSmall):
            ctx._ck(lib.hzsdr_chanbank_push(bank._h, part.data_ptr(), part.shape[0], out.data_ptr(), count - 1, count, C.byref(got)))
        assert got.value == 0 and bank.pending() == state
        if layout == "channels":
            with pytest.raises(hz.ErrDstTooSmall):
                ctx._ck(lib.hzsdr_chanbank_push(bank._h, part.data_ptr(), part.shape[0], out.data_ptr(), count, count - 1, C.byref(got)))
            assert got.value == 0 and bank.pending() == state
        torch.cuda.synchronize()
        assert not bool(out.any()), "a refused push wrote"
        rest = bank.push(part)
        torch.cuda.synchronize()
        both = np.concatenate([head.cpu().numpy(), rest.cpu().numpy()], axis=1 if layout == "channels" else 0)
        assert same(both, whole)


# ---- 9. the C++ layer and the C walkthrough -------------------------------------------------------------

def _run(exe):
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "go-sdr_amd") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    return subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)


def test_c_chanbank_walkthrough(hz):
    """tests/c/test_chanbank_abi.c compiled by gcc as C99 and run against libhzsdr_hip.so."""
    exe = os.path.join(BUILD, "test_chanbank_abi")
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "test_chanbank_abi.c"), "-L" + os.path.join(ROOT, "go-sdr_amd"),
                           "-lhzsdr_hip", "-lm", "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    p = _run(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "chanbank-abi ok" in p.stdout


def test_cxx_chanbank(hz):
    """tests/cxx/test_chanbank.cpp (hzsdr::fft::ChannelBank of go-sdr_amd/cxx/hzsdr.hpp) built with g++ and run."""
    exe = os.path.join(BUILD, "test_chanbank_cxx")
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + ROOT, os.path.join(ROOT, "tests", "cxx", "test_chanbank.cpp"),
                           "-L" + os.path.join(ROOT, "go-sdr_amd"), "-lhzsdr_hip", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    p = _run(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "chanbank-cxx ok" in p.stdout

"""The polyphase channelizer (include/hzsdr_channelizer.h) on the GPU: frames against the float64 restatements of
tests/channelizer_ref.py within B(M, P) = 3e-7 log2 M + 6e-8 (P + 2), per frame and per channel, at all six sizes,
through both fold paths and up to P = 32; every tap read out on its own by impulse trains, per bin against the
single-precision yardstick of tests/util.py (tests/readout.py); and bit for bit across pushes, memory spaces, layouts,
orders and runs.

test_tap_readout's worst ratio kernel / max(yardstick, 2^-23) over both fold paths, as max_bin | rel_l2 (it prints
them; K = 4 is asserted; the FFT core alone measures 1.43 | 0.97 on impulses at these sizes, and the fold adds one
exact product).  Observed on an MI355X:

    not measured
"""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import channelizer_ref as ref
import readout as ro
from conftest import ROOT
from util import FFT_K, FMT, assert_fft_rows_close, splitmix64

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


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


def raw(fmt, n, seed):
    """n samples of format fmt (numpy), white over the whole band: full-range bytes / i16, c64 in [-1, 1)."""
    z = splitmix64(seed, 2 * n)
    if fmt == "u8":
        return (z & np.uint64(0xFF)).astype(np.uint8).reshape(n, 2)
    if fmt == "i8":
        return (z & np.uint64(0xFF)).astype(np.uint8).view(np.int8).reshape(n, 2)
    if fmt == "i16":
        return (z & np.uint64(0xFFFF)).astype(np.uint16).view(np.int16).reshape(n, 2)
    f = ((z >> np.uint64(40)).astype(np.float64) / float(1 << 23) - 1.0).astype(np.float32)
    return f.view(np.complex64).reshape(n)


def converted(orc, x):
    """hzsdr_convert's arithmetic, by the oracle's converters."""
    if x.dtype == np.complex64:
        return x.copy()
    out = np.zeros(x.shape[0], np.complex64)
    assert orc.convert(out, x) == x.shape[0]
    return out


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits(t):
    t = t.detach().cpu() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return torch.view_as_real(t.contiguous()).contiguous().view(torch.int32)


def xpb(m):
    """fv::xpb: transforms per workgroup"""
    return max(1, 64 // (m // 16))


def push_all(ch, x, cuts=None):
    """push x whole or cut at `cuts`; the frames of all pushes, concatenated along the frame axis"""
    if cuts is None:
        cuts = [0, x.shape[0]]
    out = [ch.push(x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    if isinstance(out[0], torch.Tensor):
        torch.cuda.synchronize()
        return torch.cat(out, 1 if ch.channel_major else 0)
    return np.concatenate(out, 1 if ch.channel_major else 0)


def check_rows_and_columns(got, want, m, p, what):
    """relative L2 per frame over the channels and per channel over the frames, both within B(M, P)"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    d = got.astype(np.complex128) - want
    b = ref.bound(m, p)
    rows = np.linalg.norm(d, axis=1) / np.linalg.norm(want, axis=1)
    cols = np.linalg.norm(d, axis=0) / np.linalg.norm(want, axis=0)
    print(f"{what}: rows {rows.max():.3e} columns {cols.max():.3e} (B = {b:.3e})")
    assert (rows <= b).all(), f"{what}: frame {int(rows.argmax())}: relative L2 {rows.max():.3e} > {b:.3e}"
    assert (cols <= b).all(), f"{what}: channel {int(cols.argmax())}: relative L2 {cols.max():.3e} > {b:.3e}"
    return max(rows.max(), cols.max())


# ---- 1. accuracy against float64 -------------------------------------------------------------------

STREAMS = 4


@pytest.mark.parametrize("fmt", ["u8", "i8", "i16", "c64"])
@pytest.mark.parametrize("m", [256, 512, 1024, 2048, 4096, 8192])
def test_frames_against_float64(hz, orc, ctx, fmt, m):
    """Every frame within B over its channels, every channel within B over its frames.

    The column check rests on every channel carrying the same power, which white input gives in expectation only: a
    channel's output is a complex Gaussian value that stays correlated for about M input samples, so the 2 xpb + 5
    consecutive frames of one stream are one or two independent draws at a small hop (one, at D = 1), and a draw
    (B / 1.5e-7)^2 = 600 times below the mean power, which makes an ordinary rounding error exceed B, has probability
    1 / 600 per channel: expected in a thousand channels.  So the columns are taken over the frames of STREAMS = 4
    independent streams (reset between them, which the test thereby covers): with k independent draws the probability
    is (k / 600)^k / k! = 1e-10 per channel.  The smallest and the largest size also run the longest prototype the
    bank accepts, P = 32."""
    worst = 0.0
    for p, d in ((1, m), (3, m), (8, m // 2), (4, 3 * m // 4), (2, 100), (8, 1)) + (((32, m // 2),) if m in (256, 8192) else ()):
        frames = 2 * xpb(m) + 5  # (several workgroups, the last partly dead)
        n = (frames - 1) * d + p * m + (d - 1) // 2  # (a ragged tail shorter than the hop)
        g = hz.channelizer_taps(m, p)
        ch = ctx.channelizer(FMT[fmt], m, g, hop=d, order=hz.ZERO_FIRST)
        got, want = [], []
        for stream in range(STREAMS):
            x = raw(fmt, n, seed=m * 131 + p * 7 + d + 1000 * stream)
            ch.reset()
            assert ch.frames_for(n) == frames
            got.append(ch.push(dev(x)).cpu().numpy())
            want.append(ref.channels_fold(converted(orc, x), g, m, d))
        ch.close()
        worst = max(worst, check_rows_and_columns(np.concatenate(got), np.concatenate(want), m, p, f"{fmt} M={m} P={p} D={d}"))
    print(f"{fmt} M={m}: worst GPU / float64 relative L2 {worst:.3e}")


@pytest.mark.parametrize("fmt", ["u8", "i8", "i16", "c64"])
@pytest.mark.parametrize("m", [256, 512, 1024, 2048, 4096, 8192])
def test_frames_that_start_in_held_samples(hz, orc, ctx, fmt, m):
    """The kernel's second fold path against the reference itself, not through "cuts equal one push": the stream
    arrives in two pushes, the first leaving nearly L samples held, so that at least xpb + 2 frames of the second
    (more than one workgroup's) start in held samples, beside frames that lie wholly in the second push.  Rows and
    columns as above, the columns over STREAMS streams."""
    for p, d in ((8, m // 2), (8, 1)):
        L = p * m
        first = L + 2 * d + (d - 1) // 2  # three frames, then L - d + (d - 1) // 2 samples held
        held = first - 3 * d
        inside = -(-held // d)  # frames of the second push that start in held samples
        frames = 3 + inside + xpb(m) + 2 if d > 1 else 3 + 2 * xpb(m) + 5
        n = (frames - 1) * d + L + d // 3
        assert min(inside, frames - 3) >= xpb(m) + 2 and 0 < held < L
        g = hz.channelizer_taps(m, p)
        ch = ctx.channelizer(FMT[fmt], m, g, hop=d, order=hz.ZERO_FIRST)
        got, want = [], []
        for stream in range(STREAMS):
            x = raw(fmt, n, seed=m * 137 + p * 11 + d + 1000 * stream)
            ch.reset()
            a = ch.push(dev(x[:first]))
            assert a.shape[0] == 3 and ch.pending() == (held, 3)
            b = ch.push(dev(x[first:]))
            assert b.shape[0] == frames - 3
            got.append(torch.cat([a, b]).cpu().numpy())
            want.append(ref.channels_fold(converted(orc, x), g, m, d))
        ch.close()
        check_rows_and_columns(np.concatenate(got), np.concatenate(want), m, p, f"{fmt} M={m} P={p} D={d}, {min(inside, frames - 3)} frames from held samples")


# ---- 1b. every tap on its own ----------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["c64", "i16"])
@pytest.mark.parametrize("m,p,d,every", [(256, 2, 129, False), (512, 2, 257, False), (1024, 2, 513, False), (2048, 2, 1025, False),
                                         (4096, 2, 2049, False), (8192, 2, 4097, False), (256, 2, 1, True)])
def test_tap_readout(hz, ctx, fmt, m, p, d, every):
    """One impulse of power-of-two amplitude every L samples: every window of L samples holds exactly one, the fold
    is ONE exact product, and frame j is the M-point transform of a one-hot vector g[l_j] amp.  Every frame per bin
    against that transform within K = FFT_K of the single-precision yardstick -- relative to the frame's own tap, so
    a wrong small tap cannot hide behind large ones.  An odd hop (the rotation differs from frame to frame); once in
    one push (every frame through the first fold path) and once cut after three frames with L - D / 2 samples held,
    so that the second push's first frames start in held samples and take the second path: four of them at the hop
    M / 2 + 1 (fewer than L samples can be held, so no cut gives more at this P and hop), L - 1 of the L + 2 xpb + 2
    at D = 1, where every one of the 512 taps of M = 256, P = 2 is read, by either path.  (The second path over more
    than a workgroup's frames at every size is test_frames_that_start_in_held_samples.)  A frame whose tap is
    exactly 0 is all zero."""
    L = p * m
    frames = L + 2 * xpb(m) + 5 if every else 2 * xpb(m) + 5 + (L // d)
    n = (frames - 1) * d + L + d // 2
    g = hz.channelizer_taps(m, p)
    assert np.array_equal(g, ro.bank_taps(m, p))
    x, conv = ro.channelizer_train(fmt, n, L, first=L - 1 if every else L // 3)
    ls, u, want = ro.channelizer_onehots(conv, g, m, d, frames)
    if every:
        assert set(ls.tolist()) == set(range(L)), "not every tap is read"
    cut = L + 2 * d + d // 2  # three frames, then frames that start in held samples
    ch = ctx.channelizer(FMT[fmt], m, g, hop=d, order=hz.ZERO_FIRST)
    zero = np.flatnonzero(g[ls] == 0)
    ratio = (0.0, 0.0)
    for cuts in ([0, n], [0, cut, n]):
        ch.reset()
        got = push_all(ch, dev(x), cuts).cpu().numpy()
        assert got.shape == (frames, m) and not np.isnan(got.view(np.float32)).any()
        assert not got[zero].any(), "a frame of a zero tap is not all zero"
        r = assert_fft_rows_close(got, u, what=f"{fmt} M={m} P={p} D={d} cuts {cuts}", k=FFT_K, want64=want)
        ratio = tuple(max(a, b) for a, b in zip(ratio, r))
    ch.close()
    print(f"{fmt} M={m} P={p} D={d}: {frames} frames, {len(set(ls.tolist()))} taps read; kernel / max(yardstick, 2^-23): "
          f"max_bin {ratio[0]:.2f} rel_l2 {ratio[1]:.2f}")


# ---- 2. the definition -----------------------------------------------------------------------------

@pytest.mark.parametrize("m,p,d", [(256, 8, 192), (1024, 4, 1024), (4096, 2, 3072)])
def test_against_the_definition(hz, orc, ctx, m, p, d):
    frames = 2 * xpb(m) + 3
    n = (frames - 1) * d + p * m + d // 3
    x = raw("i16", n, seed=m + p)
    g = hz.channelizer_taps(m, p)
    ch = ctx.channelizer(hz.FMT_I16, m, g, hop=d, order=hz.ZERO_FIRST)
    got = ch.push(dev(x)).cpu().numpy().astype(np.complex128)
    ch.close()
    c = converted(orc, x)
    ks = np.array([0, 1, 37, m // 2, m - 1])
    want = ref.channels_direct(c, g, m, d, ks=ks)
    norm = np.linalg.norm(ref.channels_fold(c, g, m, d), axis=1)  # the rows' norms
    err = np.linalg.norm(got[:, ks] - want, axis=1) / norm
    print(f"M={m} P={p} D={d}: error of the five channels relative to the row norm {err.max():.3e}")
    assert got.shape[0] == frames and (err <= ref.bound(m, p)).all(), err.max()


# ---- 3. grid walk ----------------------------------------------------------------------------------

def test_many_frames(hz, orc, ctx):
    m, p, d, frames = 256, 2, 64, 5000
    n = (frames - 1) * d + p * m + 17
    x = raw("u8", n, seed=99)
    g = hz.channelizer_taps(m, p)
    ch = ctx.channelizer(hz.FMT_U8, m, g, hop=d, order=hz.ZERO_FIRST)
    got = ch.push(dev(x)).cpu().numpy()
    ch.close()
    check_rows_and_columns(got, ref.channels_fold(converted(orc, x), g, m, d), m, p, "5000 frames")


# ---- 4. bit-identity -------------------------------------------------------------------------------

def ragged_cuts(rng, n, L, d):
    """cuts of [0, n): a zero-length push, pushes shorter than the hop and shorter than the prototype among them"""
    steps = [0, 1, max(d - 1, 1), d, L - 1, L, L + 5, 3 * L + 11]
    cuts = [0, 0, min(n, 1)]
    while cuts[-1] < n:
        k = int(rng.choice(steps + [int(rng.integers(0, 4 * L))]))
        cuts.append(min(n, cuts[-1] + k))
    return cuts


@pytest.mark.parametrize("fmt,m,p,d", [("u8", 1024, 4, 512), ("i16", 256, 3, 100), ("c64", 2048, 2, 2048),
                                       ("i8", 8192, 2, 6144), ("u8", 512, 8, 1)])
def test_cuts_spaces_layouts_orders_runs_bit_identical(hz, ctx, hctx, fmt, m, p, d):
    rng = np.random.default_rng(m + d)
    L = p * m
    n = 40 * d + L + 123 if d > 1 else 3 * L + 57
    xh = raw(fmt, n, seed=5 + m)
    x = dev(xh)
    g = hz.channelizer_taps(m, p)
    z = ctx.channelizer(FMT[fmt], m, g, hop=d, order=hz.ZERO_FIRST)
    whole = push_all(z, x)
    assert whole.shape == (ref.frames_of(n, L, d), m) and whole.shape[0] >= 2
    z.reset()
    assert torch.equal(bits(push_all(z, x)), bits(whole)), "two runs differ"
    for trial in range(3):
        z.reset()
        cuts = ragged_cuts(rng, n, L, d)
        assert torch.equal(bits(push_all(z, x, cuts)), bits(whole)), f"cuts {cuts} differ from one push"
    z.close()
    # the memory space
    h = hctx.channelizer(FMT[fmt], m, g, hop=d, order=hz.ZERO_FIRST)
    cut = min(n, L + 3 * d + 1)
    assert torch.equal(bits(push_all(h, xh, [0, 7, cut, n])), bits(whole)), "HOST differs from DEVICE"
    h.close()
    # the layout, in both spaces
    for c, src in ((ctx, x), (hctx, xh)):
        t = c.channelizer(FMT[fmt], m, g, hop=d, order=hz.ZERO_FIRST, layout="channels")
        cm = push_all(t, src, [0, cut, n])
        assert tuple(cm.shape) == (m, whole.shape[0])
        cm = cm if isinstance(cm, torch.Tensor) else torch.from_numpy(cm)
        assert torch.equal(bits(cm.cpu().T), bits(whole)), "channel-major is not the transpose of frame-major"
        t.close()
    # the order
    ng = ctx.channelizer(FMT[fmt], m, g, hop=d, order=hz.NEGATIVE_FIRST)
    neg = push_all(ng, x)
    assert torch.equal(bits(torch.cat([neg[:, m // 2:], neg[:, :m // 2]], 1)), bits(whole)), "NegativeFirst is not ZeroFirst swapped"
    ng.close()


@pytest.mark.parametrize("fmt", ["u8", "i8", "i16"])
def test_byte_sources_equal_their_c64(hz, ctx, fmt):
    m, p, d = 1024, 3, 333
    n = 20 * d + p * m
    x = raw(fmt, n, seed=11)
    c = torch.zeros(n, dtype=torch.complex64, device="cuda")
    ctx.convert(c, dev(x))
    g = hz.channelizer_taps(m, p)
    a, b = ctx.channelizer(FMT[fmt], m, g, hop=d), ctx.channelizer(hz.FMT_C64, m, g, hop=d)
    ra, rb = push_all(a, dev(x)), push_all(b, c)
    assert ra.shape[0] == 21 and torch.equal(bits(ra), bits(rb))
    a.close()
    b.close()


# ---- 5. channel-major with a pitch -----------------------------------------------------------------

def test_channel_major_pitch_leaves_the_rest(hz, ctx, hctx):
    m, p, d = 512, 2, 384
    frames = 11
    n = (frames - 1) * d + p * m + 100
    xh = raw("i8", n, seed=7)
    g = hz.channelizer_taps(m, p)
    f = ctx.channelizer(hz.FMT_I8, m, g, hop=d, order=hz.NEGATIVE_FIRST)
    want = push_all(f, dev(xh)).cpu()
    f.close()
    sentinel = np.complex64(complex(-7.0, 9.0))
    for c, src in ((ctx, dev(xh)), (hctx, xh)):
        ch = c.channelizer(hz.FMT_I8, m, g, hop=d, order=hz.NEGATIVE_FIRST, layout="channels")
        if c is ctx:
            out = torch.full((m, frames + 5), complex(sentinel), dtype=torch.complex64, device="cuda")
        else:
            out = np.full((m, frames + 5), sentinel, np.complex64)
        got = ch.push(src, out=out)
        assert tuple(got.shape) == (m, frames)
        o = out.cpu() if isinstance(out, torch.Tensor) else torch.from_numpy(out)
        assert torch.equal(bits(o[:, :frames].T), bits(want))
        assert (o[:, frames:] == complex(sentinel)).all(), "columns past the frames written were touched"
        ch.close()


ZERO_COPY_MAX = 2 << 20  # Stage's kZeroCopyMax: up to this many bytes in total, a HOST call's dense buffers go through the pinned staging area


def test_host_channel_major_routes(hz, ctx, hctx):
    """HOST context, channel-major, M = 256, P = 2, hop 192, i16, every result bit for bit the DEVICE context's dense
    one: a dense destination (stride == frames) under and over the staging limit in total bytes; a pitched destination
    in ordinary memory and inside pinned_samples memory, the pitch gap and the values behind the last row intact; a
    push too short to complete a frame into either, which writes nothing and keeps its samples for the next."""
    m, p, d = 256, 2, 192
    g = hz.channelizer_taps(m, p)
    sentinel = np.complex64(complex(-7.0, 9.0))
    dch = ctx.channelizer(hz.FMT_I16, m, g, hop=d, order=hz.NEGATIVE_FIRST, layout="channels")
    hch = hctx.channelizer(hz.FMT_I16, m, g, hop=d, order=hz.NEGATIVE_FIRST, layout="channels")
    for frames, over in ((11, False), (1030, True)):
        xh = raw("i16", (frames - 1) * d + p * m + 100, seed=frames)
        dch.reset()
        want = bits(push_all(dch, dev(xh)))
        assert (m * frames * 8 > ZERO_COPY_MAX) if over else (m * frames * 8 + xh.nbytes + 512 <= ZERO_COPY_MAX)
        flat = np.full(m * frames + 8, sentinel, np.complex64)
        hch.reset()
        got = hch.push(xh, out=flat[:m * frames].reshape(m, frames))
        assert tuple(got.shape) == (m, frames)
        assert torch.equal(bits(got), want), f"dense rows of {frames} frames differ from the DEVICE context's"
        assert (flat[m * frames:] == sentinel).all(), "values behind the last row were touched"
    frames, w, short = 11, 16, p * m - 1
    xh = raw("i16", (frames - 1) * d + p * m + 100, seed=frames)
    dch.reset()
    want = bits(push_all(dch, dev(xh)))
    pinned = hctx.pinned_samples(hz.FMT_C64, m * w + 8)
    for flat in (np.empty(m * w + 8, np.complex64), pinned):
        flat[:] = sentinel
        out = flat[:m * w].reshape(m, w)
        hch.reset()
        none = hch.push(xh[:short], out=out)
        assert tuple(none.shape) == (m, 0) and hch.pending()[0] == short
        assert (flat == sentinel).all(), "a push that completes no frame wrote"
        got = hch.push(xh[short:], out=out)
        assert tuple(got.shape) == (m, frames)
        assert torch.equal(bits(got), want), "pitched rows differ from the DEVICE context's dense ones"
        assert (out[:, frames:] == sentinel).all() and (flat[m * w:] == sentinel).all(), "the pitch gap or the values behind the rows were touched"
    dch.close()
    hch.close()


# ---- 6. host logic and state -----------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["u8", "i8", "i16", "c64"])
def test_create_errors(hz, ctx, fmt):
    lib, capi = hz.lib, hz._capi
    h = C.c_void_p()
    m = 1024
    g = np.ones(33 * m + 1, np.float32)
    gp = g.ctypes.data_as(C.POINTER(C.c_float))
    bad = capi.ERR_INVALID_ARGUMENT
    for channels, n_taps, hop, order, layout, taps in [(128, 128, 1, 0, 0, gp), (16384, 16384, 1, 0, 0, gp),
                                                       (1000, 1000, 1, 0, 0, gp), (m, 0, 1, 0, 0, gp),
                                                       (m, m + 1, 1, 0, 0, gp), (m, 3 * m - 1, 1, 0, 0, gp),
                                                       (m, 33 * m, 1, 0, 0, gp), (m, m, 0, 0, 0, gp),
                                                       (m, m, m + 1, 0, 0, gp), (m, m, 1, 2, 0, gp),
                                                       (m, m, 1, 0, 2, gp), (m, m, 1, 0, 0, None)]:
        rc = lib.hzsdr_channelizer_create(ctx._h, FMT[fmt], channels, taps, n_taps, hop, order, layout, C.byref(h))
        assert rc == bad and not h.value, (channels, n_taps, hop, order, layout)
    assert lib.hzsdr_channelizer_create(ctx._h, 9, m, gp, m, 1, 0, 0, C.byref(h)) == capi.ERR_FORMAT_UNKNOWN
    # the limits themselves are accepted
    for channels, n_taps, hop in [(256, 256, 256), (8192, 8192, 1), (m, 32 * m, m)]:
        assert lib.hzsdr_channelizer_create(ctx._h, FMT[fmt], channels, gp, n_taps, hop, 1, 1, C.byref(h)) == capi.OK
        assert lib.hzsdr_channelizer_free(h) == capi.OK


def test_frames_for_and_pending(hz, ctx):
    m, p, d = 256, 2, 100
    L = p * m
    ch = ctx.channelizer(hz.FMT_U8, m, hz.channelizer_taps(m, p), hop=d)
    x = dev(raw("u8", 3000, seed=71))
    pos, frame = 0, 0
    for k in (200, 0, 311, 1, 99, 100, 1289, 1000):
        want = ref.frames_of(pos + k, L, d) - frame
        assert ch.frames_for(k) == want
        got = ch.push(x[pos:pos + k])
        assert got.shape == (want, m)
        pos, frame = pos + k, frame + want
        assert ch.pending() == (pos - frame * d, frame)
    assert frame == ref.frames_of(3000, L, d) and frame > 20
    ch.close()


def test_a_push_that_completes_no_frame_writes_nothing(hz, ctx):
    m, p, d = 256, 4, 256
    ch = ctx.channelizer(hz.FMT_C64, m, hz.channelizer_taps(m, p), hop=d)
    x = dev(raw("c64", p * m - 1, seed=3))
    out = torch.full((2, m), complex(5.0, -5.0), dtype=torch.complex64, device="cuda")
    got = ch.push(x, out=out)
    torch.cuda.synchronize()
    assert got.shape[0] == 0 and ch.pending() == (p * m - 1, 0)
    assert (out == complex(5.0, -5.0)).all()
    ch.close()


@pytest.mark.parametrize("layout", ["frames", "channels"])
def test_dst_too_small_leaves_state(hz, ctx, layout):
    m, p, d = 1024, 3, 384
    n = 30 * d + p * m
    x = dev(raw("u8", n, seed=51))
    g = hz.channelizer_taps(m, p)
    a = ctx.channelizer(hz.FMT_U8, m, g, hop=d, layout=layout)
    b = ctx.channelizer(hz.FMT_U8, m, g, hop=d, layout=layout)
    ra, rb = [a.push(x[:5000])], [b.push(x[:5000])]
    before = a.pending()
    frames = a.frames_for(n - 5000)
    assert frames >= 2
    small = torch.zeros((frames - 1, m) if layout == "frames" else (m, frames - 1), dtype=torch.complex64, device="cuda")
    with pytest.raises(hz.ErrDstTooSmall):
        a.push(x[5000:], out=small)
    assert a.pending() == before
    ra.append(a.push(x[5000:]))
    rb.append(b.push(x[5000:]))
    torch.cuda.synchronize()
    assert a.pending() == b.pending()
    axis = 0 if layout == "frames" else 1
    assert torch.equal(bits(torch.cat(ra, axis)), bits(torch.cat(rb, axis)))
    a.close()
    b.close()


def test_reset_restarts_the_rotation(hz, ctx):
    m, p, d = 512, 2, 100  # (100 does not divide 512: the rotation differs from frame to frame)
    x = dev(raw("c64", 30 * d + p * m, seed=61))
    g = hz.channelizer_taps(m, p)
    s = ctx.channelizer(hz.FMT_C64, m, g, hop=d)
    first = push_all(s, x)
    s.push(x[:1777])  # frames done, samples held, the rotation somewhere
    assert s.pending()[1] > 0 and (s.pending()[1] * d) % m != 0
    s.reset()
    assert s.pending() == (0, 0)
    again = push_all(s, x)
    fresh = ctx.channelizer(hz.FMT_C64, m, g, hop=d)
    assert torch.equal(bits(again), bits(first)) and torch.equal(bits(push_all(fresh, x)), bits(first))
    s.close()
    fresh.close()


# ---- 7. a tone -------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", ["zero", "negative"])
def test_tone_lands_in_its_channel(hz, ctx, order):
    m, p, d = 1024, 4, 768
    k0, frames = m - 3, 12
    n = (frames - 1) * d + p * m
    t = np.arange(n, dtype=np.float64)
    ph = 2.0 * np.pi * (((k0 + 0.1) * t) % m) / m
    x = (np.cos(ph) + 1j * np.sin(ph)).astype(np.complex64)
    o = hz.ZERO_FIRST if order == "zero" else hz.NEGATIVE_FIRST
    ch = ctx.channelizer(hz.FMT_C64, m, hz.channelizer_taps(m, p), hop=d, order=o)
    y = ch.push(dev(x)).cpu().numpy().astype(np.complex128)
    at = int(ref.pos(k0, m, o == hz.NEGATIVE_FIRST))
    assert y.shape == (frames, m) and (np.abs(y).argmax(axis=1) == at).all()
    assert abs(ch.channel_center(at, float(m)) - (k0 - m)) < 1e-9  # (channel M - 3 is the frequency -3 fs / M)
    step = np.angle(y[1:, at] * np.conj(y[:-1, at]))
    want = np.angle(np.exp(2j * np.pi * 0.1 * d / m))
    assert np.abs(step - want).max() < 1e-4, np.abs(step - want).max()
    ch.close()


# ---- 8. the other layers ---------------------------------------------------------------------------

def _run(exe):
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "go-sdr_amd") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    return subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)


def test_c_channelizer_walkthrough(hz):
    """tests/c/test_channelizer_abi.c compiled by gcc as C99 and run against libhzsdr_hip.so."""
    exe = os.path.join(ROOT, "build", "test_channelizer_abi")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "test_channelizer_abi.c"), "-L" + os.path.join(ROOT, "go-sdr_amd"),
                           "-lhzsdr_hip", "-lm", "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    p = _run(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "channelizer-abi ok" in p.stdout


def test_cxx_channelizer(hz):
    """tests/cxx/test_channelizer.cpp (hzsdr::fft::Channelizer of go-sdr_amd/cxx/hzsdr.hpp) built with g++ and run."""
    exe = os.path.join(ROOT, "build", "test_channelizer_cxx")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + ROOT, os.path.join(ROOT, "tests", "cxx", "test_channelizer.cpp"),
                           "-L" + os.path.join(ROOT, "go-sdr_amd"), "-lhzsdr_hip", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    p = _run(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "channelizer-cxx ok" in p.stdout


def test_channelizer_frames_of_a_reader(hz, hctx):
    """stream.channelizer_frames over a BufferReader: the blocks' frames are those of one push."""
    st = importlib.import_module("go-sdr_amd.stream")
    m, p, d = 256, 2, 192
    x = raw("u8", 5000, seed=13)
    g = hz.channelizer_taps(m, p)
    one = hctx.channelizer(hz.FMT_U8, m, g, hop=d)
    want = one.push(x)
    one.close()
    ch = hctx.channelizer(hz.FMT_U8, m, g, hop=d)
    got = []
    for frames, rate, order in st.channelizer_frames(st.BufferReader(x.copy(), 2_000_000), ch, block=700):
        assert rate == 2_000_000 / d and order == hz.NEGATIVE_FIRST
        got.append(frames.copy())
    ch.close()
    assert torch.equal(bits(np.concatenate(got)), bits(want))

"""The polyphase synthesis bank (include/hzsdr_synthesizer.h) on the GPU: the output stream against the float64
restatements of tests/synthesizer_ref.py within B(M, Q) = 3e-7 log2 M + 6e-8 (Q + 2), Q = ceil(L / D), per block of M
outputs; bit for bit across pushes, internal groups, memory spaces, layouts, orders and runs; and against the GPU
channelizer, as its adjoint and as its inverse.  All six sizes, up to P = 32; every tap read out on its own by frames
with a single non-zero value (tests/readout.py), per output position against a few float32 ulps of that position's
own tap.

test_tap_readout's worst (|got - want| / (|g[t - j0 D]| |amp|) - 2^-24) as a multiple of max(yardstick, 2^-23) (it
prints them; the transform's part of the bound allows K = 4, the yardstick is scipy's single-precision backward
transform of the same one-hot frame).  Observed on an MI355X:

    not measured
"""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import channelizer_ref as cref
import readout as ro
import synthesizer_ref as ref
from conftest import ROOT
from util import FFT_FLOOR, FMT, splitmix64

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TORCH_DT = {"c64": torch.complex64, "u8": torch.uint8, "i8": torch.int8, "i16": torch.int16}


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


def white(n, seed):
    """n complex64 values, white, components in [-1, 1)"""
    z = splitmix64(seed, 2 * n)
    f = ((z >> np.uint64(40)).astype(np.float64) / float(1 << 23) - 1.0).astype(np.float32)
    return f.view(np.complex64).reshape(n)


def frames_of(f, m, seed):
    return white(f * m, seed).reshape(f, m)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits(t):
    t = t.detach().cpu() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    t = t.contiguous()
    return (torch.view_as_real(t).contiguous() if t.is_complex() else t).view(torch.int32 if t.is_complex() else t.dtype)


def xpb(m):
    """fv::xpb: transforms per workgroup"""
    return max(1, 64 // (m // 16))


def run(sy, y, cuts=None, flush=True):
    """push the frames of y (along axis 0 for layout "frames", axis 1 for "channels") whole or cut at `cuts`, then
    flush; every push's samples and the tail, concatenated"""
    f = y.shape[1 if sy.channel_major else 0]
    if cuts is None:
        cuts = [0, f]
    out = [sy.push(y[:, a:b] if sy.channel_major else y[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    if flush:
        out.append(sy.flush())
    if isinstance(out[0], torch.Tensor):
        torch.cuda.synchronize()
        return torch.cat(out)
    return np.concatenate(out)


block_errors = ro.block_errors  # relative L2 of every block of M outputs, the ragged last one included


# ---- 1. accuracy against float64 -------------------------------------------------------------------

@pytest.mark.parametrize("m", [256, 512, 1024, 2048, 4096, 8192])
def test_stream_against_float64(hz, ctx, m):
    """Every block of M outputs within B(M, Q) of the float64 overlap-add.  The error of a block scales with the taps
    that weight it, as its norm does, so the stream's edge blocks (whose norm is far below the middle's) are held to
    the same relative bound.  The smallest and the largest size also run the longest prototype the bank accepts,
    P = 32."""
    worst = 0.0
    for p, d in ((1, m), (3, m), (8, m // 2), (4, 3 * m // 4), (2, 100), (1, 1)) + (((32, m // 2),) if m in (256, 8192) else ()):
        f = 2 * xpb(m) + 5  # (several workgroups, the last partly dead)
        L = p * m
        g = hz.channelizer_taps(m, p)
        y = frames_of(f, m, seed=m * 131 + p * 7 + d)
        sy = ctx.synthesizer(hz.FMT_C64, m, g, hop=d, order=hz.ZERO_FIRST)
        head = sy.push(dev(y))
        assert head.shape[0] == f * d and sy.pending() == (L - d, f)
        got = torch.cat([head, sy.flush()]).cpu().numpy()
        sy.close()
        assert got.shape[0] == (f - 1) * d + L
        err = block_errors(got, ref.synth_ola(y, g, m, d), m)
        b = ref.bound(m, ref.terms(L, d))
        print(f"M={m} P={p} D={d}: blocks {err.max():.3e} (B = {b:.3e})")
        assert (err <= b).all(), f"M={m} P={p} D={d}: block {int(err.argmax())}: relative L2 {err.max():.3e} > {b:.3e}"
        worst = max(worst, err.max())
    print(f"M={m}: worst GPU / float64 relative L2 per block {worst:.3e}")


# ---- 1b. every tap on its own ----------------------------------------------------------------------

@pytest.mark.parametrize("order", ["zero", "negative"])
@pytest.mark.parametrize("m", [256, 512, 1024, 2048, 4096, 8192])
def test_tap_readout(hz, ctx, m, order):
    """F frames, all zero except Y[j0][k0] = amp: output position t in [j0 D, j0 D + L) is g[t - j0 D] amp
    exp(+2 pi i k0 t / M), everything outside that span exactly zero.  Per output

        |got - want| <= (FFT_K max(y, 2^-23) + 2^-24) |g[t - j0 D]| |amp|

    with y the max_bin of scipy's single-precision backward transform of that one-hot frame and 2^-24 the one
    rounding of the product with the tap: nothing in it is measured on the kernel, and a wrong small tap cannot hide
    behind large ones.  j0 in the middle of a workgroup's frames (never the stream's first frame, which has no
    overlap partner before it and the rotation 0: frame 1 where a workgroup holds one frame), the last frame of a push
    and the first of the next; k0 = 1, M / 2 + 1 and about M / 3; an odd hop; M = 1024 also channel-major."""
    p, d = 2, m // 2 + 1
    L = p * m
    f = 2 * xpb(m) + 5
    cut = xpb(m) + 3
    g = hz.channelizer_taps(m, p)
    amp = 0.5 - 0.25j
    o = hz.ZERO_FIRST if order == "zero" else hz.NEGATIVE_FIRST
    worst = 0.0
    for layout in (("frames", "channels") if m == 1024 else ("frames",)):
        sy = ctx.synthesizer(hz.FMT_C64, m, g, hop=d, order=o, layout=layout)
        for k0 in (1, m // 2 + 1, (m // 3) | 1):
            bound = ro.synthesizer_bound(m, k0, amp)
            floor = max(ro.synthesizer_yardstick(m, k0, amp), FFT_FLOOR)
            for j0 in (max(1, xpb(m) // 2), cut - 1, cut):
                y = np.zeros((f, m), np.complex64)
                y[j0, int(cref.pos(k0, m, o == hz.NEGATIVE_FIRST))] = amp
                got = run(sy, dev(y.T if layout == "channels" else y), [0, cut, f]).cpu().numpy()
                want, scale = ro.synthesizer_want(g, m, d, f, j0, k0, amp)
                assert got.shape == want.shape and not np.isnan(got.view(np.float32)).any()
                span = scale > 0
                outside = np.ones(want.shape[0], bool)
                outside[j0 * d:j0 * d + L] = False
                assert not got[outside].any(), f"M={m} {order} {layout} k0={k0} j0={j0}: output outside the frame's span"
                assert not got[~span & ~outside].any(), "a zero tap's output is not zero"
                err = np.abs(got.astype(np.complex128) - want)[span] / scale[span]
                at = int(np.flatnonzero(span)[err.argmax()])
                assert (err <= bound).all(), (f"M={m} {order} {layout} k0={k0} j0={j0}: position {at} (tap {at - j0 * d}): "
                                              f"{err.max():.3e} of the tap > {bound:.3e}")
                worst = max(worst, (err.max() - 2.0 ** -24) / floor)
        sy.close()
    print(f"M={m} {order}: worst (error / tap - 2^-24) / max(yardstick, 2^-23) = {worst:.2f}")


# ---- 2. the definition -----------------------------------------------------------------------------

@pytest.mark.parametrize("m,p,d", [(256, 8, 192), (1024, 4, 1024), (512, 3, 100)])
def test_against_the_definition(hz, ctx, m, p, d):
    f = max(2 * xpb(m) + 5, (p * m) // d + 6)  # (a steady region exists: F D > L - D)
    L = p * m
    g = hz.channelizer_taps(m, p)
    y = frames_of(f, m, seed=m + p)
    sy = ctx.synthesizer(hz.FMT_C64, m, g, hop=d, order=hz.ZERO_FIRST)
    got = run(sy, dev(y)).cpu().numpy().astype(np.complex128)
    sy.close()
    assert L - d < f * d
    ts = np.sort(np.random.default_rng(m + d).choice(np.arange(L - d, f * d), 64, replace=False))
    want = ref.synth_direct(y, g, m, d, ts)
    err = np.linalg.norm(got[ts] - want) / np.linalg.norm(want)
    print(f"M={m} P={p} D={d}: 64 steady positions against the definition {err:.3e}")
    assert err <= ref.bound(m, ref.terms(L, d)), err


# ---- 3. bit-identity -------------------------------------------------------------------------------

def ragged_cuts(rng, f):
    """cuts of [0, f): a zero-frame push and a one-frame push among them"""
    cuts = [0, 0, 1]
    while cuts[-1] < f:
        cuts.append(min(f, cuts[-1] + int(rng.choice([0, 1, 2, 3, 5, 8]))))
    return cuts


@pytest.mark.parametrize("m,p,d", [(1024, 4, 512), (256, 3, 100), (2048, 2, 2048), (8192, 2, 6144), (512, 8, 1)])
def test_cuts_spaces_layouts_orders_runs_bit_identical(hz, ctx, hctx, m, p, d):
    rng = np.random.default_rng(m + d)
    f = 2 * xpb(m) + 11
    g = hz.channelizer_taps(m, p)
    yh = frames_of(f, m, seed=5 + m)
    y = dev(yh)
    z = ctx.synthesizer(hz.FMT_C64, m, g, hop=d, order=hz.ZERO_FIRST)
    whole = run(z, y)
    assert whole.shape[0] == (f - 1) * d + p * m
    assert torch.equal(bits(run(z, y)), bits(whole)), "two runs differ"
    for trial in range(3):
        cuts = ragged_cuts(rng, f)
        assert torch.equal(bits(run(z, y, cuts)), bits(whole)), f"cuts {cuts} differ from one push"
    z.close()
    # the memory space
    h = hctx.synthesizer(hz.FMT_C64, m, g, hop=d, order=hz.ZERO_FIRST)
    assert torch.equal(bits(run(h, yh, [0, 1, 7, f])), bits(whole)), "HOST differs from DEVICE"
    h.close()
    # the layout, with a pitch above the frame count, in both spaces
    wide = np.full((m, f + 5), np.complex64(complex(3.0, -2.0)))
    wide[:, :f] = yh.T
    for c, src in ((ctx, dev(wide)), (hctx, wide)):
        t = c.synthesizer(hz.FMT_C64, m, g, hop=d, order=hz.ZERO_FIRST, layout="channels")
        assert torch.equal(bits(run(t, src[:, :f], [0, 4, f])), bits(whole)), "channel-major input differs from its transpose"
        t.close()
    # the order
    ng = ctx.synthesizer(hz.FMT_C64, m, g, hop=d, order=hz.NEGATIVE_FIRST)
    swapped = torch.cat([y[:, m // 2:], y[:, :m // 2]], 1).contiguous()
    assert torch.equal(bits(run(ng, swapped)), bits(whole)), "NegativeFirst is not ZeroFirst swapped"
    ng.close()


def test_host_channel_major_pitched_input(hz, ctx, hctx):
    """HOST context, M = 256, P = 2, channel-major input with a pitch above the frame count, from ordinary and from
    pinned_samples memory: the samples are the DEVICE context's, bit for bit, and the input is left as it was."""
    m, p, d = 256, 2, 192
    f = 2 * xpb(m) + 11
    g = hz.channelizer_taps(m, p)
    yh = frames_of(f, m, seed=41)
    z = ctx.synthesizer(hz.FMT_C64, m, g, hop=d, order=hz.ZERO_FIRST, layout="channels")
    whole = run(z, dev(np.ascontiguousarray(yh.T)))
    z.close()
    assert whole.shape[0] == (f - 1) * d + p * m
    h = hctx.synthesizer(hz.FMT_C64, m, g, hop=d, order=hz.ZERO_FIRST, layout="channels")
    for flat in (np.empty(m * (f + 5), np.complex64), hctx.pinned_samples(hz.FMT_C64, m * (f + 5))):
        wide = flat.reshape(m, f + 5)
        wide[:] = np.complex64(complex(3.0, -2.0))
        wide[:, :f] = yh.T
        before = wide.copy()
        assert torch.equal(bits(run(h, wide[:, :f])), bits(whole)), "pitched channel-major input differs from the DEVICE context's"
        assert wide.tobytes() == before.tobytes()
    h.close()


def test_internal_groups_bit_identical(hz, ctx):
    """A push longer than two internal groups against the same frames in pushes of 1000."""
    m, p, d = 256, 2, 64
    g = hz.channelizer_taps(m, p)
    sy = ctx.synthesizer(hz.FMT_C64, m, g, hop=d, order=hz.ZERO_FIRST)
    group = sy.group_frames
    assert group >= 1
    f = 2 * group + 3
    y = dev(frames_of(f, m, seed=77))
    whole = run(sy, y)
    assert whole.shape[0] == (f - 1) * d + p * m
    cut = run(sy, y, list(range(0, f, 1000)) + [f])
    sy.close()
    assert torch.equal(bits(cut), bits(whole))


# ---- 4. integer destinations -----------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["u8", "i8", "i16"])
def test_integer_destinations_equal_converted_c64(hz, ctx, fmt):
    m, p, d = 1024, 3, 333
    f = 2 * xpb(m) + 5
    # white frames through DC-gain-1 taps come out with a standard deviation of 1 / sqrt(3 D) per component
    # (M / 3 per component of w, sum of g^2 = 1 / M spread over D phases): scaled to about 0.15
    g = (hz.channelizer_taps(m, p).astype(np.float64) * 0.15 * np.sqrt(3.0 * d)).astype(np.float32)
    y = dev(frames_of(f, m, seed=11))
    a, b = ctx.synthesizer(FMT[fmt], m, g, hop=d), ctx.synthesizer(hz.FMT_C64, m, g, hop=d)
    ra, rb = run(a, y), run(b, y)
    a.close()
    b.close()
    n = (f - 1) * d + p * m
    assert ra.dtype == TORCH_DT[fmt] and tuple(ra.shape) == (n, 2) and tuple(rb.shape) == (n,)
    comps = torch.view_as_real(rb)
    assert float(comps.abs().max()) < 1.0, "the c64 stream leaves the destination's range"
    want = torch.zeros((n, 2), dtype=TORCH_DT[fmt], device="cuda")
    assert ctx.convert(want, rb) == n
    torch.cuda.synchronize()
    assert len(torch.unique(want)) >= 16, "the destination hardly moves"
    assert torch.equal(ra, want)


# ---- 5. host logic and state -----------------------------------------------------------------------

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
        rc = lib.hzsdr_synthesizer_create(ctx._h, FMT[fmt], channels, taps, n_taps, hop, order, layout, C.byref(h))
        assert rc == bad and not h.value, (channels, n_taps, hop, order, layout)
    assert lib.hzsdr_synthesizer_create(ctx._h, 9, m, gp, m, 1, 0, 0, C.byref(h)) == capi.ERR_FORMAT_UNKNOWN
    # the limits themselves are accepted
    for channels, n_taps, hop in [(256, 256, 256), (8192, 8192, 1), (m, 32 * m, m)]:
        assert lib.hzsdr_synthesizer_create(ctx._h, FMT[fmt], channels, gp, n_taps, hop, 1, 1, C.byref(h)) == capi.OK
        assert lib.hzsdr_synthesizer_free(h) == capi.OK


def test_channel_major_stride_below_the_frames(hz, ctx):
    lib, capi = hz.lib, hz._capi
    m = 256
    sy = ctx.synthesizer(hz.FMT_C64, m, hz.channelizer_taps(m, 2), hop=m, layout="channels")
    y = dev(frames_of(4, m, seed=1).T)
    out = torch.zeros(4 * m, dtype=torch.complex64, device="cuda")
    got = C.c_size_t(7)
    rc = lib.hzsdr_synthesizer_push(sy._h, y.data_ptr(), 4, 3, out.data_ptr(), 4 * m, C.byref(got))
    assert rc == capi.ERR_INVALID_ARGUMENT and got.value == 0 and sy.pending() == (0, 0)
    sy.close()


def test_pending_along_pushes(hz, ctx):
    m, p, d = 256, 2, 100
    L = p * m
    sy = ctx.synthesizer(hz.FMT_U8, m, hz.channelizer_taps(m, p), hop=d)
    y = dev(frames_of(40, m, seed=71))
    assert sy.pending() == (0, 0)
    assert sy.flush().shape[0] == 0 and sy.pending() == (0, 0)
    done = 0
    for k in (0, 1, 0, 7, 2, 30):
        got = sy.push(y[done:done + k])
        done += k
        assert tuple(got.shape) == (k * d, 2)
        assert sy.pending() == ((L - d) if done else 0, done)
    assert done == 40
    assert tuple(sy.flush().shape) == (L - d, 2) and sy.pending() == (0, 0)
    sy.close()


def test_a_push_of_no_frames_writes_nothing(hz, ctx):
    m, p, d = 256, 4, 256
    sy = ctx.synthesizer(hz.FMT_C64, m, hz.channelizer_taps(m, p), hop=d)
    sy.push(dev(frames_of(2, m, seed=3)))
    before = sy.pending()
    out = torch.full((2 * m,), complex(5.0, -5.0), dtype=torch.complex64, device="cuda")
    got = sy.push(torch.zeros((0, m), dtype=torch.complex64, device="cuda"), out=out)
    torch.cuda.synchronize()
    assert got.shape[0] == 0 and sy.pending() == before == (p * m - d, 2)
    assert (out == complex(5.0, -5.0)).all()
    sy.close()


@pytest.mark.parametrize("layout", ["frames", "channels"])
def test_dst_too_small_leaves_state(hz, ctx, layout):
    m, p, d = 1024, 3, 384
    f = 30
    g = hz.channelizer_taps(m, p)
    yf = dev(frames_of(f, m, seed=51))
    y = yf.T.contiguous() if layout == "channels" else yf
    cut = (lambda a, b: y[:, a:b]) if layout == "channels" else (lambda a, b: y[a:b])
    a = ctx.synthesizer(hz.FMT_C64, m, g, hop=d, layout=layout)
    b = ctx.synthesizer(hz.FMT_C64, m, g, hop=d, layout=layout)
    ra, rb = [a.push(cut(0, 9))], [b.push(cut(0, 9))]
    before = a.pending()
    assert before == (p * m - d, 9)
    small = torch.zeros((f - 9) * d - 1, dtype=torch.complex64, device="cuda")
    with pytest.raises(hz.ErrDstTooSmall):
        a.push(cut(9, f), out=small)
    assert a.pending() == before
    with pytest.raises(hz.ErrDstTooSmall):
        a.flush(out=small[:p * m - d - 1])
    assert a.pending() == before
    for s, r in ((a, ra), (b, rb)):
        r.append(s.push(cut(9, f)))
        r.append(s.flush())
    torch.cuda.synchronize()
    assert a.pending() == b.pending() == (0, 0)
    assert torch.equal(bits(torch.cat(ra)), bits(torch.cat(rb)))
    a.close()
    b.close()


def test_reset_restarts_the_rotation(hz, ctx):
    m, p, d = 512, 2, 100  # (100 does not divide 512: the rotation differs from frame to frame)
    y = dev(frames_of(30, m, seed=61))
    g = hz.channelizer_taps(m, p)
    s = ctx.synthesizer(hz.FMT_C64, m, g, hop=d)
    first = run(s, y)
    s.push(y[:17])  # sums held, the rotation somewhere
    assert s.pending() == (p * m - d, 17) and (17 * d) % m != 0
    s.reset()
    assert s.pending() == (0, 0)
    again = run(s, y)
    # a flush is a reset: the second stream of `s` above was one already; a fresh object agrees with both
    fresh = ctx.synthesizer(hz.FMT_C64, m, g, hop=d)
    assert torch.equal(bits(again), bits(first)) and torch.equal(bits(run(fresh, y)), bits(first))
    s.close()
    fresh.close()


def test_flush_then_a_second_stream_equals_a_fresh_object(hz, ctx):
    m, p, d = 256, 4, 192
    g = hz.channelizer_taps(m, p)
    y1, y2 = dev(frames_of(13, m, seed=81)), dev(frames_of(9, m, seed=82))
    s = ctx.synthesizer(hz.FMT_I16, m, g, hop=d)
    run(s, y1)
    second = run(s, y2)
    fresh = ctx.synthesizer(hz.FMT_I16, m, g, hop=d)
    assert torch.equal(second, run(fresh, y2))
    s.close()
    fresh.close()


# ---- 6. the adjoint of the GPU channelizer ---------------------------------------------------------

@pytest.mark.parametrize("m,p,d,f", [(256, 4, 192, 9), (1024, 3, 100, 7)])
def test_adjoint_of_the_gpu_channelizer(hz, ctx, m, p, d, f):
    """|<Y, A x> - <A* Y, x>| <= B_ch(M, P) |Y| |A x| + B(M, Q) |A* Y| |x|: each side's error bound times the norms
    its inner product pairs (Cauchy-Schwarz); the inner products in float64 on the host."""
    L = p * m
    n = (f - 1) * d + L
    g = hz.channelizer_taps(m, p)
    x = white(n, seed=m + 1)
    y = frames_of(f, m, seed=m + 2)
    ch = ctx.channelizer(hz.FMT_C64, m, g, hop=d, order=hz.ZERO_FIRST)
    ax = ch.push(dev(x)).cpu().numpy().astype(np.complex128)
    ch.close()
    sy = ctx.synthesizer(hz.FMT_C64, m, g, hop=d, order=hz.ZERO_FIRST)
    aty = run(sy, dev(y)).cpu().numpy().astype(np.complex128)
    sy.close()
    assert ax.shape == (f, m) and aty.shape == (n,)
    x64, y64 = x.astype(np.complex128), y.astype(np.complex128)
    lhs, rhs = np.vdot(y64, ax), np.vdot(aty, x64)
    tol = (cref.bound(m, p) * np.linalg.norm(y64) * np.linalg.norm(ax) +
           ref.bound(m, ref.terms(L, d)) * np.linalg.norm(aty) * np.linalg.norm(x64))
    print(f"M={m} P={p} D={d}: |<Y,Ax> - <A*Y,x>| = {abs(lhs - rhs):.3e} (tolerance {tol:.3e}, |<Y,Ax>| = {abs(lhs):.3e})")
    assert abs(lhs - rhs) <= tol


# ---- 7. the round trip -----------------------------------------------------------------------------

@pytest.mark.parametrize("m", [256, 1024])
def test_round_trip_through_the_channelizer(hz, orc, ctx, m):
    """wola_taps at D = M / 2: channelizer then synthesizer return M c[t] x[t], c = sum_j g^2[t - jD] (an identity in
    exact arithmetic: with L <= M no aliasing term exists and the product window overlap-adds to c)."""
    d, f = m // 2, 20
    n = (f - 1) * d + m
    g = hz.wola_taps(m)
    z = splitmix64(m + 3, 2 * n)
    x = (z & np.uint64(0xFF)).astype(np.uint8).reshape(n, 2)
    c64 = np.zeros(n, np.complex64)
    assert orc.convert(c64, x) == n
    ch = ctx.channelizer(hz.FMT_U8, m, g, hop=d, layout="channels")
    sy = ctx.synthesizer(hz.FMT_C64, m, g, hop=d, layout="channels")
    assert ch.order == sy.order
    y = ch.push(dev(x))
    assert tuple(y.shape) == (m, f)
    back = run(sy, y).cpu().numpy().astype(np.complex128)
    ch.close()
    sy.close()
    assert back.shape == (n,)
    c = ref.overlap_gain(g, d, n)
    lo, hi = m - d, n - (m - d)
    want = c64[lo:hi].astype(np.complex128)
    err = np.linalg.norm(back[lo:hi] / (m * c[lo:hi]) - want) / np.linalg.norm(want)
    b = cref.bound(m, 1) + ref.bound(m, 2)
    print(f"M={m}: round trip relative L2 {err:.3e} (bound {b:.3e})")
    assert err <= b


# ---- 8. a tone -------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", ["zero", "negative"])
def test_one_channel_becomes_its_tone(hz, ctx, order):
    """Channel k0 fed with the constant 1: D x^[t] exp(-2 pi i k0 t / M) = D sum_j g[t - jD], which is the
    prototype's DC gain 1 plus its images at multiples of fs / D: below the stop-band level 1e-3 that
    test_channelizer_cpu pins for this prototype."""
    m, p, d = 1024, 4, 512
    k0, f = m - 3, 2 * xpb(m) + 12
    o = hz.ZERO_FIRST if order == "zero" else hz.NEGATIVE_FIRST
    y = np.zeros((f, m), np.complex64)
    y[:, int(cref.pos(k0, m, o == hz.NEGATIVE_FIRST))] = 1.0
    sy = ctx.synthesizer(hz.FMT_C64, m, hz.channelizer_taps(m, p), hop=d, order=o)
    got = run(sy, dev(y)).cpu().numpy().astype(np.complex128)
    sy.close()
    t = np.arange(p * m - d, f * d)  # the steady region
    assert t.shape[0] > m
    err = np.abs(d * got[t] * np.exp(-2j * np.pi * ((k0 * t) % m) / m) - 1.0)
    print(f"{order}: |D x^ e^(-i..) - 1| <= {err.max():.3e}")
    assert err.max() < 1e-3


# ---- 9. the other layers ---------------------------------------------------------------------------

def _run(exe):
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "go-sdr_amd") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    return subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)


def test_c_synthesizer_walkthrough(hz):
    """tests/c/test_synthesizer_abi.c compiled by gcc as C99 and run against libhzsdr_hip.so."""
    exe = os.path.join(ROOT, "build", "test_synthesizer_abi")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "test_synthesizer_abi.c"), "-L" + os.path.join(ROOT, "go-sdr_amd"),
                           "-lhzsdr_hip", "-lm", "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    p = _run(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "synthesizer-abi ok" in p.stdout


def test_cxx_synthesizer(hz):
    """tests/cxx/test_synthesizer.cpp (hzsdr::fft::Synthesizer of go-sdr_amd/cxx/hzsdr.hpp) built with g++ and run."""
    exe = os.path.join(ROOT, "build", "test_synthesizer_cxx")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + ROOT, os.path.join(ROOT, "tests", "cxx", "test_synthesizer.cpp"),
                           "-L" + os.path.join(ROOT, "go-sdr_amd"), "-lhzsdr_hip", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    p = _run(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "synthesizer-cxx ok" in p.stdout


def test_synthesizer_samples_of_frame_blocks(hz, hctx):
    """stream.synthesizer_samples over a list of frame blocks: the pushes' samples and the flush are those of one
    push plus flush."""
    st = importlib.import_module("go-sdr_amd.stream")
    m, p, d = 256, 2, 192
    y = frames_of(23, m, seed=13)
    g = hz.channelizer_taps(m, p)
    one = hctx.synthesizer(hz.FMT_U8, m, g * np.float32(3.6), hop=d)
    want = run(one, y)
    one.close()
    sy = hctx.synthesizer(hz.FMT_U8, m, g * np.float32(3.6), hop=d)
    got = [s.copy() for s in st.synthesizer_samples([y[:5], y[5:5], y[5:6], y[6:]], sy)]
    assert sy.pending() == (0, 0) and sy.sample_rate(10_000) == 10_000.0 * d
    sy.close()
    assert len(got) == 4 and np.array_equal(np.concatenate(got), want) and want.shape == (22 * d + p * m, 2)
    assert len(np.unique(want)) >= 16

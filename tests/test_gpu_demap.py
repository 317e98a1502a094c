"""The demapper bank (include/hzsdr_demap.h) on the GPU against the host program tests/host/demap_ref.cpp, which
tests/test_demap_cpu.py holds to the numpy restatement and to anchors of its own: the stored bit patterns are compared
EXACTLY, the destinations are full of sentinels and wider than needed, and every float outside the demapped slots must
still be a sentinel.

The chain test (frame sync on complex rows with two bits per symbol, beside the soft frame bank -> demapper -> LDPC) sends,
at one sample per symbol, a 32-bit word on the four corner points of qam_points(4) and behind it a whole codeword of the
(3, 6) code of n = 96 that regular_code(96, 3, 6, seed=1) makes, 48 data bits in front, xored with a flip sequence, passed
through block_interleaver(8, 12) and mapped onto 24 symbols of qam_points(4); one frame every 60 symbols from symbol 10
on, random 16-QAM symbols between.  Eight rows: four noise-free under the four 90 degree rotations, four under the same
rotations with white noise of sigma = 0.25 per component (the points are 0.632 apart); the frame sync bank allows three
wrong bits in the word.  Measured on the CPU from the chained host programs for the test's seeds: the noise-free rows
hold 32 frames, all found and all returned as planted; the noisy rows hold 32 frames, all 32 found; the soft path
(demapper with gain 1 / (2 sigma^2), LDPC scale 4, a = 12, 40 iterations) returns the sent data for 31 of them
(CHAIN_SOFT), hard decisions on the same values (HZSDR_LDPC_BITS, level 16) for 19 (CHAIN_HARD).  At sigma = 0.22 the
counts are 32 and 25, at 0.28 they are 28 and 10."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import demap_ref as ref
import framesync_ref
import ldpc_ref
import softframe_ref
from conftest import ROOT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BUILD = os.path.join(ROOT, "build")
SENT = 0xA5A5A5A5
WORD32 = 0x1ACFFC1D
CHAIN_SOFT, CHAIN_HARD = 31, 19  # of 32 noisy frames: measured on the CPU from the chained host programs


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


def bank_of(c, q):
    args, kw = q.create_args()
    return c.demapper(*args, **kw)


def strided(wide, shape, pitch, device):
    R, cap, w = shape
    if device:
        return torch.as_strided(wide, shape, (pitch, w, 1))
    return np.lib.stride_tricks.as_strided(wide, shape, (pitch * wide.itemsize, w * wide.itemsize, wide.itemsize))


def expected_plan(q):
    """hz_demap_plan.h's dealing, restated: (frames per workgroup, threads per frame, a frame's LDS bytes, form)"""
    up = lambda v, to: (v + to - 1) // to * to
    T = min(1024, up(q.S, 64))
    frame = 4 * up(q.S * q.m, 4)
    G = min(8, 1024 // T, 65536 // frame)
    form = (ref.FORM_GROUPED if G > 1 else 0) | (ref.FORM_PERM if q.perm is not None else 0) | (ref.FORM_TREE if q.kind != ref.LLR_F32 and q.m >= ref.TREE_FROM else 0)
    return G, T, frame, form


def run_checked(c, q, frames, counts, device, want, pads=(3, 5)):
    """frames (R, cap, W) through a new bank, input and output inside wider buffers, against the program's bit patterns:
    the demapped slots exactly, every other float of the destination still a sentinel -> the bank's plan"""
    R, cap, W = frames.shape
    ipitch, opitch = cap * W + pads[0], cap * q.N + pads[1]
    wide_in = np.zeros((R, ipitch), np.float32)
    wide_in[:, :cap * W] = frames.reshape(R, -1)
    wide_out = np.full((R, opitch), SENT, np.uint32).view(np.float32)
    cin = None if counts is None else np.asarray(counts, np.uint32)
    if device:
        wide_in, wide_out = dev(wide_in), dev(wide_out)
        cin = None if cin is None else dev(cin.view(np.int32))
    with bank_of(c, q) as d:
        assert d.sizes() == (q.S, q.W, q.m, q.N)
        d.run(strided(wide_in, (R, cap, W), ipitch, device), cin, cap, out=strided(wide_out, (R, cap, q.N), opitch, device))
        if device:
            torch.cuda.synchronize()
        plan = d.plan()
    got = host(wide_out).view(np.uint32)
    for r in range(R):
        k = cap if counts is None else min(int(counts[r]), cap)
        g = got[r, :k * q.N].reshape(k, q.N)
        assert np.array_equal(g, want[r, :k]), (r, np.argwhere(g != want[r, :k])[:4])
        assert (got[r, k * q.N:] == SENT).all(), r
    return plan


def constellation(hz, kind, m):
    if kind == ref.LLR_F32:
        return None
    if kind == ref.REAL_F32:
        return hz.pam_points(m)
    if m % 2 == 0:
        return hz.qam_points(m)
    if m <= 3:
        return hz.psk_points(m)
    g = ref.gaussian(100 + m, 2 << m)
    return (g[:1 << m] + 1j * g[1 << m:]).astype(np.complex64)


def noisy_frames(q, shape, sigma, seed):
    """frames (*shape, W) of random symbols of q's points under noise (values for LLR_F32)"""
    F = int(np.prod(shape))
    if q.kind == ref.LLR_F32:
        return ref.gaussian(seed, F * q.S).reshape(*shape, q.S).astype(np.float32)
    bits = np.stack([ref.random_bits(q.S * q.m, seed * 1000 + f) for f in range(F)])
    return ref.as_floats(q, ref.noisy_symbols(q, bits, sigma, seed)).reshape(*shape, q.W)


KINDS = [(ref.C64, m) for m in range(1, 9)] + [(ref.REAL_F32, m) for m in (1, 2, 4)] + [(ref.LLR_F32, 1)]


# ---- 1. kinds, rows, counts, memory spaces ------------------------------------------------------------------------

@pytest.mark.parametrize("space", ["device", "host"])
@pytest.mark.parametrize("R", [1, 3])
def test_kinds_rows_counts_and_spaces(hz, ctx, hctx, R, space):
    """C64 with m = 1 ... 8, REAL_F32 with m = 1, 2, 4 and LLR_F32, cap in {1, 3}, counts of 0, below cap and above cap
    (and none at all), with a perm that holds holes and repeats and a flip on every second bank"""
    device = space == "device"
    c = ctx if device else hctx
    cases = []
    for i, (kind, m) in enumerate(KINDS):
        pts, S = constellation(hz, kind, m), 21
        for cap in (1, 3):
            perm = flip = None
            if (i + cap) % 2:
                perm = (np.arange(S * m + 5) * 5 + 1) % (S * m)
                perm[[1, S * m + 4]] = ref.ERASED
                flip = ref.random_bits(len(perm), i)
            q = ref.Config(kind, pts, S, perm=perm, flip=flip, gains=[0.5 + i], rows=R)
            frames = noisy_frames(q, (R, cap), 0.2, 10 * i + cap)
            counts = np.array([cap + 2, 0, cap - 1][:R], np.uint32)
            cases += [(q, frames, counts), (q, frames, None)]
    for (q, frames, counts), want in zip(cases, ref.exact(BUILD, cases)):
        assert run_checked(c, q, frames, counts, device, want) == expected_plan(q)


# ---- 2. frame edges and frame counts ---------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 129, 1025])
def test_frame_sizes_around_the_tiles(hz, ctx, S):
    """S around a wave and one past the tile edges plan() reports (T = 64 at S = 64, 128 at S = 128, 1024 at S = 1024),
    16-QAM and 8PSK"""
    cases = []
    for pts in (hz.qam_points(4), hz.psk_points(3)):
        q = ref.Config(ref.C64, pts, S, gains=[2.0], rows=2)
        cases.append((q, noisy_frames(q, (2, 2), 0.15, S), np.array([2, 1], np.uint32)))
    for (q, frames, counts), want in zip(cases, ref.exact(BUILD, cases)):
        plan = run_checked(ctx, q, frames, counts, True, want)
        assert plan == expected_plan(q) and plan[1] == min(1024, (S + 63) // 64 * 64)
    if S in (65, 129, 1025):
        assert plan[1] - 64 == S - 1 or plan[1] == 1024  # one past the edge the smaller frame's plan reported


def test_the_largest_frames(hz, ctx):
    """S = 8192 at m = 2 and S = 2048 at m = 8: 16384 values, 64 KiB of LDS, one frame per workgroup, N = 8192 through a
    perm that keeps every second value; N = 1"""
    cases = []
    for pts, S in ((hz.qam_points(2), 8192), (hz.qam_points(8), 2048)):
        q = ref.Config(ref.C64, pts, S, perm=np.arange(8192) * 2 + 1, gains=[3.0])
        assert expected_plan(q)[:3] == (1, 1024, 65536)
        cases.append((q, noisy_frames(q, (1, 2), 0.05, S), None))
    q = ref.Config(ref.C64, hz.qam_points(8), 2048, perm=[16383], gains=[3.0])
    cases.append((q, cases[-1][1], None))
    for (q, frames, counts), want in zip(cases, ref.exact(BUILD, cases)):
        assert run_checked(ctx, q, frames, counts, True, want) == expected_plan(q)


def test_frame_counts_around_a_workgroup(hz, ctx):
    """frames one below, at and one above the plan's frames per workgroup G, counts that end inside a group"""
    q1 = ref.Config(ref.C64, hz.qam_points(4), 40, gains=[1.0], rows=1)
    G = expected_plan(q1)[0]
    assert G == 8
    cases = []
    for cap in (G - 1, G, G + 1, 2 * G + 1):
        q = ref.Config(ref.C64, hz.qam_points(4), 40, gains=[1.0, 2.0], rows=2)
        frames = noisy_frames(q, (2, cap), 0.1, cap)
        cases += [(q, frames, np.array([cap, cap - 3], np.uint32)), (q1, frames[:1], None)]
    for (q, frames, counts), want in zip(cases, ref.exact(BUILD, cases)):
        assert run_checked(ctx, q, frames, counts, True, want)[0] == G


# ---- 3. perm, flip and gains -------------------------------------------------------------------------------------------

def test_perm_flip_and_gains(hz, ctx, hctx):
    """perm: identity, reversal, block_interleaver, all holes, repeats, N < S m and N > S m; flip: all ones and random;
    shared and per-row gains"""
    pts, S, m = hz.qam_points(4), 24, 4
    L = S * m
    perms = {"none": None, "identity": np.arange(L), "reversal": np.arange(L)[::-1], "block": hz.block_interleaver(8, 12), "holes": np.full(L, ref.ERASED),
             "repeats": np.repeat(np.arange(L // 4), 4), "short": np.arange(7) * 13, "long": np.arange(3 * L + 1) % L}
    assert sorted(perms["block"].tolist()) == list(range(L))
    cases = []
    for i, (name, perm) in enumerate(perms.items()):
        N = L if perm is None else len(perm)
        for flip in (None, np.ones(N, np.uint8), ref.random_bits(N, i)):
            for gains in ([0.7], [0.25, 1.0, 4.5]):
                q = ref.Config(ref.C64, pts, S, perm=perm, flip=flip, gains=gains, rows=3)
                cases.append((q, noisy_frames(q, (3, 2), 0.2, 5), np.array([2, 1, 2], np.uint32)))
    wants = ref.exact(BUILD, cases)
    for k, ((q, frames, counts), want) in enumerate(zip(cases, wants)):
        run_checked(ctx if k % 3 else hctx, q, frames, counts, bool(k % 3), want)
    # the forms agree with one another: identity is no perm, all ones flips every sign, holes are erasures
    assert np.array_equal(wants[0], wants[6]) and np.array_equal(wants[0][[0, 2]] ^ 0x80000000, wants[2][[0, 2]]) and (wants[24][[0, 2]] == ref.NAN_BITS).all()
    assert np.array_equal(wants[12][..., ::-1], wants[0]) and not np.array_equal(wants[0], wants[1])


# ---- 4. special values and invariance -------------------------------------------------------------------------------

def test_a_frame_does_not_depend_on_its_place_or_its_neighbours(hz, ctx, hctx):
    """ordinary frames and frames with NaN, infinities, -0, 3e19 and denormals, in other slots, under other R, cap,
    strides and memory spaces, beside frames that are all NaN or infinite: the same floats"""
    pts, S = hz.qam_points(6), 70
    perm = (np.arange(S * 6) * 11) % (S * 6)
    flip = ref.random_bits(S * 6, 4)
    base = ref.Config(ref.C64, pts, S, perm=perm, flip=flip, gains=[1.5], rows=1)
    frames = noisy_frames(base, (1, 6), 0.1, 55)
    frames[0, 1, [0, 3, 8, 9, 20, 31, 44]] = np.nan, np.inf, -np.inf, -0.0, 3e19, 1e-40, -1e-42
    frames[0, 4, 1::2] = np.nan
    (want,) = ref.exact(BUILD, [(base, frames, None)])
    assert (want[0, 1] == ref.NAN_BITS).sum() >= 24 and (want[0, 4] == ref.NAN_BITS).all() and not (want[0, 0] == ref.NAN_BITS).any()
    seen = []
    for R, cap, device, junk in ((1, 6, True, 0.0), (2, 3, True, np.nan), (6, 1, False, np.inf), (7, 5, True, np.nan), (70, 2, True, -np.inf)):
        q = ref.Config(ref.C64, pts, S, perm=perm, flip=flip, gains=[1.5], rows=R)
        block = np.full((R, cap, q.W), junk, np.float32)
        block[1::2, :, ::3] = 0.25
        slots = [(int(s) // cap, int(s) % cap) for s in (ref.splitmix64(R * cap, 6) % np.uint64(R * cap))] if R * cap > 6 else \
            [(s // cap, s % cap) for s in range(6)]
        slots = list(dict.fromkeys(slots))
        for k, (r, f) in enumerate(slots):
            block[r, f] = frames[0, k]
        with bank_of(ctx if device else hctx, q) as d:
            got = host(d.run(dev(block) if device else block)).view(np.uint32)
        for k, (r, f) in enumerate(slots):
            assert np.array_equal(got[r, f], want[0, k]), (R, cap, k)
        seen.append(len(slots))
    assert min(seen) >= 4


# ---- 5. refusals -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", [1, 3])
def test_refused_calls_leave_the_outputs(hz, ctx, R):
    lib = importlib.import_module("go-sdr_amd._capi").lib
    q = ref.Config(ref.C64, hz.qam_points(4), 10, gains=[1.0], rows=R)  # W = 20, N = 40
    cap = 2
    frames = noisy_frames(q, (R, cap), 0.1, 3)
    x = dev(frames)
    both = torch.from_numpy(np.full(R * cap * (q.W + q.N), SENT, np.uint32).view(np.float32)).cuda()
    out = both[:R * cap * q.N]
    with bank_of(ctx, q) as d:
        call = lambda *a: ctx._ck(lib.hzsdr_demap_run(d._h, *a))
        i, o = x.data_ptr(), out.data_ptr()
        if R > 1:
            with pytest.raises(hz.ErrDstTooSmall):
                call(i, cap * q.W, None, cap, o, cap * q.N - 1)
            with pytest.raises(hz.ErrInvalidArgument):
                call(i, cap * q.W - 1, None, cap, o, cap * q.N)
        for bad in ((None, cap * q.W, None, cap, o, cap * q.N), (i, cap * q.W, None, cap, None, cap * q.N), (i, cap * q.W, None, 0, o, cap * q.N),
                    (i, cap * q.W, None, hz.DEMAP_MAX_FRAMES // R + 1, o, cap * q.N),
                    (o, cap * q.W, None, cap, o, cap * q.N),                      # in place
                    (o + 4 * (R * cap * q.N - 1), cap * q.W, None, cap, o, cap * q.N),  # in begins on out's last float
                    (o, cap * q.W, None, cap, o + 4 * (R * cap * q.W - 1), cap * q.N)):
            with pytest.raises(hz.ErrInvalidArgument):
                call(*bad)
        assert lib.hzsdr_demap_run(None, i, cap * q.W, None, cap, o, cap * q.N) == hz.ErrInvalidArgument.status
        torch.cuda.synchronize()
        assert (host(both).view(np.uint32) == SENT).all()
        with pytest.raises(ValueError):
            d.run(dev(np.zeros((R, cap, q.W + 1), np.float32)))
        with pytest.raises(ValueError):
            d.run(dev(np.zeros((R, cap, q.W), np.float64)))
        call(i, cap * q.W, None, cap, o, cap * q.N)
        torch.cuda.synchronize()
        (want,) = ref.exact(BUILD, [(q, frames, None)])
        assert np.array_equal(host(out).view(np.uint32).reshape(R, cap, q.N), want)
        assert (host(both[R * cap * q.N:]).view(np.uint32) == SENT).all()


def test_create_errors(hz, ctx):
    """every create refusal of the header through the library (every bound's edge and the forged perm entries:
    tests/test_demap_cpu.py and tests/test_demap_plan.py against the same hz_demap_plan.h)"""
    lib = importlib.import_module("go-sdr_amd._capi").lib
    out = C.c_void_p()
    fp, u32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
    q4 = hz.qam_points(2)

    def create(q, kind=None, m=None, n_gains=None, null_points=False, null_gains=False):
        pts, perm, flip = q.point_floats(), None if q.perm is None else (q.perm & 0xFFFFFFFF).astype(np.uint32), q.packed_flip()
        ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
        return lib.hzsdr_demap_create(ctx._h, q.kind if kind is None else kind, q.m if m is None else m, None if null_points or not len(pts) else ptr(pts, fp),
                                      q.S, ptr(perm, u32p), q.N, ptr(flip, u8p), None if null_gains else ptr(q.gains, fp), len(q.gains) if n_gains is None else n_gains,
                                      q.rows, C.byref(out))

    def cfg(kind=ref.C64, points=q4, S=8, **kw):
        return ref.Config(kind, points, S, **kw)

    inval = hz.ErrInvalidArgument.status
    for kind in (-1, 0, 2, 31, 34):
        assert create(cfg(), kind=kind) == hz.ErrSampleFormatUnknown.status, kind
    perm = np.arange(16)
    hole, at, above = perm.copy(), perm.copy(), perm.copy()
    hole[3], at[3], above[15] = ref.ERASED, 16, 0xFFFFFFFE
    bad_point = q4.copy()
    bad_point[1] = complex(np.nan, 0)
    refused = [cfg(points=np.zeros(512, np.complex64)), cfg(S=0), cfg(S=8193, points=hz.psk_points(1), perm=perm), cfg(S=2049, points=hz.qam_points(8), perm=perm),
               cfg(perm=np.zeros(0, np.int64)), cfg(perm=np.arange(8193) % 16), cfg(N=15), cfg(perm=at), cfg(perm=above), cfg(points=bad_point),
               cfg(gains=[0.0]), cfg(gains=[-1.0]), cfg(gains=[np.inf]), cfg(gains=[np.nan]), cfg(gains=[1.0, 2.0], rows=3), cfg(rows=0), cfg(rows=8193),
               cfg(ref.LLR_F32, None, m=2, N=16), cfg(ref.REAL_F32, np.array([1.0, np.inf], np.float32))]
    for k, bad in enumerate(refused):
        assert not ref.accepted(bad) and create(bad) == inval, k
    assert create(cfg(), m=0) == inval and create(cfg(), m=9) == inval and create(cfg(), null_points=True) == inval and create(cfg(), null_gains=True) == inval
    assert create(cfg(), n_gains=0) == inval and create(cfg(rows=3), n_gains=2) == inval
    llr_with_points = ref.Config(ref.LLR_F32, None, 8)
    assert lib.hzsdr_demap_create(ctx._h, ref.LLR_F32, 1, q4.view(np.float32).ctypes.data_as(fp), 8, None, 8, None, llr_with_points.gains.ctypes.data_as(fp), 1, 1,
                                  C.byref(out)) == inval
    for good in (cfg(perm=hole), cfg(rows=8192), cfg(gains=[1e-45]), cfg(S=8192, perm=perm), cfg(ref.LLR_F32, None), cfg(perm=[0]), cfg(gains=[1.0, 2.0, 3.0], rows=3)):
        assert ref.accepted(good) and create(good) == 0 and lib.hzsdr_demap_free(out) == 0
    with pytest.raises(hz.ErrInvalidArgument):
        ctx.demapper(hz.DEMAP_C64, q4, 8, rows=0)
    with pytest.raises(hz.ErrInvalidArgument):
        ctx.demapper(hz.DEMAP_C64, q4[:3], 8)
    with pytest.raises(hz.ErrInvalidArgument):
        ctx.demapper(hz.DEMAP_C64, q4, 8, flip=np.zeros(3, np.uint8))


# ---- 6. the chain ------------------------------------------------------------------------------------------------

CHAIN_EVERY, CHAIN_SIGMA, CHAIN_ROWS = 60, 0.25, 8
CHAIN_IL = (8, 12)


@pytest.fixture(scope="module")
def code96(hz):
    """the (3, 6) code of n = 96, systematic: 48 data bits in front"""
    return hz.ldpc_systematic(hz.regular_code(96, 3, 6, seed=1))[0]


def chain_configs(hz, code, hard=False):
    pts = hz.qam_points(4)
    fq = framesync_ref.Config(32, framesync_ref.rotated_words(WORD32, 32), 48, B=2, cplx=True, thr=3, maps=[0, 1, 2, 3])
    dq = ref.Config(ref.C64, pts, 24, perm=hz.block_interleaver(*CHAIN_IL), flip=ref.random_bits(96, 0xF11B), gains=[hz.demap_gain(CHAIN_SIGMA)], rows=CHAIN_ROWS)
    lq = ldpc_ref.Config.of(code, kind=ldpc_ref.BITS if hard else ldpc_ref.SOFT_F32, D=code.k, scale=4.0, level=16, max_iters=40, a=12)
    return fq, dq, lq


def chain_rows(hz, fq, dq, code, nsym=500):
    """CHAIN_ROWS rows of 16-QAM symbols at one sample per symbol -> (x complex64 (rows, nsym), per row [(first symbol of
    the word, data bits)]): row r arrives times i^(r % 4); rows 4 ... 7 carry noise"""
    pts = dq.points
    corner = np.float32(np.abs(pts.real).max())
    rows, sent = [], []
    for r in range(CHAIN_ROWS):
        sym = pts[(ref.splitmix64(900 + r, nsym) >> np.uint64(60)).astype(np.int64)].copy()
        planted = []
        for k, at in enumerate(range(10, nsym - 40 - 1, CHAIN_EVERY)):
            data = ref.random_bits(code.k, 1000 * r + k)
            word = framesync_ref.word_bits(WORD32, 32).astype(np.float32) * 2 - 1
            sym[at:at + 16] = (word[0::2] + 1j * word[1::2]) * corner
            tx = np.empty(96, np.uint8)
            tx[dq.perm] = hz.ldpc_encode(code, data) ^ dq.flip
            sym[at + 16:at + 40] = hz.map_bits(pts, tx)
            planted.append((at, data))
        x = sym.astype(np.complex128) * (1, 1j, -1, -1j)[r % 4]  # (exact: components swap and change sign)
        if r >= 4:
            n = ref.gaussian(7000 + r, 2 * nsym) * CHAIN_SIGMA
            x = x + n[:nsym] + 1j * n[nsym:]
        rows.append(x.astype(np.complex64))
        sent.append(planted)
    return np.stack(rows), sent


def host_chain(fq, dq, lq, x, cap=16):
    """the chained host programs over the rows x in one push -> per row {payload's first symbol: (data bytes, info)}: frame
    sync, the soft frame program, the demapper program, then the LDPC program over its floats (SOFT_F32) or over their
    hard decisions (BITS)"""
    ((per, _),) = framesync_ref.exact(BUILD, [(fq, [x], cap)])
    frames, positions, info, counts = per[0]
    assert int(counts.max()) <= cap
    ((sper, _),) = softframe_ref.exact(BUILD, [(softframe_ref.of_framesync(fq), [(x, None, counts, positions, info)], cap)])
    (bits,) = ref.exact(BUILD, [(dq, sper[0][0].view(np.float32), counts)])
    values = bits.view(np.float32)
    ((data, linfo),) = ldpc_ref.exact(BUILD, [(lq, ldpc_ref.hard_frames(values) if lq.kind == ldpc_ref.BITS else values, counts)])
    return [{int(positions[r, f]): (bytes(data[r, f]), int(linfo[r, f])) for f in range(min(int(counts[r]), cap))} for r in range(x.shape[0])]


def recovered(want, sent, rows):
    """over `rows`: (frames planted, found, decoded to the sent data)"""
    all_ = [(r, at, data) for r in rows for at, data in sent[r]]
    got = [want[r].get(at + 16) for r, at, _ in all_]
    return len(all_), sum(g is not None for g in got), sum(g is not None and g[0] == bytes(np.packbits(d)) for g, (_, _, d) in zip(got, all_))


def test_the_chain_to_checked_data(hz, ctx, code96):
    """frame sync beside the soft frame bank -> demapper -> LDPC on the device, with nothing read in between, equal the
    chained host programs exactly, frame for frame.  The noise-free rows return the planted data for every frame, under
    all four rotations; on the noisy rows the host chain recovers 31 of 32 frames (CHAIN_SOFT) where hard decisions on the
    same values recover 19 (CHAIN_HARD) (measured on the CPU from the chained host programs for these seeds; the module's
    header has the setting)."""
    st = importlib.import_module("go-sdr_amd.stream")
    fq, dq, lq = chain_configs(hz, code96)
    x, sent = chain_rows(hz, fq, dq, code96)
    want = host_chain(fq, dq, lq, x)
    clean, noisy = recovered(want, sent, range(4)), recovered(want, sent, range(4, 8))
    print("chain: clean", clean, "noisy soft", noisy)
    assert clean == (32, 32, 32) and noisy[0] == 32 and noisy[1] == 32 and noisy[2] >= CHAIN_SOFT
    fargs, fkw = fq.create_args()
    code = hz.LdpcCode(lq.n, lq.row_ptr, lq.col)
    largs, lkw = lq.create_args(code)
    with ctx.frame_sync(fq.kind, *fargs, rows=CHAIN_ROWS, **fkw) as fs, ctx.soft_frames(fs) as sf, bank_of(ctx, dq) as dm, \
            ctx.ldpc(*largs, rows=CHAIN_ROWS, **lkw) as ld:
        xd = dev(x)
        blocks = [xd[:, a:b] for a, b in ((0, 173), (173, 174), (174, x.shape[1]))]
        parts = list(st.ldpc_frames(blocks, fs, sf, ld, cap=16, demap=dm))
        for r in range(CHAIN_ROWS):
            got = {int(p): (bytes(d), int(u) | (int(it) << 16) | (int(ok) << 31)) for part in parts
                   for d, p, u, it, ok in zip(part[r][0], part[r][1], part[r][3], part[r][4], part[r][5])}
            assert got == want[r], r
        # the checks of the keyword: a demapper of other rows, another W, another N; without it the decoder's N is the bank's P
        qs = (ref.Config(ref.C64, dq.points, 24, gains=[1.0], rows=3), ref.Config(ref.C64, dq.points, 23, gains=[1.0], rows=CHAIN_ROWS),
              ref.Config(ref.C64, dq.points, 24, perm=np.arange(95), gains=[1.0], rows=CHAIN_ROWS))
        for q in qs:
            with bank_of(ctx, q) as bad, pytest.raises(ValueError):
                list(st.ldpc_frames([], fs, sf, ld, demap=bad))
        with pytest.raises(ValueError):
            list(st.ldpc_frames([], fs, sf, ld))


# ---- 7. the other layers -----------------------------------------------------------------------------------------

def _run(exe):
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "go-sdr_amd") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    return subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)


def test_c_demap_walkthrough(hz):
    """tests/c/test_demap_abi.c compiled by gcc as C99 and run against libhzsdr_hip.so."""
    exe = os.path.join(BUILD, "test_demap_abi")
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "test_demap_abi.c"), "-L" + os.path.join(ROOT, "go-sdr_amd"),
                           "-lhzsdr_hip", "-lm", "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    p = _run(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "demap-abi ok" in p.stdout


def test_cxx_demap(hz):
    """tests/cxx/test_demap.cpp (hzsdr::stream::Demapper of go-sdr_amd/cxx/hzsdr.hpp) built with g++ and run."""
    exe = os.path.join(BUILD, "test_demap_cxx")
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + ROOT, os.path.join(ROOT, "tests", "cxx", "test_demap.cpp"),
                           "-L" + os.path.join(ROOT, "go-sdr_amd"), "-lhzsdr_hip", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    p = _run(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "demap-cxx ok" in p.stdout

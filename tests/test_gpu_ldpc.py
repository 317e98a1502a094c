"""The LDPC decoder bank (include/hzsdr_ldpc.h) on the GPU against the host program tests/host/ldpc_ref.cpp, which
tests/test_ldpc_cpu.py holds to the numpy restatement and to anchors of its own: decoded bytes and info are compared
EXACTLY, the destinations are full of sentinels, the pitches are above the need, and every slot that is not decoded is
checked byte for byte.  Wherever it is provable -- clean codewords, planted codewords that the program recovers -- the
tests also assert that the reference decoded what was planted, so that two wrong answers cannot agree.

The chain test (carrier -> symbol timing -> frame sync beside the soft frame bank -> LDPC on BPSK rows) is the Viterbi
chain test's signal path: a 32-bit word and a payload, one frame every 140 symbols from symbol 10 on, 5 samples per
symbol, three carrier offsets and phases.  The payload is a whole codeword of the (3, 6) code of n = 96 that
regular_code(96, 3, 6, seed=1) makes, 48 data bits in front; white noise 5 dB below the symbol power per component, at
which the loops in front lose frames of their own.  Measured on the CPU from the chained host programs over the seeds
1 ... 12 with the three offsets and phases (36 rows, 9 frames each whose word starts at symbol 20 or later, 324 frames):
the frame sync program finds 255 of them; the soft path (HZSDR_LDPC_SOFT_F32 behind the soft frame bank, scale 16,
a = 12) returns the sent data for 244 of those, hard decisions (HZSDR_LDPC_BITS over the frame sync bank's bits, level
16) for 232.  The three rows of the test itself: 27 frames, 21 found, 21 recovered (hard decisions: 20)."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import carrier_ref
import framesync_ref
import ldpc_ref as ref
import softframe_ref
import symsync_ref
from conftest import ROOT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BUILD = os.path.join(ROOT, "build")
SENT8, SENT32 = 0xA5, 0xA5A5A5A5
WORD32 = 0x1ACFFC1D
CHAIN_A = 20


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
def code96(hz):
    """the (3, 6) code of n = 96, systematic: 48 data bits in front"""
    return hz.ldpc_systematic(hz.regular_code(96, 3, 6, seed=1))[0]


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def bank_of(hz, c, q, rows):
    code = hz.LdpcCode(q.n, q.row_ptr, q.col)
    args, kw = q.create_args(code)
    return c.ldpc(*args, rows=rows, **kw)


def strided(wide, shape, pitch, device):
    R, cap, w = shape
    if device:
        return torch.as_strided(wide, shape, (pitch, w, 1))
    return np.lib.stride_tricks.as_strided(wide, shape, (pitch * wide.itemsize, w * wide.itemsize, wide.itemsize))


def decode_checked(hz, c, q, frames, counts, device, want, pads=(3, 5)):
    """frames (R, cap, width) through a new bank, input and output inside wider buffers, against the program's (data,
    info): the decoded slots exactly, every other byte of the destinations still a sentinel -> the bank's plan"""
    R, cap, width = frames.shape
    ipitch, opitch = cap * width + pads[0], cap * q.DB + pads[1]
    wide_in = np.zeros((R, ipitch), frames.dtype)
    wide_in[:, :cap * width] = frames.reshape(R, -1)
    wide_out, info = np.full((R, opitch), SENT8, np.uint8), np.full((R, cap), SENT32, np.uint32)
    cin = None if counts is None else np.asarray(counts, np.uint32)
    if device:
        wide_in, wide_out, info = dev(wide_in), dev(wide_out), dev(info.view(np.int32))
        cin = None if cin is None else dev(cin.view(np.int32))
    with bank_of(hz, c, q, R) as v:
        assert v.sizes() == (q.N, q.FB, q.n, q.m, q.E, q.DB)
        v.decode(strided(wide_in, (R, cap, width), ipitch, device), cin, cap, out=(strided(wide_out, (R, cap, q.DB), opitch, device), info))
        if device:
            torch.cuda.synchronize()
        plan = v.plan()
    wd, wi = want
    gw, gi = host(wide_out), host(info).view(np.uint32)
    for r in range(R):
        m = cap if counts is None else min(int(counts[r]), cap)
        assert np.array_equal(gw[r, :m * q.DB].reshape(m, q.DB), wd[r, :m]), (r, np.flatnonzero((gw[r, :m * q.DB].reshape(m, q.DB) != wd[r, :m]).any(axis=1)))
        assert (gw[r, m * q.DB:] == SENT8).all(), r
        assert np.array_equal(gi[r, :m], wi[r, :m]) and (gi[r, m:] == SENT32).all(), (r, gi[r, :m], wi[r, :m])
    return plan


def noisy(hz, code, shape, sigma, seed):
    """(soft frames (*shape, n), data bits (*shape, k)) of planted codewords under noise"""
    F = int(np.prod(shape))
    data = np.stack([ref.random_bits(code.k, seed * 1000 + f) for f in range(F)])
    return ref.bpsk(hz.ldpc_encode(code, data), sigma, seed).reshape(*shape, code.n), data.reshape(*shape, code.k)


def inputs(q, values):
    """soft values (..., n) -> what the bank of q takes: its received positions, as floats or packed hard bits"""
    v = values[..., q.head:q.head + q.N]
    return ref.hard_frames(v) if q.kind == ref.BITS else np.ascontiguousarray(v)


def expected_plan(q):
    """hz_ldpc_plan.h's dealing, restated: (frames per workgroup, threads per frame, a frame's LDS bytes, form)"""
    up = lambda v, to: (v + to - 1) // to * to
    T = min(1024, up(max(q.m, (q.n + 1) // 2), 64))
    frame = up(up(2 * q.n, 4) + up(q.n, 4) + q.E, 16)
    tables = up(4 * (q.m + 1) + 4 * (q.n + 1) + 4 * q.E, 16)
    in_lds = 64 + tables + frame <= 160 * 1024
    G = min(8, 1024 // T, (160 * 1024 - 64 - (tables if in_lds else 0)) // frame)
    return G, T, frame, ref.FORM_TABLES_LDS if in_lds else ref.FORM_TABLES_CACHE


# ---- 1. tiny and short codes: rows, counts, memory spaces ------------------------------------------------------------

@pytest.mark.parametrize("space", ["device", "host"])
@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("which", ["hamming", "n96"])
def test_short_codes_rows_counts_and_spaces(hz, ctx, hctx, code96, which, R, space):
    """the (7, 4) code and the (3, 6) code of n = 96, both inputs, cap in {1, 3, 4} with ragged counts, 0 and counts
    above cap among them (and none at all); the frames are planted codewords under noise"""
    device = space == "device"
    c = ctx if device else hctx
    code = hz.ldpc_systematic(hz.LdpcCode.from_dense(ref.HAMMING74))[0] if which == "hamming" else code96
    most = 0
    for cap in (1, 3, 4):
        for kind in (ref.SOFT_F32, ref.BITS):
            q = ref.Config.of(code, kind=kind, D=code.k, scale=12.0, level=7, max_iters=20, a=(12, 16)[cap % 2], beta=cap % 2)
            x, _ = noisy(hz, code, (R, cap), 0.75, 10 * R + cap)
            frames = inputs(q, x)
            counts = (ref.splitmix64(R * 8 + cap, R) % np.uint64(cap + 3)).astype(np.uint32)
            counts[0] = cap + 2
            if R > 2:
                counts[1], counts[2] = 0, cap
            for cnt in (counts, None):
                ((wd, wi),) = ref.exact(BUILD, [(q, frames, cnt)])
                assert decode_checked(hz, c, q, frames, cnt, device, (wd, wi)) == expected_plan(q)
            most = max(most, int(ref.split(wi)[1].max()))
    assert most >= 1


def test_frame_counts_around_a_workgroup(hz, ctx, code96):
    """frames one below, at and one above one and two workgroups' worth, from plan(); counts that end inside a group"""
    q = ref.Config.of(code96, D=code96.k, scale=16.0, max_iters=30)
    G = expected_plan(q)[0]
    assert G == 8
    for cap in (G - 1, G, G + 1, 2 * G - 1, 2 * G, 2 * G + 1):
        x, data = noisy(hz, code96, (2, cap), 0.7, cap)
        counts = np.array([cap, cap - 3], np.uint32)
        ((wd, wi),) = ref.exact(BUILD, [(q, x, counts)])
        assert decode_checked(hz, ctx, q, x, counts, True, (wd, wi))[0] == G
        x1 = x[:1]
        ((wd, wi),) = ref.exact(BUILD, [(q, x1, None)])
        decode_checked(hz, ctx, q, x1, None, True, (wd, wi))
        u, it, ok = ref.split(wi)
        assert len(set(it[0].tolist())) > 1  # the frames of a workgroup stop at different iterations
        for f in np.flatnonzero(ok[0]):
            assert np.array_equal(wd[0, f], np.packbits(data[0, f])), (cap, f)


# ---- 2. degree and size edges ------------------------------------------------------------------------------------

def test_degrees_64_and_2(hz, ctx):
    """a code with a check of degree 64 and a variable of degree 64; a code whose checks all have degree 2 (a cycle:
    its codewords are the two constant words)"""
    rows = [list(range(64))] + [[0, 64 + 2 * (c - 1), 65 + 2 * (c - 1)] for c in range(1, 64)]
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    q = ref.Config(190, rp, np.concatenate(rows), scale=9.0, max_iters=15, a=12)
    assert ref.accepted(q) and np.bincount(q.col).max() == 64
    x = ref.bpsk(np.zeros((1, 2, 190), np.uint8), 0.6, 4)
    ((wd, wi),) = ref.exact(BUILD, [(q, x, None)])
    decode_checked(hz, ctx, q, x, None, True, (wd, wi))
    n = 130
    ring = np.stack([np.arange(n), (np.arange(n) + 1) % n], axis=1)
    ring.sort(axis=1)
    q = ref.Config(n, np.arange(n + 1) * 2, ring.reshape(-1), scale=9.0, max_iters=40, a=16)
    x = ref.bpsk(np.ones((1, 2, n), np.uint8), 0.9, 5)
    ((wd, wi),) = ref.exact(BUILD, [(q, x, None)])
    decode_checked(hz, ctx, q, x, None, True, (wd, wi))
    assert ref.split(wi)[1].max() >= 1


def test_the_largest_code(hz, ctx):
    """n = 16384 with N = 8192 received behind a head of 100 at E = 65536: the frame's state asks 112 KiB of LDS and the
    tables come through the cache.  The all-zero codeword, clean (iters = 0) and under noise (to max_iters)"""
    code = hz.regular_code(16384, 4, 8, seed=3)
    q = ref.Config.of(code, head=100, N=8192, D=16384, scale=8.0, max_iters=5, a=12)
    assert q.E == 65536 and expected_plan(q) == (1, 1024, 114688, ref.FORM_TABLES_CACHE)
    x = np.stack([np.full(8192, -1.0, np.float32), ref.bpsk(np.zeros(8192, np.uint8), 0.5, 8)])[None]
    ((wd, wi),) = ref.exact(BUILD, [(q, x, None)])
    assert int(wi[0, 0]) == 1 << 31 and not wd[0, 0].any() and ref.split(wi)[1][0, 1] == 5
    assert decode_checked(hz, ctx, q, x, None, True, (wd, wi)) == expected_plan(q)


@pytest.mark.parametrize("D", [1, 9, 65])
def test_n_65_and_the_data_lengths(hz, ctx, D):
    """n = 65 (an odd size, one more than a wave), D = 1, D = 9 and D = n: pad bits 0, neighbours untouched"""
    code = hz.regular_code(65, 3, 5, seed=2)
    q = ref.Config.of(code, D=D, scale=10.0, max_iters=10, a=12)
    x = ref.bpsk(np.ones((2, 3, 65), np.uint8), 0.8, D)
    ((wd, wi),) = ref.exact(BUILD, [(q, x, None)])
    decode_checked(hz, ctx, q, x, None, True, (wd, wi), pads=(1, 1))
    assert wd.any() and (D % 8 == 0 or not (wd[..., -1] & ((1 << (8 - D % 8)) - 1)).any())


# ---- 3. stopping ---------------------------------------------------------------------------------------------------

def test_stopping(hz, ctx, code96):
    """a clean frame stops at iters = 0; max_iters = 1; a frame of noise alone runs all 255 iterations and leaves with
    ok = 0, u > 0 and its bits emitted; a frame that converges at exactly it = max_iters, and not one iteration sooner"""
    x, data = noisy(hz, code96, (1, 8), 0.8, 21)
    q = ref.Config.of(code96, D=code96.k, scale=14.0, max_iters=60, a=12)
    ((wd, wi),) = ref.exact(BUILD, [(q, x, None)])
    u, it, ok = ref.split(wi)
    f = int(np.argmax(np.where(ok[0] == 1, it[0], 0)))
    k = int(it[0, f])
    assert k >= 3 and np.array_equal(wd[0, f], np.packbits(data[0, f]))
    clean = ((hz.ldpc_encode(code96, data[0, 0]).astype(np.float32) * 2 - 1) * np.float32(0.2))
    noise = ref.gaussian(77, 96).astype(np.float32)
    cases = []
    for max_iters in (1, k - 1, k, 255):
        frames = np.stack([clean, x[0, f], noise, x[0, 0]])[None]
        cases.append((ref.Config.of(code96, D=code96.k, scale=14.0, max_iters=max_iters, a=12), frames, None))
    for (qq, frames, _), (wd, wi) in zip(cases, ref.exact(BUILD, cases)):
        u, it, ok = ref.split(wi)
        assert (u[0, 0], it[0, 0], ok[0, 0]) == (0, 0, 1) and np.array_equal(wd[0, 0], np.packbits(data[0, 0]))
        assert (it[0, 1], ok[0, 1]) == ((k, 1) if qq.max_iters >= k else (qq.max_iters, 0))
        assert (it[0, 2], ok[0, 2]) == (qq.max_iters, 0) and u[0, 2] > 0 and wd[0, 2].any()
        decode_checked(hz, ctx, qq, frames, None, True, (wd, wi))


# ---- 4. extreme values and invariance ---------------------------------------------------------------------------------

@pytest.mark.parametrize("space", ["device", "host"])
def test_extreme_frames_beside_ordinary_ones(hz, ctx, hctx, code96, space):
    """frames of NaN, +infinity, -infinity, -0 and zeros (all erasures) set beside ordinary frames, and special values
    inside an ordinary frame: the device agrees with the program, and the ordinary frames' results are what they are
    alone"""
    device = space == "device"
    q = ref.Config.of(code96, D=code96.k, scale=12.0, max_iters=25, a=12)
    x, _ = noisy(hz, code96, (6,), 0.75, 33)
    x[5, [3, 17, 40, 41]] = np.nan, -0.0, np.inf, -np.inf
    ((alone, alone_info),) = ref.exact(BUILD, [(q, x[None], None)])
    block = np.zeros((2, 6, 96), np.float32)
    block[0, 0], block[0, 2], block[0, 4] = np.nan, np.inf, -0.0
    block[1, 1], block[1, 3] = -np.inf, np.frombuffer(np.uint32(0xFFC00001).tobytes(), np.float32)[0]
    where = [(0, 1), (0, 3), (0, 5), (1, 0), (1, 2), (1, 4)]
    for k, (r, f) in enumerate(where):
        block[r, f] = x[k]
    ((wd, wi),) = ref.exact(BUILD, [(q, block, None)])
    for k, (r, f) in enumerate(where):
        assert np.array_equal(wd[r, f], alone[0, k]) and wi[r, f] == alone_info[0, k], k
    for r, f in ((0, 0), (0, 4), (1, 1), (1, 3), (1, 5)):
        assert not wd[r, f].any() and int(wi[r, f]) == 1 << 31, (r, f)
    assert (wd[0, 2] == 0xFF).all() and int(wi[0, 2]) == 1 << 31  # (every check has even degree: all ones is a codeword)
    decode_checked(hz, ctx if device else hctx, q, block, None, device, (wd, wi))


def test_a_frame_does_not_depend_on_its_place_or_its_neighbours(hz, ctx, hctx, code96):
    """the same frames in other slots, under other R, cap, pitches and memory spaces, beside NaN, infinite and
    all-erasure frames: the same bytes and info"""
    q = ref.Config.of(code96, D=code96.k, scale=12.0, max_iters=25, a=12, beta=1)
    frames, _ = noisy(hz, code96, (1, 6), 0.8, 55)
    ((wd, wi),) = ref.exact(BUILD, [(q, frames, None)])
    seen = []
    for R, cap, device, junk in ((1, 6, True, 0.0), (2, 3, True, np.nan), (6, 1, False, np.inf), (7, 5, True, np.nan), (70, 2, True, -np.inf)):
        block = np.full((R, cap, q.N), junk, np.float32)
        block[1::2, :, ::3] = 0.0
        slots = [(int(s) // cap, int(s) % cap) for s in (ref.splitmix64(R * cap, 6) % np.uint64(R * cap))] if R * cap > 6 else \
            [(s // cap, s % cap) for s in range(6)]
        slots = list(dict.fromkeys(slots))
        for k, (r, f) in enumerate(slots):
            block[r, f] = frames[0, k]
        c = ctx if device else hctx
        with bank_of(hz, c, q, R) as v:
            data, info = v.decode(dev(block) if device else block)
            data, info = host(data), host(info).view(np.uint32)
        for k, (r, f) in enumerate(slots):
            assert np.array_equal(data[r, f], wd[0, k]) and info[r, f] == wi[0, k], (R, cap, k)
        seen.append(len(slots))
    assert min(seen) >= 4


# ---- 5. planted codewords -------------------------------------------------------------------------------------------

def test_planted_codewords(hz, ctx):
    """one (3, 6) code of n = 512, a = 12, beta = 0, scale 16, 64 frames of planted codewords over BPSK at sigma = 0.7:
    the program recovers every one (tests/test_ldpc_cpu.py checks the same frames without a GPU), and the device equals
    the program, so the planted data came back"""
    code = hz.ldpc_systematic(hz.regular_code(512, 3, 6, seed=1))[0]
    data = np.stack([ref.random_bits(code.k, 7 + i) for i in range(64)])
    x = ref.bpsk(hz.ldpc_encode(code, data), 0.7, 99).reshape(4, 16, 512)
    q = ref.Config.of(code, D=code.k, scale=16.0, max_iters=50, a=12, beta=0)
    ((wd, wi),) = ref.exact(BUILD, [(q, x, None)])
    u, it, ok = ref.split(wi)
    assert ok.all() and np.array_equal(wd.reshape(64, -1), np.packbits(data, axis=1)) and it.max() > 2
    plan = decode_checked(hz, ctx, q, x, None, True, (wd, wi))
    assert plan == expected_plan(q) and plan[3] == ref.FORM_TABLES_LDS


# ---- 6. refusals -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", [1, 3])
def test_refused_calls_leave_the_outputs(hz, ctx, code96, R):
    lib = importlib.import_module("go-sdr_amd._capi").lib
    q = ref.Config.of(code96, kind=ref.BITS, D=30, level=3)
    cap = 2
    cw = hz.ldpc_encode(code96, np.stack([ref.random_bits(48, f) for f in range(R * cap)]))
    frames = np.packbits(cw, axis=1).reshape(R, cap, q.FB)
    x = dev(frames)
    out, info = torch.full((R, cap * q.DB), SENT8, dtype=torch.uint8, device="cuda"), torch.full((R, cap), 7, dtype=torch.int32, device="cuda")
    with bank_of(hz, ctx, q, R) as v:
        call = lambda *a: ctx._ck(lib.hzsdr_ldpc_decode(v._h, *a))
        i, o, p = x.data_ptr(), out.data_ptr(), info.data_ptr()
        if R > 1:
            with pytest.raises(hz.ErrDstTooSmall):
                call(i, cap * q.FB, None, cap, o, cap * q.DB - 1, p)
            with pytest.raises(hz.ErrInvalidArgument):
                call(i, cap * q.FB - 1, None, cap, o, cap * q.DB, p)
        for bad in ((None, cap * q.FB, None, cap, o, cap * q.DB, p), (i, cap * q.FB, None, cap, None, cap * q.DB, p), (i, cap * q.FB, None, cap, o, cap * q.DB, None),
                    (i, cap * q.FB, None, 0, o, cap * q.DB, p), (i, cap * q.FB, None, hz.LDPC_MAX_FRAMES // R + 1, o, cap * q.DB, p)):
            with pytest.raises(hz.ErrInvalidArgument):
                call(*bad)
        assert lib.hzsdr_ldpc_decode(None, i, cap * q.FB, None, cap, o, cap * q.DB, p) == hz.ErrInvalidArgument.status
        torch.cuda.synchronize()
        assert (out == SENT8).all() and (info == 7).all()
        with pytest.raises(ValueError):
            v.decode(dev(np.zeros((R, cap, q.FB + 1), np.uint8)))
        with pytest.raises(ValueError):
            v.decode(dev(np.zeros((R, cap, q.FB), np.float32)))
        call(i, cap * q.FB, None, cap, o, cap * q.DB, p)
        torch.cuda.synchronize()
        ((wd, wi),) = ref.exact(BUILD, [(q, frames, None)])
        assert np.array_equal(host(out).reshape(R, cap, q.DB), wd) and np.array_equal(host(info).view(np.uint32), wi) and (wi == 1 << 31).all()


def test_create_errors(hz, ctx, code96):
    """rows 0 and 8193, other kinds, null arrays, and one bound of each sort through the library (every bound's edge and
    the forged arrays: tests/test_ldpc_cpu.py and tests/test_ldpc_plan.py against the same hz_ldpc_plan.h)"""
    lib = importlib.import_module("go-sdr_amd._capi").lib
    out = C.c_void_p()
    u32p = C.POINTER(C.c_uint32)

    def create(q, rows=1, kind=None, m=None, E=None):
        rp, col = ((np.asarray(a, np.int64) & 0xFFFFFFFF).astype(np.uint32) for a in (q.row_ptr, q.col))
        return lib.hzsdr_ldpc_create(ctx._h, q.kind if kind is None else kind, q.m if m is None else m, q.n, rp.ctypes.data_as(u32p), col.ctypes.data_as(u32p),
                                     q.E if E is None else E, q.head, q.N, q.D, q.scale, q.level, q.max_iters, q.a, q.beta, rows, C.byref(out))

    def cfg(**kw):
        return ref.Config.of(code96, **kw)

    inval = hz.ErrInvalidArgument.status
    assert create(cfg(), 0) == inval and create(cfg(), hz.LDPC_MAX_ROWS + 1) == inval
    assert create(cfg(), hz.LDPC_MAX_ROWS) == 0 and lib.hzsdr_ldpc_free(out) == 0
    for kind in (-1, 0, 2, 31, 33):
        assert create(cfg(), 1, kind) == hz.ErrSampleFormatUnknown.status, kind
    q = cfg()
    rp = q.row_ptr.astype(np.uint32)
    assert lib.hzsdr_ldpc_create(ctx._h, 32, q.m, q.n, None, rp.ctypes.data_as(u32p), q.E, 0, 96, 96, 1.0, 1, 10, 12, 0, 1, C.byref(out)) == inval
    assert lib.hzsdr_ldpc_create(ctx._h, 32, q.m, q.n, rp.ctypes.data_as(u32p), None, q.E, 0, 96, 96, 1.0, 1, 10, 12, 0, 1, C.byref(out)) == inval
    bad_rp, bad_col = q.row_ptr.copy(), q.col.copy()
    bad_rp[5], bad_col[9] = 0xFFFFFFFF, 96
    for bad in (cfg(N=0), cfg(N=97), cfg(head=1, N=96), cfg(D=0), cfg(D=97), cfg(max_iters=0), cfg(max_iters=256), cfg(a=0), cfg(a=17), cfg(beta=127),
                cfg(scale=0.0), cfg(scale=np.inf), cfg(kind=ref.BITS, level=0), cfg(kind=ref.BITS, level=128),
                ref.Config(96, bad_rp, q.col), ref.Config(96, q.row_ptr, bad_col), ref.Config(97, q.row_ptr, q.col, N=96)):
        assert not ref.accepted(bad) and create(bad) == inval
    assert create(cfg(), m=q.m - 1) == inval and create(cfg(), E=q.E - 1) == inval and create(cfg(), E=hz.LDPC_MAX_EDGES + 1) == inval
    for good in (cfg(N=1, head=95, D=1), cfg(max_iters=255, a=16, beta=126), cfg(kind=ref.BITS, level=127, scale=0.0), cfg(scale=1e-30)):
        assert ref.accepted(good) and create(good) == 0 and lib.hzsdr_ldpc_free(out) == 0
    with pytest.raises(hz.ErrInvalidArgument):
        ctx.ldpc(hz.LDPC_SOFT_F32, code96, rows=0)


# ---- 7. the chain ------------------------------------------------------------------------------------------------

CHAIN_SPS, CHAIN_NOISE_DB, CHAIN_EVERY = 5.0, -5.0, 140
CHAIN_CASES = ((1, 0.0005, 0.3), (2, -0.001, 1.9), (3, 0.0015, 4.0))  # seed, carrier offset in cycles per sample, phase


def chain_configs(hz, code, kind=ref.SOFT_F32):
    words, maps = hz.sync_hypotheses(WORD32, 32, 1, "invert")
    fq = framesync_ref.Config(32, words, code.n, B=1, cplx=True, thr=3, maps=maps)
    lq = ref.Config.of(code, kind=kind, D=code.k, scale=16.0, level=16, max_iters=40, a=12)
    return fq, lq


def coded_frames_signal(hz, fq, code, nsym, seed):
    """BPSK symbols (bit 1 is +) that carry a frame -- the 32-bit word, then a codeword of 48 random data bits -- every
    CHAIN_EVERY symbols from symbol 10 on, random bits between -> (a complex (nsym,), [(first symbol of the word, data)])"""
    bits = framesync_ref.random_bits(nsym, seed)
    sent = []
    for k, at in enumerate(range(10, nsym - fq.W - fq.P - 1, CHAIN_EVERY)):
        data = ref.random_bits(code.k, 1000 * seed + k)
        framesync_ref.plant(bits, at, fq.words[0], fq.W, hz.ldpc_encode(code, data))
        sent.append((at, data))
    return (bits.astype(np.float64) * 2.0 - 1.0).astype(np.complex128), sent


def chain_inputs(hz, fq, code, cases=CHAIN_CASES):
    rows, sent = [], []
    for seed, off, phase in cases:
        a, s = coded_frames_signal(hz, fq, code, 1500, seed)
        x = symsync_ref.signal(a, CHAIN_SPS, 0.25 * (seed % 4), noise_db=CHAIN_NOISE_DB, seed=seed).astype(np.complex128)
        rows.append((x * np.exp(2j * np.pi * (off * np.arange(len(x)) + phase))).astype(np.complex64))
        sent.append(s)
    n = min(len(r) for r in rows)
    return np.stack([r[:n] for r in rows]), sent


def chain_params(hz):
    return (np.array([*carrier_ref.gains(0.01), 0.0, -0.01, 0.01], np.float32), np.array([CHAIN_SPS, 0.01, *hz.loop_gains(CHAIN_SPS)], np.float32))


def host_chain(hz, fq, lq, x, cap=16):
    """the chained host programs over the rows x in one push -> per row {payload's first symbol: (data bytes, info)}:
    carrier, symbol timing, frame sync, then the soft frame program and the LDPC program over its floats (SOFT_F32), or
    the LDPC program over the frame sync program's bits (BITS)"""
    cp, sp = chain_params(hz)
    ((derot, _, _),) = carrier_ref.exact(BUILD, [(carrier_ref.BPSK, cp, x)])
    ((sym, cnt, _, _),) = symsync_ref.exact(BUILD, [(sp, derot)])
    ((per, _),) = framesync_ref.exact(BUILD, [(fq, [(sym, cnt)], cap)])
    frames, positions, info, counts = per[0]
    assert int(counts.max()) <= cap
    if lq.kind == ref.SOFT_F32:
        ((sper, _),) = softframe_ref.exact(BUILD, [(softframe_ref.of_framesync(fq), [(sym, cnt, counts, positions, info)], cap)])
        frames = sper[0][0].view(np.float32)
    ((data, linfo),) = ref.exact(BUILD, [(lq, frames, counts)])
    return [{int(positions[r, f]): (bytes(data[r, f]), int(linfo[r, f])) for f in range(int(counts[r]))} for r in range(x.shape[0])]


def recovered(want, sent, fq):
    """frames whose word starts at symbol CHAIN_A or later: (how many, found, decoded to the sent data)"""
    late = [(r, at, data) for r, s in enumerate(sent) for at, data in s if at >= CHAIN_A]
    got = [want[r].get(at + fq.W) for r, at, _ in late]
    return len(late), sum(g is not None for g in got), sum(g is not None and g[0] == bytes(np.packbits(d)) for g, (_, _, d) in zip(got, late))


def test_the_chain_to_checked_data(hz, ctx, code96):
    """carrier_rows -> symbol_rows -> ldpc_frames on the device equal the chained host programs exactly, frame for
    frame; of the frames whose word starts at symbol CHAIN_A or later the host chain finds most at this noise and
    returns the sent data for every one it finds (the module's header has the soft and hard counts over the seeds
    1 ... 12)"""
    st = importlib.import_module("go-sdr_amd.stream")
    fq, lq = chain_configs(hz, code96)
    x, sent = chain_inputs(hz, fq, code96)
    want = host_chain(hz, fq, lq, x)
    late, found, good = recovered(want, sent, fq)
    assert late >= 24 and 2 * found > late and good == found
    cp, sp = chain_params(hz)
    fargs, fkw = fq.create_args()
    with ctx.carrier_loop(hz.CARRIER_BPSK, cp, rows=3) as cr, ctx.symbol_sync(hz.FMT_C64, sp, rows=3) as ts, \
            ctx.frame_sync(fq.kind, *fargs, rows=3, **fkw) as fs, ctx.soft_frames(fs) as sf, bank_of(hz, ctx, lq, 3) as ld:
        xd = dev(x)
        blocks = [xd[:, a:b] for a, b in ((0, 3000), (3000, 3001), (3001, x.shape[1]))]
        parts = list(st.ldpc_frames(st.symbol_rows(st.carrier_rows(blocks, cr), ts), fs, sf, ld, cap=16))
        with pytest.raises(st.ErrShortBuffer):
            fs.reset(), sf.reset()
            list(st.ldpc_frames(st.symbol_rows(st.carrier_rows([xd], cr), ts), fs, sf, ld, cap=2))
    for r in range(3):
        got = {int(p): (bytes(d), int(u) | (int(it) << 16) | (int(ok) << 31)) for part in parts
               for d, p, u, it, ok in zip(part[r][0], part[r][1], part[r][3], part[r][4], part[r][5])}
        assert got == want[r], r
    qb = ref.Config.of(code96, kind=ref.BITS, D=code96.k, level=16)
    with bank_of(hz, ctx, qb, 3) as hard, bank_of(hz, ctx, ref.Config.of(code96, N=90), 3) as short, bank_of(hz, ctx, lq, 2) as two, \
            ctx.frame_sync(fq.kind, *fargs, rows=3, **fkw) as fs, ctx.soft_frames(fs) as sf:
        for bad in (hard, short, two):
            with pytest.raises(ValueError):
                list(st.ldpc_frames([], fs, sf, bad))


# ---- 8. the other layers -----------------------------------------------------------------------------------------

def _run(exe):
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "go-sdr_amd") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    return subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)


def test_c_ldpc_walkthrough(hz):
    """tests/c/test_ldpc_abi.c compiled by gcc as C99 and run against libhzsdr_hip.so."""
    exe = os.path.join(BUILD, "test_ldpc_abi")
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "test_ldpc_abi.c"), "-L" + os.path.join(ROOT, "go-sdr_amd"),
                           "-lhzsdr_hip", "-lm", "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    p = _run(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "ldpc-abi ok" in p.stdout


def test_cxx_ldpc(hz):
    """tests/cxx/test_ldpc.cpp (hzsdr::stream::Ldpc of go-sdr_amd/cxx/hzsdr.hpp) built with g++ and run."""
    exe = os.path.join(BUILD, "test_ldpc_cxx")
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + ROOT, os.path.join(ROOT, "tests", "cxx", "test_ldpc.cpp"),
                           "-L" + os.path.join(ROOT, "go-sdr_amd"), "-lhzsdr_hip", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    p = _run(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "ldpc-cxx ok" in p.stdout

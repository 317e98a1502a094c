"""The Viterbi decoder bank (include/hzsdr_viterbi.h) on the GPU against the host program tests/host/viterbi_ref.cpp, which
tests/test_viterbi_cpu.py holds to the numpy restatements: decoded bytes and info are compared EXACTLY, the destinations
are full of sentinels, the pitches are above the need, and every slot that is not decoded is checked byte for byte.
Wherever it is provable -- clean frames, or at most 4 flipped hard bits under the K = 7 code, whose free distance is 10
-- the tests also assert that the reference decoded what was planted, so that two wrong answers cannot agree.

The chain test (carrier -> symbol timing -> frame sync -> Viterbi on QPSK rows) is the frame sync chain test's signal: a
32-bit word and 168 payload bits, one frame every 110 symbols from symbol 10 on, 5 samples per symbol, white noise 20 dB
below the symbol power, the same three carrier offsets.  The payload is now the K = 7 rate 1/2 TAIL code (CCSDS: the second
output inverted) of D = 78 bits: 62 data bits and their CRC-16/CCITT-FALSE.  Measured on the CPU from the four chained
host programs over the seeds 1 ... 12 with the three offsets and phases (36 rows, 13 frames each, 468 frames): every
frame is found, the first one included (its word starts at symbol 10), decodes to the sent data with the CRC ok, and
NO frame has a single channel bit error to correct (every metric is 0).  No frame failed, so the frame sync test's
CHAIN_A = 20 stands: asserted is every frame whose word starts at symbol 20 or later."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import carrier_ref
import framesync_ref
import symsync_ref
import viterbi_ref as ref
from conftest import ROOT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BUILD = os.path.join(ROOT, "build")
SENT8, SENT32 = 0xA5, 0xA5A5A5A5
CCITT = (16, 0x1021, 0xFFFF, 0)
CRCS = (None, CCITT, (8, 0x07, 0, 0x55), (24, 0x864CFB, 0xB704CE, 0), (32, 0x04C11DB7, 0xFFFFFFFF, 0))
GENS = {3: (5, 7, 7, 5), 5: (0o23, 0o35, 0o27, 0o33), 7: (0o171, 0o133, 0o165, 0o117), 9: (0o557, 0o663, 0o711, 0o745)}
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


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def cfg(**kw):
    return ref.Config(**kw)


def bank_of(c, q, rows):
    args, kw = q.create_args()
    return c.viterbi(*args, rows=rows, **kw)


def strided(wide, shape, pitch, device):
    R, cap, w = shape
    if device:
        return torch.as_strided(wide, shape, (pitch, w, 1))
    return np.lib.stride_tricks.as_strided(wide, shape, (pitch * wide.itemsize, w * wide.itemsize, wide.itemsize))


def decode_checked(c, q, frames, counts, device, want, pads=(3, 5)):
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
    with bank_of(c, q, R) as v:
        assert v.sizes() == (q.N, q.FB, q.T, q.DB)
        v.decode(strided(wide_in, (R, cap, width), ipitch, device), cin, cap, out=(strided(wide_out, (R, cap, q.DB), opitch, device), info))
        if device:
            torch.cuda.synchronize()
        plan = v.plan()
    wd, wi = want
    gw, gi = host(wide_out), host(info).view(np.uint32)
    for r in range(R):
        m = cap if counts is None else min(int(counts[r]), cap)
        assert np.array_equal(gw[r, :m * q.DB].reshape(m, q.DB), wd[r, :m]), (vars(q), r)
        assert (gw[r, m * q.DB:] == SENT8).all(), (vars(q), r)
        assert np.array_equal(gi[r, :m], wi[r, :m]) and (gi[r, m:] == SENT32).all(), (vars(q), r)
    return plan


def hurt_block(q, R, cap, seed, flips):
    """(frames, data bits): clean coded frames with `flips` positions hurt each: hard bits inverted, soft values made a
    weak value of the wrong sign"""
    frames, data = ref.clean_block(q, R, cap, seed)
    for r in range(R):
        for f in range(cap):
            where = np.argsort(ref.splitmix64(seed * 977 + r * cap + f, q.N), kind="stable")[:flips]  # `flips` distinct positions
            if q.kind == ref.BITS:
                bits = np.unpackbits(frames[r, f])
                bits[where] ^= 1
                frames[r, f] = np.packbits(bits)
            else:
                frames[r, f, where] *= np.float32(-0.4)
    return frames, data


def planted(q, data, got, info, r, f, flips):
    """the reference decoded what was planted: the data, the CRC verdict, and (hard bits) the flips as the metric"""
    assert np.array_equal(got[r, f], np.packbits(data[r, f])), (vars(q), r, f)
    assert int(info[r, f]) >> 31 == (1 if q.C else 0), (vars(q), r, f)
    if q.kind == ref.BITS:
        assert int(info[r, f]) & 0x7FFFFFFF == flips, (vars(q), r, f)


# ---- 1. every lane shape, every size ---------------------------------------------------------------------

@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("K", [3, 5, 7, 9])
def test_codes_and_sizes(ctx, K, n):
    """K in {3, 5, 7, 9} (16 and 4 frames per wave, one state per lane, 4 states per lane) x n in {2, 3, 4}, D around
    K - 1 (states still at INF at the end), around a tile of 64 steps, 78 and 1000, both terminations, both inputs, every
    CRC width with D - C no multiple of 8; R = 3 and cap = 3 with counts that leave slots out and no full last wave"""
    cases = []
    for i, D in enumerate([1, 2, K - 2, K - 1, K, 63, 64, 65, 78, 1000]):
        for term in (ref.TAIL, ref.TRUNCATED):
            crc = CRCS[(i + term) % len(CRCS)]
            q = cfg(K=K, gens=GENS[K][:n], D=D, term=term, inv=(5 * K + n) % (1 << n), kind=(ref.BITS, ref.SOFT_F32)[(i + term) % 2], scale=0.7,
                    crc=crc if crc and crc[0] < D else None)
            frames, _ = hurt_block(q, 3, 3, 31 * K + 7 * n + i, flips=max(1, q.N // 8))
            cases.append((q, frames, np.array([3, 1, 7], np.uint32)))
    shapes = set()
    for (q, frames, counts), want in zip(cases, ref.exact(BUILD, cases)):
        g, spl, dbytes, form = decode_checked(ctx, q, frames, counts, True, want)
        assert (g, spl) == (max(1, 64 >> (K - 1)), max(1, (1 << (K - 1)) // 64)) and dbytes == q.T * q.S // 8 and form == ref.FORM_LDS
        shapes.add((g, spl))
    assert len(shapes) == 1


@pytest.mark.parametrize("K,one_bit_per_step", [(3, False), (5, False), (7, False), (9, False), (3, True), (7, True), (9, True)])
def test_the_largest_frames_and_both_decision_forms(ctx, K, one_bit_per_step):
    """the largest D of each K with N = 2 T = 8192, and T = 8192 itself under a pattern that sends one bit per step:
    decisions in LDS where they fit, in the bank's scratch otherwise (the traceback's chunks, T no multiple of one);
    the frames are clean but for 4 flips, so at K = 7 the planted data must come back"""
    pattern = (0b10, 2) if one_bit_per_step else None
    D = (8192 if one_bit_per_step else 4096) - (K - 1)
    q = cfg(K=K, gens=GENS[K][:2], D=D, pattern=pattern, crc=CCITT)
    assert q.N == 8192 and q.T == (8192 if one_bit_per_step else 4096)
    frames, data = hurt_block(q, 2, 2, K, flips=4)
    counts = np.array([2, 1], np.uint32)
    ((wd, wi),) = ref.exact(BUILD, [(q, frames, counts)])
    plan = decode_checked(ctx, q, frames, counts, True, (wd, wi))
    lds = plan[0] * 256 + plan[0] * ((D + 63) // 64) * 8 + 1024 + q.T * plan[1] * 8  # the tile, the decoded words, the CRC table, the decisions
    assert plan[3] == (ref.FORM_LDS if lds <= 66 * 1024 else ref.FORM_SCRATCH)
    assert plan[3] == (ref.FORM_SCRATCH if one_bit_per_step or K == 9 else ref.FORM_LDS)
    if K == 7 and not one_bit_per_step:
        for r, f in ((0, 0), (0, 1), (1, 0)):
            planted(q, data, wd, wi, r, f, 4)


@pytest.mark.parametrize("kind", [ref.BITS, ref.SOFT_F32])
def test_puncture_patterns(ctx, kind):
    """no puncturing, 2/3, 3/4, 7/8 and a 64-bit pattern, D = 78 and 65, both terminations; clean TAIL frames come back"""
    cases, sent = [], []
    for i, pattern in enumerate([None, ref.PATTERNS["2/3"], ref.PATTERNS["3/4"], ref.PATTERNS["7/8"], ref.PATTERN64]):
        for term, D, flips in ((ref.TAIL, 78, 0), (ref.TRUNCATED, 65, 3), (ref.TAIL, 65, 5)):
            q = cfg(D=D, term=term, pattern=pattern, kind=kind, scale=1.5, inv=0b10, crc=CCITT)
            frames, data = hurt_block(q, 2, 4, 50 + i, flips)
            cases.append((q, frames, None))
            sent.append((data, flips))
    for (q, frames, _), (data, flips), want in zip(cases, sent, ref.exact(BUILD, cases)):
        decode_checked(ctx, q, frames, None, True, want)
        if flips == 0:
            for r in range(2):
                for f in range(4):
                    planted(q, data, want[0], want[1], r, f, 0)


# ---- 2. rows, caps, counts, memory spaces ----------------------------------------------------------------

@pytest.mark.parametrize("space", ["device", "host"])
@pytest.mark.parametrize("R", [1, 2, 63, 64, 65, 1025])
def test_rows_caps_and_counts(ctx, hctx, space, R):
    """R x cap in {1, 3, 4}, counts ragged, zero and above cap (and none at all), K = 7 and K = 5 (4 frames per wave: a
    wave's frames in several rows), D = 29 (DB = 4: neighbours inside one 64-bit word); <= 4 flips: the data comes back"""
    device = space == "device"
    c = ctx if device else hctx
    for cap in (1, 3, 4):
        K = 7 if (R + cap) % 2 else 5
        q = cfg(K=K, gens=GENS[K][:2], D=29, inv=0b10, crc=(8, 0x07, 0, 0))
        frames, data = hurt_block(q, R, cap, R + cap, flips=(R + cap) % 5)
        counts = (ref.splitmix64(R * 8 + cap, R) % np.uint64(cap + 3)).astype(np.uint32)
        counts[0] = cap + 2
        if R > 2:
            counts[1], counts[2] = 0, cap
        for cnt in (counts, None) if R < 100 else (counts,):
            ((wd, wi),) = ref.exact(BUILD, [(q, frames, cnt)])
            decode_checked(c, q, frames, cnt, device, (wd, wi))
        if K == 7:
            for r in range(min(R, 5)):
                for f in range(min(int(counts[r]), cap)):
                    planted(q, data, wd, wi, r, f, (R + cap) % 5)


# ---- 3. ties, erasures, special values -------------------------------------------------------------------

def test_ties_on_purpose(ctx):
    """all-erasure frames (zeros, -0, NaNs) decode to the tie rule's answer: all zeros with metric 0.  Planted ties: the
    K = 7 code's impulse response has weight 10, so 5 flips on it leave the sent word and its neighbour at the same
    metric 5 -- the exhaustive decoder confirms at least two minimisers, and the device takes the program's"""
    for term in (ref.TAIL, ref.TRUNCATED):
        q = cfg(D=100, term=term, kind=ref.SOFT_F32, crc=CCITT)
        frames = np.zeros((1, 4, q.N), np.float32)
        frames[0, 1], frames[0, 2] = np.nan, -0.0
        frames[0, 3, ::2] = np.nan
        ((wd, wi),) = ref.exact(BUILD, [(q, frames, None)])
        assert not wd.any() and not (wi & 0x7FFFFFFF).any()
        decode_checked(ctx, q, frames, None, True, (wd, wi))
    q = cfg(D=12)
    tied = 0
    frames = np.zeros((1, 8, q.FB), np.uint8)
    for f in range(8):
        data = ref.random_bits(12, 70 + f)
        other = data.copy()
        other[3 + f % 5] ^= 1
        differ = np.flatnonzero(ref.encode(q, data) != ref.encode(q, other))
        assert len(differ) == 10
        frames[0, f] = ref.frame_of(q, ref.encode(q, data), flips=differ[f % 2::2])
        best, words = ref.exhaustive(q, frames[0, f])
        assert best == 5 and len(words) >= 2
        tied += 1
    ((wd, wi),) = ref.exact(BUILD, [(q, frames, None)])
    assert tied == 8 and (wi == 5).all()
    decode_checked(ctx, q, frames, None, True, (wd, wi))


@pytest.mark.parametrize("space", ["device", "host"])
def test_special_values_inside_a_clean_frame(ctx, hctx, space):
    """-0, both infinities and NaNs of both signs inside otherwise clean soft frames: the data comes back, an infinity on
    the wrong side costs 127, and the device agrees with the program"""
    q = cfg(D=40, kind=ref.SOFT_F32, scale=1.0, crc=CCITT, inv=0b10)
    frames, data = ref.clean_block(q, 2, 3, 9)
    x = frames[0, 1]
    x[3], x[17], x[18] = np.nan, -0.0, np.frombuffer(np.uint32(0xFFC00001).tobytes(), np.float32)[0]
    x[40] = np.inf if x[40] > 0 else -np.inf
    x[60] = -np.inf if x[60] > 0 else np.inf
    frames[1, 2, 5] = np.float32(3e38) if frames[1, 2, 5] > 0 else np.float32(-3e38)
    frames[1, 2, 7] = np.float32(1e-40)
    ((wd, wi),) = ref.exact(BUILD, [(q, frames, None)])
    for r in range(2):
        for f in range(3):
            planted(q, data, wd, wi, r, f, 0)
    assert int(wi[0, 1]) & 0x7FFFFFFF == 127 and int(wi[0, 0]) & 0x7FFFFFFF == 0
    decode_checked(ctx if space == "device" else hctx, q, frames, None, space == "device", (wd, wi))


# ---- 4. invariance -----------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [5, 7, 9])
def test_a_frame_does_not_depend_on_its_place_or_its_neighbours(ctx, hctx, K):
    """the same frames in other slots, under other R, cap, pitches and memory spaces, beside NaN, infinite and
    all-erasure frames: the same bytes and info"""
    q = cfg(K=K, gens=GENS[K][:3], D=50, kind=ref.SOFT_F32, scale=0.5, crc=CCITT)
    frames, _ = hurt_block(q, 1, 6, 21 + K, flips=9)
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
        with bank_of(c, q, R) as v:
            data, info = v.decode(dev(block) if device else block)
            data, info = host(data), host(info).view(np.uint32)
        for k, (r, f) in enumerate(slots):
            assert np.array_equal(data[r, f], wd[0, k]) and info[r, f] == wi[0, k], (R, cap, k)
        seen.append(len(slots))
    assert min(seen) >= 4


# ---- 5. refusals -------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", [1, 3])
def test_refused_calls_leave_the_outputs(hz, ctx, R):
    lib = importlib.import_module("go-sdr_amd._capi").lib
    q = cfg(D=30)
    cap = 2
    frames, _ = ref.clean_block(q, R, cap, 4)
    x = dev(frames)
    out, info = torch.full((R, cap * q.DB), SENT8, dtype=torch.uint8, device="cuda"), torch.full((R, cap), 7, dtype=torch.int32, device="cuda")
    with bank_of(ctx, q, R) as v:
        call = lambda *a: ctx._ck(lib.hzsdr_viterbi_decode(v._h, *a))
        i, o, p = x.data_ptr(), out.data_ptr(), info.data_ptr()
        if R > 1:
            with pytest.raises(hz.ErrDstTooSmall):
                call(i, cap * q.FB, None, cap, o, cap * q.DB - 1, p)
            with pytest.raises(hz.ErrInvalidArgument):
                call(i, cap * q.FB - 1, None, cap, o, cap * q.DB, p)
        for bad in ((None, cap * q.FB, None, cap, o, cap * q.DB, p), (i, cap * q.FB, None, cap, None, cap * q.DB, p), (i, cap * q.FB, None, cap, o, cap * q.DB, None),
                    (i, cap * q.FB, None, 0, o, cap * q.DB, p), (i, cap * q.FB, None, hz.VITERBI_MAX_FRAMES // R + 1, o, cap * q.DB, p)):
            with pytest.raises(hz.ErrInvalidArgument):
                call(*bad)
        assert lib.hzsdr_viterbi_decode(None, i, cap * q.FB, None, cap, o, cap * q.DB, p) == hz.ErrInvalidArgument.status
        torch.cuda.synchronize()
        assert (out == SENT8).all() and (info == 7).all()
        with pytest.raises(ValueError):
            v.decode(dev(np.zeros((R, cap, q.FB + 1), np.uint8)))
        with pytest.raises(ValueError):
            v.decode(dev(np.zeros((R, cap, q.FB), np.float32)))
        call(i, cap * q.FB, None, cap, o, cap * q.DB, p)
        torch.cuda.synchronize()
        ((wd, wi),) = ref.exact(BUILD, [(q, frames, None)])
        assert np.array_equal(host(out).reshape(R, cap, q.DB), wd) and np.array_equal(host(info).view(np.uint32), wi) and not wi.any()


def test_create_errors(hz, ctx):
    """rows 0 and 8193, other kinds, and one bound of each sort through the library (every bound's edge:
    tests/test_viterbi_cpu.py against the same hz_viterbi_plan.h)"""
    lib = importlib.import_module("go-sdr_amd._capi").lib
    out = C.c_void_p()

    def create(q, rows=1, kind=None):
        g = (C.c_uint * max(1, q.n))(*q.gens)
        return lib.hzsdr_viterbi_create(ctx._h, q.kind if kind is None else kind, q.K, q.n, g, q.inv, q.pattern, q.Lp, q.term, q.D, q.scale, *q.crc,
                                        rows, C.byref(out))

    inval = hz.ErrInvalidArgument.status
    assert create(cfg(), 0) == inval and create(cfg(), hz.VITERBI_MAX_ROWS + 1) == inval
    assert create(cfg(), hz.VITERBI_MAX_ROWS) == 0 and lib.hzsdr_viterbi_free(out) == 0
    for kind in (-1, 0, 2, 31, 33):
        assert create(cfg(), 1, kind) == hz.ErrSampleFormatUnknown.status, kind
    assert lib.hzsdr_viterbi_create(ctx._h, 1, 7, 2, None, 0, 3, 2, 0, 78, 1.0, 0, 0, 0, 0, 1, C.byref(out)) == inval
    for bad in (cfg(K=2, gens=(1, 3)), cfg(K=10, gens=(1, 3)), cfg(gens=(0o171,)), cfg(gens=(0o171, 0o133, 0o165, 0o117, 0o155)), cfg(gens=(0, 0o133)),
                cfg(gens=(0o200, 0o133)), cfg(inv=4), cfg(pattern=(0b1100, 4)), cfg(pattern=(0b111, 3)), cfg(pattern=(0b10000, 4)), cfg(term=2), cfg(D=0),
                cfg(D=4091), cfg(D=8187, pattern=(0b10, 2)), cfg(kind=ref.SOFT_F32, scale=0.0), cfg(kind=ref.SOFT_F32, scale=np.inf), cfg(crc=(12, 1, 0, 0)),
                cfg(D=16, crc=CCITT), cfg(crc=(8, 0x100, 0, 0)), cfg(crc=(0, 1, 0, 0))):
        assert not ref.accepted(bad) and create(bad) == inval, vars(bad)
    for good in (cfg(K=3, gens=(5, 7), D=1), cfg(K=9, gens=GENS[9], D=2040, inv=15), cfg(D=8186, pattern=(0b10, 2)), cfg(pattern=ref.PATTERN64),
                 cfg(kind=ref.SOFT_F32, scale=1e-30), cfg(D=33, crc=(32, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF))):
        assert ref.accepted(good) and create(good) == 0 and lib.hzsdr_viterbi_free(out) == 0, vars(good)
    with pytest.raises(hz.ErrInvalidArgument):
        ctx.viterbi(hz.VITERBI_BITS, 7, (0o171, 0o133), 78, rows=0)


# ---- 6. the chain ------------------------------------------------------------------------------------

CHAIN_SPS, CHAIN_NOISE_DB = 5.0, -20.0
CHAIN_CASES = ((1, 0.0005, 0.3), (2, -0.001, 1.9), (3, 0.0015, 4.0))  # seed, carrier offset in cycles per sample, phase


def chain_configs(hz):
    words, maps = hz.sync_hypotheses(WORD32, 32, 2, "rotate")
    fq = framesync_ref.Config(32, words, 168, B=2, cplx=True, thr=2, maps=maps)
    K, gens, inv = hz.CCSDS_K7
    vq = cfg(K=K, gens=gens, inv=inv, D=78, crc=CCITT)
    assert vq.N == fq.P
    return fq, vq


def coded_frames_signal(fq, vq, nsym, seed, every=110):
    """QPSK symbols (b0 on Re, b1 on Im: bit 1 is +) that carry a frame -- the 32-bit word, then the 168 code bits of 62
    random data bits and their CRC-16 -- every `every` symbols from symbol 10 on, random dibits between -> (a complex
    (nsym,), [(first symbol of the word, the 78 data bits)])"""
    bits = framesync_ref.random_bits(2 * nsym, seed)
    sent = []
    for k, at in enumerate(range(10, nsym - (fq.W + fq.P) // 2 - 1, every)):
        data = ref.with_crc(vq, framesync_ref.random_bits(62, 1000 * seed + k))
        framesync_ref.plant(bits, 2 * at, fq.words[0], fq.W, ref.encode(vq, data))
        sent.append((at, data))
    v = bits.astype(np.float64) * 2.0 - 1.0
    return (v[0::2] + 1j * v[1::2]) / np.sqrt(2.0), sent


def chain_inputs(fq, vq, cases=CHAIN_CASES):
    rows, sent = [], []
    for seed, off, phase in cases:
        a, s = coded_frames_signal(fq, vq, 1500, seed)
        x = symsync_ref.signal(a, CHAIN_SPS, 0.25 * (seed % 4), noise_db=CHAIN_NOISE_DB, seed=seed).astype(np.complex128)
        rows.append((x * np.exp(2j * np.pi * (off * np.arange(len(x)) + phase))).astype(np.complex64))
        sent.append(s)
    n = min(len(r) for r in rows)
    return np.stack([r[:n] for r in rows]), sent


def chain_params(hz):
    return (np.array([*carrier_ref.gains(0.01), 0.0, -0.01, 0.01], np.float32), np.array([CHAIN_SPS, 0.01, *hz.loop_gains(CHAIN_SPS)], np.float32))


def host_chain(hz, fq, vq, x, cap=16):
    """the four chained host programs over the rows x in one push -> per row {payload's first symbol: (data bytes, info)}"""
    cp, sp = chain_params(hz)
    ((derot, _, _),) = carrier_ref.exact(BUILD, [(carrier_ref.QPSK, cp, x)])
    ((sym, cnt, _, _),) = symsync_ref.exact(BUILD, [(sp, derot)])
    ((per, _),) = framesync_ref.exact(BUILD, [(fq, [(sym, cnt)], cap)])
    frames, positions, _, counts = per[0]
    assert int(counts.max()) <= cap
    ((data, info),) = ref.exact(BUILD, [(vq, frames, counts)])
    return [{int(positions[r, f]): (bytes(data[r, f]), int(info[r, f])) for f in range(int(counts[r]))} for r in range(x.shape[0])]


def test_the_chain_to_checked_data(hz, ctx):
    """carrier_rows -> symbol_rows -> decoded_frames on the device equal the four chained host programs exactly; and the
    host chain returns the sent data with the CRC ok for every frame whose word starts at symbol CHAIN_A or later (the
    module's header has the measurement over the seeds 1 ... 12)"""
    st = importlib.import_module("go-sdr_amd.stream")
    fq, vq = chain_configs(hz)
    x, sent = chain_inputs(fq, vq)
    want = host_chain(hz, fq, vq, x)
    for r in range(3):
        late = [(at, data) for at, data in sent[r] if at >= CHAIN_A]
        assert len(late) >= 8
        for at, data in late:
            got = want[r].get(at + fq.W // 2)
            assert got is not None and got[0] == bytes(np.packbits(data)) and got[1] >> 31 == 1, (r, at)
    cp, sp = chain_params(hz)
    fargs, fkw = fq.create_args()
    with ctx.carrier_loop(hz.CARRIER_QPSK, cp, rows=3) as cr, ctx.symbol_sync(hz.FMT_C64, sp, rows=3) as ts, \
            ctx.frame_sync(fq.kind, *fargs, rows=3, **fkw) as fs, bank_of(ctx, vq, 3) as vd:
        xd = dev(x)
        blocks = [xd[:, a:b] for a, b in ((0, 3000), (3000, 3001), (3001, x.shape[1]))]
        parts = list(st.decoded_frames(st.symbol_rows(st.carrier_rows(blocks, cr), ts), fs, vd, cap=16))
    for r in range(3):
        got = {int(p): (bytes(d), int(m) | (int(ok) << 31)) for part in parts for d, p, m, ok in zip(part[r][0], part[r][1], part[r][3], part[r][4])}
        assert got == want[r], r
    with bank_of(ctx, cfg(D=30), 3) as other, ctx.frame_sync(fq.kind, *fargs, rows=3, **fkw) as fs, pytest.raises(ValueError):
        list(st.decoded_frames([], fs, other))


# ---- 7. the other layers -----------------------------------------------------------------------------

def _run(exe):
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "go-sdr_amd") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    return subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)


def test_c_viterbi_walkthrough(hz):
    """tests/c/test_viterbi_abi.c compiled by gcc as C99 and run against libhzsdr_hip.so."""
    exe = os.path.join(BUILD, "test_viterbi_abi")
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "test_viterbi_abi.c"), "-L" + os.path.join(ROOT, "go-sdr_amd"),
                           "-lhzsdr_hip", "-lm", "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    p = _run(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "viterbi-abi ok" in p.stdout


def test_cxx_viterbi(hz):
    """tests/cxx/test_viterbi.cpp (hzsdr::stream::Viterbi behind hzsdr::stream::FrameSync) built with g++ and run."""
    exe = os.path.join(BUILD, "test_viterbi_cxx")
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + ROOT, os.path.join(ROOT, "tests", "cxx", "test_viterbi.cpp"),
                           "-L" + os.path.join(ROOT, "go-sdr_amd"), "-lhzsdr_hip", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    p = _run(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "viterbi-cxx ok" in p.stdout

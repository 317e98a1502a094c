"""The HDLC deframer bank (include/hzsdr_hdlc.h) on the GPU against the host program tests/host/hdlc_ref.cpp, which
tests/test_hdlc_cpu.py holds to the numpy restatement and to the textbook decoder: frames, positions, info, counts and
state are compared EXACTLY, in DEVICE and HOST contexts, the destinations are full of sentinels (slot tails, the slots
behind a row's count and the pad behind a row's slots must keep them) and every pitch is above the need.  Every test
asserts on the host side that the program finds the frames that were sent, so that two empty lists cannot pass.

The tile (64 bits) and the ring come from hzsdr_hdlc_plan; the chunk is 16 tiles (the header says so).

The chain test: NRZI bits from hdlc_encode at 4 samples per symbol with white noise 20 dB below the symbol power through
the symbol-timing bank, whose (symbols, counts) go into the bank as they are.  Measured on the CPU from the chained
host programs at timing offsets 0, 0.3 and 0.7: all seven frames come back, the first included, which stands behind 24
flag bits only; asserted is every frame from the second on, since acquisition is the timing loop's business."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import hdlc_ref as ref
import symsync_ref
from conftest import ROOT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BUILD = os.path.join(ROOT, "build")
SENT8, SENT32, SENT64 = 0xA5, 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
FLAG = [0, 1, 1, 1, 1, 1, 1, 0]
TILE, CHUNK = 64, 64 * ref.CHUNK_TILES


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


@pytest.fixture(params=["device", "host"])
def space(request, ctx, hctx):
    return (ctx, True) if request.param == "device" else (hctx, False)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def bank_of(c, q, rows):
    return c.hdlc(q.kind, rows=rows, **q.create_kw())


def pitched(x, pad, device):
    """x (R, n) inside a wider buffer of pitch n + pad (R > 1) -> the view of the rows"""
    if x.ndim == 1:
        return dev(x) if device else x.copy()
    wide = np.zeros((x.shape[0], x.shape[1] + pad), x.dtype)
    wide[:, :x.shape[1]] = x
    wide = dev(wide) if device else wide
    return wide[:, :x.shape[1]]


def destinations(R, cap, FB, pad, device):
    """(frames view (R, cap, FB) of a buffer of pitch cap * FB + pad, positions, info, counts, the wide buffer), all sentinels"""
    pitch = cap * FB + pad
    wide = np.full((R, pitch), SENT8, np.uint8)
    pos, info, cnt = np.full((R, cap), SENT64, np.uint64), np.full((R, cap), SENT32, np.uint32), np.full((R,), SENT32, np.uint32)
    if device:
        wide, pos, info, cnt = dev(wide), dev(pos.view(np.int64)), dev(info.view(np.int32)), dev(cnt.view(np.int32))
        frames = torch.as_strided(wide, (R, cap, FB), (pitch, FB, 1))
    else:
        frames = np.lib.stride_tricks.as_strided(wide, (R, cap, FB), (pitch, FB, 1))
    return frames, pos, info, cnt, wide


def push_checked(f, q, x, counts, cap, device, want, pads=(3, 5)):
    """one push of the rows x (numpy (R, n) or (n,)) against the program's (frames, positions, info, counts) of that
    push: the stored frames' bytes exactly, everything else still a sentinel"""
    R = f.rows
    frames, pos, info, cnt, wide = destinations(R, cap, q.FB, pads[1], device)
    xin = pitched(x, pads[0], device)
    cin = None if counts is None else (dev(np.asarray(counts, np.uint32).view(np.int32)) if device else np.asarray(counts, np.uint32))
    f.push(xin, cin, cap, out=(frames, pos, info, cnt))
    if device:
        torch.cuda.synchronize()
    wf, wp, wi, wc = want
    gw, gp, gi, gc = host(wide), host(pos).view(np.uint64), host(info).view(np.uint32), host(cnt).view(np.uint32)
    assert np.array_equal(gc, wc), (gc, wc)
    for r in range(R):
        m = min(int(wc[r]), cap)
        assert np.array_equal(gp[r, :m], wp[r, :m]) and (gp[r, m:] == SENT64).all(), r
        assert np.array_equal(gi[r, :m], wi[r, :m]) and (gi[r, m:] == SENT32).all(), r
        for s in range(m):
            nb = int(wi[r, s]) & 0x7FFFFFFF
            slot = gw[r, s * q.FB:(s + 1) * q.FB]
            assert np.array_equal(slot[:nb], wf[r, s, :nb]), (r, s)
            assert (slot[nb:] == SENT8).all(), (r, s)
        assert (gw[r, m * q.FB:] == SENT8).all(), r


def same_state(got, want):
    return all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(got, want))


def compare(c, q, pushes, cap, device, state=None):
    """the pushes through a new bank against the program, push by push, and the state behind them -> the program's
    ([per push (frames, positions, info, counts)], state)"""
    first = pushes[0][0] if isinstance(pushes[0], tuple) else pushes[0]
    R = 1 if np.asarray(first).ndim == 1 else np.asarray(first).shape[0]
    case = (q, pushes, cap) if state is None else (q, pushes, cap, state)
    ((per, wstate),) = ref.exact(BUILD, [case])
    with bank_of(c, q, R) as f:
        if state is not None:
            f.set_state(*state)
        for k, p in enumerate(pushes):
            x, cnt = p if isinstance(p, tuple) else (p, None)
            push_checked(f, q, np.asarray(x), cnt, cap, device, per[k], pads=(3 + k % 4, 5 + 2 * (k % 3)))
        assert same_state(f.state(), wstate)
        assert np.array_equal(f.positions(), wstate[0])
    return per, wstate


def cut(x, edges):
    return [x[..., a:b] for a, b in zip(edges, edges[1:])]


def payloads_of(per, row=0):
    return [g[0] for g in ref.stored(per, row)]


def frame_of(q, payload):
    """the bytes the bank emits for a payload: its bits and FCS packed in the bank's bit order"""
    return np.packbits(ref.frame_bits(payload, q.fcs, bool(q.msb_first)), bitorder="big" if q.msb_first else "little").tobytes()


def encode(hz, q, payloads, **kw):
    return hz.hdlc_encode(payloads, fcs=q.fcs, msb_first=bool(q.msb_first), **kw)


def ending_at(bits, target):
    """zeros in front of `bits` so that its last bit is bit `target` of the stream"""
    lead = target + 1 - len(bits)
    assert lead >= 0
    return np.concatenate([np.zeros(lead, np.uint8), bits])


def traffic(hz, q, seed, count, lo=1, hi=None, gap=5):
    """`count` frames of random payloads with flags, shared zeros, mark idle and aborted frames between -> (bits, payloads)"""
    hi = q.max_bytes - q.fcs // 8 if hi is None else hi
    lo = max(lo, q.min_bytes - q.fcs // 8)
    parts, payloads = [np.zeros(seed % 7, np.uint8)], []
    for k in range(count):
        p = ref.random_bytes(lo + (seed * 7 + k * 5) % (hi - lo + 1), seed * 100 + k)
        payloads.append(p)
        parts.append(encode(hz, q, [p], flags=1 + k % 2, shared_zero=bool(k % 3 == 1)))
        if k % 4 == 2:
            parts.append(np.array(FLAG + ref.stuffed(ref.random_bits(29, seed + k)).tolist() + [0] + [1] * 8, np.uint8))
        parts.append(np.ones(gap, np.uint8) if k % 2 else np.zeros(gap, np.uint8))
    return np.concatenate(parts), payloads


# ---- 1. a closing flag around a tile edge, a chunk edge and a push edge ---------------------------------

@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("edge", ["tile", "chunk", "push"])
def test_closing_flag_at_every_offset_around_an_edge(hz, space, edge, shared):
    """the closing flag's last bit at each of the 8 positions edge - 4 ... edge + 3, separate flags and flags that share
    their 0 with a second frame's opening flag"""
    c, device = space
    q = ref.Config(fcs=16, max_bytes=24)
    where = {"tile": 3 * TILE, "chunk": CHUNK, "push": 333}[edge]
    first, second = b"edge\xff\xfe", b"\x00next"
    head = hz.hdlc_encode([first], fcs=16, shared_zero=shared)
    tail = hz.hdlc_encode([second], fcs=16, shared_zero=shared)
    for off in range(8):
        b = np.concatenate([ending_at(head, where - 4 + off), tail[1:] if shared else tail, np.zeros(70, np.uint8)])
        x = ref.soft(b, off)
        pushes = cut(x, [0, 333, len(x)]) if edge == "push" else [x]
        per, _ = compare(c, q, pushes, 3, device)
        got = ref.stored(per, 0)
        assert [g[0] for g in got] == [frame_of(q, first), frame_of(q, second)] and got[1][1] == where - 4 + off + (8 if shared else 9)
        if edge == "push":  # the frame comes with the push that delivers the flag's last bit
            assert int(per[0][3][0]) == (1 if where - 4 + off < 333 else 0)


# ---- 2. stuffed bits across the words of a span; lanes that delete 0, 1 and the most ----------------------

def test_stuffed_bit_whose_ones_straddle_a_span_word(hz, space):
    c, device = space
    q = ref.Config(fcs=16, max_bytes=40)
    straddles = set()
    for lead in range(10):  # (0x3e in front: one stuffed bit, which moves the rest by an odd number of bits)
        payload = b"\x3e" * (lead % 2) + b"\x00" * (lead // 2) + b"\xff" * 20
        span = ref.stuffed(ref.frame_bits(payload, 16))
        for k in range(64, len(span), 64):  # a stuffed 0 at k + s whose five 1s begin in the word before
            for s in range(0, 5):
                if k + s < len(span) and span[k + s] == 0 and span[k + s - 5:k + s].all():
                    straddles.add(s)
        per, _ = compare(c, q, [ref.soft(np.concatenate([encode(hz, q, [payload]), np.zeros(9, np.uint8)]), lead)], 2, device)
        assert payloads_of(per) == [frame_of(q, payload)]
    assert straddles == {0, 1, 2, 3, 4}, straddles  # 5 ... 1 of the five 1s in the word before


def test_lanes_that_delete_none_one_and_the_most(hz, space):
    """one span whose 64-bit words hold 0, 1 and 11 stuffed bits"""
    c, device = space
    q = ref.Config(fcs=32, max_bytes=64)
    payload = b"\x00" * 8 + b"\x1f" + b"\x00" * 7 + b"\xff" * 40
    span = ref.stuffed(ref.frame_bits(payload, 32))
    bits = ref.frame_bits(payload, 32)
    deleted, at = [], 0
    marks = np.zeros(len(span), np.uint8)  # 1 where the span's bit is a stuffed one
    ones = 0
    for b in bits:
        at += 1
        ones = ones + 1 if b else 0
        if ones == 5:
            marks[at] = 1
            at += 1
            ones = 0
    deleted = [int(marks[k:k + 64].sum()) for k in range(0, len(span), 64)]
    assert deleted[0] == 0 and deleted[1] == 1 and max(deleted) == 11, deleted
    per, _ = compare(c, q, [ref.soft(np.concatenate([np.zeros(3, np.uint8), encode(hz, q, [payload]), np.zeros(5, np.uint8)]), 1)], 2, device)
    assert payloads_of(per) == [frame_of(q, payload)]


# ---- 3. the sizes --------------------------------------------------------------------------------------

@pytest.mark.parametrize("fcs", [0, 16])
def test_frames_of_the_smallest_and_largest_size_and_beyond(hz, space, fcs):
    """min_bytes and max_bytes come out; min_bytes - 1, max_bytes + 1 and a frame with a bit too many are dropped"""
    c, device = space
    q = ref.Config(fcs=fcs, min_bytes=fcs // 8 + 3, max_bytes=21, keep_bad=1)
    n = fcs // 8
    sizes = [q.min_bytes - n, q.max_bytes - n, q.min_bytes - n - 1, q.max_bytes - n + 1, 9]
    payloads = [ref.random_bytes(s, 40 + s) for s in sizes] + [b"\xff" * (q.max_bytes - n), b"\xff" * (q.max_bytes - n + 1)]
    odd = np.concatenate([FLAG, ref.stuffed(np.concatenate([ref.frame_bits(b"seven+1", fcs), [1]])), FLAG]).astype(np.uint8)
    b = np.concatenate([encode(hz, q, payloads[:3]), odd, encode(hz, q, payloads[3:]), np.zeros(4, np.uint8)])
    per, _ = compare(c, q, cut(ref.soft(b, fcs), [0, 500, len(b)]), 8, device)
    assert payloads_of(per) == [frame_of(q, payloads[k]) for k in (0, 1, 4, 5)]


def test_frames_of_1024_bytes(hz, space):
    """max_bytes = 1024: a span over more than 64 lanes' words, three passes, the ring wrapped inside a frame"""
    c, device = space
    q = ref.Config(fcs=16, max_bytes=1024)
    payloads = [ref.random_bytes(1022, 1), b"\xff" * 1022, ref.random_bytes(1023, 2), ref.random_bytes(700, 3)]
    b = np.concatenate([np.zeros(11, np.uint8), encode(hz, q, payloads, flags=2), np.zeros(7, np.uint8)])
    with bank_of(c, q, 1) as f:
        assert f.plan()[:3] == (1, TILE, 256)
    assert 64 * 128 < len(ref.stuffed(ref.frame_bits(payloads[1], 16))) <= q.Lmax  # (a span over three passes of the lanes)
    per, _ = compare(c, q, cut(ref.soft(b, 5), [0, 3000, 9000, 9001, 20000, len(b)]), 2, device)
    assert payloads_of(per) == [frame_of(q, p) for p in (payloads[0], payloads[1], payloads[3])]


# ---- 4. cut invariance -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def long_stream(hz):
    q = ref.Config(fcs=16, max_bytes=40, diff=2)
    b, payloads = traffic(hz, q, 3, 30, lo=4)
    total = 3 * CHUNK + 37
    assert len(b) >= total
    b = b[:total]
    x = ref.soft(ref.line(b, 2), 8)
    ((per, state),) = ref.exact(BUILD, [(q, [x], 40)])
    found, _ = ref.frames_of(b, q)
    assert len(found) >= 8 and [f[1] for f in found] == payloads_of(per)
    return q, b, x, ref.stored(per, 0), state, [f[0] for f in found]


def run_cut(c, device, q, x, edges, cap=40):
    """the stream in the pushes `edges` cut -> (stored frames over the pushes, counts per push, state)"""
    got, counts = [], []
    with bank_of(c, q, 1) as f:
        for part in cut(x, edges):
            res = f.push(dev(part) if device else part, None, cap)
            per = tuple(host(t) for t in res)
            per = (per[0], per[1].view(np.uint64), per[2].view(np.uint32), per[3].view(np.uint32))
            got += ref.stored([per], 0)
            counts.append(int(per[3][0]))
        return got, counts, f.state()


def test_cut_invariance_whole_and_around_a_closing_flag(long_stream, space):
    c, device = space
    q, b, x, want, wstate, ends = long_stream
    got, counts, state = run_cut(c, device, q, x, [0, len(x)])
    assert got == want and counts == [len(want)] and same_state(state, wstate)
    e2 = ends[len(ends) // 2]
    for k in range(e2 - 70, e2 + 71):
        got, counts, state = run_cut(c, device, q, x, [0, k, len(x)])
        assert got == want and same_state(state, wstate), k
        assert counts[0] == sum(e < k for e in ends), k  # a frame comes with the push that delivers its closing flag's last bit


@pytest.mark.parametrize("size", [1, 63, 64, 65])
def test_cut_invariance_in_pushes_of_one_size(long_stream, ctx, size):
    q, b, x, want, wstate, ends = long_stream
    edges = list(range(0, len(x), size)) + [len(x)]
    edges = sorted(edges + edges[5::9])  # n = 0 pushes in between
    got, counts, state = run_cut(ctx, True, q, x, edges, cap=2)
    assert got == want and same_state(state, wstate) and max(counts) <= 2


# ---- 5. the state ------------------------------------------------------------------------------------

def test_state_round_trip_mid_frame_and_reset(long_stream, space):
    c, device = space
    q, b, x, want, wstate, ends = long_stream
    mid = ends[3] - 100  # inside a frame
    ((first, zmid),) = ref.exact(BUILD, [(q, [x[:mid]], 8)])
    with bank_of(c, q, 1) as f, bank_of(c, q, 1) as g:
        push_checked(f, q, x[:mid], None, 8, device, first[0])
        z = f.state()
        assert same_state(z, zmid) and int(z[0][0]) == mid
        g.set_state(*z)
        assert same_state(g.state(), z)
        ((second, zend),) = ref.exact(BUILD, [(q, [x[mid:]], 40, zmid)])
        push_checked(g, q, x[mid:], None, 40, device, second[0])
        assert same_state(g.state(), wstate) and same_state(zend, wstate)
        assert ref.stored(first, 0) + ref.stored(second, 0) == want
        f.reset()
        zero = f.state()
        assert not any(np.asarray(a).any() for a in zero)
        ((again, _),) = ref.exact(BUILD, [(q, [x], 40)])
        push_checked(f, q, x, None, 40, device, again[0])
        assert same_state(f.state(), wstate)


# ---- 6. rows -----------------------------------------------------------------------------------------

def rows_of(hz, q, R, n, seed):
    xs, sent = [], []
    for r in range(R):
        b, payloads = traffic(hz, q, seed + r, 6, gap=3 + r % 5)
        b = np.resize(b, n)
        xs.append(ref.soft(ref.line(b, q.diff), seed * 31 + r, q.cplx))
        sent.append(payloads)
    return np.stack(xs), sent


@pytest.mark.parametrize("R", [1, 2, 3, 65])
def test_rows_and_ragged_counts(hz, space, R):
    """rows_per_wave is 1: R = 1 and 2 are its edges; ragged in_counts with 0 and with counts above n"""
    c, device = space
    q = ref.Config(fcs=16, max_bytes=16, diff=1)
    with bank_of(c, q, R) as f:
        assert f.plan() == (1, TILE, 32, ref.FORM_DIFF | ref.FORM_FCS16)
    n = 700
    x, sent = rows_of(hz, q, R, n, 21)
    pushes = []
    for k, (a, e) in enumerate(((0, 300), (300, 301), (301, 700))):
        cnt = np.array([(e - a) if (r + k) % 3 else ((e - a) // 2 if r % 2 else 0) for r in range(R)], np.uint32)
        cnt[-1] = e - a + 9  # (clamped)
        pushes.append((np.ascontiguousarray(x[:, a:e]) if R > 1 else x[0, a:e], cnt))
    per, st = compare(c, q, pushes, 6, device)
    assert sum(int(p[3].sum()) for p in per) >= R
    assert frame_of(q, sent[R - 1][0]) in payloads_of(per, R - 1)


def test_special_values_decide_by_their_sign_bit(hz, space):
    """-0, NaNs of both signs, infinities and denormals carry a frame"""
    c, device = space
    pos = np.array([0x00000000, 0x7FC00000, 0x7F800000, 0x00000001, 0x7FFFFFFF, 0x3F800000], np.uint32)
    q = ref.Config(fcs=16, max_bytes=16)
    b = np.concatenate([np.zeros(5, np.uint8), encode(hz, q, [b"NaN\xff-0"]), np.zeros(5, np.uint8)])
    words = np.where(b == 1, pos[np.arange(len(b)) % 6], pos[np.arange(len(b)) % 6] | np.uint32(0x80000000)).astype(np.uint32)
    x = words.view(np.float32)
    assert np.isnan(x).sum() > 10 and np.isinf(x).sum() > 10
    per, _ = compare(c, q, [x[:40], x[40:]], 2, device)
    assert payloads_of(per) == [frame_of(q, b"NaN\xff-0")]


def test_other_rows_do_not_matter(hz, ctx):
    q = ref.Config(fcs=16, max_bytes=16)
    x, sent = rows_of(hz, q, 9, 600, 51)
    per, st = compare(ctx, q, cut(x, [0, 250, 600]), 6, True)
    y = x.copy()
    y[np.arange(9) != 4] = rows_of(hz, q, 8, 600, 77)[0]
    per2, st2 = compare(ctx, q, cut(y, [0, 250, 600]), 6, True)
    assert ref.stored(per, 4) == ref.stored(per2, 4) and all(np.array_equal(a[4], b[4]) for a, b in zip(st, st2))
    assert ref.stored(per, 3) != ref.stored(per2, 3)
    one, st1 = compare(ctx, q, cut(x[4], [0, 250, 600]), 9, True)
    assert ref.stored(one, 0) == ref.stored(per, 4) and all(np.array_equal(a[0], b[4]) for a, b in zip(st1, st))
    assert len(ref.stored(per, 4)) >= 3


# ---- 7. cap ------------------------------------------------------------------------------------------

def test_cap_zero_counts_and_cap_one_stores_one(hz, space):
    c, device = space
    q = ref.Config(fcs=16, max_bytes=16)
    payloads = [b"one", b"two", b"three"]
    x = ref.soft(np.concatenate([encode(hz, q, payloads), np.zeros(3, np.uint8)]), 2)
    per, _ = compare(c, q, [x], 1, device)
    assert int(per[0][3][0]) == 3 and payloads_of(per) == [frame_of(q, b"one")]
    per, _ = compare(c, q, [x], 0, device)
    assert int(per[0][3][0]) == 3
    with bank_of(c, q, 1) as f:
        res = f.push(dev(x) if device else x, None, 0)
        assert host(res[3]).view(np.uint32).tolist() == [3] and res[0].shape == (1, 0, 16)


# ---- 8. the options ------------------------------------------------------------------------------------

@pytest.mark.parametrize("diff", [0, 1, 2])
@pytest.mark.parametrize("fcs", [0, 16, 32])
def test_options(hz, space, fcs, diff):
    """fcs x keep_bad x msb_first x diff, real rows and complex rows (Re decides, Im is noise), one frame with a bit error"""
    c, device = space
    for keep_bad in (0, 1):
        for msb_first in (0, 1):
            q = ref.Config(diff=diff, fcs=fcs, max_bytes=30, msb_first=msb_first, keep_bad=keep_bad, cplx=bool((keep_bad + msb_first) % 2))
            payloads = [b"\x01\x80plain", b"\xff" * 9, b"broken frame", ref.random_bytes(30 - fcs // 8, fcs + diff)]
            parts = [encode(hz, q, [p]) for p in payloads]
            parts[2][8 + 3] ^= 1  # (in 'b': a flip that makes no run of five in either bit order)
            b = np.concatenate(parts + [np.zeros(3, np.uint8)])
            x = ref.soft(ref.line(b, diff), 3, q.cplx)
            per, _ = compare(c, q, cut(x, [0, 130, len(x)]), 5, device)
            got = ref.stored(per, 0)
            good = [frame_of(q, p) for p in payloads]
            if fcs == 0:
                assert len(got) == 4 and [g[0] for k, g in enumerate(got) if k != 2] == good[:2] + good[3:] and all(g[2] for g in got)
            elif keep_bad:
                assert [g[2] for g in got] == [1, 1, 0, 1] and len(got[2][0]) == len(good[2]) and got[2][0] != good[2]
            else:
                assert [g[0] for g in got] == good[:2] + good[3:] and all(g[2] for g in got)
            with bank_of(c, q, 1) as f:
                form = (ref.FORM_COMPLEX if q.cplx else 0) | (ref.FORM_DIFF if diff else 0) | {0: 0, 16: ref.FORM_FCS16, 32: ref.FORM_FCS32}[fcs]
                assert f.plan()[3] == form | (ref.FORM_MSB_FIRST if msb_first else 0) | (ref.FORM_KEEP_BAD if keep_bad else 0)


# ---- 9. noise ----------------------------------------------------------------------------------------

def test_noise_rows(space):
    """4096 symbols of random signs over 8 rows, fcs = 0, min_bytes = 1: an event every 128 bits, every frame compared"""
    c, device = space
    q = ref.Config(fcs=0, min_bytes=1, max_bytes=64)
    x = np.stack([ref.soft(ref.random_bits(4096, 900 + r), r) for r in range(8)])
    per, _ = compare(c, q, cut(x, [0, 1500, 4096]), 8, device)
    events = sum(len(ref.find_events(ref.decided_bits(ref.floats_of(x[r]), 0)[0])) for r in range(8))
    assert events > 8 * 20 and sum(int(p[3].sum()) for p in per) >= 3


# ---- 10. the chain -----------------------------------------------------------------------------------

def test_the_chain_symbol_timing_to_frames(hz, ctx):
    """NRZI bits at 4 samples per symbol -> the symbol-timing bank -> (symbols, counts) as they are, on the device, with
    no host read in between -> frames, byte for byte"""
    q = ref.Config(diff=2, fcs=16, max_bytes=40)
    sent = [[ref.random_bytes(30, 10 * r + 1)] + [ref.random_bytes(10 + 3 * k, 10 * r + 5 + k) for k in range(5)] + [b"\xff" * 12] for r in range(3)]
    rows = []
    for r in range(3):
        d = hz.hdlc_encode(sent[r], fcs=16, flags=3, diff=2)
        rows.append(symsync_ref.signal(d.astype(np.float32) * 2 - 1, 4.0, (0.0, 0.3, 0.7)[r], noise_db=-20.0, seed=r).astype(np.float32))
    n = min(len(r) for r in rows)
    x = np.stack([r[:n] for r in rows])
    sp = np.array([4.0, 0.01, *hz.loop_gains(4.0)], np.float32)
    with ctx.symbol_sync(hz.SYMSYNC_REAL_F32, sp, rows=3) as ts, bank_of(ctx, q, 3) as f:
        parts, res = [], []
        for part in cut(dev(x), [0, 2500, 2501, x.shape[1]]):
            s, cnt = ts.push(part)
            res.append(f.push(s, cnt, 8))
            parts.append((s, cnt))
        state = f.state()
    pushes = [(host(s), host(c).view(np.uint32)) for s, c in parts]
    ((per, wstate),) = ref.exact(BUILD, [(q, pushes, 8)])
    assert same_state(state, wstate) and np.array_equal(wstate[0], sum(c for _, c in pushes))
    got = [(host(fr), host(ps).view(np.uint64), host(inf).view(np.uint32), host(cnt).view(np.uint32)) for fr, ps, inf, cnt in res]
    for r in range(3):
        assert ref.stored(got, r) == ref.stored(per, r), r
        frames = payloads_of(got, r)
        for p in sent[r][1:]:
            assert frame_of(q, p) in frames, r


# ---- 11. refusals --------------------------------------------------------------------------------------

@pytest.mark.parametrize("r", [1, 3])
def test_refused_pushes_leave_the_state(hz, ctx, r):
    lib = importlib.import_module("go-sdr_amd._capi").lib
    q = ref.Config(fcs=16, max_bytes=16)
    n, cap = 150, 2
    x, _ = rows_of(hz, q, 3, 2 * n, 61)
    x = x[:r]
    ((per, wstate),) = ref.exact(BUILD, [(q, [x[:, :n], x[:, n:]], cap)])
    with bank_of(ctx, q, r) as f:
        push_checked(f, q, x[:, :n] if r > 1 else x[0, :n], None, cap, True, per[0])
        z0 = f.state()
        part = dev(x[:, n:])
        out, pos = torch.zeros((r, cap * q.FB), dtype=torch.uint8, device="cuda"), torch.zeros((r, cap), dtype=torch.int64, device="cuda")
        info, cnt = torch.zeros((r, cap), dtype=torch.int32, device="cuda"), torch.zeros(r, dtype=torch.int32, device="cuda")
        push = lambda *a: ctx._ck(lib.hzsdr_hdlc_push(f._h, *a))
        o, p, i, k = out.data_ptr(), pos.data_ptr(), info.data_ptr(), cnt.data_ptr()
        if r > 1:
            with pytest.raises(hz.ErrDstTooSmall):
                push(part.data_ptr(), n, n, None, o, cap, cap * q.FB - 1, p, i, k, None)
            with pytest.raises(hz.ErrInvalidArgument):
                push(part.data_ptr(), n, n - 1, None, o, cap, cap * q.FB, p, i, k, None)
        for bad in ((None, n, n, None, o, cap, cap * q.FB, p, i, k, None), (part.data_ptr(), n, n, None, None, cap, cap * q.FB, p, i, k, None),
                    (part.data_ptr(), n, n, None, o, cap, cap * q.FB, None, i, k, None), (part.data_ptr(), n, n, None, o, cap, cap * q.FB, p, None, k, None),
                    (part.data_ptr(), n, n, None, o, cap, cap * q.FB, p, i, None, None), (part.data_ptr(), 2 ** 31, 2 ** 31, None, o, cap, cap * q.FB, p, i, k, None),
                    (part.data_ptr(), n, n, None, o, 2 ** 32, 2 ** 36, p, i, k, None)):
            with pytest.raises(hz.ErrInvalidArgument):
                push(*bad)
        assert lib.hzsdr_hdlc_push(None, part.data_ptr(), n, n, None, o, cap, cap * q.FB, p, i, k, None) == hz.ErrInvalidArgument.status
        torch.cuda.synchronize()
        assert same_state(f.state(), z0) and not out.any() and not cnt.any()
        most = C.c_size_t(99)
        push(part.data_ptr(), n, n, None, o, cap, cap * q.FB, p, i, k, C.byref(most))
        assert same_state(f.state(), wstate) and most.value == int(per[1][3].max())
        assert np.array_equal(host(cnt).view(np.uint32), per[1][3])
        u64, u8 = (C.c_uint64 * (r + 1))(), (C.c_uint8 * ((r + 1) * q.HB))()
        if r > 1:
            with pytest.raises(hz.ErrDstTooSmall):
                ctx._ck(lib.hzsdr_hdlc_get_state(f._h, u64, u64, u8, u8, u8, r - 1))
            with pytest.raises(hz.ErrDstTooSmall):
                ctx._ck(lib.hzsdr_hdlc_positions(f._h, u64, r - 1))
        with pytest.raises(hz.ErrInvalidArgument):
            ctx._ck(lib.hzsdr_hdlc_set_state(f._h, u64, u64, u8, u8, u8, r + 1))
        z = [np.array(a) for a in wstate]
        z[1][0] = z[0][0] + 1  # an event the stream has not reached
        with pytest.raises(hz.ErrInvalidArgument):
            f.set_state(*z)
        assert same_state(f.state(), wstate)
    assert sum(int(p[3].sum()) for p in per) >= r


def test_create_errors(hz, ctx):
    """rows 0 and 8193, other kinds, and every bound through the library (tests/test_hdlc_cpu.py has the same sets
    against the same hz_hdlc_plan.h)"""
    lib = importlib.import_module("go-sdr_amd._capi").lib
    out = C.c_void_p()

    def create(q, rows=1, kind=None):
        return lib.hzsdr_hdlc_create(ctx._h, q.kind if kind is None else kind, q.diff, q.fcs, q.min_bytes, q.max_bytes, q.msb_first, q.keep_bad, rows,
                                     C.byref(out))

    Q = ref.Config
    inval = hz.ErrInvalidArgument.status
    assert create(Q(), 0) == inval and create(Q(), hz.HDLC_MAX_ROWS + 1) == inval
    assert create(Q(), hz.HDLC_MAX_ROWS) == 0 and lib.hzsdr_hdlc_free(out) == 0
    for kind in (-1, 0, hz.FMT_U8, hz.FMT_I16, 31, 33):
        assert create(Q(), 1, kind) == hz.ErrSampleFormatUnknown.status, kind
    for bad in (Q(fcs=0, min_bytes=0), Q(fcs=16, min_bytes=2), Q(fcs=32, min_bytes=4), Q(max_bytes=1025), Q(min_bytes=65, max_bytes=64), Q(diff=3), Q(diff=-1),
                Q(fcs=8), Q(fcs=24), Q(msb_first=2), Q(keep_bad=2), Q(msb_first=-1)):
        assert not bad.accepted() and create(bad) == inval, vars(bad)
    for good in (Q(fcs=0, min_bytes=1, max_bytes=1), Q(fcs=16, min_bytes=3, max_bytes=3), Q(fcs=32, min_bytes=5, max_bytes=1024),
                 Q(diff=2, msb_first=1, keep_bad=1, cplx=True)):
        assert good.accepted() and create(good) == 0 and lib.hzsdr_hdlc_free(out) == 0, vars(good)
    with bank_of(ctx, Q(), 1) as f, pytest.raises(ValueError):
        f.push(dev(np.zeros(8, np.complex64)))
    with bank_of(ctx, Q(), 2) as f, pytest.raises(hz.ErrInvalidArgument):
        f.set_state(np.zeros(3, np.uint64), np.zeros(3, np.uint64), np.zeros(3, np.uint8), np.zeros((3, Q().HB), np.uint8), np.zeros(3, np.uint8))


# ---- 12. the other layers -----------------------------------------------------------------------------

def _run(exe):
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "go-sdr_amd") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    return subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)


def test_c_hdlc_walkthrough(hz):
    """tests/c/test_hdlc_abi.c compiled by gcc as C99 and run against libhzsdr_hip.so."""
    exe = os.path.join(BUILD, "test_hdlc_abi")
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "test_hdlc_abi.c"), "-L" + os.path.join(ROOT, "go-sdr_amd"),
                           "-lhzsdr_hip", "-lm", "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    p = _run(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "hdlc-abi ok" in p.stdout


def test_cxx_hdlc(hz):
    """tests/cxx/test_hdlc.cpp (hzsdr::stream::Hdlc of go-sdr_amd/cxx/hzsdr.hpp) built with g++ and run."""
    exe = os.path.join(BUILD, "test_hdlc_cxx")
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + ROOT, os.path.join(ROOT, "tests", "cxx", "test_hdlc.cpp"),
                           "-L" + os.path.join(ROOT, "go-sdr_amd"), "-lhzsdr_hip", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    p = _run(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "hdlc-cxx ok" in p.stdout


def test_hdlc_frames_over_a_reader(hz, hctx):
    """stream.hdlc_frames over a BufferReader with short reads finds the frames of one push of the whole stream; fed
    with blocks or (symbols, counts) pairs it takes them as they are; a real bank behind a Reader is refused; more
    frames in a push than cap raises"""
    st = importlib.import_module("go-sdr_amd.stream")
    q = ref.Config(fcs=16, max_bytes=40, diff=2, cplx=True)
    b, payloads = traffic(hz, q, 9, 12, lo=2)
    x = ref.soft(ref.line(b, 2), 4, True)
    ((per, wstate),) = ref.exact(BUILD, [(q, [x], 16)])
    want = ref.stored(per, 0)
    assert [w[0] for w in want] == [frame_of(q, p) for p in payloads]
    with bank_of(hctx, q, 1) as f:
        parts = list(st.hdlc_frames(st.BufferReader(x, 48_000, max_read=333), f, block=512))
        assert same_state(f.state(), wstate)
    got = [(pk, int(p), int(g)) for part in parts for pk, p, g in zip(*part[0])]
    assert len(parts) > 3 and got == want
    with bank_of(hctx, q, 1) as f:
        pairs = [(x[i:i + 500], np.array([400], np.uint32)) for i in range(0, 1500, 500)]
        list(st.hdlc_frames(pairs, f))
        assert f.positions()[0] == 1200
        f.reset()
        with pytest.raises(st.ErrShortBuffer):
            list(st.hdlc_frames([x], f, cap=1))
    with bank_of(hctx, ref.Config(), 1) as f, pytest.raises(hz.ErrSampleFormatMismatch):
        list(st.hdlc_frames(st.BufferReader(x, 48_000), f))

"""The frame sync bank (include/hzsdr_framesync.h) on the GPU against the host program tests/host/framesync_ref.cpp, which
tests/test_framesync_cpu.py holds to the numpy brute force: frames, positions, info, counts and state are compared
EXACTLY, the destinations are full of sentinels and every pitch is above the need.  Random rows produce false
candidates, which is fine since whole lists are compared; every test asserts on the host side that the reference finds
the frames it planted (or, for words short enough to match noise, at least as many), so that two empty lists cannot pass.

The chain test (carrier -> symbol timing -> frame sync on QPSK rows): frames of a 32-bit word and 168 payload bits, 100
symbols each, one every 110 symbols, at 5 samples per symbol with white noise 20 dB below the symbol power.  Measured on
the CPU from the chained host programs over the seeds 1 ... 12 with the test's three carrier offsets and phases (36
rows, 13 frames each): NO frame is lost, the first one included, whose word starts at symbol CHAIN_FIRST_WORD = 10 --
the loops are inside a symbol or two of their lock at these offsets, and the four hypotheses take whatever rotation the
Costas loop settles on.  So there is no lost frame to double; asserted is every frame whose word starts at
CHAIN_A = 20 = twice the earliest start measured, or later, since acquisition varies with the seed."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import carrier_ref
import framesync_ref as ref
import symsync_ref
from conftest import ROOT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BUILD = os.path.join(ROOT, "build")
WORD32 = 0x1ACFFC1D
SENT8, SENT32, SENT64 = 0xA5, 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
CHAIN_FIRST_WORD, CHAIN_A = 10, 20


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
    base = dict(W=32, words=[WORD32], P=168, B=1, cplx=False, mask=None, thr=2, maps=None, diff=0, holdoff=None)
    base.update(kw)
    return ref.Config(**base)


def bank_of(c, q, rows):
    args, kw = q.create_args()
    return c.frame_sync(q.kind, *args, rows=rows, **kw)


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
    push: the stored slots exactly, everything else still a sentinel"""
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
        assert np.array_equal(gw[r, :m * q.FB].reshape(m, q.FB), wf[r, :m]), r
        assert (gw[r, m * q.FB:] == SENT8).all(), r
        assert np.array_equal(gp[r, :m], wp[r, :m]) and (gp[r, m:] == SENT64).all(), r
        assert np.array_equal(gi[r, :m], wi[r, :m]) and (gi[r, m:] == SENT32).all(), r


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
            push_checked(f, q, np.asarray(x), cnt, cap, device, per[k], pads=(3 + k, 5 + 2 * k))
        got = f.state()
        assert same_state(got, wstate)
        assert np.array_equal(f.positions(), wstate[0])
    return per, wstate


def found(per, row):
    """{position: frame bytes} of everything the program stored for `row`, over the pushes"""
    out = {}
    for fr, ps, inf, cnt in per:
        for k in range(min(int(cnt[row]), fr.shape[1])):
            out[int(ps[row, k])] = (bytes(fr[row, k]), int(inf[row, k]))
    return out


def rows_with_plants(q, R, nsym, seed, plants, hyp=0, rotate=0):
    """R random rows of nsym symbols, the word of hypothesis `hyp` and a payload planted at bit plants(r)[k] of row r
    -> (x numpy (R, nsym), [[(bit, payload)]])"""
    xs, where = [], []
    for r in range(R):
        bits = ref.random_bits(nsym * q.B, seed * 1009 + r)
        row = []
        for k, at in enumerate(plants(r)):
            pay = ref.random_bits(q.P, seed * 7919 + 31 * r + k)
            ref.plant(bits, at, q.words[hyp], q.W, pay)
            row.append((at, pay))
        xs.append(ref.soft(ref.encode_diff(bits, q.diff), seed + r, q, rotate=rotate))
        where.append(row)
    return np.stack(xs), where


def assert_plants_found(q, per, where, rows=None, h=0):
    """every planted frame of the rows is among the program's frames, with its payload, distance 0 and hypothesis h"""
    for r in (range(len(where)) if rows is None else rows):
        got = found(per, r)
        for at, pay in where[r]:
            s = (at + q.W) // q.B
            assert s in got, (r, at)
            assert got[s] == (bytes(np.packbits(pay)), h << 8), (r, at)


def cut(x, edges):
    return [x[..., a:b] for a, b in zip(edges, edges[1:])]


EDGES = np.cumsum([0, 0, 1, 63, 64, 65, 127, 128, 129, 300]).tolist()  # pushes of n = 0, 1, 63, 64, 65, 127, 128, 129, 300


# ---- 1. rows, push lengths, both spaces ------------------------------------------------------------------

@pytest.mark.parametrize("space", ["device", "host"])
@pytest.mark.parametrize("R", [1, 2, 63, 64, 65, 130])
def test_rows_and_push_lengths(ctx, hctx, space, R):
    """a stream of 877 symbols in pushes of 0, 1, 63, 64, 65, 127, 128, 129 and 300, two frames planted per row at
    places that move with the row"""
    q = cfg(holdoff=150)
    x, where = rows_with_plants(q, R, EDGES[-1], 11, lambda r: (40 + 2 * r, 40 + 2 * r + 230))
    x = x if R > 1 else x[0]
    per, _ = compare(ctx if space == "device" else hctx, q, cut(x, EDGES), 3, space == "device")
    assert_plants_found(q, per, where)


@pytest.mark.parametrize("R", [1024, 1025, 2049, 8192])
def test_rows_per_wave_edges(hz, ctx, R):
    """the row counts at which the row-wave banks go from one row per wave to two, three and eight: this bank keeps one
    row per wave throughout (DESIGN.md section 4 has the measurement behind that), and plan() says so"""
    q = cfg(W=24, words=[0xFAF320], P=64, thr=1, holdoff=80)
    with bank_of(ctx, q, R) as f:
        g, tile, ring, form = f.plan()
    assert g == 1 and tile == 64 and ring == 32 and form == 0
    x, where = rows_with_plants(q, R, 300, 12, lambda r: (30 + r % 97, 150 + r % 61))
    per, _ = compare(ctx, q, cut(x, [0, 129, 300]), 3, True)
    assert_plants_found(q, per, where, rows=(0, 1, g - 1, g, R - g, R - 1))


# ---- 2. word and payload sizes -----------------------------------------------------------------------

@pytest.mark.parametrize("W", [1, 7, 8, 24, 32, 63, 64])
def test_word_and_payload_sizes(ctx, W):
    word = (0xF0F0AA5512345678 >> (64 - W)) | 1
    for P in (1, 8, 13, 64, 168):
        q = cfg(W=W, words=[word], P=P, thr=0, holdoff=max(1, (W + P) // 2))
        x, where = rows_with_plants(q, 3, 600, 20 + P, lambda r: (50 + r, 50 + r + W + P + 9))
        per, _ = compare(ctx, q, cut(x, [0, 130, 300, 600]), 64, True)
        if W >= 24:
            assert_plants_found(q, per, where)
        else:  # a short word matches the random bits too, and a false candidate may hold a plant off
            assert all(sum(int(c[3][r]) for c in per) >= 2 for r in range(3))


def test_the_largest_payload(hz, ctx):
    """P = 8192 behind a 64-bit word: 129 words of history, the 256-word ring, a frame of 1024 bytes cut in three pushes"""
    q = cfg(W=64, words=[0xF0F0AA5512345678], P=8192, thr=3)
    x, where = rows_with_plants(q, 2, 9000, 31, lambda r: (100 + 37 * r,))
    with bank_of(ctx, q, 2) as f:
        assert f.plan()[2] == 256
    per, _ = compare(ctx, q, cut(x, [0, 4000, 8200, 9000]), 2, True)
    assert_plants_found(q, per, where)


# ---- 3. tile bit offsets -------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 2])
def test_word_and_payload_ends_on_tile_bits(ctx, B):
    """the word's last bit, and the payload's last bit, on the tile's bits 0, 1, 62 and 63 (B = 2: a window ends on an odd
    bit, so 1 and 63, and 61 and 3 beside them)"""
    q = cfg(P=168) if B == 1 else cfg(P=168, B=2, cplx=True, words=ref.rotated_words(WORD32, 32), maps=[0, 1, 2, 3])
    ends = (0, 1, 62, 63) if B == 1 else (1, 3, 61, 63)
    at = [128 + e - (q.W - 1) for e in ends] + [256 + e - (q.W + q.P - 1) for e in ends]
    x, where = rows_with_plants(q, len(at), 600 // B, 41, lambda r: (at[r],))
    per, _ = compare(ctx, q, [x], 2, True)
    assert_plants_found(q, per, where)
    assert [(a + q.W - 1) % 64 for a in at[:4]] == list(ends) and [(a + q.W + q.P - 1) % 64 for a in at[4:]] == list(ends)


# ---- 4. cuts and the state carried --------------------------------------------------------------------

@pytest.mark.parametrize("space", ["device", "host"])
def test_cuts_and_state_into_a_new_object(ctx, hctx, space):
    """a word split between two pushes, a payload split between two and between three pushes; then the same stream with
    the state moved into a new object by get_state / set_state at every cut"""
    c, device = (ctx, True) if space == "device" else (hctx, False)
    q = cfg()
    x, where = rows_with_plants(q, 3, 700, 51, lambda r: (90, 400))
    edges = [0, 100, 150, 420, 500, 570, 700]  # 100: inside the word at 90; 150: inside its payload; 420, 500, 570: word, payload, payload
    per, wstate = compare(c, q, cut(x, edges), 2, device)
    assert_plants_found(q, per, where)
    emitted = [int(p[3][0]) for p in per]
    assert emitted[2] == 1 and emitted[5] == 1 and sum(emitted) == 2  # each by the push that delivers its last bit
    state = None
    for k, part in enumerate(cut(x, edges)):
        ((want, wst),) = ref.exact(BUILD, [(q, [part], 2) if state is None else (q, [part], 2, state)])
        with bank_of(c, q, 3) as f:
            if state is not None:
                f.set_state(*state)
            push_checked(f, q, part, None, 2, device, want[0])
            state = f.state()
        assert same_state(state, wst) and np.array_equal(want[0][3], per[k][3])
    assert same_state(state, wstate)


# ---- 5. ragged input ---------------------------------------------------------------------------------

@pytest.mark.parametrize("space", ["device", "host"])
def test_ragged_counts(ctx, hctx, space):
    """in_counts with zeros, ones and n among the rows and counts above n (clamped); then every row's consumed stream
    pushed again with equal counts in another cut: the same frames at the same positions"""
    c, device = (ctx, True) if space == "device" else (hctx, False)
    q = cfg(W=16, words=[0xEB90], P=40, thr=0, holdoff=50)
    R, n = 9, 200
    x, where = rows_with_plants(q, R, 3 * n, 61, lambda r: (30, 330))
    counts = [np.array([0, 1, n, n + 7, 64, 65, 0, 2 ** 32 - 1, 199], np.uint32), np.array([n, n, 1, 0, n, 63, 0, n, 1], np.uint32),
              np.array([n, 0, n, n, 1, n, 0, n, n], np.uint32)]
    pushes = [(x[:, k * n:(k + 1) * n], counts[k]) for k in range(3)]
    per, wstate = compare(c, q, pushes, 4, device)
    assert wstate[0][6] == 0 and wstate[0][7] == 3 * n and wstate[0][3] == 2 * n
    assert_plants_found(q, per, where, rows=(7,))
    streams = [np.concatenate(ref.consumed(pushes, r, R)) for r in range(R)]
    for r in (0, 2, 4, 7, 8):
        s = streams[r]
        per1, st1 = compare(c, q, cut(s, [0, len(s) // 3, len(s)]), 8, device)
        assert {k: v for k, v in found(per1, 0).items()} == found(per, r)
        assert st1[0][0] == wstate[0][r] and st1[1][0] == wstate[1][r] and np.array_equal(st1[2][0], wstate[2][r])


# ---- 6. errors, threshold, mask ------------------------------------------------------------------------

def test_errors_at_and_above_the_threshold_and_under_the_mask(ctx):
    q = cfg(W=32, words=[WORD32], P=40, thr=3, mask=0xFFFF00FF, holdoff=10)
    word = ref.word_bits(WORD32, 32)
    rows, starts = [], []
    for r, flips in enumerate([(0, 5, 31), (0, 5, 31, 9), (16, 17, 18, 19, 20, 21, 22, 23), (16, 23, 0, 5, 31), ()]):
        bits = np.zeros(300, np.uint8)
        bits[1::2] = 1  # a background far from the word
        pay = ref.random_bits(40, 70 + r)
        ref.plant(bits, 100, WORD32, 32, pay)
        for k in flips:
            bits[100 + k] ^= 1
        rows.append(ref.soft(bits, 80 + r, q))
        starts.append(pay)
    x = np.stack(rows)
    per, _ = compare(ctx, q, [x[:, :111], x[:, 111:]], 2, True)
    got = [found(per, r) for r in range(5)]
    # mask 0xFFFF00FF: the bits 16 ... 23 (counted from the first received) do not care
    assert got[0][132] == (bytes(np.packbits(starts[0])), 3) and 132 not in got[1]
    assert got[2][132][1] == 0 and got[3][132][1] == 3 and got[4][132][1] == 0
    assert (word != ref.word_bits(WORD32 ^ 0x0000FF00, 32)).sum() == 8


# ---- 7. the hold-off ------------------------------------------------------------------------------------

def test_holdoff(ctx):
    """two plants closer than the hold-off in one tile; in neighbouring tiles; on either side of a cut; the first alone is
    accepted each time, and a third plant outside the hold-off again.  holdoff = 1 on a word that matches at
    consecutive symbols: every match is a frame"""
    q = cfg(W=16, words=[0xEB90], P=8, thr=0, holdoff=40)
    plants = [(70, 100, 180), (100, 130, 200), (40, 64, 150)]  # windows end in one tile (85, 115); in tiles 1 and 2 (115, 145); 55 | 79 across the cut at 72
    rows = []
    for r, ps in enumerate(plants):
        bits = np.zeros(300, np.uint8)
        for k, at in enumerate(ps):
            ref.plant(bits, at, 0xEB90, 16, ref.word_bits(0xC0 + 3 * r + k, 8))
        rows.append(ref.soft(bits, 90 + r, q))
    x = np.stack(rows)
    assert (70 + 15) // 64 == (100 + 15) // 64 and (100 + 15) // 64 + 1 == (130 + 15) // 64
    per, _ = compare(ctx, q, [x[:, :72], x[:, 72:]], 4, True)
    for r, ps in enumerate(plants):
        got = found(per, r)
        assert sorted(got) == [ps[0] + 16, ps[2] + 16], (r, sorted(got))
        assert got[ps[0] + 16][0] == bytes([0xC0 + 3 * r]) and got[ps[2] + 16][0] == bytes([0xC0 + 3 * r + 2])
    q1 = cfg(W=4, words=[0xF], P=4, thr=0, holdoff=1)
    bits = np.zeros(200, np.uint8)
    bits[50:70] = 1
    per, _ = compare(ctx, q1, [ref.soft(bits, 5, q1)], 32, True)
    assert sorted(found(per, 0)) == list(range(54, 71))
    q9 = cfg(W=4, words=[0xF], P=4, thr=0, holdoff=9)
    per, _ = compare(ctx, q9, [ref.soft(bits, 5, q9)], 32, True)
    assert sorted(found(per, 0)) == [54, 63]


# ---- 8. capacity --------------------------------------------------------------------------------------

@pytest.mark.parametrize("space", ["device", "host"])
def test_more_frames_than_cap(ctx, hctx, space):
    """a row with more frames than cap reports them all in counts, stores cap of them, and leaves the slots of its
    neighbours -- rows with fewer frames -- as they were (push_checked looks at every byte of the destinations)"""
    c, device = (ctx, True) if space == "device" else (hctx, False)
    q = cfg(W=8, words=[0xA7], P=13, thr=0, holdoff=21)
    x, where = rows_with_plants(q, 3, 400, 101, lambda r: [40 + 30 * k for k in range(1 if r != 1 else 10)])
    per, _ = compare(c, q, [x], 3, device)
    assert int(per[0][3][1]) >= 10 > 3 and int(per[0][3][0]) < int(per[0][3][1])
    per0, _ = compare(c, q, [x], 0, device)  # cap 0: counted only
    assert np.array_equal(per0[0][3], per[0][3])


# ---- 9. hypotheses --------------------------------------------------------------------------------------

def test_inverted_real_row_and_re_only_complex_rows(hz, ctx):
    words, maps = hz.sync_hypotheses(WORD32, 32, 1, "invert")
    for cplx in (False, True):
        q = cfg(words=words, maps=maps, cplx=cplx)
        x, where = rows_with_plants(q, 2, 500, 111, lambda r: (77 + r,))
        x[1] = -x[1]  # (a complex row's Im is noise either way)
        per, _ = compare(ctx, q, [x[:, :260], x[:, 260:]], 2, True)
        assert_plants_found(q, per, where, rows=(0,), h=0)
        assert_plants_found(q, per, where, rows=(1,), h=1)


@pytest.mark.parametrize("space", ["device", "host"])
def test_qpsk_rows_times_i_to_the_q(hz, ctx, hctx, space):
    """a QPSK row times i^q hits hypothesis q, and its payload comes out as sent"""
    c, device = (ctx, True) if space == "device" else (hctx, False)
    words, maps = hz.sync_hypotheses(WORD32, 32, 2, "rotate")
    assert words == ref.rotated_words(WORD32, 32)
    q = cfg(words=words, maps=maps, B=2, cplx=True)
    rows, where = [], []
    for k in range(4):
        x, w = rows_with_plants(q, 1, 300, 120, lambda r: (66, 330), rotate=k)  # the same row, turned
        rows.append(x[0]), where.append(w[0])
    per, _ = compare(c, q, cut(np.stack(rows), [0, 101, 300]), 3, device)
    for k in range(4):
        assert_plants_found(q, per, where, rows=(k,), h=k)


def test_ties_and_the_smallest_distance(ctx):
    """two hypotheses at equal distance: the smaller h; a later hypothesis nearer: that one, with its map"""
    a, b = 0xF0F0, 0xF0F3  # two bits apart; 0xF0F1 is one from each
    q = cfg(W=16, words=[a, b], maps=[0, 1], P=8, thr=2, holdoff=30)
    rows = []
    for word in (0xF0F1, 0xF0F3, 0xF0F0, 0xF0F7):
        bits = np.zeros(120, np.uint8)
        ref.plant(bits, 40, word, 16, ref.word_bits(0x96, 8))
        rows.append(ref.soft(bits, 130, q))
    per, _ = compare(ctx, q, [np.stack(rows)], 2, True)
    got = [found(per, r)[56] for r in range(4)]
    assert got[0] == (b"\x96", 1) and got[1] == (b"\x69", 0 | 1 << 8) and got[2] == (b"\x96", 0) and got[3] == (b"\x69", 1 | 1 << 8)


# ---- 10. differential decodings ----------------------------------------------------------------------------

@pytest.mark.parametrize("diff", [1, 2])
def test_diff_across_a_cut_and_on_an_inverted_row(ctx, diff):
    """the carried raw decision joins two pushes (cuts inside the word and in front of it); an inverted row decodes to the
    same bits from its second decision on, so the same frames"""
    q = cfg(W=16, words=[0xEB90], P=40, diff=diff, thr=0)
    x, where = rows_with_plants(q, 2, 300, 141, lambda r: (64,))
    x[1] = -x[0]
    for edges in ([0, 64, 300], [0, 65, 300], [0, 63, 64, 65, 128, 300]):
        per, _ = compare(ctx, q, cut(x, edges), 2, True)
        assert_plants_found(q, per, [where[0], where[0]])


# ---- 11. special values ---------------------------------------------------------------------------------

def test_special_values_decide_by_their_sign_bit(ctx, hctx):
    """-0, NaNs of both signs, infinities and denormals inside a word and a payload; an all-zero word against an empty
    history"""
    pos = np.array([0x00000000, 0x7FC00000, 0x7F800000, 0x00000001, 0x7FFFFFFF, 0x3F800000], np.uint32)
    q = cfg(W=16, words=[0xEB90], P=24, thr=0)
    bits = np.zeros(200, np.uint8)
    pay = ref.random_bits(24, 150)
    ref.plant(bits, 60, 0xEB90, 16, pay)
    words = np.where(bits == 1, pos[np.arange(200) % 6], pos[np.arange(200) % 6] | np.uint32(0x80000000)).astype(np.uint32)
    x = words.view(np.float32)
    assert np.isnan(x).sum() > 40 and np.isinf(x).sum() > 20
    for c, device in ((ctx, True), (hctx, False)):
        per, _ = compare(c, q, [x[:70], x[70:]], 2, device)
        assert found(per, 0)[76] == (bytes(np.packbits(pay)), 0)
    qz = cfg(W=8, words=[0], P=8, thr=0, holdoff=1)
    bits = np.ones(100, np.uint8)
    bits[40:48] = 0
    per, _ = compare(ctx, qz, [ref.soft(bits, 3, qz)], 8, True)
    assert sorted(found(per, 0)) == [48]


# ---- 12. the other rows ---------------------------------------------------------------------------------

def test_other_rows_do_not_matter(ctx):
    q = cfg(W=24, words=[0xFAF320], P=64, thr=1)
    x, where = rows_with_plants(q, 17, 400, 161, lambda r: (50 + 5 * r,))
    per, st = compare(ctx, q, cut(x, [0, 190, 400]), 2, True)
    y = x.copy()
    y[np.arange(17) != 8] = rows_with_plants(q, 16, 400, 162, lambda r: (90, 200))[0]
    per2, st2 = compare(ctx, q, cut(y, [0, 190, 400]), 2, True)
    assert found(per, 8) == found(per2, 8) and all(np.array_equal(a[8], b[8]) for a, b in zip(st, st2))
    one, st1 = compare(ctx, q, cut(x[8], [0, 190, 400]), 5, True)
    assert found(one, 0) == found(per, 8) and all(np.array_equal(a[0], b[8]) for a, b in zip(st1, st))
    assert_plants_found(q, per, where)


# ---- 13. refusals, reset ----------------------------------------------------------------------------------

@pytest.mark.parametrize("r", [1, 3])
def test_refused_pushes_leave_the_state_and_reset(hz, ctx, r):
    lib = importlib.import_module("go-sdr_amd._capi").lib
    q = cfg(W=16, words=[0xEB90], P=40, thr=0)
    n, cap = 150, 2
    x, where = rows_with_plants(q, 3, 2 * n, 171, lambda r: (130,))
    x = x[:r]
    ((per, wstate),) = ref.exact(BUILD, [(q, [x[:, :n], x[:, n:]], cap)])
    with bank_of(ctx, q, r) as f:
        push_checked(f, q, x[:, :n] if r > 1 else x[0, :n], None, cap, True, per[0])
        z0 = f.state()
        part = dev(x[:, n:])
        out, pos = torch.zeros((r, cap * q.FB), dtype=torch.uint8, device="cuda"), torch.zeros((r, cap), dtype=torch.int64, device="cuda")
        info, cnt = torch.zeros((r, cap), dtype=torch.int32, device="cuda"), torch.zeros(r, dtype=torch.int32, device="cuda")
        push = lambda *a: ctx._ck(lib.hzsdr_framesync_push(f._h, *a))
        o, p, i, k = out.data_ptr(), pos.data_ptr(), info.data_ptr(), cnt.data_ptr()
        if r > 1:
            with pytest.raises(hz.ErrDstTooSmall):
                push(part.data_ptr(), n, n, None, o, cap, cap * q.FB - 1, p, i, k, None)
            with pytest.raises(hz.ErrInvalidArgument):
                push(part.data_ptr(), n, n - 1, None, o, cap, cap * q.FB, p, i, k, None)
        for bad in ((None, n, n, None, o, cap, cap * q.FB, p, i, k, None), (part.data_ptr(), n, n, None, None, cap, cap * q.FB, p, i, k, None),
                    (part.data_ptr(), n, n, None, o, cap, cap * q.FB, None, i, k, None), (part.data_ptr(), n, n, None, o, cap, cap * q.FB, p, None, k, None),
                    (part.data_ptr(), n, n, None, o, cap, cap * q.FB, p, i, None, None), (part.data_ptr(), 2 ** 31, 2 ** 31, None, o, cap, cap * q.FB, p, i, k, None)):
            with pytest.raises(hz.ErrInvalidArgument):
                push(*bad)
        assert lib.hzsdr_framesync_push(None, part.data_ptr(), n, n, None, o, cap, cap * q.FB, p, i, k, None) == hz.ErrInvalidArgument.status
        torch.cuda.synchronize()
        assert same_state(f.state(), z0) and not out.any() and not cnt.any()
        most = C.c_size_t(99)
        push(part.data_ptr(), n, n, None, o, cap, cap * q.FB, p, i, k, C.byref(most))
        assert same_state(f.state(), wstate) and most.value == int(per[1][3].max()) >= 1
        assert np.array_equal(host(cnt).view(np.uint32), per[1][3]) and np.array_equal(host(out).reshape(r, cap, q.FB)[:, :1], per[1][0][:, :1])
        u64, u8 = (C.c_uint64 * (r + 1))(), (C.c_uint8 * ((r + 1) * q.HB))()
        if r > 1:
            with pytest.raises(hz.ErrDstTooSmall):
                ctx._ck(lib.hzsdr_framesync_get_state(f._h, u64, u64, u8, u8, r - 1))
            with pytest.raises(hz.ErrDstTooSmall):
                ctx._ck(lib.hzsdr_framesync_positions(f._h, u64, r - 1))
        with pytest.raises(hz.ErrInvalidArgument):
            ctx._ck(lib.hzsdr_framesync_set_state(f._h, u64, u64, u8, u8, r + 1))
        assert same_state(f.state(), wstate)
        f.reset()
        zero = f.state()
        assert not zero[0].any() and not zero[1].any() and not zero[2].any() and not zero[3].any()
        push_checked(f, q, x[:, :n] if r > 1 else x[0, :n], None, cap, True, per[0])
        assert same_state(f.state(), z0)
    assert_plants_found(q, per, where[:r])


def test_create_errors(hz, ctx):
    """rows 0 and 8193, other kinds, and one bound of each sort through the library (every bound's edge:
    tests/test_framesync_cpu.py against the same hz_framesync_plan.h)"""
    lib = importlib.import_module("go-sdr_amd._capi").lib
    out = C.c_void_p()

    def create(q, rows=1, kind=None):
        w, m = (C.c_uint64 * max(1, len(q.words)))(*q.words), (C.c_uint * max(1, len(q.maps)))(*q.maps)
        return lib.hzsdr_framesync_create(ctx._h, q.kind if kind is None else kind, q.B, q.W, q.mask, q.thr, len(q.words), w, m, q.P, q.diff, q.holdoff,
                                          rows, C.byref(out))

    inval = hz.ErrInvalidArgument.status
    assert create(cfg(), 0) == inval and create(cfg(), hz.FRAMESYNC_MAX_ROWS + 1) == inval
    assert create(cfg(), hz.FRAMESYNC_MAX_ROWS) == 0 and lib.hzsdr_framesync_free(out) == 0
    for kind in (-1, 0, hz.FMT_U8, hz.FMT_I16, 31, 33):
        assert create(cfg(), 1, kind) == hz.ErrSampleFormatUnknown.status, kind
    for bad in (cfg(W=0, words=[0], mask=1, thr=0), cfg(W=65, words=[0], mask=1, thr=0), cfg(P=0), cfg(P=8200), cfg(words=[]), cfg(words=[1] * 5),
                cfg(thr=32), cfg(mask=0, thr=0), cfg(mask=1 << 32, thr=0), cfg(B=2, cplx=True, W=31, words=[1]), cfg(B=2, cplx=True, P=167),
                cfg(B=2, cplx=True, diff=1), cfg(B=2), cfg(holdoff=0), cfg(holdoff=2 ** 31 + 1), cfg(diff=3), cfg(words=[1, 2], maps=[0, 2])):
        assert not ref.accepted(bad) and create(bad) == inval, vars(bad)
    for good in (cfg(W=1, words=[1], thr=0, P=1), cfg(W=64, words=[2 ** 64 - 1], P=8192, thr=63), cfg(B=2, cplx=True, W=2, words=[3], thr=1, P=2),
                 cfg(holdoff=2 ** 31), cfg(words=[1, 2, 3, 4], maps=[1, 0, 1, 0])):
        assert ref.accepted(good) and create(good) == 0 and lib.hzsdr_framesync_free(out) == 0, vars(good)
    with pytest.raises(hz.ErrInvalidArgument):
        ctx.frame_sync(hz.FMT_C64, 32, [1, 2], [0], 168)
    with bank_of(ctx, cfg(), 1) as f, pytest.raises(ValueError):
        f.push(dev(np.zeros(8, np.complex64)))


# ---- 14. the symbol-timing bank straight in, the chain ----------------------------------------------------

def frames_signal(q, nsym, seed, every=110):
    """QPSK symbols (b0 on Re, b1 on Im: bit 1 is +) that carry a frame -- the 32-bit word, 168 payload bits -- every
    `every` symbols from symbol 10 on, random dibits between -> (a complex (nsym,), [(first symbol of the word, payload)])"""
    bits = ref.random_bits(2 * nsym, seed)
    sent = []
    for k, at in enumerate(range(10, nsym - (q.W + q.P) // 2 - 1, every)):
        pay = ref.random_bits(q.P, 1000 * seed + k)
        ref.plant(bits, 2 * at, q.words[0], q.W, pay)
        sent.append((at, pay))
    v = bits.astype(np.float64) * 2.0 - 1.0
    return (v[0::2] + 1j * v[1::2]) / np.sqrt(2.0), sent


CHAIN_SPS, CHAIN_NOISE_DB = 5.0, -20.0
CHAIN_CASES = ((1, 0.0005, 0.3), (2, -0.001, 1.9), (3, 0.0015, 4.0))  # seed, carrier offset in cycles per sample, phase


def chain_inputs(q, carrier=True, cases=CHAIN_CASES):
    """the cases' rows at CHAIN_SPS samples per symbol with their noise, turned by their carriers unless not `carrier`"""
    rows, sent = [], []
    for seed, off, phase in cases:
        a, s = frames_signal(q, 1500, seed)
        x = symsync_ref.signal(a, CHAIN_SPS, 0.25 * (seed % 4), noise_db=CHAIN_NOISE_DB, seed=seed).astype(np.complex128)
        rows.append((x * np.exp(2j * np.pi * (off * np.arange(len(x)) + phase) * carrier)).astype(np.complex64))
        sent.append(s)
    n = min(len(r) for r in rows)
    return np.stack([r[:n] for r in rows]), sent


def chain_params(hz):
    return (np.array([*carrier_ref.gains(0.01), 0.0, -0.01, 0.01], np.float32), np.array([CHAIN_SPS, 0.01, *hz.loop_gains(CHAIN_SPS)], np.float32))


def test_the_symbol_timing_bank_straight_in(hz, ctx):
    """(symbols, counts) of SymbolSync.push go into the bank as they are -- the pitched block, the int32 counts, on the
    device, nothing read in between -- against the program over the same block and counts"""
    q = cfg(words=ref.rotated_words(WORD32, 32), maps=[0, 1, 2, 3], B=2, cplx=True)
    x, _ = chain_inputs(q, carrier=False)
    _, sp = chain_params(hz)
    with ctx.symbol_sync(hz.FMT_C64, sp, rows=3) as ts, bank_of(ctx, q, 3) as f:
        parts, res = [], []
        for part in cut(dev(x), [0, 2500, 2501, x.shape[1]]):
            s, cnt = ts.push(part)
            res.append(f.push(s, cnt, 4))
            parts.append((s, cnt))
        state = f.state()
    pushes = [(host(s), host(c).view(np.uint32)) for s, c in parts]
    ((per, wstate),) = ref.exact(BUILD, [(q, pushes, 4)])
    assert same_state(state, wstate) and np.array_equal(wstate[0], sum(c for _, c in pushes))
    for (fr, ps, inf, cnt), (wf, wp, wi, wc) in zip(res, per):
        assert np.array_equal(host(cnt).view(np.uint32), wc)
        for r in range(3):
            m = int(wc[r])
            assert np.array_equal(host(fr)[r, :m], wf[r, :m]) and np.array_equal(host(ps).view(np.uint64)[r, :m], wp[r, :m])
            assert np.array_equal(host(inf).view(np.uint32)[r, :m], wi[r, :m])
    assert sum(int(p[3].sum()) for p in per) >= 3


def test_the_chain_carrier_symbol_timing_frame_sync(hz, ctx):
    """QPSK rows with a carrier offset, frames behind a 32-bit word, ambiguity "rotate": the GPU chain's frames equal the
    chained host programs' exactly, and the host chain recovers every frame whose word starts at symbol CHAIN_A or later
    with zero bit errors (the module's header has the measurement)"""
    st = importlib.import_module("go-sdr_amd.stream")
    words, maps = hz.sync_hypotheses(WORD32, 32, 2, "rotate")
    q = cfg(words=words, maps=maps, B=2, cplx=True)
    x, sent = chain_inputs(q)
    cp, sp = chain_params(hz)
    ((derot, _, _),) = carrier_ref.exact(BUILD, [(carrier_ref.QPSK, cp, x)])
    ((sym, cnt, _, _),) = symsync_ref.exact(BUILD, [(sp, derot)])
    ((per, _),) = ref.exact(BUILD, [(q, [(sym, cnt)], 16)])
    want = [found(per, r) for r in range(3)]
    for r in range(3):
        payloads = {v[0] for v in want[r].values()}
        late = [(at, pay) for at, pay in sent[r] if at >= CHAIN_A]
        assert len(late) >= 8 and int(per[0][3][r]) <= 16
        for at, pay in late:
            assert bytes(np.packbits(pay)) in payloads, (r, at)
    with ctx.carrier_loop(hz.CARRIER_QPSK, cp, rows=3) as cr, ctx.symbol_sync(hz.FMT_C64, sp, rows=3) as ts, bank_of(ctx, q, 3) as f:
        blocks = cut(dev(x), [0, 3000, 3001, x.shape[1]])
        parts = list(st.frame_rows(st.symbol_rows(st.carrier_rows(blocks, cr), ts), f, cap=16))
    for r in range(3):
        got = {int(p): (bytes(fr), int(i)) for part in parts for fr, p, i in zip(*part[r])}
        assert got == want[r], r


# ---- 15. the other layers -----------------------------------------------------------------------------

def _run(exe):
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "go-sdr_amd") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    return subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)


def test_c_framesync_walkthrough(hz):
    """tests/c/test_framesync_abi.c compiled by gcc as C99 and run against libhzsdr_hip.so."""
    exe = os.path.join(BUILD, "test_framesync_abi")
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "test_framesync_abi.c"), "-L" + os.path.join(ROOT, "go-sdr_amd"),
                           "-lhzsdr_hip", "-lm", "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    p = _run(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "framesync-abi ok" in p.stdout


def test_cxx_framesync(hz):
    """tests/cxx/test_framesync.cpp (hzsdr::stream::FrameSync of go-sdr_amd/cxx/hzsdr.hpp) built with g++ and run."""
    exe = os.path.join(BUILD, "test_framesync_cxx")
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + ROOT, os.path.join(ROOT, "tests", "cxx", "test_framesync.cpp"),
                           "-L" + os.path.join(ROOT, "go-sdr_amd"), "-lhzsdr_hip", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    p = _run(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "framesync-cxx ok" in p.stdout


def test_frame_rows_over_a_reader(hz, hctx):
    """stream.frame_rows over a BufferReader with short reads finds the frames of one push of the whole stream; fed
    with blocks, or with (symbols, counts) pairs, it takes them as they are; a Reader of another format, or a real bank
    behind a Reader, is refused; more frames in a push than cap raises"""
    st = importlib.import_module("go-sdr_amd.stream")
    q = cfg(words=ref.rotated_words(WORD32, 32), maps=[0, 1, 2, 3], B=2, cplx=True)
    x, where = rows_with_plants(q, 1, 3000, 181, lambda r: (200, 2000, 4400))
    x = x[0]
    ((per, wstate),) = ref.exact(BUILD, [(q, [x], 8)])
    want = found(per, 0)
    assert_plants_found(q, per, where)
    with bank_of(hctx, q, 1) as f:
        parts = list(st.frame_rows(st.BufferReader(x, 48_000, max_read=777), f, block=1024))
        assert same_state(f.state(), wstate)
    got = {int(p): (bytes(fr), int(i)) for part in parts for fr, p, i in zip(*part[0])}
    assert len(parts) > 3 and got == want
    with bank_of(hctx, q, 1) as f:
        pairs = [(x[i:i + 1000], np.array([900], np.uint32)) for i in range(0, 3000, 1000)]
        list(st.frame_rows(pairs, f))
        assert f.positions()[0] == 2700
        with pytest.raises(st.ErrShortBuffer):
            list(st.frame_rows([x], f, cap=1))
    qr = cfg()
    with bank_of(hctx, qr, 1) as f, pytest.raises(hz.ErrSampleFormatMismatch):
        list(st.frame_rows(st.BufferReader(x, 48_000), f))
    u8 = np.zeros((64, 2), np.uint8)
    with bank_of(hctx, q, 1) as f, pytest.raises(hz.ErrSampleFormatMismatch):
        list(st.frame_rows(st.BufferReader(u8, 48_000), f))

"""The Reed-Solomon decoder bank (include/hzsdr_rs.h) on the GPU against the host program tests/host/rs_ref.cpp, which
tests/test_rs_cpu.py holds to the numpy restatement and to the exhaustive search: data bytes and info are compared
EXACTLY, the destinations are full of sentinels, and every byte that is not a decoded frame's data -- the bytes behind
I k in a slot, the slots behind a row's count, the row padding -- is checked.  Wherever it is provable (at most t errors
per codeword) the tests also assert that the reference returned what was planted, so that two wrong answers cannot
agree; beyond t the restatement decides between fail and miscorrection and the kernel must say the same."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import rs_ref as ref
from conftest import ROOT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BUILD = os.path.join(ROOT, "build")
SENT8, SENT32 = 0xA5, 0xA5A5A5A5
CODES = {"2of3": (0x11D, 3, 7, 2, 3), "5of6": (0x187, 112, 11, 5, 6), "3of255": (0x11D, 200, 254, 3, 255), "64of255": (0x187, 0, 1, 64, 255),
         "64of65": (0x11D, 1, 2, 64, 65), "ccsds": ref.CCSDS_223, "dvb": ref.DVB}
SMALL = (0x11D, 0, 1, 4, 20)
WORD32 = 0x1ACFFC1D


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


def bank_of(c, q, rows):
    args, kw = q.create_args()
    return c.reed_solomon(*args, rows=rows, **kw)


def strided(wide, shape, strides, device):
    if device:
        return torch.as_strided(wide, shape, strides)
    return np.lib.stride_tricks.as_strided(wide, shape, strides)


def decode_checked(c, q, frames, counts, device, want, pads=(0, 0, 0, 0), in_place=False):
    """frames (R, cap, F) through a new bank, input and output inside wider buffers with slot pitches F + pads[0] and
    I k + pads[1] and row pads pads[2], pads[3], against the program's (data, info): the decoded slots exactly, every
    other byte of the destinations still a sentinel (in place: still the input) -> (data, info) as decoded"""
    R, cap, F = frames.shape
    assert F == q.F
    ipitch, opitch = F + pads[0], q.IK + pads[1]
    if in_place:
        opitch = ipitch
    istride, ostride = cap * ipitch + pads[2], cap * opitch + (pads[2] if in_place else pads[3])
    wide_in = np.full((R, istride), 0x3C, np.uint8)
    for f in range(cap):
        wide_in[:, f * ipitch:f * ipitch + F] = frames[:, f]
    before = wide_in.copy()
    wide_out, info = np.full((R, ostride), SENT8, np.uint8), np.full((R, cap), SENT32, np.uint32)
    cin = None if counts is None else np.asarray(counts, np.uint32)
    if device:
        wide_in, wide_out, info = dev(wide_in), dev(wide_out), dev(info.view(np.int32))
        cin = None if cin is None else dev(cin.view(np.int32))
    if in_place:
        wide_out = wide_in
    with bank_of(c, q, R) as v:
        assert v.sizes() == (q.k, q.t, q.F, q.IK)
        vin = strided(wide_in, (R, cap, F), (istride, ipitch, 1), device)
        vout = strided(wide_out, (R, cap, F if in_place else q.IK), (ostride, opitch, 1), device)
        v.decode(vin, cin, cap, out=(vout, info))
        if device:
            torch.cuda.synchronize()
    wd, wi = want
    gw, gi = host(wide_out), host(info).view(np.uint32)
    rest = before if in_place else np.full_like(gw, SENT8)
    got = np.zeros((R, cap, q.IK), np.uint8)
    for r in range(R):
        m = cap if counts is None else min(int(counts[r]), cap)
        expect = rest[r].copy()
        for f in range(m):
            expect[f * opitch:f * opitch + q.IK] = wd[r, f]
            got[r, f] = gw[r, f * opitch:f * opitch + q.IK]
        assert np.array_equal(gw[r], expect), (q.code, q.I, r)
        assert np.array_equal(gi[r, :m], wi[r, :m]) and (gi[r, m:] == SENT32).all(), (q.code, q.I, r, gi[r], wi[r])
    if not in_place:
        assert np.array_equal(host(wide_in), before)
    return got, gi


def edge_frames(q, seed):
    """[(frame, errors planted per codeword or None)]: 0, 1, t - 1, t, t + 1 and nroots errors at random places; single
    errors at the first symbol, the last data symbol, the first and the last parity symbol with the values 0x01 and
    0xFF; t errors into the all-zero codeword; an all-0xFF frame; a frame of random bytes"""
    out = []
    for j, errs in enumerate([0, 1, q.t - 1, q.t, q.t + 1, q.nroots]):
        frame, _ = ref.clean_frame(q, seed + j)
        for i in range(q.I if errs > 0 else 0):
            where = np.argsort(ref.splitmix64(seed * 64 + 8 * j + i, q.n), kind="stable")[:errs]
            frame = ref.hurt(q, frame, i, where, ref.random_bytes(errs, seed + j + i) | 1)
        out.append((frame, max(errs, 0)))
    for j, p in enumerate([0, q.k - 1, q.k, q.n - 1]):
        frame, _ = ref.clean_frame(q, seed + 10 + j)
        for i in range(q.I):
            frame = ref.hurt(q, frame, i, [p], [0x01 if (i + j) % 2 else 0xFF])
        out.append((frame, 1))
    zero = q.unprepare(np.zeros(q.F, np.uint8))
    for i in range(q.I):
        zero = ref.hurt(q, zero, i, np.argsort(ref.splitmix64(seed + i, q.n), kind="stable")[:q.t], [0xFF] * q.t)
    out.append((zero, q.t))
    out.append((np.full(q.F, 0xFF, np.uint8), None))
    out.append((ref.random_bytes(q.F, seed), None))
    return out


# ---- 1. every code, every error count, every edge position ---------------------------------------------

@pytest.mark.parametrize("name,I,pads", [("2of3", 1, (0, 0, 0, 0)), ("2of3", 8, (1, 2, 3, 5)), ("5of6", 3, (0, 0, 0, 0)), ("5of6", 2, (5, 1, 0, 2)),
                                         ("3of255", 2, (0, 0, 1, 1)), ("64of255", 1, (0, 0, 0, 0)), ("64of255", 8, (8, 0, 0, 0)), ("64of65", 3, (0, 3, 0, 0)),
                                         ("ccsds", 1, (1, 1, 1, 1)), ("ccsds", 8, (0, 0, 0, 0)), ("dvb", 1, (0, 0, 0, 0)), ("dvb", 2, (4, 4, 4, 4))])
def test_codes_errors_and_positions(ctx, name, I, pads):
    """the codes of the edges (nroots 2 and 64, n 3 and 255, nroots = n - 1, an odd nroots) and the shipped ones, I = 1, 2,
    3 and 8, pitches at the frame bytes and above: frames with 0, 1, t - 1, t, t + 1 and nroots errors per codeword, errors
    at the first symbol, the last data symbol and the first and last parity symbols, of value 0x01 and 0xFF, the all-zero
    codeword, an all-0xFF frame; R = 2, cap = 7 with counts that leave slots out"""
    q = ref.Config(CODES[name], I)
    made = edge_frames(q, 1 + len(name) + I)
    assert len(made) == 13
    frames = np.stack([m[0] for m in made] + [made[0][0]]).reshape(2, 7, q.F)
    counts = np.array([7, 6], np.uint32)
    (want,) = ref.exact(BUILD, [(q, frames, counts)])
    decode_checked(ctx, q, frames, counts, True, want, pads)
    for s, (_, errs) in enumerate(made):
        if errs is not None and errs <= q.t:
            assert int(want[1][s // 7, s % 7]) == (q.I * errs | 1 << 31), (name, s)
        elif errs == q.t + 1 and q.t >= 8:
            assert int(want[1][s // 7, s % 7]) == q.I << 16, (name, s)  # (a miscorrection of t + 1 random errors is out of reach here)


@pytest.mark.parametrize("code", [ref.DVB, (0x187, 112, 11, 8, 40), (0x11D, 0, 1, 3, 4)])
def test_a_root_in_the_shortened_region_fails(ctx, code):
    """a word whose syndromes are those of ONE error at a position the shortened code does not have (the parity of the
    full-length codeword of that single symbol): the locator has degree 1 <= t and its root lies outside the n valid
    positions.  No shortened codeword is within t of it (the difference would be a full-length codeword of weight at
    most t + 1 <= nroots), so it FAILS and passes through"""
    full = (*code[:4], 255)
    q = ref.Config(code, 2)
    frames = []
    for d in (q.n, (q.n + 254) // 2, 254):  # the degree of the symbol that is not there: n ... 254
        data = np.zeros(255 - q.nroots, np.uint8)
        data[254 - d] = 0x5A
        parity = ref.encode(full, data)[-q.nroots:]
        word = np.zeros(q.n, np.uint8)
        word[-q.nroots:] = parity
        assert np.array_equal(ref.syndromes(code, word), ref.syndromes(full, np.concatenate([data, np.zeros(q.nroots, np.uint8)])))
        frame, _ = ref.clean_frame(q, d)
        sym = q.prepare(frame)
        sym[1::2] ^= word
        frames.append(q.unprepare(sym))
    frames = np.stack(frames)[None]
    (want,) = ref.exact(BUILD, [(q, frames, None)])
    assert (want[1] == (1 << 16)).all()  # codeword 0 clean, codeword 1 failed
    got, _ = decode_checked(ctx, q, frames, None, True, want)
    assert np.array_equal(got[0, :, 1::2], frames[0, :, 1:q.IK:2])  # passed through unchanged


# ---- 2. rows, caps, counts, both memory spaces -----------------------------------------------------------

@pytest.fixture(scope="module")
def row_cases():
    """one block of hurt frames for all the row tests, and the program's answer to it: (q, frames (1025, 3, F), data, info)"""
    q = ref.Config(SMALL, 2, scramble=ref.random_bytes(7, 3))
    base = []
    for j in range(64):
        frame, _ = ref.clean_frame(q, 900 + j)
        for i in range(q.I):
            errs = (j + i) % (q.t + 2)
            frame = ref.hurt(q, frame, i, np.argsort(ref.splitmix64(j * 2 + i, q.n), kind="stable")[:errs], ref.random_bytes(errs, j) | 1)
        base.append(frame)
    base = np.stack(base)
    frames = base[(np.arange(1025 * 3) * 7) % 64].reshape(1025, 3, q.F)
    ((data, info),) = ref.exact(BUILD, [(q, frames, None)])
    return q, frames, data, info


@pytest.mark.parametrize("space", ["device", "host"])
@pytest.mark.parametrize("R", [1, 2, 63, 64, 65, 1025])
def test_rows_caps_and_counts(ctx, hctx, row_cases, space, R):
    """R = 1, 2, 63, 64, 65, 1025; cap = 1 and 3; counts of 0, below cap, at cap and above cap, and null counts; sentinels
    behind I k, behind a count and in the row padding"""
    q, frames, data, info = row_cases
    c, device = (ctx, True) if space == "device" else (hctx, False)
    for cap, pads in ((1, (0, 0, 0, 0)), (3, (2, 3, 5, 7))):
        counts = np.array([(0, 1, cap, cap + 2, 2)[r % 5] for r in range(R)], np.uint32)
        for cnt in (counts, None):
            decode_checked(c, q, frames[:R, :cap], cnt, device, (data[:R, :cap], info[:R, :cap]), pads)


@pytest.mark.parametrize("space", ["device", "host"])
def test_in_place_equals_out_of_place(ctx, hctx, row_cases, space):
    q, frames, data, info = row_cases
    c, device = (ctx, True) if space == "device" else (hctx, False)
    counts = np.array([3, 0, 2, 5, 1], np.uint32)
    for R, pads in ((1, (0, 0, 0, 0)), (5, (0, 0, 0, 0)), (5, (3, 0, 9, 0))):
        want = (data[:R], info[:R])
        a = decode_checked(c, q, frames[:R], counts[:R], device, want, pads, in_place=True)
        b = decode_checked(c, q, frames[:R], counts[:R], device, want, pads)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_a_frame_does_not_depend_on_its_place_or_its_neighbours(ctx, row_cases):
    """the same frames permuted over the slots, and with every other slot replaced by garbage: each frame's bytes and info
    follow it"""
    q, frames, data, info = row_cases
    R, cap = 9, 3
    flat, fd, fi = frames[:R].reshape(-1, q.F), data[:R].reshape(-1, q.IK), info[:R].reshape(-1)
    perm = np.argsort(ref.splitmix64(77, R * cap), kind="stable")
    got, gi = decode_checked(ctx, q, flat[perm].reshape(R, cap, q.F), None, True, (fd[perm].reshape(R, cap, -1), fi[perm].reshape(R, cap)))
    assert np.array_equal(got.reshape(-1, q.IK)[np.argsort(perm)], fd)
    junk = flat.copy()
    junk[1::2] = ref.random_bytes(junk[1::2].size, 5).reshape(junk[1::2].shape)
    ((jd, ji),) = ref.exact(BUILD, [(q, junk.reshape(R, cap, q.F), None)])
    got, gi = decode_checked(ctx, q, junk.reshape(R, cap, q.F), None, True, (jd, ji))
    assert np.array_equal(got.reshape(-1, q.IK)[0::2], fd[0::2]) and np.array_equal(gi.reshape(-1)[0::2], fi[0::2])


# ---- 3. scrambling and maps --------------------------------------------------------------------------------

@pytest.mark.parametrize("slen", [1, 255, "F+1"])
def test_scramble_lengths(ctx, slen):
    q0 = ref.Config(ref.CCSDS_239, 3)
    slen = q0.F + 1 if slen == "F+1" else slen
    perm = np.argsort(ref.splitmix64(9, 256), kind="stable").astype(np.uint8)
    back = np.argsort(perm).astype(np.uint8)
    q = ref.Config(ref.CCSDS_239, 3, in_map=perm, out_map=back, scramble=ref.random_bytes(slen, slen) | 0x80)
    made = edge_frames(q, slen)
    frames = np.stack([m[0] for m in made[:6]])[None]
    (want,) = ref.exact(BUILD, [(q, frames, None)])
    decode_checked(ctx, q, frames, None, True, want, (1, 0, 0, 0))
    assert [int(w) for w in want[1][0, :4]] == [e * 3 | 1 << 31 for e in (0, 1, q.t - 1, q.t)]


@pytest.mark.parametrize("space", ["device", "host"])
def test_ccsds_dual_basis_and_randomiser_end_to_end(hz, ctx, hctx, space):
    """a CCSDS transfer frame as a spacecraft makes it: data in the dual basis, encoded there (conventional symbols inside
    the encoder), I = 4 interleaved, randomised; 16 symbol errors per codeword come back corrected, in the dual basis"""
    to_dual, from_dual = hz.ccsds_dual_basis()
    I, code = 4, hz.CCSDS_RS_255_223
    data = ref.random_bytes(I * 223, 21).reshape(I, 223)                       # as the user sees it: dual basis
    words = to_dual[hz.rs_encode(code, from_dual[data])]                       # the codewords on the link, dual basis
    sent = hz.interleave_codewords(words) ^ hz.ccsds_randomizer(I * 255)
    hurt_ = sent.copy()
    where = np.argsort(ref.splitmix64(4, I * 255), kind="stable")[:16]         # 16 bytes of the frame: at most 16 per codeword
    hurt_[where] ^= 0xFF
    q = ref.Config(code, I, in_map=from_dual, out_map=to_dual, scramble=hz.ccsds_randomizer(255))
    frames = np.stack([sent, hurt_])[None]
    (want,) = ref.exact(BUILD, [(q, frames, None)])
    assert [int(w) for w in want[1][0]] == [1 << 31, 16 | 1 << 31]
    assert np.array_equal(want[0][0, 1], hz.interleave_codewords(data)) and np.array_equal(want[0][0, 0], want[0][0, 1])
    c, device = (ctx, True) if space == "device" else (hctx, False)
    decode_checked(c, q, frames, None, device, want, (0, 1, 0, 0))
    with c.reed_solomon(code, I, from_dual, to_dual, hz.ccsds_randomizer(255)) as rs:
        x = dev(frames[0]) if device else frames[0]
        clean, info = rs.decode(x)
        (d, E, nfail, ok), = rs.ragged(clean, info)
        assert np.array_equal(d, want[0][0]) and E.tolist() == [0, 16] and nfail.tolist() == [0, 0] and ok.all()
        assert rs.plan() == (4, 1280 + 1024 + 4 * 192 + 16, 8, 65536)


# ---- 4. refusals -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", [1, 3])
def test_refused_calls_leave_the_outputs(hz, ctx, R):
    lib = importlib.import_module("go-sdr_amd._capi").lib
    q = ref.Config(SMALL, 2)
    cap, F, IK = 2, q.F, q.IK
    frames = np.stack([ref.clean_frame(q, s)[0] for s in range(R * cap)]).reshape(R, cap, F)
    x = dev(frames)
    out, info = torch.full((R, cap * F), SENT8, dtype=torch.uint8, device="cuda"), torch.full((R, cap), 7, dtype=torch.int32, device="cuda")
    with bank_of(ctx, q, R) as v:
        call = lambda *a: ctx._ck(lib.hzsdr_rs_decode(v._h, *a))
        i, o, p = x.data_ptr(), out.data_ptr(), info.data_ptr()
        good = (i, cap * F, F, None, cap, o, cap * F, IK, p)

        def but(**kw):
            names = ("i", "istride", "ipitch", "counts", "cap", "o", "ostride", "opitch", "p")
            return tuple(kw.get(n, g) for n, g in zip(names, good))
        if R > 1:
            with pytest.raises(hz.ErrDstTooSmall):
                call(*but(ostride=cap * IK - 1))
            with pytest.raises(hz.ErrInvalidArgument):
                call(*but(istride=cap * F - 1))
            with pytest.raises(hz.ErrInvalidArgument):  # in place with other strides
                call(*but(o=i, ostride=cap * F + 1, opitch=F))
        for bad in (but(i=None), but(o=None), but(p=None), but(cap=0), but(cap=hz.RS_MAX_FRAMES // R + 1), but(ipitch=F - 1), but(opitch=IK - 1),
                    but(o=i, ostride=cap * F, opitch=F - 1), but(o=i + 1, ostride=cap * F, opitch=F), but(i=o + (R - 1) * cap * F + cap * IK - 1),
                    but(o=i + (R - 1) * cap * F + cap * F - 1)):
            with pytest.raises(hz.ErrInvalidArgument):
                call(*bad)
        assert lib.hzsdr_rs_decode(None, *good) == hz.ErrInvalidArgument.status
        torch.cuda.synchronize()
        assert (out == SENT8).all() and (info == 7).all() and np.array_equal(host(x), frames)
        with pytest.raises(ValueError):
            v.decode(dev(np.zeros((R, cap, F - 1), np.uint8)))
        with pytest.raises(ValueError):
            v.decode(dev(np.zeros((R, cap, F), np.float32)))
        call(*good)
        torch.cuda.synchronize()
        ((wd, wi),) = ref.exact(BUILD, [(q, frames, None)])
        assert np.array_equal(host(out)[:, :cap * IK].reshape(R, cap, IK), wd) and np.array_equal(host(info).view(np.uint32), wi) and (wi == 1 << 31).all()
        assert (host(out)[:, cap * IK:] == SENT8).all()  # (the row pitch is cap * F: the rest of a row stays)


def test_create_errors(hz, ctx):
    """rows 0 and 8193, a scramble length without a sequence, and one bound of each sort through the library (every bound's
    edge: tests/test_rs_cpu.py and tests/host/rs_plan.cpp against the same hz_rs_plan.h)"""
    lib = importlib.import_module("go-sdr_amd._capi").lib
    out = C.c_void_p()
    scr = (C.c_uint8 * 2041)()

    def create(code=ref.CCSDS_223, I=1, rows=1, slen=0, s=None):
        return lib.hzsdr_rs_create(ctx._h, *code, I, None, None, s, slen, rows, C.byref(out))

    inval = hz.ErrInvalidArgument.status
    assert create(rows=0) == inval and create(rows=hz.RS_MAX_ROWS + 1) == inval and create(slen=4) == inval and create(slen=2041, s=scr) == inval
    assert create(rows=hz.RS_MAX_ROWS, slen=2040, s=scr, I=8) == 0 and lib.hzsdr_rs_free(out) == 0
    sets = [(0x11B, 0, 1, 4, 20), (0x87, 0, 1, 4, 20), (0x31D, 0, 1, 4, 20), (0x11D, 255, 1, 4, 20), (0x11D, 0, 0, 4, 20), (0x11D, 0, 3, 4, 20), (0x11D, 0, 85, 4, 20),
            (0x11D, 0, 255, 4, 20), (0x11D, 0, 1, 1, 20), (0x11D, 0, 1, 65, 255), (0x11D, 0, 1, 4, 4), (0x11D, 0, 1, 4, 256)]
    for bad, (ok, _, _) in zip(sets, ref.check(BUILD, [(*s, 1, 0) for s in sets])):
        assert not ok and create(bad) == inval, bad
    assert create(I=0) == inval and create(I=9) == inval
    for code in CODES.values():
        assert create(code, 8) == 0 and lib.hzsdr_rs_free(out) == 0
    with pytest.raises(hz.ErrInvalidArgument):
        ctx.reed_solomon(ref.CCSDS_223, rows=0)
    with pytest.raises(hz.ErrInvalidArgument):
        ctx.reed_solomon(ref.CCSDS_223, in_map=np.zeros(255, np.uint8))


# ---- 5. the chain --------------------------------------------------------------------------------------------

def test_the_chain_to_corrected_data(hz, ctx):
    """rs_encode -> randomise -> conv_encode (CCSDS_K7) -> symbols with a burst of flipped bits -> frame sync -> Viterbi
    -> Reed-Solomon, all in a DEVICE context through stream.corrected_frames: a shortened code, n = 40, k = 32, I = 2, so
    that D = 640 bits.  The burst of 40 inverted channel bits is more than the inner code corrects: the Viterbi decoder
    hands on a frame with a run of wrong bytes, the outer code takes them out: the data comes back and E is not zero.
    (The full CCSDS size that fits the Viterbi bank's 8192 received positions is 255/223 at I = 2: N = 2 (8 * 510 + 6) =
    8172.)"""
    st = importlib.import_module("go-sdr_amd.stream")
    code, I = (0x187, 112, 11, 8, 40), 2
    K, gens, inv = hz.CCSDS_K7
    D = 8 * I * code[4]
    N = 2 * (D + K - 1)
    rows, nframes = 2, 3
    sym = np.zeros((rows, 200 + nframes * (32 + N + 50)), np.float32)
    sym[:] = (ref.splitmix64(1, sym.size) >> np.uint64(63)).astype(np.float32).reshape(sym.shape) * 2 - 1
    sent = np.zeros((rows, nframes, I * (code[4] - code[3])), np.uint8)
    word_bits = np.array([(WORD32 >> (31 - b)) & 1 for b in range(32)], np.uint8)
    for r in range(rows):
        for f in range(nframes):
            data = ref.random_bytes(I * 32, 50 + r * nframes + f).reshape(I, 32)
            sent[r, f] = hz.interleave_codewords(data)
            frame = hz.interleave_codewords(hz.rs_encode(code, data)) ^ hz.ccsds_randomizer(I * code[4])
            coded = hz.conv_encode(np.unpackbits(frame), K, gens, inv)
            assert coded.size == N
            coded[300 + 100 * f:340 + 100 * f] ^= 1  # the burst
            at = 100 + f * (32 + N + 50) + 7 * r
            sym[r, at:at + 32 + N] = np.concatenate([word_bits, coded]).astype(np.float32) * 2 - 1
    with ctx.frame_sync(hz.SYMSYNC_REAL_F32, 32, [WORD32], [0], N, rows=rows) as fs, \
            ctx.viterbi(hz.VITERBI_BITS, K, gens, D, inv=inv, rows=rows) as vd, \
            ctx.reed_solomon(code, I, scramble=hz.ccsds_randomizer(255), rows=rows) as rs:
        x = dev(sym)
        cut = sym.shape[1] // 2
        parts = list(st.corrected_frames([x[:, :cut], x[:, cut:]], fs, vd, rs, cap=4))
        with ctx.reed_solomon(code, 1, rows=rows) as other, pytest.raises(ValueError):
            list(st.corrected_frames([], fs, vd, other))
    for r in range(rows):
        got = [(d, int(e), int(nf), bool(ok), int(m)) for part in parts for d, e, nf, ok, m in zip(part[r][0], part[r][5], part[r][6], part[r][7], part[r][3])]
        assert len(got) == nframes, (r, len(got))
        for f, (d, e, nf, ok, metric) in enumerate(got):
            print("row", r, "frame", f, "viterbi metric", metric, "E", e, "nfail", nf)
            assert np.array_equal(d, sent[r, f]) and ok and nf == 0 and 0 < e <= I * 4, (r, f, e, nf)


# ---- 6. the other layers ---------------------------------------------------------------------------------

def _run(exe):
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "go-sdr_amd") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    return subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)


def test_c_rs_walkthrough(hz):
    """tests/c/test_rs_abi.c compiled by gcc as C99 and run against libhzsdr_hip.so."""
    exe = os.path.join(BUILD, "test_rs_abi")
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "test_rs_abi.c"), "-L" + os.path.join(ROOT, "go-sdr_amd"),
                           "-lhzsdr_hip", "-lm", "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    p = _run(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "rs-abi ok" in p.stdout


def test_cxx_rs(hz):
    """tests/cxx/test_rs.cpp (hzsdr::stream::ReedSolomon) built with g++ -Werror and run."""
    exe = os.path.join(BUILD, "test_rs_cxx")
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + ROOT, os.path.join(ROOT, "tests", "cxx", "test_rs.cpp"),
                           "-L" + os.path.join(ROOT, "go-sdr_amd"), "-lhzsdr_hip", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    p = _run(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "rs-cxx ok" in p.stdout

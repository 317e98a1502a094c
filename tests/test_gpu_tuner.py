"""The tuner bank (include/hzsdr_tuner.h) on the GPU: every format and shape BIT FOR BIT against the outputs of
tests/host/tuner_ref.cpp (the host program over the header the kernel evaluates, fed the operands the library reads out)
and, within the bound derived in tests/tuner_ref.py, against the independent float64 restatement; the two cases that
settle the order of the terms inside the float32 MFMA; bit for bit across cuts, memory spaces, pitches, bank sizes,
permutations and runs; w = 0 against the resampler; retune; a tone; in front of the demodulator and behind a Reader;
errors and state; the C++ layer."""
import ctypes as C
import importlib
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import tuner_ref as ref
from conftest import ROOT
from util import FMT, splitmix64

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BUILD = os.path.join(ROOT, "build")


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


def bits(t):
    t = t.detach().cpu() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return torch.view_as_real(t.contiguous()).contiguous().view(torch.int32) if t.is_complex() else t.contiguous().view(torch.int32)


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


def run(bank, x, cuts=None, flush=True, check=None):
    """push x whole or cut at `cuts`, then flush; the pushes' outputs and the flush's, concatenated along the columns"""
    n = x.shape[0]
    if cuts is None:
        cuts = [0, n]
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        out.append(bank.push(x[a:b]))
        if check:
            check(b)
    if flush:
        out.append(bank.flush())
    if isinstance(out[0], torch.Tensor):
        torch.cuda.synchronize()
        return torch.cat(out, dim=-1)
    return np.concatenate(out, axis=-1)


def operands(bank):
    """the modulated taps of every tuner and the three tables, as the library reads them out"""
    hz = importlib.import_module("go-sdr_amd")
    g = np.stack([bank.readout(hz.TUNER_READ_TAPS, k) for k in range(bank.tuners)])
    return g, bank.readout(hz.TUNER_READ_T2), bank.readout(hz.TUNER_READ_T1), bank.readout(hz.TUNER_READ_T0)


def first_difference(got, want):
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    bad = np.argwhere(g != w)
    row, col = (int(v) for v in bad[0])
    return f"{bad.shape[0]} of {w.size} components differ, the first in row {row}, m = {col // 2}: {got[row, col // 2]!r} for {want[row, col // 2]!r}"


def stream_length(bank):
    """about three output tiles and an odd remainder"""
    tile = bank.plan()[0]
    return 3 * tile * bank.down + 37


# ---- 1. bit for bit against the host program, and within the bound of float64 ------------------------

@pytest.mark.parametrize("fmt", ["c64", "u8", "i8", "i16"])
@pytest.mark.parametrize("k,q,down", ref.SHAPES)
def test_streams_exact_and_float64(hz, ctx, k, q, down, fmt):
    words, h = ref.words_for(k, seed=q), ref.taps_of(q)
    with ctx.tuner_bank(FMT[fmt], words, h, down) as bank:
        tile, rows, form = bank.plan()
        assert tile in (32, 64, 128) and tile * rows == 4096 and bool(form & hz.TUNER_FORM_TRANSPOSED) == (down > 1)
        assert bool(form & hz.TUNER_FORM_CHUNKED) == ((q, down) in ((1024, 256), (1023, 255)))
        n = stream_length(bank)
        x = dev(white(fmt, n, seed=q * 131 + down))
        n1 = n // 2 + 1
        assert bank.outputs_for(n1) == ref.outputs_after(n1, down)

        def check(done):
            assert bank.pending() == (done, ref.outputs_after(done, down), ref.total_outputs(done, q, down) - ref.outputs_after(done, down))

        got = run(bank, x, [0, n1, n], check=check).cpu().numpy().reshape(k, -1)
        assert bank.pending() == (0, 0, 0)
        ops = operands(bank)
    xc = as_c64(ctx, x).cpu().numpy()
    ((want, _, _),) = ref.exact(BUILD, [(words, down, h, xc, ops)])
    what = f"K={k} Q={q} D={down} {fmt} T={tile} n={n}"
    assert got.shape == want.shape == (k, ref.total_outputs(n, q, down))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{what}: {first_difference(got, want)}"
    err, bnd = np.abs(got.astype(np.complex128) - ref.tune(words, h, xc, down)), ref.bound(h, xc)
    row, m = np.unravel_index(int(np.argmax(err)), err.shape)
    print(f"{what}: max err {err.max():.3e} at tuner {row}, m = {m}; bound {bnd:.3e}")
    assert err.max() <= bnd, f"{what}: tuner {row} output {m}: {err[row, m]:.3e} > {bnd:.3e}"


# ---- 2. the order of the terms inside the MFMA --------------------------------------------------------

def rn32(fr):
    """a Fraction rounded to the nearest float32, ties to even (normal range)"""
    if fr == 0:
        return np.float32(0.0)
    sign, fr = (-1.0 if fr < 0 else 1.0), abs(fr)
    e = fr.numerator.bit_length() - fr.denominator.bit_length()
    if Fraction(2) ** e > fr:
        e -= 1
    scaled = fr / Fraction(2) ** (e - 23)  # in [2^23, 2^24)
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    return np.float32(sign * n * 2.0 ** (e - 23))


def chain(terms, fused=True):
    """terms: [(a, b)] float32 pairs -> the float32 sum of the products from +0: fused steps, or every product and sum
    rounded by itself"""
    acc = Fraction(0)
    for a, b in terms:
        prod = Fraction(float(a)) * Fraction(float(b))
        acc = Fraction(float(rn32(acc + prod))) if fused else Fraction(float(rn32(acc + Fraction(float(rn32(prod))))))
    return np.float32(float(acc))


def terms_of(g, a):
    """the contract's terms of one output, q ascending: (re terms, im terms) of g[q] and a[q] = c(x[m D - q])"""
    re, im = [], []
    for gq, aq in zip(g, a):
        gr, gi, ar, ai = np.float32(gq.real), np.float32(gq.imag), np.float32(aq.real), np.float32(aq.imag)
        re += [(gr, ar), (-gi, ai)]
        im += [(gi, ar), (gr, ai)]
    return re, im


@pytest.mark.parametrize("q", [2, 4])
def test_mfma_term_order(hz, ctx, q):
    """K = 1, D = 1, w = 2^29 (an eighth turn per sample, so that G has both components from q = 1 on), Q = 2: the whole
    sum is ONE 16x16x4 step; Q = 4: two steps chained through C.  The outputs looked at are m = 8 j, where the phase word
    is 0 and the rotator is exactly 1, so that y is the sum itself.  Their samples are drawn from magnitudes that cancel
    (2^24, 2^24 + 2, 2^27, 1, 3, 1/3, 2^12 + 1; the products with G[1] = RN(sqrt(1/2)) are inexact in float32), and only
    outputs are kept where the contract's chain, emulated in exact rational arithmetic, differs from the reversed order,
    from the unfused chain, from the pairwise tree AND from the two halves exchanged: there any other order or an unfused
    product shows, in whole units of the last place or more.  The device must give the contract's chain there."""
    w, h = np.array([1 << 29], np.uint32), np.ones(q, np.float32)
    mags = np.array([2.0 ** 24, 2.0 ** 24 + 2, 2.0 ** 27, 1.0, 3.0, np.float32(1.0) / np.float32(3.0), 2.0 ** 12 + 1], np.float32)
    rng = np.random.default_rng(2026 + q)
    outs = 400
    x = np.zeros(8 * outs + 1, np.complex64)
    for j in range(1, outs + 1):
        for t in range(q):
            v = mags[rng.integers(0, len(mags), 2)] * rng.choice(np.array([-1.0, 1.0], np.float32), 2)
            x[8 * j - t] = complex(v[0], v[1])
    with ctx.tuner_bank(hz.FMT_C64, w, h, 1) as bank:
        got = run(bank, dev(x)).cpu().numpy().reshape(-1)
        ops = operands(bank)
    ((want, _, _),) = ref.exact(BUILD, [(w, 1, h, x, ops)])
    g = ops[0][0]
    assert g[1].real != 0 and g[1].imag != 0
    kept, shown = 0, 0
    for j in range(1, outs + 1):
        m = 8 * j
        re, im = terms_of(g[:q], [x[m - t] for t in range(q)])
        for terms, have, ref_value in ((re, got[m].real, want[0, m].real), (im, got[m].imag, want[0, m].imag)):
            contract = chain(terms)
            assert contract == ref_value, "the emulation and the host program disagree: the test itself is wrong"
            half = len(terms) // 2
            others = [chain(terms[::-1]), chain(terms, fused=False),
                      np.float32(chain(terms[:half]) + chain(terms[half:])), chain(terms[half:] + terms[:half])]
            if any(o == contract for o in others):
                continue
            kept += 1
            if have != contract and shown < 5:
                shown += 1
                print(f"m = {m}: device {have!r}, contract {contract!r}; reversed {others[0]!r}, unfused {others[1]!r}, tree {others[2]!r}, "
                      f"halves swapped {others[3]!r}; terms {[(float(a), float(b)) for a, b in terms]}")
            assert shown or have == contract
    assert kept >= 8, f"only {kept} outputs tell the orders apart"
    assert not shown, "the MFMA's sum is not the k-ordered chain of fused steps"
    assert np.array_equal(got.view(np.uint32), want[0].view(np.uint32))


# ---- 3. cuts ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,q,down,fmt", [(3, 7, 3, "c64"), (8, 64, 5, "u8"), (5, 1024, 256, "i16"), (2, 33, 1, "i8"), (17, 129, 16, "u8")])
def test_cuts_bit_identical(hz, ctx, k, q, down, fmt):
    bank = ctx.tuner_bank(FMT[fmt], ref.words_for(k, seed=3), ref.taps_of(q), down)
    tile = bank.plan()[0]
    n = 2 * tile * down + 37
    x = dev(white(fmt, n, seed=n + q))
    one = run(bank, x)
    assert one.shape == (k, ref.total_outputs(n, q, down))
    edge = tile * down  # the samples after which one tile's outputs are written

    def check(done):
        assert bank.pending() == (done, ref.outputs_after(done, down), ref.total_outputs(done, q, down) - ref.outputs_after(done, down))
        assert bank.outputs_for(5) == ref.outputs_after(done + 5, down) - ref.outputs_after(done, down)

    inside = max(1, (q - 1) // 2)  # a cut inside the first Q - 1 samples
    for cuts in ([0, 1, n], [0, inside, n], [0, down - 1, down, down + 1, n] if down > 1 else [0, 2, n], [0, edge - 1, n], [0, edge, n],
                 [0, edge + 1, n], [0, 2 * edge - 1, 2 * edge, 2 * edge + 1, n], [0, 0, 3, 3, edge, edge, n, n]):
        assert same(run(bank, x, cuts, check=check), one), f"cuts {cuts}"
    # pushes of one sample, through the held samples and across output boundaries
    small = x[:min(n, 2 * q + 3 * down + 5, 400)]
    want = run(bank, small)
    got = run(bank, small, list(range(small.shape[0] + 1)), check=check)
    assert same(got, want) and got.shape[-1] == ref.total_outputs(small.shape[0], q, down)
    bank.close()


# ---- 4. memory space, pitch, bank size, order, run -------------------------------------------------

@pytest.fixture(scope="module")
def seventeen(hz, ctx):
    """the K = 17 bank's whole stream, computed once: (words, h, down, x on the host, rows on the device)"""
    k, q, down = 17, 129, 16
    words, h = ref.words_for(k, seed=q), ref.taps_of(q)
    with ctx.tuner_bank(hz.FMT_U8, words, h, down) as bank:
        x = white("u8", stream_length(bank), seed=17)
        rows = run(bank, dev(x))
    return words, h, down, x, rows


def test_host_context_and_pitch(hz, ctx, hctx, seventeen):
    """two output pitches on the device and on the host (pinned and not), the sentinels behind `written` and in the
    pitch gap untouched; HOST results bit-equal to DEVICE ones"""
    words, h, down, x, rows = seventeen
    k, n, q = len(words), x.shape[0], len(h)
    n1 = n // 3
    counts = [ref.outputs_after(n1, down), ref.outputs_after(n, down) - ref.outputs_after(n1, down),
              ref.total_outputs(n, q, down) - ref.outputs_after(n, down)]
    total = sum(counts)
    assert rows.shape == (k, total)
    for pad in (7, 64):
        out = torch.full((k, total + pad), complex(float("nan"), float("nan")), dtype=torch.complex64, device="cuda")
        with ctx.tuner_bank(hz.FMT_U8, words, h, down) as bank:
            dx, done = dev(x), 0
            for part, c in zip((dx[:n1], dx[n1:], None), counts):
                w = bank.push(part, out=out[:, done:]) if part is not None else bank.flush(out=out[:, done:])
                assert w.shape == (k, c)
                torch.cuda.synchronize()
                assert torch.isnan(out[:, done + c:].real).all(), "columns behind the outputs written were touched"
                done += c
        assert same(out[:, :total], rows)
    pinned = hctx.pinned_samples(hz.FMT_C64, k * (total + 7))[:k * (total + 7)].reshape(k, total + 7)
    with hctx.tuner_bank(hz.FMT_U8, words, h, down) as hbank:
        for dst in (np.empty((k, total + 7), np.complex64), pinned, np.empty((k, total), np.complex64)):
            dst[:] = np.nan
            done = 0
            for part, c in zip((x[:n1], x[n1:], None), counts):
                w = hbank.push(part, out=dst[:, done:]) if part is not None else hbank.flush(out=dst[:, done:])
                assert w.shape == (k, c)
                done += c
            assert same(dst[:, :total], rows) and np.isnan(dst[:, total:].real).all()


def test_rows_do_not_depend_on_the_other_tuners(hz, ctx, seventeen):
    """row k of the K = 17 bank equals a K = 1 bank of the same word; the bank permuted gives the rows permuted; a
    second run gives the same bits"""
    words, h, down, x, rows = seventeen
    dx = dev(x)
    for k in (0, 1, 2, 7, 8, 16):
        with ctx.tuner_bank(hz.FMT_U8, words[k:k + 1], h, down) as single:
            assert same(run(single, dx), rows[k]), f"row {k} differs from the bank of one tuner"
    perm = np.random.default_rng(5).permutation(len(words))
    with ctx.tuner_bank(hz.FMT_U8, words[perm], h, down) as bank:
        assert same(run(bank, dx), rows[torch.from_numpy(perm).cuda()])
        assert same(run(bank, dx), rows[torch.from_numpy(perm).cuda()]), "a second run"
    with ctx.tuner_bank(hz.FMT_U8, np.concatenate([words, words[::-1], words[:3]]), h, down) as bank:
        big = run(bank, dx)
        assert same(big[:17], rows) and same(big[17:34], rows.flip(0)) and same(big[34:], rows[:3])


# ---- 5. w = 0 against the resampler ----------------------------------------------------------------

@pytest.mark.parametrize("q,down,fmt", [(64, 5, "c64"), (129, 16, "u8"), (7, 1, "i16")])
def test_word_zero_is_the_resampler(hz, ctx, q, down, fmt):
    """A tuner at w = 0 is the FIR and the decimation alone: the resampler at up = 1 with the same taps, on the same
    device input; equal as values (signed zeros do not count).  No new restatement is involved."""
    h = ref.taps_of(q)
    bank = ctx.tuner_bank(FMT[fmt], [5, 0, 1 << 31], h, down)
    rs = ctx.resampler(FMT[fmt], 1, down, h)
    x = dev(white(fmt, stream_length(bank), seed=q))
    n1 = x.shape[0] // 2
    got = torch.cat([bank.push(x[:n1]), bank.push(x[n1:])], dim=-1)[1]
    want = torch.cat([rs.push(x[:n1]), rs.push(x[n1:])], dim=-1)
    torch.cuda.synchronize()
    assert got.shape == want.shape and got.shape[0] == ref.outputs_after(x.shape[0], down)
    assert bool((got == want).all()), f"{int((got != want).sum())} outputs differ"
    bank.close(), rs.close()


# ---- 6. retune -------------------------------------------------------------------------------------

def test_retune(hz, ctx):
    k, q, down = 9, 33, 2
    words, h = ref.words_for(k, seed=1), ref.taps_of(q)
    new = words.copy()
    new[2:6] = ref.words_for(k, seed=2)[5:9]
    bank = ctx.tuner_bank(hz.FMT_C64, words, h, down)
    n = stream_length(bank)
    x = dev(white("c64", n, seed=6))
    cut = n // 2 + 1  # (odd: the retune falls between two outputs' samples)
    plain = run(bank, x, [0, cut, n])
    # to the same words: no bit changes
    a = bank.push(x[:cut])
    bank.retune(0, words)
    bank.retune(3, words[3:5])
    assert same(torch.cat([a, bank.push(x[cut:]), bank.flush()], dim=-1), plain)
    # to new words: from the retune's first output on, a fresh bank of the new words fed the whole stream
    a = bank.push(x[:cut])
    state = bank.pending()
    bank.retune(2, new[2:6])
    assert bank.pending() == state and [int(v) for v in bank.words] == [int(v) for v in new]
    b = torch.cat([bank.push(x[cut:]), bank.flush()], dim=-1)
    with ctx.tuner_bank(hz.FMT_C64, new, h, down) as fresh:
        want = run(fresh, x)
        assert np.array_equal(operands(fresh)[0].view(np.uint32), operands(bank)[0].view(np.uint32))
    first = ref.outputs_after(cut, down)
    assert a.shape[-1] == first and same(a, plain[:, :first]) and same(b, want[:, first:])
    assert not same(b[2:6], plain[2:6, first:]) and same(b[:2], plain[:2, first:]) and same(b[6:], plain[6:, first:])
    bank.close()


# ---- 7. a tone -------------------------------------------------------------------------------------

def test_a_tone(hz, ctx):
    """K = 4, one tuner on the tone's word: that row is constant at sum(h) times the tone's amplitude after the first
    ceil(Q / D) outputs, within the derived bound (plus the float32 rounding of the tone's own samples, sum|h| 2^-24
    per component); the rows an eighth of fs away stay below the prototype's stopband level there, from h in float64."""
    q, down, n, amp = 96, 8, 4000, 0.75
    t = np.arange(q) - (q - 1) / 2
    h64 = np.sinc(t / 16) * np.blackman(q + 2)[1:-1] / 16  # a low-pass at fs / 32, its stopband from fs / 10 on
    h = h64.astype(np.float32)
    word = hz.tuner_word(0.2371, 1.0)
    words = np.array([word, (word + (1 << 29)) % (1 << 32), (word - (1 << 29)) % (1 << 32), (word + (1 << 31)) % (1 << 32)], np.uint32)
    x64 = amp * ref.unit(word * np.arange(n, dtype=np.int64))
    x = x64.astype(np.complex64)
    with ctx.tuner_bank(hz.FMT_C64, words, h, down) as bank:
        y = bank.push(dev(x)).cpu().numpy().astype(np.complex128)
    skip = -(-q // down)
    assert y.shape == (4, n // down) and skip < y.shape[1] // 2
    s = float(h.astype(np.float64).sum())
    bnd = ref.bound(h, x) + float(np.abs(h).sum()) * np.sqrt(2.0) * 2.0 ** -24 * amp
    err = np.abs(y[0, skip:] - amp * s).max()
    print(f"on the tone: |y - A sum h| <= {err:.3e} (bound {bnd:.3e})")
    assert err <= bnd
    # a row d away sees the tone at -d: |H(d)| A, H the prototype's response in float64
    for row, d in ((1, 1 << 29), (2, -(1 << 29)), (3, 1 << 31)):
        level = abs(np.sum(h.astype(np.float64) * np.conj(ref.unit(-d * np.arange(q, dtype=np.int64))))) * amp
        stop = np.abs(np.fft.fft(h.astype(np.float64), 4096))[4096 // 10:4096 - 4096 // 10].max() * amp
        worst = np.abs(y[row, skip:]).max()
        print(f"row {row}: |y| <= {worst:.3e}; |H| A = {level:.3e}, stopband level {stop:.3e}, bound {bnd:.3e}")
        assert level <= stop and worst <= stop + bnd and stop < 1e-3 * amp * s


# ---- 8. behind and in front of its neighbours ------------------------------------------------------

def test_feeds_the_demodulator(hz, ctx):
    """the bank's output block, with its pitch, straight into a K-stream FM demodulator: the demodulator fed a
    contiguous copy gives the same bits"""
    k, q, down = 8, 64, 5
    bank = ctx.tuner_bank(hz.FMT_U8, ref.words_for(k, seed=9), ref.taps_of(q), down)
    x = dev(white("u8", stream_length(bank), seed=12))
    count = bank.outputs_for(x.shape[0])
    buf = torch.zeros((k, count + 9), dtype=torch.complex64, device="cuda")
    rows = bank.push(x, out=buf)
    assert rows.shape == (k, count) and rows.stride(0) == count + 9
    lp = ref.taps_of(16, seed=1)
    with ctx.demodulator(hz.FMT_C64, hz.DEMOD_FM, lp, 2, streams=k) as dm:
        a = torch.cat([dm.push(rows), dm.flush()], dim=-1)
        b = torch.cat([dm.push(rows.contiguous()), dm.flush()], dim=-1)
        torch.cuda.synchronize()
    assert a.shape[0] == k and a.shape[1] > 0 and same(a, b) and not torch.isnan(a).any()
    bank.close()


@pytest.mark.parametrize("block", [1000, 4096])
def test_tuner_rows(hz, hctx, block):
    """stream.tuner_rows over a BufferReader with short reads: the pushes' rows and the flush last, i.e. one push plus
    flush"""
    st = importlib.import_module("go-sdr_amd.stream")
    k, q, down = 3, 33, 4
    words, h = ref.words_for(k, seed=4), ref.taps_of(q)
    x = white("i16", 5000, seed=3)
    with hctx.tuner_bank(hz.FMT_I16, words, h, down) as one:
        want = run(one, x)
        assert one.sample_rate(48_000) == 12_000.0
    bank = hctx.tuner_bank(hz.FMT_I16, words, h, down)
    blocks = list(st.tuner_rows(st.BufferReader(x, 48_000, max_read=777), bank, block=block))
    bank.close()
    assert len(blocks) > 2 and all(b.dtype == np.complex64 and b.shape[0] == k for b in blocks)
    assert blocks[-1].shape[1] == ref.total_outputs(5000, q, down) - ref.outputs_after(5000, down)
    assert same(np.concatenate(blocks, axis=1), want) and want.shape == (k, ref.total_outputs(5000, q, down))


# ---- 9. errors and state ---------------------------------------------------------------------------

def test_create_errors(hz, ctx):
    h = ref.taps_of(24)
    lib = importlib.import_module("go-sdr_amd._capi").lib
    out = C.c_void_p()

    def create(fmt, words, k, down, taps, n):
        wp = words.ctypes.data_as(C.POINTER(C.c_uint32)) if words is not None else None
        tp = taps.ctypes.data_as(C.POINTER(C.c_float)) if taps is not None else None
        return lib.hzsdr_tuner_create(ctx._h, fmt, wp, k, down, tp, n, C.byref(out))

    w = np.zeros(257, np.uint32)
    inval = hz.ErrInvalidArgument.status
    assert create(hz.FMT_C64, w, 0, 2, h, 24) == create(hz.FMT_C64, w, 257, 2, h, 24) == inval, "tuners out of range"
    assert create(hz.FMT_C64, w, 4, 0, h, 24) == create(hz.FMT_C64, w, 4, 257, h, 24) == inval, "down out of range"
    assert create(hz.FMT_C64, None, 4, 2, h, 24) == create(hz.FMT_C64, w, 4, 2, None, 24) == inval, "null words, null taps"
    big = np.ones(1025, np.float32)
    assert create(hz.FMT_C64, w, 4, 2, h, 0) == create(hz.FMT_C64, w, 4, 2, big, 1025) == inval, "Q out of range"
    assert create(hz.FMT_C64, w, 256, 256, big, 1024) == 0 and lib.hzsdr_tuner_free(out) == 0
    for bad in (np.nan, np.inf, -np.inf):
        g = h.copy()
        g[7] = bad
        assert create(hz.FMT_C64, w, 4, 2, g, 24) == inval, "a non-finite tap"
    assert lib.hzsdr_tuner_create(ctx._h, hz.FMT_C64, w.ctypes.data_as(C.POINTER(C.c_uint32)), 4, 2, h.ctypes.data_as(C.POINTER(C.c_float)),
                                  24, None) == inval, "null result"
    with pytest.raises(hz.HzsdrError) as e:
        ctx.tuner_bank(9, [0], h)
    assert type(e.value).__name__ == "ErrSampleFormatUnknown"
    with pytest.raises(hz.ErrInvalidArgument):
        ctx.tuner_bank(hz.FMT_C64, [1 << 32], h)
    with ctx.tuner_bank(hz.FMT_C64, [1, 2, 3], h, 2) as bank:
        for first, words in ((3, [1]), (2, [1, 2]), (4, [])):
            with pytest.raises(hz.ErrInvalidArgument):
                bank.retune(first, words)
        assert lib.hzsdr_tuner_set_words(bank._h, 0, 2, None) == inval
        buf = np.zeros(4096, np.complex64)
        assert lib.hzsdr_tuner_readout(bank._h, 0, 0, buf.ctypes.data, 4096) == lib.hzsdr_tuner_readout(bank._h, 5, 0, buf.ctypes.data, 4096) == inval
        assert lib.hzsdr_tuner_readout(bank._h, hz.TUNER_READ_TAPS, 3, buf.ctypes.data, 4096) == inval, "no such tuner"
        assert lib.hzsdr_tuner_readout(bank._h, hz.TUNER_READ_TAPS, 0, None, 4096) == inval
        assert lib.hzsdr_tuner_readout(bank._h, hz.TUNER_READ_TAPS, 0, buf.ctypes.data, 23) == hz.ErrDstTooSmall.status
        assert lib.hzsdr_tuner_readout(bank._h, hz.TUNER_READ_T2, 0, buf.ctypes.data, 2047) == hz.ErrDstTooSmall.status
        assert lib.hzsdr_tuner_readout(bank._h, hz.TUNER_READ_TAPS, 2, buf.ctypes.data, 24) == 0
        x = torch.zeros(10, dtype=torch.complex64, device="cuda")
        out2 = torch.zeros((3, 8), dtype=torch.complex64, device="cuda")
        got = C.c_size_t(5)
        assert lib.hzsdr_tuner_push(bank._h, None, 10, out2.data_ptr(), 8, 8, C.byref(got)) == inval and got.value == 0, "null input"
        assert lib.hzsdr_tuner_push(bank._h, x.data_ptr(), 10, None, 8, 8, C.byref(got)) == inval, "null output"
        assert bank.pending() == (0, 0, 0)


@pytest.mark.parametrize("k", [1, 3])
def test_dst_too_small_leaves_state(hz, ctx, k):
    q, down = 24, 2
    h = ref.taps_of(q)
    lib = importlib.import_module("go-sdr_amd._capi").lib
    x = dev(white("c64", 200, seed=5))
    bank = ctx.tuner_bank(hz.FMT_C64, ref.words_for(3, seed=8)[3 - k:], h, down)
    want = run(bank, x, [0, 51, 200])
    first = bank.push(x[:51]).clone()
    state = bank.pending()
    assert state[2] > 1
    count = bank.outputs_for(149)
    out = torch.zeros((k, count), dtype=torch.complex64, device="cuda")
    got = C.c_size_t(7)
    part = x[51:].contiguous()
    with pytest.raises(hz.ErrDstTooSmall):
        ctx._ck(lib.hzsdr_tuner_push(bank._h, part.data_ptr(), 149, out.data_ptr(), count - 1, count, C.byref(got)))
    assert got.value == 0 and bank.pending() == state
    if k > 1:
        with pytest.raises(hz.ErrDstTooSmall):
            ctx._ck(lib.hzsdr_tuner_push(bank._h, part.data_ptr(), 149, out.data_ptr(), count, count - 1, C.byref(got)))
        assert bank.pending() == state
    with pytest.raises(hz.ErrDstTooSmall):
        ctx._ck(lib.hzsdr_tuner_flush(bank._h, out.data_ptr(), state[2] - 1, count, C.byref(got)))
    assert bank.pending() == state
    rest = torch.cat([bank.push(part), bank.flush()], dim=-1)
    torch.cuda.synchronize()
    assert same(torch.cat([first, rest], dim=-1), want)
    bank.close()


def test_reset_flush_and_runs(hz, ctx):
    k, q, down = 3, 64, 5
    words, h = ref.words_for(k, seed=2), ref.taps_of(q)
    x = dev(white("u8", 1500, seed=8))
    bank = ctx.tuner_bank(hz.FMT_U8, words, h, down)
    assert bank.flush().shape == (k, 0) and bank.pending() == (0, 0, 0), "flush on a fresh object writes nothing"
    a = run(bank, x)
    assert bank.pending() == (0, 0, 0)
    b = run(bank, x)  # (flush, then a push: a new stream)
    bank.push(x[:700])
    bank.reset()
    assert bank.pending() == (0, 0, 0)
    c = run(bank, x)
    with ctx.tuner_bank(hz.FMT_U8, words, h, down) as other:
        d = run(other, x)
    assert same(a, b) and same(a, c) and same(a, d)
    assert a.shape == (k, ref.total_outputs(1500, q, down))
    bank.close()


def test_cxx_tuner(hz):
    """tests/cxx/test_tuner.cpp (hzsdr::stream::TunerBank of go-sdr_amd/cxx/hzsdr.hpp) built with g++ and run."""
    exe = os.path.join(BUILD, "test_tuner_cxx")
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + ROOT, os.path.join(ROOT, "tests", "cxx", "test_tuner.cpp"),
                           "-L" + os.path.join(ROOT, "go-sdr_amd"), "-lhzsdr_hip", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "go-sdr_amd") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "tuner-cxx ok" in p.stdout

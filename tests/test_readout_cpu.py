"""The read-out constructions of tests/readout.py pinned without a GPU and without the library: the impulse trains
have one non-zero term per output or frame; their float64 references round to float32 exactly (resampler) or are
one-hot transforms (the banks); the table coverage is 100 % for the shapes the GPU tests use; a float32 emulation of
the resampler's sum passes the read-out, the same emulation with two neighbouring table entries swapped at the
filter's edge fails it -- and passes the white-noise block bound, which is why the read-out exists."""
import numpy as np
import pytest

import channelizer_ref as cref
import readout as ro
import resampler_ref as rref
import synthesizer_ref as sref
from util import FFT_FLOOR, FFT_K, assert_fft_rows_close, rand_c64

FMTS = ("c64", "i8", "i16")


def test_amplitudes_are_exact():
    for fmt in FMTS:
        seen = set()
        for k in range(24):
            raw, a = ro.train_amp(fmt, k)
            seen.add(a)
            assert a.real != a.imag and a != 0
            for c in (a.real, a.imag):
                assert c == 0 or np.frexp(abs(c))[0] == 0.5, (fmt, k, c)  # (a power of two)
            if fmt == "i8":
                assert (raw[0] / 128.0, raw[1] / 128.0) == (a.real, a.imag) and -128 <= min(raw) and max(raw) <= 127
            if fmt == "i16":
                assert all(v in (0, 32767, -32767) for v in raw)
        assert len(seen) >= 4, "the amplitudes hardly differ"
    with pytest.raises(ValueError):
        ro.train_amp("u8", 0)


def rows_of(shape):
    """the rows of the read-out a CPU test walks: all Q of a small Q, else the first, second, a middle and the last"""
    q = -(-shape[2] // shape[0])
    return range(q) if q <= 4 else (0, 1, q // 2, q - 1)


@pytest.mark.parametrize("shape", ro.RESAMPLER_SHAPES, ids=lambda s: "U%d-D%d-L%d" % s[:3])
def test_resampler_train(shape):
    """One non-zero term at most per output, exactly one wherever the Q samples lie in the stream; the float64
    reference is exact in float32; the float32 emulation of the kernel's sum equals it."""
    up, down, ntaps, tile = shape
    q = -(-ntaps // up)
    h = ro.kaiser_taps(up, down, ntaps)
    hp = ro.polyphase_table(h, up)
    count = min(ro.readout_outputs(shape), 300)  # (the property does not depend on the length: kept short here)
    n = max(ro.samples_for(count, up, down), 3 * q)
    for fmt in (("i8",) if shape == ro.READOUT_SMALL else FMTS):
        for r in rows_of(shape):
            raw, conv = ro.train(fmt, n, q, first=r)
            assert np.count_nonzero(conv) == len(range(r, n, q))
            terms = ro.resampler_terms(conv, ntaps, up, down)
            phi, i = ro.resampler_indices(n, ntaps, up, down)
            assert terms.max() <= 1
            assert (terms[(i >= q - 1) & (i < n)] == 1).all()
            want = rref.upfirdn_poly(h, conv, up, down)
            assert np.array_equal(want.astype(np.complex64).astype(np.complex128), want), "the reference is not exact in float32"
            if ntaps >= up:
                assert np.count_nonzero(want) > 0, "the train reads nothing out"
            assert ro.readout_equal(ro.resampler_f32(hp, conv, ntaps, up, down), want), (fmt, r)


@pytest.mark.parametrize("shape", ro.RESAMPLER_SHAPES, ids=lambda s: "U%d-D%d-L%d" % s[:3])
def test_resampler_coverage(shape):
    up, down, ntaps, tile = shape
    count = ro.readout_outputs(shape)
    n = ro.samples_for(count, up, down)
    read, exist = ro.resampler_coverage(n, ntaps, up, down)
    print(f"U={up} D={down} L={ntaps}: {read} of {exist} table entries read over {count}+ outputs of Q rows")
    assert read == exist > 0


def test_one_row_does_not_cover_the_table():
    """What the Q rows are for: a single train of spacing Q resonates with D/U (at (3, 20, 90) a row reads a tenth of
    the table), and the coverage formula agrees with a count over the rows' own non-zero samples."""
    up, down, ntaps = 3, 20, 90
    q = -(-ntaps // up)
    n = ro.samples_for(515, up, down)
    phi, i = ro.resampler_indices(n, ntaps, up, down)

    def read_by(rows):
        seen = np.zeros((up, q), bool)
        for r in rows:
            conv = ro.train("c64", n, q, first=r)[1]
            nz = np.concatenate([np.zeros(q - 1, bool), conv != 0, np.zeros(int(i.max()) + 1, bool)])
            for k in range(q):
                hit = nz[i - k + (q - 1)]
                seen[phi[hit], k] = True
        return int(seen.sum())

    one, everything = read_by([0]), read_by(range(q))
    print(f"(3, 20, 90): one row reads {one} of 90 entries, the {q} rows {everything}")
    assert one < 20 and everything == 90 == ro.resampler_coverage(n, ntaps, up, down)[0]


def swapped(hp, a, b):
    """the table with entries a = (phi, q) and b exchanged"""
    out = hp.copy()
    out[a], out[b] = hp[b], hp[a]
    return out


def edge_defects(hp, up, q):
    """off-by-one table indices at the filter's two edges: a neighbour in q and a neighbour in phi, exchanged"""
    return [("hp[0][0] <-> hp[0][1]", swapped(hp, (0, 0), (0, 1))), ("hp[U-1][Q-2] <-> hp[U-1][Q-1]", swapped(hp, (up - 1, q - 2), (up - 1, q - 1))),
            ("hp[1][0] <-> hp[2][0]", swapped(hp, (1, 0), (2 % up, 0))), ("hp[U-2][Q-1] <-> hp[U-1][Q-1]", swapped(hp, (up - 2, q - 1), (up - 1, q - 1)))]


@pytest.mark.parametrize("up,down,ntaps", [(160, 147, 1920), (2, 5, 50), (3, 20, 90)])
def test_a_swapped_edge_entry_fails_the_readout(up, down, ntaps):
    q = -(-ntaps // up)
    h = ro.kaiser_taps(up, down, ntaps)
    hp = ro.polyphase_table(h, up)
    n = ro.samples_for(2 * 1024 + 3, up, down)
    for name, bad in edge_defects(hp, up, q):
        if np.array_equal(bad, hp):
            continue  # (U = 2: no second neighbour in phi)
        caught = 0
        for r in range(q):
            conv = ro.train("c64", n, q, first=r)[1]
            want = rref.upfirdn_poly(h, conv, up, down)
            assert ro.readout_equal(ro.resampler_f32(hp, conv, ntaps, up, down), want)
            caught += not ro.readout_equal(ro.resampler_f32(bad, conv, ntaps, up, down), want)
        assert caught >= 1, f"{name} passes the read-out"


def test_the_white_noise_bound_does_not_see_an_edge_entry():
    """The experiment behind the read-out, at the 44.1 -> 48 kHz shape, on every block of 256 outputs of white input
    against bound(Q) = 6e-8 (Q + 2) = 8.4e-7.  Inside the bound: h[1] replaced by h[2], h[L - 2] by h[L - 1], and
    neighbouring phases exchanged at either edge (an off-by-one in phi: 2.6e-7 ... 4.3e-7).  The exchange of hp[phi][q]
    and hp[phi][q + 1], an off-by-one in q, is U taps apart and IS seen at both edges (3.9e-6, 4.5e-6): the white
    bound misses the table's phase index, not its tap index."""
    up, down, ntaps = 160, 147, 1920
    q = ntaps // up
    h = ro.kaiser_taps(up, down, ntaps)
    hp = ro.polyphase_table(h, up)
    n = ro.samples_for(2 * 1024 + 3, up, down)
    x = rand_c64(1920, n)
    want = rref.upfirdn_poly(h, x, up, down)
    clean = ro.block_errors(ro.resampler_f32(hp, x, ntaps, up, down), want).max()
    front, back = hp.copy(), hp.copy()
    front[1, 0] = hp[2, 0]
    back[up - 2, q - 1] = hp[up - 1, q - 1]
    seen = {}
    for name, table in edge_defects(hp, up, q) + [("h[1] := h[2]", front), ("h[L-2] := h[L-1]", back)]:
        seen[name] = e = ro.block_errors(ro.resampler_f32(table, x, ntaps, up, down), want).max()
        print(f"{name}: worst block {e:.3e} (clean {clean:.3e}, bound {rref.bound(q):.3e})")
    assert clean <= 0.2 * rref.bound(q)
    assert seen.pop("hp[0][0] <-> hp[0][1]") > rref.bound(q) and seen.pop("hp[U-1][Q-2] <-> hp[U-1][Q-1]") > rref.bound(q)
    assert all(clean < e <= rref.bound(q) for e in seen.values()), seen


@pytest.mark.parametrize("m,p,d", [(256, 2, 129), (256, 2, 1), (512, 3, 257), (4096, 2, 2049)])
@pytest.mark.parametrize("fmt", ["c64", "i16"])
def test_channelizer_train(fmt, m, p, d):
    """Every frame of the train is the transform of a one-hot vector g[l_j] amp, and the float64 fold agrees."""
    L = p * m
    g = ro.bank_taps(m, p)
    frames = 13
    n = (frames - 1) * d + L + 3
    raw, conv = ro.channelizer_train(fmt, n, L, first=L // 3)
    ls, u, want = ro.channelizer_onehots(conv, g, m, d, frames)
    assert (np.count_nonzero(u, axis=1) == 1).all() and len(set(ls.tolist())) == frames
    fold = cref.channels_fold(conv, g, m, d, frames=frames)
    peak = np.abs(want).max(axis=1, keepdims=True)
    assert (np.abs(fold - want) <= 1e-12 * peak).all()
    # the checker accepts the float64 frames rounded once, and refuses a frame whose tap is a neighbour's
    assert max(assert_fft_rows_close(fold.astype(np.complex64), u, want64=want, what="rounded float64")) <= 1.0
    j = int(np.argmin(np.abs(g[ls])))  # the smallest tap read: where a relative-L2 bound over the frame set sees nothing
    wrong = fold.copy()
    wrong[j] *= float(g[ls[j] + 1]) / float(g[ls[j]])
    with pytest.raises(AssertionError):
        assert_fft_rows_close(wrong.astype(np.complex64), u, want64=want, what="a neighbour's tap")


def test_channelizer_train_reads_every_tap():
    m, p, d = 256, 2, 1
    L = p * m
    frames = L + 2 * 4 + 5
    conv = ro.channelizer_train("c64", (frames - 1) * d + L, L, first=L - 1)[1]
    ls = ro.channelizer_onehots(conv, ro.bank_taps(m, p), m, d, frames)[0]
    assert set(ls.tolist()) == set(range(L))


def test_the_banks_bound_does_not_see_an_edge_tap():
    """The same experiment for the banks' B(M, P), in float64 (no rounding error at all beside the defect): the
    prototype with g[1] replaced by g[2], or g[L - 2] by g[L - 1], moves every frame and every block by far less than
    B, so a kernel with that defect has its whole rounding budget left."""
    m, p, d = 1024, 4, 768
    L = p * m
    g = ro.bank_taps(m, p)
    x = rand_c64(7, 12 * d + L)
    y = rand_c64(8, 12 * m).reshape(12, m)
    for a, b in ((1, 2), (L - 2, L - 1)):
        bad = g.copy()
        bad[a] = g[b]
        w, v = cref.channels_fold(x, g, m, d), cref.channels_fold(x, bad, m, d)
        rows = (np.linalg.norm(w - v, axis=1) / np.linalg.norm(w, axis=1)).max()
        s, t = sref.synth_ola(y, g, m, d), sref.synth_ola(y, bad, m, d)
        steady = slice(L, 11 * d)  # (the blocks every frame count covers)
        blocks = ro.block_errors(t[steady], s[steady], m).max()
        print(f"g[{a}] := g[{b}]: channelizer frames move by {rows:.3e} (B = {cref.bound(m, p):.3e}), synthesizer blocks by "
              f"{blocks:.3e} (B = {sref.bound(m, sref.terms(L, d)):.3e})")
        assert 0 < rows <= 0.1 * cref.bound(m, p) and 0 < blocks <= 0.1 * sref.bound(m, sref.terms(L, d))


@pytest.mark.parametrize("m,p,d", [(256, 2, 129), (512, 2, 257), (4096, 2, 2049)])
def test_synthesizer_onehot(m, p, d):
    """One non-zero frame value: the float64 overlap-add is g[t - j0 D] amp exp(+2 pi i k0 t / M) over the frame's L
    positions and zero elsewhere; the bound is a few float32 ulps of that, measured on scipy's transform."""
    g = ro.bank_taps(m, p)
    frames, amp = 9, 0.5 - 0.25j
    for j0, k0 in ((0, 1), (4, m // 2 + 1), (8, (m // 3) | 1)):
        y = np.zeros((frames, m), np.complex64)
        y[j0, k0] = amp
        want, scale = ro.synthesizer_want(g, m, d, frames, j0, k0, amp)
        ola = sref.synth_ola(y, g, m, d)
        assert (np.abs(ola - want) <= 1e-12 * scale).all()
        assert np.count_nonzero(scale) <= p * m and not want[:j0 * d].any() and not want[j0 * d + p * m:].any()
        b = ro.synthesizer_bound(m, k0, amp)
        assert FFT_K * FFT_FLOOR + 2.0 ** -24 <= b <= FFT_K * 4 * FFT_FLOOR + 2.0 ** -24, b

"""Streaming operations on Go sub-slices of guarded device buffers.

Go callers hand the library `buf.Slice(n, len)` after a short read (reader.go:104, pipe.go:124): a c64 sub-slice is
only 8-byte aligned, an i16 one 4-byte, a u8 / i8 one 2-byte.  Each operation picks its kernels by the caller's
pointers and sizes (a vector body at 16 / 8 / 32-byte alignment, a scalar kernel for the head, the tail or the whole
call, a non-temporal or tiled form past a cache threshold), so the cases here run each operation on slices whose start
offsets cover every residue of 16 (or 32) bytes, at lengths either side of each split, against the C oracle.

A guarded slice (`Guarded`) sits 64 bytes plus `off` samples into an allocation filled with a sentinel byte.  The 64
bytes in front of it and behind it must still hold the sentinel after the call, and an output slice starts as the
sentinel too, so an element the kernel never wrote is caught.  The slice's address modulo 32 is asserted, so an
allocator that changes its alignment fails here instead of quietly testing the aligned path.

Bars: bit-exact against the oracle wherever the rest of the suite is bit-exact; the opt-in ULP1 Shift within one ulp
of the rotation factor (as in tests/test_gpu_parity.py); FFT-based operations and the FIR-decimate terminal within the
bounds the other tests hold them to.  Case IDs name the formats and offsets; the lengths of LENS run inside each case
and a failure names its length."""
import functools
import importlib

import numpy as np
import pytest

from util import (ES, GUARD, SENT, Guarded, assert_fir_close, bits_equal, dtype_of, rand_c64, rand_i16, rand_i8, rand_u8,
                  zeros)

pytestmark = pytest.mark.gpu

FMTS = {"c64": 1, "u8": 2, "i16": 3, "i8": 4}
OFFS = {"c64": range(4), "i16": range(4), "u8": range(8), "i8": range(8)}  # every residue of 16 bytes
LENS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4097, 100_003]
GEN = {"c64": rand_c64, "u8": rand_u8, "i16": rand_i16, "i8": rand_i8}
BIG = (1 << 24) + 3  # a large call: past every cache threshold, several laps of the grid-stride loops
ULP1_BOUND = 1.5 * 2.0 ** -24  # ULP1 factor against the reference's, components of size <= 1 (test_gpu_parity.py)
RATE, SHIFT = 2_400_000, -333_333.25


@pytest.fixture(scope="module")
def hz():
    return importlib.import_module("go-sdr_amd")


@pytest.fixture(scope="module")
def torch():
    return importlib.import_module("torch")


@pytest.fixture(scope="module")
def ctx(hz, torch):
    c = hz.Context(0, hz.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


# ---- data and guarded slices ---------------------------------------------------------------------------------------

_C64_SPECIALS = np.array([complex(float("nan"), float("inf")), complex(float("-inf"), -0.0), complex(-0.0, 0.0),
                          complex(1e12, -1e12), complex(0.999999, -0.999999), complex(-1.0, 1.0),
                          complex(3.0, -3.0), complex(1.5e-42, -2.0)], np.complex64)


def _make(fmt, n, seed):
    if fmt != "c64":
        return GEN[fmt](seed, n)
    x = rand_c64(seed, n) * np.float32(1.25)
    k = np.arange(0, n, 37)
    x[k] = _C64_SPECIALS[k % len(_C64_SPECIALS)]
    return x


@functools.lru_cache(maxsize=None)
def _small(fmt, n, seed):
    x = _make(fmt, n, seed)
    x.flags.writeable = False
    return x


def data(fmt, n, seed=1):
    """Seeded data over the format's whole range.  c64 runs past [-1, 1] and holds NaN, +-Inf, -0 and out-of-range
    values every 37 samples, so the float -> integer converters meet them in every kernel."""
    return _small(fmt, n, seed) if n <= (1 << 20) else _make(fmt, n, seed)


def sentinel(fmt, n):
    """A host array of the format holding the sentinel byte everywhere: what an unwritten output slice holds."""
    return np.full(n * ES[fmt], SENT, np.uint8).view(dtype_of(fmt)).reshape(zeros(fmt, n).shape)


def _tables(orc, src_fmt, dst_fmt):
    ident = orc.lut_identity()
    tab = zeros(dst_fmt, 65536)
    if dst_fmt == src_fmt:
        return ident.view(tab.dtype).copy()
    orc.convert(tab, ident.view(np.int8) if src_fmt == "i8" else ident)
    return tab


def _to_c64(orc, fmt, x):
    y = zeros("c64", len(x))
    if fmt == "c64":
        np.copyto(y, x)
    else:
        orc.convert(y, x)
    return y


def _close_to_factor(got, want, scale, what):
    """ULP1: per component |got - want| <= ULP1_BOUND * scale."""
    d = np.abs(got.view(np.float32).astype(np.float64) - want.view(np.float32).astype(np.float64))
    assert np.all(d <= ULP1_BOUND * scale), (what, float((d / scale).max()) * 2.0 ** 24, int(np.argmax(d)))


def P(*vals, id):
    return pytest.param(*vals, id=id)


OFF_IDS = {"ids": lambda v: "off%d" % v}


# ---- 2. offset x length sweep: converters and copies ---------------------------------------------------------------

PAIRS = [(s, d) for s in FMTS for d in FMTS if s != d]


@pytest.mark.parametrize("src_fmt,so,dst_fmt,do", [P(s, so, d, do, id="%s@%d-%s@%d" % (s, so, d, do))
                                                   for s, d in PAIRS for so in OFFS[s] for do in OFFS[d]])
def test_convert_subslices(torch, ctx, orc, src_fmt, so, dst_fmt, do):
    for n in LENS:
        x = data(src_fmt, n)
        want = sentinel(dst_fmt, n)
        assert orc.convert(want, x) == n
        s, d = Guarded(torch, src_fmt, n, so, x), Guarded(torch, dst_fmt, n, do)
        assert ctx.convert(d.t, s.t) == n
        d.check(want, ("convert", src_fmt, so, dst_fmt, do, "n=%d" % n))
        s.check(x, ("convert source", "n=%d" % n))


@pytest.mark.parametrize("fmt,so,do", [P(f, so, do, id="%s@%d-%s@%d" % (f, so, f, do))
                                       for f in FMTS for so in OFFS[f] for do in OFFS[f]])
def test_same_format_convert_subslices(torch, ctx, fmt, so, do):
    """CopySamples (copy.go:31-52) between sub-slices."""
    for n in LENS:
        x = data(fmt, n, 3)
        s, d = Guarded(torch, fmt, n, so, x), Guarded(torch, fmt, n, do)
        assert ctx.convert(d.t, s.t) == n
        d.check(x, ("copy", fmt, so, do, "n=%d" % n))


@pytest.mark.parametrize("off", range(4), **OFF_IDS)
def test_i16_shift_lsb_to_msb_subslices(torch, ctx, orc, off):
    for n in LENS:
        x = data("i16", n, 5)
        want = x.copy()
        orc.i16_shift_lsb_to_msb(want, 12)
        b = Guarded(torch, "i16", n, off, x)
        ctx.i16_shift_lsb_to_msb(b.t, 12)
        b.check(want, ("i16_shift_lsb_to_msb", off, "n=%d" % n))


FOREIGN = ([P(s, d, True, id="%s_foreign-%s" % (s, d)) for s in ("i16", "c64") for d in FMTS if d != s]
           + [P(s, d, False, id="%s-%s_foreign" % (s, d)) for d in ("i16", "c64") for s in FMTS if d != s])


@pytest.mark.parametrize("src_fmt,dst_fmt,src_foreign", FOREIGN)
def test_convert_foreign_subslices(torch, ctx, orc, src_fmt, dst_fmt, src_foreign):
    """byteswap -> ConvertBuffer -> byteswap fused, with the swapped side on each swap side, every source offset."""
    for n in LENS:
        native = data(src_fmt, n, 7)
        if src_fmt == "c64":
            with np.errstate(invalid="ignore"):  # (the specials: NaN and Inf stay what they are)
                native = native * np.float32(0.79)  # mostly in range for the float -> int converters
        wire = native.copy()
        if src_foreign:
            orc.byteswap(wire)
        want = sentinel(dst_fmt, n)
        orc.convert(want, native)
        if not src_foreign:
            orc.byteswap(want)
        for so in OFFS[src_fmt]:
            for do in (0, 1, 3):
                s, d = Guarded(torch, src_fmt, n, so, wire), Guarded(torch, dst_fmt, n, do)
                assert ctx.convert_foreign(d.t, s.t, not src_foreign, src_foreign) == n
                d.check(want, ("convert_foreign", src_fmt, so, dst_fmt, do, "n=%d" % n))


# ---- lookup tables -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("src_fmt,dst_fmt", [P(s, d, id="%s-%s" % (s, d)) for s in ("u8", "i8") for d in FMTS])
def test_lookup_subslices(torch, ctx, orc, src_fmt, dst_fmt):
    tab = _tables(orc, src_fmt, dst_fmt)
    lut = ctx.lut(FMTS[src_fmt], torch.from_numpy(tab).cuda())
    try:
        for n in LENS:
            x = data(src_fmt, n, 9)
            want = sentinel(dst_fmt, n)
            assert orc.lut_apply(want, tab, x.view(np.uint8)) == n
            for so in OFFS[src_fmt]:
                for do in OFFS[dst_fmt]:
                    s, d = Guarded(torch, src_fmt, n, so, x), Guarded(torch, dst_fmt, n, do)
                    assert lut.lookup(d.t, s.t) == n
                    d.check(want, ("lookup", src_fmt, so, dst_fmt, do, "n=%d" % n))
    finally:
        lut.close()


@pytest.mark.parametrize("fmt", ["u8", "i8"])
def test_rotate_lut_subslices(torch, ctx, orc, fmt):
    m = np.complex64(0.6 + 0.3j)
    tab = orc.rotate_table_u8(m) if fmt == "u8" else orc.rotate_table_i8(m)
    t = ctx.rotlut(FMTS[fmt], m)
    try:
        for n in LENS:
            x = data(fmt, n, 13)
            want = x.copy()
            if fmt == "u8":
                orc.rotate_u8_apply(tab, want)
            else:
                orc.lut_apply(want, tab, x.view(np.uint8))
            for off in OFFS[fmt]:
                b = Guarded(torch, fmt, n, off, x)
                t.apply(b.t)
                b.check(want, ("rotlut", fmt, off, "n=%d" % n))
    finally:
        t.close()


# ---- c64 vector ops ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("op", ["scale", "rotate"])
@pytest.mark.parametrize("off", range(4), **OFF_IDS)
def test_scale_rotate_subslices(torch, ctx, orc, op, off):
    for n in LENS:
        x = data("c64", n, 17)
        want = x.copy()
        b = Guarded(torch, "c64", n, off, x)
        if op == "scale":
            orc.scale(want, 0.3)
            ctx.scale(b.t, 0.3)
        else:
            orc.rotate(want, 0.70710678 + 0.25881904j)
            ctx.rotate(b.t, 0.70710678 + 0.25881904j)
        b.check(want, (op, off, "n=%d" % n))


@pytest.mark.parametrize("ao,bo", [P(a, b, id="a@%d-b@%d" % (a, b)) for a in range(4) for b in range(4)])
def test_add_subslices(torch, ctx, orc, ao, bo):
    for n in LENS:
        x, y = data("c64", n, 19), data("c64", n, 20)
        want = sentinel("c64", n)
        orc.add(x, y, want)
        for co in range(4):
            a, b, c = Guarded(torch, "c64", n, ao, x), Guarded(torch, "c64", n, bo, y), Guarded(torch, "c64", n, co)
            ctx.add(a.t, b.t, c.t)
            c.check(want, ("add", ao, bo, co, "n=%d" % n))
            a.check(x, "add a")
            b.check(y, "add b")


@pytest.mark.parametrize("fmt", ["c64", "i16", "i8"])
@pytest.mark.parametrize("which", ["out", "b0", "b1", "b2"])
def test_sum_one_buffer_misaligned(torch, ctx, orc, fmt, which):
    """hzsdr_sum ORs every pointer: one misaligned buffer sends the call to sum_scalar_kernel."""
    for n in LENS:
        src = [data(fmt, n, 30 + i) for i in range(3)]
        want = sentinel(fmt, n)
        orc.sum_(want, src)
        for off in OFFS[fmt][1:]:
            bufs = [Guarded(torch, fmt, n, off if which == "b%d" % i else 0, s) for i, s in enumerate(src)]
            out = Guarded(torch, fmt, n, off if which == "out" else 0)
            ctx.sum(out.t, [b.t for b in bufs])
            out.check(want, ("sum", fmt, which, off, "n=%d" % n))


@pytest.mark.parametrize("fmt", ["c64", "u8", "i16", "i8"])
@pytest.mark.parametrize("which", ["out", "ch0", "ch1", "ch3"])
def test_beamform_one_pointer_misaligned(hz, torch, ctx, orc, fmt, which):
    """Exactly one misaligned channel (or the output) sends every channel to beamform_kernel<FMT, 1>."""
    w = hz.beamform_angles(433e6, 30.0, [0.0, 0.1, 0.2, 0.3])
    offs = range(1, 4) if which == "out" else OFFS[fmt][1:]
    for n in LENS:
        chans = [data(fmt, n, 40 + i) for i in range(4)]
        want = sentinel("c64", n)
        if n:
            orc.beamform(want, [_to_c64(orc, fmt, x) for x in chans], w)
        for off in offs:
            ch = [Guarded(torch, fmt, n, off if which == "ch%d" % i else 0, x) for i, x in enumerate(chans)]
            out = Guarded(torch, "c64", n, off if which == "out" else 0)
            ctx.beamform(out.t, [c.t for c in ch], w)
            out.check(want, ("beamform", fmt, which, off, "n=%d" % n))


# ---- NCO -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ulp1", [False, True], ids=["exact", "ulp1"])
@pytest.mark.parametrize("off", range(4), **OFF_IDS)
def test_nco_shift_subslices(torch, ctx, orc, off, ulp1):
    """The exact NCO against the oracle bit for bit on random inputs; the ULP1 one on unit inputs, whose output IS
    the factor, within one ulp of it.  The ULP1 form's 32-byte lead is 3, 2, 1 samples at offsets 1, 2, 3."""
    nco = ctx.nco(RATE)
    if ulp1:
        nco.set_ulp1()
    try:
        for n in LENS:
            x = np.ones(n, np.complex64) if ulp1 else data("c64", n, 50)
            want = x.copy()
            ref = orc.Shifter(RATE)
            ref.ts.value = 1.25
            ref(SHIFT, want)
            nco.ts = 1.25
            b = Guarded(torch, "c64", n, off, x)
            nco(SHIFT, b.t)
            assert nco.ts == ref.ts.value
            what = ("nco", "ulp1" if ulp1 else "exact", off, "n=%d" % n)
            if ulp1:
                b.check(None, what)
                _close_to_factor(b.values(), want, 1.0, what)
            else:
                b.check(want, what)
    finally:
        nco.close()


# ---- decimate / downsample -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("op", ["decimate", "downsample"])
@pytest.mark.parametrize("fmt", ["c64", "i16", "u8"])
@pytest.mark.parametrize("factor", [4, 8, 12, 16], ids=lambda v: "by%d" % v)
@pytest.mark.parametrize("offset", [0, 5], ids=lambda v: "offset%d" % v)
def test_decimate_downsample_subslices(torch, ctx, orc, op, fmt, factor, offset):
    """`offset` is accepted and ignored (stream/decimate.go:59-101).  Downsample's kernel branches hang on factor % W
    and the source's 16-byte alignment; the output slice is one sample longer than the count, and that sample must
    stay unwritten."""
    to_fmt = fmt if op == "decimate" else "c64"
    fn_o, fn_g = (orc.decimate, ctx.decimate) if op == "decimate" else (orc.downsample, ctx.downsample)
    for n in LENS:
        x = data(fmt, n, 60)
        m = n // factor + 1
        want = sentinel(to_fmt, m)
        cnt = fn_o(want, x, factor, offset)
        assert cnt == n // factor
        for so in OFFS[fmt]:
            for do in (0, 1):
                s, d = Guarded(torch, fmt, n, so, x), Guarded(torch, to_fmt, m, do)
                assert fn_g(d.t, s.t, factor, offset) == cnt
                d.check(want, (op, fmt, factor, offset, so, do, "n=%d" % n))


# ---- wire ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["i16", "c64"])
@pytest.mark.parametrize("off", range(4), **OFF_IDS)
def test_byteswap_subslices(torch, ctx, orc, fmt, off):
    for n in LENS:
        x = data(fmt, n, 70)
        want = x.copy()
        orc.byteswap(want)
        b = Guarded(torch, fmt, n, off, x)
        ctx.byteswap(b.t)
        b.check(want, ("byteswap", fmt, off, "n=%d" % n))


@pytest.mark.parametrize("off", range(4), **OFF_IDS)
def test_fftshift_scale_subslices(torch, ctx, orc, off):
    for n in LENS:
        x = data("c64", n, 80)
        want = x.copy()
        orc.fftshift_scale(want, 3.0)
        b = Guarded(torch, "c64", n, off, x)
        ctx.fftshift_scale(b.t, 3.0)
        b.check(want, ("fftshift_scale", off, "n=%d" % n))


# ---- map chains ----------------------------------------------------------------------------------------------------

def _map_want(orc, fmt, x, gain, t0=0.75):
    want = _to_c64(orc, fmt, x)
    ref = orc.Shifter(RATE)
    ref.ts.value = t0
    ref(SHIFT, want)
    if gain is not None:
        orc.scale(want, gain)
    return want, ref.ts.value


@pytest.mark.parametrize("fmt", ["u8", "i8", "i16", "c64"])
@pytest.mark.parametrize("gain", [None, 0.5], ids=["shift", "shift_gain"])
@pytest.mark.parametrize("ulp1", [False, True], ids=["exact", "ulp1"])
def test_map_chain_subslices(torch, ctx, orc, fmt, gain, ulp1):
    """Converter -> Shift (-> Gain): shift_exact_kernel where both pointers allow two-sample vectors, chain_map_kernel
    with four where they allow those, the scalar map path otherwise.  Exact: bit for bit.  ULP1 on unit c64 inputs:
    within one ulp of the factor.  ULP1 from the integer formats: within 1.5 ulp of the factor times |I| + |Q| of the
    converted sample, plus one rounding of each of the two complex products (2 x 2^-24 (|I| + |Q|)); the gain is 0.5,
    a power of two, and adds no rounding."""
    ch = ctx.chain(FMTS[fmt], RATE).shift(SHIFT)
    if gain is not None:
        ch = ch.gain(gain)
    if ulp1:
        ch.shift_ulp1()
    try:
        for n in LENS:
            if fmt == "c64":
                x = np.ones(n, np.complex64) if ulp1 else rand_c64(91, n)
            else:
                x = data(fmt, n, 90)
            want, ts_end = _map_want(orc, fmt, x, gain)
            if ulp1:
                xc = _to_c64(orc, fmt, x)
                mag = (np.abs(xc.real) + np.abs(xc.imag)).astype(np.float64) * (gain or 1.0)
                scale = np.repeat(mag if fmt == "c64" else mag * (3.5 / 1.5), 2)
            for so in OFFS[fmt]:
                for do in range(4):
                    s, d = Guarded(torch, fmt, n, so, x), Guarded(torch, "c64", n, do)
                    ch.set_time(0.75)
                    assert ch.run(s.t, d.t) == (n, n)
                    assert ch.time() == ts_end
                    what = ("map chain", fmt, gain, "ulp1" if ulp1 else "exact", so, do, "n=%d" % n)
                    if ulp1:
                        d.check(None, what)
                        _close_to_factor(d.values(), want, scale, what)
                    else:
                        d.check(want, what)
    finally:
        ch.close()


# ---- 3. exhaustive tables through the scalar kernels ---------------------------------------------------------------

def _exhaustive(fmt):
    """test_gpu_parity.py's tables: every (I, Q) byte pair, every int16 value, and random c64 led by its specials."""
    allb = np.arange(65536, dtype=np.uint32)
    if fmt in ("u8", "i8"):
        a = np.stack([(allb & 255), (allb >> 8)], 1).astype(np.uint8)
        return a.view(np.int8) if fmt == "i8" else a
    if fmt == "i16":
        v = allb.astype(np.uint16).view(np.int16)
        return np.stack([v, v[::-1]], 1).copy()
    x = rand_c64(11, 65536)
    x[:16] = np.array([complex(1, -1), 0, complex(-0.0, 0.5), complex(1e12, -1e12),
                       complex(float("nan"), float("inf")), complex(-3, 3), complex(0.999999, -0.999999),
                       complex(2.0, -2.0), complex(float("-inf"), -0.0), complex(-0.0, -0.0), complex(0.5, -0.5),
                       complex(-1.0, 1.0), complex(1.0000001, -1.0000001), complex(127.5, -128.5),
                       complex(32767.5, -32768.5), complex(1e-45, -1e-45)], np.complex64)
    return x


@pytest.mark.parametrize("src_fmt,dst_fmt", [P(s, d, id="%s-%s" % (s, d)) for s, d in PAIRS])
def test_convert_exhaustive_through_the_scalar_kernel(torch, ctx, orc, src_fmt, dst_fmt):
    """test_convert_exhaustive_bit_exact's tables with source and destination one sample in: every value goes
    through convert_scalar_kernel."""
    x = _exhaustive(src_fmt)
    want = sentinel(dst_fmt, len(x))
    assert orc.convert(want, x) == len(x)
    s, d = Guarded(torch, src_fmt, len(x), 1, x), Guarded(torch, dst_fmt, len(x), 1)
    assert ctx.convert(d.t, s.t) == len(x)
    d.check(want, ("exhaustive", src_fmt, dst_fmt))


@pytest.mark.parametrize("src_fmt,dst_fmt", [P(s, d, id="%s-%s" % (s, d)) for s in ("u8", "i8") for d in FMTS])
def test_lookup_exhaustive_through_the_scalar_kernel(torch, ctx, orc, src_fmt, dst_fmt):
    """All 65 536 source byte pairs through lut_kernel (source and destination one sample in)."""
    tab = _tables(orc, src_fmt, dst_fmt)
    x = _exhaustive(src_fmt)
    want = sentinel(dst_fmt, len(x))
    assert orc.lut_apply(want, tab, x.view(np.uint8)) == len(x)
    lut = ctx.lut(FMTS[src_fmt], torch.from_numpy(tab).cuda())
    s, d = Guarded(torch, src_fmt, len(x), 1, x), Guarded(torch, dst_fmt, len(x), 1)
    assert lut.lookup(d.t, s.t) == len(x)
    lut.close()
    d.check(want, ("lookup exhaustive", src_fmt, dst_fmt))


# ---- 4. large calls off alignment ----------------------------------------------------------------------------------

@pytest.mark.parametrize("src_fmt,dst_fmt", [P(s, d, id="%s-%s" % (s, d)) for s, d in
                                             [("u8", "c64"), ("c64", "i16"), ("i16", "c64")]])
@pytest.mark.parametrize("so,do", [P(1, 0, id="src@1"), P(0, 1, id="dst@1"), P(1, 1, id="both@1")])
def test_large_convert_off_alignment(torch, ctx, orc, src_fmt, dst_fmt, so, do):
    x = data(src_fmt, BIG, 100)
    want = sentinel(dst_fmt, BIG)
    orc.convert(want, x)
    s, d = Guarded(torch, src_fmt, BIG, so, x), Guarded(torch, dst_fmt, BIG, do)
    assert ctx.convert(d.t, s.t) == BIG
    d.check(want, ("large convert", src_fmt, so, dst_fmt, do))


@pytest.mark.parametrize("fmt,so,do", [P("c64", 0, 1, id="c64-dst@1"), P("c64", 1, 0, id="c64-src@1"),
                                       P("i16", 0, 0, id="i16-aligned-ragged-bytes")])
def test_large_copy_off_alignment(torch, ctx, fmt, so, do):
    """Same-format copies past 96 MiB: a misaligned pointer, and aligned pointers whose byte count (4 x odd) is not a
    multiple of 16 -- the streaming copy kernel and its ragged end."""
    x = data(fmt, BIG, 101)
    assert (BIG * ES[fmt]) % 16 != 0
    s, d = Guarded(torch, fmt, BIG, so, x), Guarded(torch, fmt, BIG, do)
    assert ctx.convert(d.t, s.t) == BIG
    d.check(x, ("large copy", fmt, so, do))


@pytest.mark.parametrize("fmt", ["i16", "c64"])
@pytest.mark.parametrize("factor", [8, 16], ids=lambda v: "by%d" % v)
def test_large_downsample_from_offset_one(torch, ctx, orc, fmt, factor):
    x = data(fmt, BIG, 102)
    m = BIG // factor
    want = sentinel("c64", m)
    assert orc.downsample(want, x, factor) == m
    s, d = Guarded(torch, fmt, BIG, 1, x), Guarded(torch, "c64", m, 0)
    assert ctx.downsample(d.t, s.t, factor) == m
    d.check(want, ("large downsample", fmt, factor))


@pytest.mark.parametrize("op", ["scale", "rotate"])
def test_large_scale_rotate_offset_one(torch, ctx, orc, op):
    x = data("c64", BIG, 103)
    want = x.copy()
    b = Guarded(torch, "c64", BIG, 1, x)
    if op == "scale":
        orc.scale(want, 0.3)
        ctx.scale(b.t, 0.3)
    else:
        orc.rotate(want, 0.6 - 0.8j)
        ctx.rotate(b.t, 0.6 - 0.8j)
    b.check(want, ("large", op))


@pytest.mark.parametrize("ulp1", [False, True], ids=["exact", "ulp1"])
@pytest.mark.parametrize("off", [1, 2, 3], **OFF_IDS)
def test_large_nco_shift_off_alignment(torch, ctx, orc, off, ulp1):
    rate, shift, t0 = 20_000_000, 2.5e6, 3.25
    x = np.ones(BIG, np.complex64) if ulp1 else data("c64", BIG, 104)
    want = x.copy()
    ref = orc.Shifter(rate)
    ref.ts.value = t0
    ref(shift, want)
    nco = ctx.nco(rate)
    if ulp1:
        nco.set_ulp1()
    nco.ts = t0
    b = Guarded(torch, "c64", BIG, off, x)
    nco(shift, b.t)
    assert nco.ts == ref.ts.value
    nco.close()
    what = ("large nco", "ulp1" if ulp1 else "exact", off)
    if ulp1:
        b.check(None, what)
        _close_to_factor(b.values(), want, 1.0, what)
    else:
        b.check(want, what)


@pytest.mark.parametrize("off", [1, 2], **OFF_IDS)
def test_large_u8_shift_gain_chain_off_alignment(torch, ctx, orc, off):
    x = data("u8", BIG, 105)
    want, ts_end = _map_want(orc, "u8", x, 0.5)
    ch = ctx.chain(FMTS["u8"], RATE).shift(SHIFT).gain(0.5)
    ch.set_time(0.75)
    s, d = Guarded(torch, "u8", BIG, off, x), Guarded(torch, "c64", BIG, 0)
    assert ch.run(s.t, d.t) == (BIG, BIG)
    assert ch.time() == ts_end
    ch.close()
    d.check(want, ("large chain", off))


@pytest.mark.parametrize("which", ["ch2", "out"])
def test_large_beamform_past_the_cache_one_misaligned(hz, torch, ctx, orc, which):
    """4 c64 channels of 2^23 + 5 samples and the output, 320 MiB: past the 192 MiB threshold.  One pointer one
    sample in sends the whole call to beamform_kernel<C64, 1>."""
    n = (1 << 23) + 5
    w = hz.beamform_angles(433e6, 30.0, [0.0, 0.1, 0.2, 0.3])
    chans = [data("c64", n, 110 + i) for i in range(4)]
    want = sentinel("c64", n)
    orc.beamform(want, chans, w)
    ch = [Guarded(torch, "c64", n, 1 if which == "ch%d" % i else 0, x) for i, x in enumerate(chans)]
    out = Guarded(torch, "c64", n, 1 if which == "out" else 0)
    ctx.beamform(out.t, [c.t for c in ch], w)
    out.check(want, ("large beamform", which))


# ---- 5. aliasing contracts -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("alias", ["c_is_a", "c_is_b"])
@pytest.mark.parametrize("off", range(4), **OFF_IDS)
def test_add_in_place(torch, ctx, orc, alias, off):
    """include/hzsdr.h: c may alias a or b."""
    for n in LENS:
        x, y = data("c64", n, 120), data("c64", n, 121)
        want = zeros("c64", n)
        orc.add(x, y, want)
        a, b = Guarded(torch, "c64", n, off, x), Guarded(torch, "c64", n, 3 - off, y)
        out, other, kept = (a, b, y) if alias == "c_is_a" else (b, a, x)
        ctx.add(a.t, b.t, out.t)
        out.check(want, ("add", alias, off, "n=%d" % n))
        other.check(kept, ("add, the other input", alias, off, "n=%d" % n))


@pytest.mark.parametrize("src_fmt,dst_fmt", [P(s, d, id="%s-%s" % (s, d)) for s, d in
                                             [("u8", "i8"), ("i8", "u8"), ("u8", "u8")]])
@pytest.mark.parametrize("off", range(8), **OFF_IDS)
def test_lookup_in_place(torch, ctx, orc, src_fmt, dst_fmt, off):
    """include/hzsdr.h: src may alias dst when the formats have equal size."""
    tab = _tables(orc, src_fmt, dst_fmt)
    tab = (tab.view(np.uint8) ^ np.uint8(0x5A)).view(tab.dtype)  # (a table that changes every byte)
    lut = ctx.lut(FMTS[src_fmt], torch.from_numpy(tab).cuda())
    try:
        for n in LENS:
            x = data(src_fmt, n, 122)
            want = sentinel(dst_fmt, n)
            orc.lut_apply(want, tab, x.view(np.uint8))
            s = Guarded(torch, src_fmt, n, off, x)
            d = Guarded(torch, dst_fmt, n, off, raw=s.raw)
            assert d.t.data_ptr() == s.t.data_ptr()
            assert lut.lookup(d.t, s.t) == n
            d.check(want, ("lookup in place", src_fmt, dst_fmt, off, "n=%d" % n))
    finally:
        lut.close()


def _rel_l2(got, want):
    want = want.astype(np.complex128)
    return float(np.linalg.norm(got.astype(np.complex128) - want) / max(np.linalg.norm(want), 1e-30))


@pytest.mark.parametrize("kind", ["convolve", "xcorr"])
@pytest.mark.parametrize("alias", ["dst_is_iq2", "dst_is_iq1"])
@pytest.mark.parametrize("n", [1024, 1000, 4099], ids=lambda v: "n%d" % v)
def test_convolve_dst_aliases_an_input(torch, ctx, orc, kind, alias, n):
    """include/hzsdr.h: dst may alias iq1 / iq2.  Bound as test_convolve_closures: relative L2 <= 3e-6."""
    a, b = rand_c64(5, n), rand_c64(6, n)
    want = zeros("c64", n)
    orc.convolve(want, a, b, conj=(kind == "xcorr"))
    ga, gb = Guarded(torch, "c64", n, 0, a), Guarded(torch, "c64", n, 0, b)
    dst = gb if alias == "dst_is_iq2" else ga
    cv = (ctx.convolve if kind == "convolve" else ctx.cross_correlate)(dst.t, ga.t, gb.t)
    cv()
    cv.close()
    dst.check(None, (kind, alias, n))
    assert _rel_l2(dst.values(), want) < 3e-6, (kind, alias, n)


@pytest.mark.parametrize("n", [1024, 1000, 4099], ids=lambda v: "n%d" % v)
def test_convolve_freq_dst_is_src(torch, ctx, orc, n):
    a = rand_c64(7, n)
    t = np.arange(n) - (n - 1) / 2
    H = np.fft.fft((np.sinc(t / 8) / 8 * np.hamming(n)).astype(np.complex128) / n).astype(np.complex64)
    want = zeros("c64", n)
    orc.convolve_freq(want, a, H)
    s, h = Guarded(torch, "c64", n, 0, a), Guarded(torch, "c64", n, 0, H)
    cv = ctx.convolve_freq(s.t, s.t, h.t)
    cv()
    cv.close()
    s.check(None, ("convolve_freq in place", n))
    assert _rel_l2(s.values(), want) < 3e-6, n


@pytest.mark.parametrize("gain", [None, 0.5], ids=["shift", "shift_gain"])
@pytest.mark.parametrize("ulp1", [False, True], ids=["exact", "ulp1"])
@pytest.mark.parametrize("off", range(4), **OFF_IDS)
def test_map_chain_in_place_equals_out_of_place(torch, ctx, orc, gain, ulp1, off):
    for n in (1, 2, 3, 5, 17, 257, 4097, 100_003):
        x = rand_c64(130, n)
        ch = ctx.chain(FMTS["c64"], RATE).shift(SHIFT)
        if gain is not None:
            ch = ch.gain(gain)
        if ulp1:
            ch.shift_ulp1()
        outs = []
        for inplace in (False, True):
            s = Guarded(torch, "c64", n, off, x)
            d = s if inplace else Guarded(torch, "c64", n, off)
            ch.set_time(0.75)
            assert ch.run(s.t, d.t) == (n, n)
            outs.append(d.check(None, ("chain", "in place" if inplace else "out of place", off, "n=%d" % n))[d.lo:d.hi].copy())
        ch.close()
        assert bits_equal(outs[0], outs[1]), ("chain in place", gain, ulp1, off, "n=%d" % n)
        if not ulp1:
            want, _ = _map_want(orc, "c64", x, gain)
            assert bits_equal(outs[1], want.view(np.uint8)), ("chain in place against the oracle", gain, off, "n=%d" % n)


@functools.lru_cache(maxsize=1)
def _overlap_data(fmt, n):
    return _make(fmt, n, 140)


@pytest.mark.parametrize("fmt,nbytes", [P("u8", 4096, id="u8-4KiB"), P("c64", 4096, id="c64-4KiB"),
                                        P("c64", 96 << 20, id="c64-96MiB")])
@pytest.mark.parametrize("where", ["dst_before_src", "dst_after_src"])
@pytest.mark.parametrize("dist", ["1", "7", "4096", "n-1"], ids=lambda v: "dist" + v)
def test_same_format_convert_overlapping(torch, ctx, fmt, nbytes, where, dist):
    """CopySamples is Go's copy, with memmove semantics for overlapping slices (copy.go:31-52): n samples from one
    part of a buffer to another `dist` samples away.  Expected: numpy's buf[d:d + n] = buf[s:s + n].copy()."""
    n = nbytes // ES[fmt]
    k = n - 1 if dist == "n-1" else int(dist)
    total = n + k
    x = _overlap_data(fmt, n + max(n, 4096))[:total]
    s_at, d_at = (k, 0) if where == "dst_before_src" else (0, k)
    buf = Guarded(torch, fmt, total, 0, x)
    assert ctx.convert(buf.t[d_at:d_at + n], buf.t[s_at:s_at + n]) == n
    want = x.copy()
    want[d_at:d_at + n] = x[s_at:s_at + n]
    buf.check(want, ("overlapping copy", fmt, nbytes, where, "dist=%d" % k))


# ---- 6. FIR chains on sub-slices -----------------------------------------------------------------------------------

def _fir_taps(ntaps=1024):
    k = np.arange(ntaps) - (ntaps - 1) / 2
    return (2 / 32 * np.sinc(2 / 32 * k) * np.hamming(ntaps) * np.exp(0.3j * k)).astype(np.complex64)


def _fir_want(orc, x, rate, shift, taps, D, ts0):
    xc = _to_c64(orc, "u8", x)
    sh = orc.Shifter(rate)
    sh.ts.value = ts0
    sh(shift, xc)
    want = zeros("c64", len(x) // D)
    orc.par_fir_decimate_f64(want, xc, taps, D)
    return want, float(np.abs(xc).max())


@pytest.mark.parametrize("off", range(1, 8), **OFF_IDS)
def test_fir_chain_on_a_subslice_takes_the_transforms(hz, torch, ctx, orc, off):
    """u8 -> Shift -> 1024-tap FIR / 8 on an input one to seven samples in: the matrix form needs 16-byte aligned
    buffers, so the transform kernels run, within the FIR bound of tests/util.py."""
    rate, D, n = 20_000_000, 8, 1 << 18
    taps = _fir_taps()
    x = data("u8", n, 150 + off)
    want, xmax = _fir_want(orc, x, rate, -rate / 8, taps, D, 1.0)
    ch = ctx.chain(hz.FMT_U8, rate).shift(-rate / 8).fir_decimate(taps, D)
    ch.set_time(1.0)
    s, d = Guarded(torch, "u8", n, off, x), Guarded(torch, "c64", n // D, 0)
    assert ch.run(s.t, d.t) == (n, n // D)
    assert ch.last_fir_kernel() == hz.FIR_KERNEL_TRANSFORM
    ch.close()
    d.check(None, ("fir", off))
    s.check(x, ("fir source", off))
    assert_fir_close(d.values(), want, taps, xmax, ("fir subslice", off))


@pytest.mark.parametrize("off", [1, 3], **OFF_IDS)
def test_fir_run_batch_with_a_misaligned_buffer(hz, torch, ctx, orc, off):
    """hzsdr_chain_run_batch over [aligned, misaligned, aligned]: the one-launch form needs every buffer aligned
    (hz_chain_fir.hip, mm2_plan), so the call falls back -- and still gives, bit for bit, what three single run()
    calls give, within the FIR bound of the oracle over the whole stream."""
    rate, D, n = 20_000_000, 8, 1 << 18
    taps = _fir_taps()
    x = data("u8", 3 * n, 160)
    parts = [x[j * n:(j + 1) * n] for j in range(3)]
    offs = [0, off, 0]
    want, xmax = _fir_want(orc, x, rate, -rate / 8, taps, D, 1.0)
    outs = {}
    for mode in ("single", "batch"):
        ch = ctx.chain(hz.FMT_U8, rate).shift(-rate / 8).fir_decimate(taps, D)
        ch.set_time(1.0)
        ins = [Guarded(torch, "u8", n, o, p) for o, p in zip(offs, parts)]
        ys = [Guarded(torch, "c64", n // D, 0) for _ in range(3)]
        if mode == "single":
            for i, y in zip(ins, ys):
                assert ch.run(i.t, y.t) == (n, n // D)
        else:
            assert ch.run_batch([i.t for i in ins], [y.t for y in ys]) == (n, n // D)
        ch.close()
        outs[mode] = [y.check(None, (mode, j))[y.lo:y.hi].copy() for j, y in enumerate(ys)]
    for j in range(3):
        assert bits_equal(outs["batch"][j], outs["single"][j]), ("run_batch buffer", j, off)
    got = np.concatenate([b.view(np.complex64) for b in outs["batch"]])
    assert_fir_close(got, want, taps, xmax, ("run_batch", off))


# ---- 7. library-pinned host memory ---------------------------------------------------------------------------------

class PinnedGuarded:
    """Guarded's layout in host memory the library pinned (hzsdr_malloc_pinned), which HOST-space calls hand to the
    kernels as it is, unstaged."""

    def __init__(self, hctx, fmt, n, off, fill=None):
        es = ES[fmt]
        self.lo, self.hi = GUARD + off * es, GUARD + (off + n) * es
        total = (self.hi + GUARD + 7) // 8 * 8
        self.raw = hctx.pinned_samples(FMTS["u8"], total // 2).reshape(-1)
        assert self.raw.ctypes.data % 256 == 0
        self.raw[:] = SENT
        self.t = self.raw[self.lo:self.hi].view(dtype_of(fmt)).reshape(zeros(fmt, n).shape)
        assert self.t.ctypes.data % 32 == (off * es) % 32
        if fill is not None:
            self.t[...] = fill

    def check(self, want, what):
        b = self.raw
        assert (b[:self.lo] == SENT).all() and (b[self.hi:] == SENT).all(), (what, "guard written")
        assert bits_equal(b[self.lo:self.hi], np.ascontiguousarray(want).view(np.uint8).ravel()), what


@pytest.fixture(scope="module")
def hctx(hz):
    c = hz.Context(0, hz.MEM_HOST)
    yield c
    c.close()


@pytest.mark.parametrize("op", ["u8_to_c64", "scale", "add", "downsample8", "byteswap"])
@pytest.mark.parametrize("off", range(4), **OFF_IDS)
def test_pinned_host_subslices(hctx, orc, op, off):
    for n in (1, 5, 17, 257, 4097):
        if op == "u8_to_c64":
            x = data("u8", n, 170)
            want = _to_c64(orc, "u8", x)
            s, d = PinnedGuarded(hctx, "u8", n, off, x), PinnedGuarded(hctx, "c64", n, (off + 1) % 4)
            assert hctx.convert(d.t, s.t) == n
        elif op == "scale":
            x = data("c64", n, 171)
            want = x.copy()
            orc.scale(want, 0.3)
            d = PinnedGuarded(hctx, "c64", n, off, x)
            hctx.scale(d.t, 0.3)
        elif op == "add":
            x, y = data("c64", n, 172), data("c64", n, 173)
            want = zeros("c64", n)
            orc.add(x, y, want)
            a, b = PinnedGuarded(hctx, "c64", n, off, x), PinnedGuarded(hctx, "c64", n, 0, y)
            d = PinnedGuarded(hctx, "c64", n, (off + 2) % 4)
            hctx.add(a.t, b.t, d.t)
        elif op == "downsample8":
            x = data("i16", 8 * n + 3, 174)
            want = zeros("c64", n)
            assert orc.downsample(want, x, 8) == n
            s, d = PinnedGuarded(hctx, "i16", len(x), off, x), PinnedGuarded(hctx, "c64", n, off)
            assert hctx.downsample(d.t, s.t, 8) == n
        else:
            x = data("i16", n, 175)
            want = x.copy()
            orc.byteswap(want)
            d = PinnedGuarded(hctx, "i16", n, off, x)
            hctx.byteswap(d.t)
        d.check(want, (op, off, "n=%d" % n))

"""The fused power spectrum (include/hzsdr_spectrum.h) on the GPU: rows against a float64 restatement of the
definition, against scipy.signal.welch where scipy imports, and bit for bit across pushes, kernel forms, source
formats, memory spaces, orders and runs."""
import importlib

import numpy as np
import pytest

from spectrum_ref import want_rows
from util import FMT, splitmix64

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def hz():
    return importlib.import_module("go-sdr_amd")


@pytest.fixture(scope="module")
def sp():
    return importlib.import_module("go-sdr_amd.spectrum")


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


def raw(fmt, n, seed):
    """n samples of format fmt (numpy): full-range bytes / i16, c64 in [-1, 1)."""
    z = splitmix64(seed, 2 * n)
    if fmt == "u8":
        return (z & np.uint64(0xFF)).astype(np.uint8).reshape(n, 2)
    if fmt == "i8":
        return (z & np.uint64(0xFF)).astype(np.uint8).view(np.int8).reshape(n, 2)
    if fmt == "i16":
        return (z & np.uint64(0xFFFF)).astype(np.uint16).view(np.int16).reshape(n, 2)
    f = ((z >> np.uint64(40)).astype(np.float64) / float(1 << 23) - 1.0).astype(np.float32)
    return f.view(np.complex64).reshape(n)


def converted(orc, x):
    """hzsdr_convert's arithmetic, by the oracle's converters."""
    if x.dtype == np.complex64:
        return x.copy()
    out = np.zeros(x.shape[0], np.complex64)
    assert orc.convert(out, x) == x.shape[0]
    return out


def bound(n, avg):
    return 2 * (3e-7 * np.log2(n) + 1e-7) + 6e-8 * (avg + 4)


def check_rows(got, want, n, avg, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    got = got.astype(np.float64)
    err = np.abs(got - want).sum(axis=1) / want.sum(axis=1)
    b = bound(n, avg)
    assert (err <= b).all(), f"{what}: relative L1 error {err.max():.3e} > {b:.3e}"
    return err.max()


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits(t):
    t = t.detach().cpu() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return t.contiguous().view(torch.int32)


def push_all(s, x, cuts=None):
    """push x (a device tensor) whole or cut at `cuts`; the rows of all pushes, concatenated"""
    if cuts is None:
        cuts = [0, x.shape[0]]
    out = [s.push(x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    torch.cuda.synchronize()
    return torch.cat([o.reshape(-1, s.n) for o in out], 0)


# ---- 1. accuracy -------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["u8", "i8", "i16", "c64"])
@pytest.mark.parametrize("n", [256, 512, 1024, 2048, 4096, 8192])
def test_rows_against_float64(hz, sp, orc, ctx, fmt, n):
    worst = 0.0
    for hop in (1, n // 2, n, n + 37):
        for avg in (1, 3, 16):
            for win in (None, sp.hann(n)):
                frames = 2 * avg + 1
                L = (frames - 1) * hop + n + hop // 3
                x = raw(fmt, L, seed=n * 131 + hop * 7 + avg + (0 if win is None else 1))
                s = ctx.spectrum(FMT[fmt], n, hop=hop, avg=avg, window=win, scale="power", order=sp.ZeroFirst)
                got = s.push(dev(x)).cpu().numpy()
                s.close()
                want = want_rows(converted(orc, x), n, hop, avg, win, s.scale)
                what = f"{fmt} n={n} hop={hop} avg={avg} {'hann' if win is not None else 'rect'}"
                worst = max(worst, check_rows(got, want, n, avg, what))
    print(f"{fmt} n={n}: worst relative L1 {worst:.3e}")


# ---- 2. independent check --------------------------------------------------------------------

@pytest.mark.parametrize("n,hop,avg", [(1024, 512, 16), (256, 256, 3), (4096, 1024, 5)])
def test_against_scipy_welch(hz, sp, orc, ctx, n, hop, avg):
    signal = pytest.importorskip("scipy.signal")
    fs = 2_048_000
    L = (avg - 1) * hop + n
    x = raw("u8", L, seed=77 + n)
    w = sp.hann(n)
    s = ctx.spectrum(hz.FMT_U8, n, hop=hop, avg=avg, window=w, scale="density", order=sp.ZeroFirst, sample_rate=fs)
    got = s.push(dev(x)).cpu().numpy()
    s.close()
    assert got.shape == (1, n)
    c = converted(orc, x)
    _, pxx = signal.welch(c, fs, window=w.astype(np.float64), nperseg=n, noverlap=n - hop, return_onesided=False,
                          detrend=False, scaling="density", average="mean")
    err = np.abs(got[0].astype(np.float64) - pxx).sum() / pxx.sum()
    assert err <= 2 * bound(n, avg), f"welch: relative L1 {err:.3e}"


# ---- 3. bit-identity -------------------------------------------------------------------------

def random_cuts(rng, L, n):
    cuts = [0]
    while cuts[-1] < L:
        k = int(rng.choice([0, 1, 7, n // 3, n - 1, n, n + 5, 3 * n + 11, int(rng.integers(0, 4 * n))]))
        cuts.append(min(L, cuts[-1] + k))
    return cuts


@pytest.mark.parametrize("fmt,n,hop,avg", [("u8", 1024, 512, 4), ("i16", 256, 293, 3), ("c64", 2048, 1, 16),
                                           ("i8", 8192, 4096, 2), ("u8", 512, 700, 5)])
def test_cuts_forms_runs_bit_identical(hz, sp, ctx, fmt, n, hop, avg):
    rng = np.random.default_rng(n + hop)
    L = 40 * max(hop, n // 4) + n + 123
    x = dev(raw(fmt, L, seed=5 + n))
    w = sp.hann(n)
    outs = {}
    for form in (hz.SPECTRUM_FORM_ROW_WALK, hz.SPECTRUM_FORM_FRAME_PARALLEL):
        s = ctx.spectrum(FMT[fmt], n, hop=hop, avg=avg, window=w, scale="power")
        s.options(form)
        whole = push_all(s, x)
        assert s.last_form() == form
        s.reset()
        again = push_all(s, x)
        for trial in range(3):
            s.reset()
            cut = push_all(s, x, random_cuts(rng, L, n))
            assert torch.equal(bits(cut), bits(whole)), f"form {form}: cuts (trial {trial}) differ from one push"
        assert torch.equal(bits(again), bits(whole)), f"form {form}: two runs differ"
        outs[form] = whole
        s.close()
    assert outs[1].shape[0] >= 2
    assert torch.equal(bits(outs[1]), bits(outs[2])), "row walk differs from frame-parallel"


def test_forms_with_open_rows_across_pushes(hz, sp, ctx):
    """Alternating forms push by push: the partial row's sums carry over between the forms bit for bit."""
    n, hop, avg = 1024, 512, 7
    L = 60 * hop + n
    x = dev(raw("u8", L, seed=3))
    ref = ctx.spectrum(hz.FMT_U8, n, hop=hop, avg=avg, window=sp.hann(n))
    want = push_all(ref, x)
    s = ctx.spectrum(hz.FMT_U8, n, hop=hop, avg=avg, window=sp.hann(n))
    got = []
    cuts = [0, 1000, 5000, 5001, 17000, L]
    for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        s.options(1 + i % 2)
        got.append(s.push(x[a:b]))
    torch.cuda.synchronize()
    assert torch.equal(bits(torch.cat(got)), bits(want))
    ref.close()
    s.close()


@pytest.mark.parametrize("fmt", ["u8", "i8", "i16"])
def test_byte_sources_equal_their_c64(hz, sp, orc, ctx, fmt):
    n, hop, avg = 1024, 333, 5
    L = 30 * hop + n
    x = raw(fmt, L, seed=11)
    c = torch.zeros(L, dtype=torch.complex64, device="cuda")
    ctx.convert(c, dev(x))
    a = ctx.spectrum(FMT[fmt], n, hop=hop, avg=avg, window=sp.hann(n))
    b = ctx.spectrum(hz.FMT_C64, n, hop=hop, avg=avg, window=sp.hann(n))
    ra, rb = push_all(a, dev(x)), push_all(b, c)
    assert ra.shape[0] >= 5
    assert torch.equal(bits(ra), bits(rb))
    a.close()
    b.close()


def test_host_equals_device(hz, sp, ctx, hctx):
    n, hop, avg = 2048, 1024, 3
    L = 20 * hop + n + 17
    x = raw("i16", L, seed=21)
    d = ctx.spectrum(hz.FMT_I16, n, hop=hop, avg=avg, window=sp.hann(n), db=True)
    h = hctx.spectrum(hz.FMT_I16, n, hop=hop, avg=avg, window=sp.hann(n), db=True)
    rd = push_all(d, dev(x))
    rh = np.concatenate([h.push(x[:5000]), h.push(x[5000:])])
    assert torch.equal(bits(rd), bits(rh))
    d.close()
    h.close()


def test_negative_first_is_swapped_zero_first(hz, sp, ctx):
    n, hop, avg = 4096, 2048, 2
    x = dev(raw("u8", 10 * hop + n, seed=31))
    z = ctx.spectrum(hz.FMT_U8, n, hop=hop, avg=avg, order=sp.ZeroFirst)
    g = ctx.spectrum(hz.FMT_U8, n, hop=hop, avg=avg, order=sp.NegativeFirst)
    rz, rg = push_all(z, x), push_all(g, x)
    assert torch.equal(bits(sp.shift(rz.clone())), bits(rg))
    z.close()
    g.close()


# ---- 4. dB -----------------------------------------------------------------------------------

def test_db_output(hz, sp, ctx):
    n, hop, avg = 1024, 512, 4
    L = 20 * hop + n
    x = raw("u8", L, seed=41)
    x[: 3 * n] = 127  # (127, 127): every converted sample is -1/255 -- a DC-only stretch: exact zeros off DC
    lin = ctx.spectrum(hz.FMT_U8, n, hop=hop, avg=avg, scale="power")
    db = ctx.spectrum(hz.FMT_U8, n, hop=hop, avg=avg, scale="power", db=True)
    pl = push_all(lin, dev(x)).cpu().numpy()
    pd = push_all(db, dev(x)).cpu().numpy()
    zero = pl == 0
    assert zero.any(), "the test stream has no zero bins"
    assert np.isneginf(pd[zero]).all()
    assert np.isfinite(pd[~zero]).all()
    want = 10 * np.log10(pl[~zero].astype(np.float64))
    got = pd[~zero].astype(np.float64)
    ulp = np.spacing(np.abs(pd[~zero])).astype(np.float64)
    assert (np.abs(got - want) <= np.maximum(2e-5, 4 * ulp)).all()
    lin.close()
    db.close()


# ---- 5. errors and state ---------------------------------------------------------------------

def test_errors(hz, sp, ctx):
    lib = hz.lib
    import ctypes as C
    h = C.c_void_p()
    for n, hop, avg, order, output, want in [(128, 1, 1, 0, 0, hz._capi.ERR_INVALID_ARGUMENT),
                                             (16384, 1, 1, 0, 0, hz._capi.ERR_INVALID_ARGUMENT),
                                             (1000, 1, 1, 0, 0, hz._capi.ERR_INVALID_ARGUMENT),
                                             (1024, 0, 1, 0, 0, hz._capi.ERR_INVALID_ARGUMENT),
                                             (1024, 1, 0, 0, 0, hz._capi.ERR_INVALID_ARGUMENT),
                                             (1024, 1, 1, 2, 0, hz._capi.ERR_INVALID_ARGUMENT),
                                             (1024, 1, 1, 0, 2, hz._capi.ERR_INVALID_ARGUMENT)]:
        assert lib.hzsdr_spectrum_create(ctx._h, hz.FMT_U8, n, hop, avg, None, 1.0, order, output, C.byref(h)) == want
    assert lib.hzsdr_spectrum_create(ctx._h, 9, 1024, 1, 1, None, 1.0, 0, 0, C.byref(h)) == hz._capi.ERR_FORMAT_UNKNOWN


def test_dst_too_small_leaves_state(hz, sp, ctx):
    n, hop, avg = 1024, 384, 3
    L = 30 * hop + n
    x = dev(raw("u8", L, seed=51))
    a = ctx.spectrum(hz.FMT_U8, n, hop=hop, avg=avg, window=sp.hann(n))
    b = ctx.spectrum(hz.FMT_U8, n, hop=hop, avg=avg, window=sp.hann(n))
    ra = [a.push(x[:2000])]
    rb = [b.push(x[:2000])]
    before = a.pending()
    assert a.rows_for(L - 2000) >= 2
    small = torch.zeros((1, n), dtype=torch.float32, device="cuda")
    with pytest.raises(hz.ErrDstTooSmall):
        a.push(x[2000:], out=small)
    assert a.pending() == before
    ra.append(a.push(x[2000:]))
    rb.append(b.push(x[2000:]))
    torch.cuda.synchronize()
    assert a.pending() == b.pending()
    assert torch.equal(bits(torch.cat(ra)), bits(torch.cat(rb)))
    a.close()
    b.close()


def test_reset_restarts_frame_zero(hz, sp, ctx):
    n, hop, avg = 512, 1000, 2
    x = dev(raw("c64", 20 * hop, seed=61))
    s = ctx.spectrum(hz.FMT_C64, n, hop=hop, avg=avg)
    first = push_all(s, x)
    s.push(x[:1700])  # inside a skip gap, a frame open
    s.reset()
    assert s.pending() == (0, 0)
    assert torch.equal(bits(push_all(s, x)), bits(first))
    s.close()


def test_pending_and_skip_gaps(hz, sp, ctx):
    n, hop, avg = 256, 300, 4
    s = ctx.spectrum(hz.FMT_U8, n, hop=hop, avg=avg)
    x = dev(raw("u8", 2000, seed=71))
    s.push(x[:200])
    assert s.pending() == (0, 200)
    s.push(x[200:260])  # frame 0 completes at 256; 4 samples past it fall into the gap
    assert s.pending() == (1, 0)
    s.push(x[260:300])  # the rest of the gap
    assert s.pending() == (1, 0)
    s.push(x[300:301])
    assert s.pending() == (1, 1)
    s.close()


# ---- 6. full size ----------------------------------------------------------------------------

def test_full_size_u8(hz, sp, orc, ctx):
    n, hop, avg = 1024, 512, 16
    L = 1 << 24
    x = raw("u8", L, seed=81)
    s = ctx.spectrum(hz.FMT_U8, n, hop=hop, avg=avg, window=sp.hann(n), scale="power", order=sp.ZeroFirst)
    got = s.push(dev(x)).cpu().numpy()
    form = s.last_form()
    s.close()
    c = converted(orc, x)
    rows = ((L - n) // hop + 1) // avg
    assert got.shape == (rows, n)
    worst = 0.0
    for r0 in range(0, rows, 256):  # (float64 reference in slices of rows)
        r1 = min(rows, r0 + 256)
        seg = c[r0 * avg * hop: (r1 * avg - 1) * hop + n]
        worst = max(worst, check_rows(got[r0:r1], want_rows(seg, n, hop, avg, sp.hann(n), s.scale), n, avg, f"rows {r0}.."))
    print(f"full size: {rows} rows, form {form}, worst relative L1 {worst:.3e}")


# ---- the C walkthrough -----------------------------------------------------------------------

def test_c_spectrum_walkthrough(hz):
    """tests/c/test_spectrum_abi.c compiled by gcc as C99 and run against libhzsdr_hip.so."""
    import os
    import subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "build", "test_spectrum_abi")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "test_spectrum_abi.c"), "-L" + os.path.join(ROOT, "go-sdr_amd"),
                           "-lhzsdr_hip", "-lm", "-Wl,-rpath," + os.path.join(ROOT, "go-sdr_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "go-sdr_amd") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "spectrum-abi ok" in p.stdout

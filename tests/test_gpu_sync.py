"""The coherent-sync path in front of Beamform on the GPU: hzsdr_peak_lag, hzsdr_mean_phase (csrc/hz_kerberos.hip), the
three FFT closures they sit on (csrc/hz_conv.hip, pointwise_mul_kernel of csrc/hz_fft.hip) and the glue of kerberos.py,
against the numpy restatements of tests/sync_ref.py (held to the oracle, and shown able to fail, by
tests/test_sync_ref_cpu.py).  A DEVICE context on torch's stream unless a test says HOST.

The grid of the two reductions, read from the source, not asked of the device: kThreads = 256 (csrc/hz_common.h) and
kRedBlocks = 1024 (csrc/hz_kerberos.hip) give min(ceil(n / 256), 1024) workgroups, a grid-stride of S = 262144 from
n = S on.  The lengths L = 1, 2, 3, 255, 256, 257, 1000, 65536, S - 1, S, S + 1, 2 S + 256, 3 S + 77 reach
    one trip, every thread at most one element        n <= S        (a full last workgroup: 256, 65536, S)
    a partial last workgroup                          1, 2, 3, 255, 257, 1000, S - 1 (255 threads of the 1024th)
    the cap of 1024 workgroups                        S - 1 and up
    two trips                                         S + 1 (one thread takes a second element)
    three trips                                       2 S + 256 (every thread two elements, the first 256 a third)
    four trips                                        3 S + 77 (every thread three, the first 77 a fourth)

Sections:  P  peak search: one-hot sweep, ties, float32 arithmetic, extremes, white noise, HOST and sub-slice routes
           M  mean phase: exactly-once sweep, branch cut, signed zeros, NaN, random data, routes, errors
           C  the closures per sample: every length family, four input classes, lag, state, memory space
           K  check_alignment and phase_offsets

Section M, random data, |mean - fsum mean| / (pi (n + 16) 2^-53), worst over L on an MI355X: 3.5e-2, at n = 2, where
the bound is only 18 pi 2^-53 and the mean is one ulp off; 1.5e-4 at 256, 5.3e-8 and below from 1000 on, and exactly 0
at nine of the thirteen lengths (each printed, `pytest -s`).  The sums are
compensated (Sum2 of csrc/hz_kerberos.hip) since this module's branch-cut case: S + 1 phases of -pi, summed plainly in
the kernel's order, gave a mean 8.5 * 2^-49 from -pi against the 2^-49 the case allows; now it is -pi to the bit.

Section C, worst ratio kernel / max(yardstick, 2^-23), max_sample | rel_l2, over the three kinds, on an MI355X
(printed when the module ends, `pytest -s`):

    family                            noise         impulse       tone          burst
    tiny (1, 2, 3)                    1.36 | 1.14   1.68 | 1.37   0.93 | 0.62   1.12 | 1.18
    radix-4 core (4 ... 128)          1.13 | 1.14   1.67 | 1.12   1.41 | 0.93   1.33 | 1.01
    radix-16 core (256 ... 8192)      1.34 | 1.15   1.60 | 1.30   1.90 | 1.38   1.68 | 1.51
    two-step (2^14 ... 2^18)          1.36 | 1.24   1.39 | 1.40   1.70 | 1.73   1.70 | 1.31
    Bluestein (12, 1000, 4099, 65537) 1.53 | 1.47   1.47 | 1.42   1.72 | 2.73   1.89 | 1.53
    K = 4 (util.FFT_K) for every family: none needs a factor of its own.

The whole module takes 5 s on an MI355X, 3 s of it after the context is open.
"""
import ctypes
import importlib
import math
import time

import numpy as np
import pytest

import sync_ref as R
from sync_ref import LENGTHS, S
from util import FFT_K, Guarded, bits_equal, rand_c64

pytestmark = pytest.mark.gpu

assert (R.THREADS, R.RED_BLOCKS, S) == (256, 1024, 262144)  # kThreads, kRedBlocks: see the docstring

FUSED = [4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192]  # one block of the fused convolution kernels
TINY = [1, 2, 3]
TWO_STEP = [1 << 14, 1 << 15, 1 << 16, 1 << 18]
BLUESTEIN = [12, 1000, 4099, 65537]
CLOSURE_LENGTHS = TINY + FUSED + TWO_STEP + BLUESTEIN

# m(kernel) <= K * max(m(yardstick), 2^-23): the project's FFT_K for every family unless one is named here with its
# measurement (its measured ratio * 1.5 rounded up, at most 8, and for a broadband error only: an error that sits in a
# few samples is a defect whatever its size)
CLOSURE_K = {}

RATIOS = {}  # (family, input class) -> [worst max_sample ratio, worst rel_l2 ratio]
MEAN_WORST = [0.0]
T0 = [None]


@pytest.fixture(scope="module")
def hz():
    return importlib.import_module("go-sdr_amd")


@pytest.fixture(scope="module")
def torch():
    return importlib.import_module("torch")


@pytest.fixture(scope="module")
def ctx(hz, torch):
    T0[0] = time.perf_counter()
    c = hz.Context(0, hz.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


@pytest.fixture(scope="module")
def host(hz):
    c = hz.Context(0, hz.MEM_HOST)
    yield c
    c.close()


@pytest.fixture(scope="module", autouse=True)
def report():
    """Prints what the module measured (`pytest -s`): the figures of the docstring."""
    yield
    print("\nMEAN worst error / bound %.3e" % MEAN_WORST[0], end="")
    for (fam, cls), (ms, l2) in sorted(RATIOS.items()):
        print("\nRATIO %-10s %-8s max_sample %5.2f  rel_l2 %5.2f" % (fam, cls, ms, l2), end="")
    if T0[0] is not None:
        print("\nMODULE %.1f s" % (time.perf_counter() - T0[0]))


def put(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


REF_LAG = {}  # case name -> the restatement's lag, taken (and held to the oracle and the expected value) once


def ref_lag(orc, name, c, want):
    if name not in REF_LAG:
        ref = R.peak_lag(c)
        R.assert_peak(ref, c, orc, want, name)
        REF_LAG[name] = ref
    return REF_LAG[name]


# ---- P. peak search -----------------------------------------------------------------------------------------------------

def test_peak_one_hot_sweep(torch, ctx, orc):
    """One sample (3, -4) in a buffer of zeros, at both ends, either side of every edge: p, or p - n above n // 2."""
    count = 0
    for n in LENGTHS:
        t = torch.zeros(n, dtype=torch.complex64, device="cuda")
        c = np.zeros(n, np.complex64)
        for p in R.hot_positions(n):
            t[p] = complex(3, -4)
            c[p] = R.cval(3, -4)
            R.assert_peak(ctx.peak_lag(t), c, orc, R.fold(p, n), "one-hot n=%d p=%d" % (n, p))
            t[p] = 0
            c[p] = 0
            count += 1
    assert count > 100


@pytest.mark.parametrize("n", [2, 3, 257, 1000, 65536, S + 1, 2 * S + 256, 3 * S + 77], ids=lambda v: "n%d" % v)
def test_peak_ties_the_smallest_index_wins(torch, ctx, orc, n):
    count = 0
    for name, c, want in R.tie_cases(n):
        assert ctx.peak_lag(put(torch, c)) == ref_lag(orc, name, c, want), name
        count += 1
    assert count >= 2


@pytest.mark.parametrize("n", [2, 1000, S + 1], ids=lambda v: "n%d" % v)
def test_peak_power_is_unfused_float32(torch, ctx, orc, n):
    name, c, want, ic, ia = R.arithmetic_case(n)
    assert ic < ia
    a = c[[ia, ic]].view(np.float32).reshape(2, 2)
    f32 = R.powers(c[[ia, ic]])
    f64 = a[:, 0].astype(np.float64) ** 2 + a[:, 1].astype(np.float64) ** 2  # exact, and what a fused sum rounds once
    assert f32[0] == f32[1] == 1 + 2.0 ** -11 and f64[0] > f64[1] and np.float32(f64[0]) > np.float32(f64[1])
    assert ctx.peak_lag(put(torch, c)) == ref_lag(orc, name, c, want), name


@pytest.mark.parametrize("n", [8, 257, 1000, 2 * S + 256], ids=lambda v: "n%d" % v)
def test_peak_extremes(torch, ctx, orc, n):
    """Overflow to +Inf, denormal powers, powers that underflow to 0, NaN, zeros of every sign, all zeros."""
    for name, c, want in R.extreme_cases(n):
        assert ctx.peak_lag(put(torch, c)) == ref_lag(orc, name, c, want), name


def test_peak_white_noise(torch, ctx, orc):
    for n in LENGTHS:
        c = rand_c64(50 + n, n)
        assert ctx.peak_lag(put(torch, c)) == ref_lag(orc, "white noise n=%d" % n, c, None), n


@pytest.mark.parametrize("n", [1000, S + 1, 3 * S + 77], ids=lambda v: "n%d" % v)
def test_peak_host_context(host, orc, n):
    """HOST: 1000 samples go through the 2 MiB staging area, S + 1 and 3 S + 77 samples through a device slot."""
    for name, c, want in R.peak_cases(n):
        keep = c.copy()
        assert host.peak_lag(c) == ref_lag(orc, name, c, want), name
        assert bits_equal(c, keep), name


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", [1000, S + 1, 3 * S + 77], ids=lambda v: "n%d" % v)
def test_peak_on_sub_slices(torch, ctx, orc, n, off):
    """A c64 slice 8-byte aligned only (off = 1): the guards either side and the input itself stay as they were."""
    for name, c, want in R.peak_cases(n):
        g = Guarded(torch, "c64", n, off, c)
        assert ctx.peak_lag(g.t) == ref_lag(orc, name, c, want), (name, off)
        g.check(c, (name, off))


# ---- M. mean phase ------------------------------------------------------------------------------------------------------

def test_mean_exactly_once_sweep(torch, ctx):
    """Every pair (1, 0) (1, 0), phase +0, but one of phase pi / 2: mean * n is pi / 2 to 2^-49 wherever the one sits.
    A dropped or doubled element is off by pi / 2."""
    count = 0
    for n in LENGTHS:
        a = torch.ones(n, dtype=torch.complex64, device="cuda")
        b = torch.ones(n, dtype=torch.complex64, device="cuda")
        for p in R.hot_positions(n):
            a[p] = 1j
            R.assert_census(ctx.mean_phase(a, b), n, math.pi / 2, "census n=%d p=%d" % (n, p))
            a[p] = 1
            count += 1
        # opposite signs in two trips of one thread, and one in each of three trips
        for p in (0, 255, n - S - 1):
            if 0 <= p and p + S < n:
                a[p], a[p + S] = 1j, -1j
                R.assert_census(ctx.mean_phase(a, b), n, 0.0, "census +- n=%d p=%d" % (n, p))
                a[p], a[p + S] = 1, 1
                count += 1
        for p in (0, 76, 255, n - 2 * S - 1):
            if 0 <= p and p + 2 * S < n:
                a[p], a[p + S], a[p + 2 * S] = 1j, 1j, 1j
                R.assert_census(ctx.mean_phase(a, b), n, 3 * (math.pi / 2), "census x3 n=%d p=%d" % (n, p))
                a[p], a[p + S], a[p + 2 * S] = 1, 1, 1
                count += 1
    assert count > 110


@pytest.mark.parametrize("n", [257, S + 1], ids=lambda v: "n%d" % v)
def test_mean_branch_cut(torch, ctx, orc, n):
    """a = (1, 0) against b = (-1, +0): every product is (-1, -0), the mean -pi; against b = (-1, -0) it is +pi."""
    for negative_zero in (False, True):
        a, b = R.cut_pair(n, negative_zero)
        ph = R.phases(a, b)
        want = -math.pi if not negative_zero else math.pi
        assert (ph == want).all()
        assert math.copysign(1.0, orc.mean_phase(a, b)) == math.copysign(1.0, want)
        got = ctx.mean_phase(put(torch, a), put(torch, b))
        print("branch cut n=%d %+.0f pi: got %.17g, off by %.2f * 2^-49" % (n, want / math.pi, got, abs(got - want) * 2.0 ** 49))
        assert math.copysign(1.0, got) == math.copysign(1.0, want), (n, negative_zero, got)
        assert abs(got - want) <= 2.0 ** -49, (n, negative_zero, got, abs(got - want) * 2.0 ** 49)


@pytest.mark.parametrize("n", [16, 257, 1000, S + 1], ids=lambda v: "n%d" % v)
def test_mean_signed_zeros(torch, ctx, n):
    """a = (+-0, +-0) against b = (+-1, +-1): phases +0, -0 and pi, by the signs of the product's zeros."""
    a, b = R.zero_pair(n)
    assert np.isin(np.abs(R.phases(a, b)), [0.0, math.pi]).all() and (R.phases(a, b) == math.pi).any()
    R.assert_mean(ctx.mean_phase(put(torch, a), put(torch, b)), a, b, "zeros n=%d" % n)


@pytest.mark.parametrize("n", [257, 2 * S + 256], ids=lambda v: "n%d" % v)
def test_mean_nan(torch, ctx, n):
    a0, b0 = R.noise_pair(n)
    da, db = put(torch, a0), put(torch, b0)
    assert not math.isnan(ctx.mean_phase(da, db))
    for p in (0, n // 2, n - 1):
        for which, part in (("a", 0), ("a", 1), ("b", 0), ("b", 1)):
            t = da if which == "a" else db
            old = t[p].item()
            t[p] = complex(math.nan, old.imag) if part == 0 else complex(old.real, math.nan)
            assert math.isnan(ctx.mean_phase(da, db)), (n, p, which, part)
            t[p] = old
    R.assert_mean(ctx.mean_phase(da, db), a0, b0, "restored n=%d" % n)


def test_mean_random_data(torch, ctx):
    worst = 0.0
    for n in LENGTHS:
        a, b = R.noise_pair(n)
        r = R.assert_mean(ctx.mean_phase(put(torch, a), put(torch, b)), a, b, "noise n=%d" % n)
        print("mean phase n=%d: error / bound %.3e" % (n, r))
        worst = max(worst, r)
    print("mean phase, worst error / bound over L: %.3e" % worst)
    MEAN_WORST[0] = max(MEAN_WORST[0], worst)


@pytest.mark.parametrize("n", [131072, 131073, S, S + 1], ids=lambda v: "n%d" % v)
def test_mean_host_context(host, n):
    """HOST: at 131072 samples both inputs fit the 2 MiB staging area together, at 131073 and S the first does and the
    second goes through a device slot, at S + 1 neither fits."""
    a, b = R.noise_pair(n)
    ka, kb = a.copy(), b.copy()
    R.assert_mean(host.mean_phase(a, b), a, b, "HOST noise n=%d" % n)
    got = host.mean_phase(a, a)  # one buffer twice: every product is real and positive or zero
    R.assert_mean(got, a, a, "HOST a is b n=%d" % n)
    p = min(n - 1, S)
    a2, b2 = R.census_pair(n, plus=[p])
    R.assert_census(host.mean_phase(a2, b2), n, math.pi / 2, "HOST census n=%d" % n)
    assert bits_equal(a, ka) and bits_equal(b, kb)


@pytest.mark.parametrize("offs", [(0, 1), (1, 0), (1, 1)], ids=lambda v: "off%d_%d" % v)
@pytest.mark.parametrize("n", [1000, S + 1], ids=lambda v: "n%d" % v)
def test_mean_on_sub_slices(torch, ctx, n, offs):
    for name, a, b in ((("noise",) + R.noise_pair(n)), (("census",) + R.census_pair(n, plus=[n - 1]))):
        ga, gb = Guarded(torch, "c64", n, offs[0], a), Guarded(torch, "c64", n, offs[1], b)
        got = ctx.mean_phase(ga.t, gb.t)
        if name == "census":
            R.assert_census(got, n, math.pi / 2, (name, n, offs))
        else:
            R.assert_mean(got, a, b, (name, n, offs))
        ga.check(a, (name, "a", n, offs))
        gb.check(b, (name, "b", n, offs))
    g = Guarded(torch, "c64", n, offs[0], a)
    R.assert_census(ctx.mean_phase(g.t, g.t), n, 0.0, ("a is b", n, offs))  # (0, 1) and (1, 0), conjugated: both +0
    g.check(a, ("a is b", n, offs))


def test_reductions_refuse_null_and_take_nothing(hz, torch, ctx, host):
    bad = hz.ErrInvalidArgument.status
    buf = torch.ones(4, dtype=torch.complex64, device="cuda")
    lag, mean = ctypes.c_int64(7), ctypes.c_double(7.0)
    lib, h, p = hz.lib, ctx._h, buf.data_ptr()
    assert lib.hzsdr_peak_lag(h, None, 4, ctypes.byref(lag)) == bad
    assert lib.hzsdr_peak_lag(h, p, 4, None) == bad
    assert lib.hzsdr_peak_lag(None, p, 4, ctypes.byref(lag)) == bad
    assert lib.hzsdr_mean_phase(h, None, p, 4, ctypes.byref(mean)) == bad
    assert lib.hzsdr_mean_phase(h, p, None, 4, ctypes.byref(mean)) == bad
    assert lib.hzsdr_mean_phase(h, p, p, 4, None) == bad
    assert lib.hzsdr_mean_phase(None, p, p, 4, ctypes.byref(mean)) == bad
    for c, empty in ((ctx, torch.zeros(0, dtype=torch.complex64, device="cuda")), (host, np.zeros(0, np.complex64))):
        assert c.peak_lag(empty) == -1
        assert c.mean_phase(empty, empty) == 0.0
    assert ctx.peak_lag(buf) == 0 and ctx.mean_phase(buf, buf) == 0.0  # the context still works


# ---- C. the closures, per sample ------------------------------------------------------------------------------------------

def make_closure(ctx, kind, dd, dx, dy):
    return {"freq": ctx.convolve_freq, "convolve": ctx.convolve, "xcorr": ctx.cross_correlate}[kind](dd, dx, dy)


def note(n, cls, ratio):
    r = RATIOS.setdefault((R.closure_family(n), cls), [0.0, 0.0])
    r[0], r[1] = max(r[0], ratio[0]), max(r[1], ratio[1])


@pytest.mark.parametrize("n", CLOSURE_LENGTHS, ids=lambda v: "n%d" % v)
def test_closures_per_sample(torch, ctx, n):
    """Each kind's closure is made once for the length and run on every input class from the same three buffers (the
    ConvolveFreq one gets each class's spectrum through set_filter): white noise, x against an impulse at 0, 1, n // 2
    and n - 1 (analytic for convolve and xcorr), a tone pair on one bin, a noise burst against its own rotation."""
    inputs = R.closure_inputs(n)
    dx, dy, dd = (torch.zeros(n, dtype=torch.complex64, device="cuda") for _ in range(3))
    k = CLOSURE_K.get(R.closure_family(n), FFT_K)
    for kind in R.KINDS:
        dy.copy_(put(torch, R.closure_operand(kind, inputs[0][2])))
        cv = make_closure(ctx, kind, dd, dx, dy)
        try:
            for cls, x, y, d in inputs:
                yk = R.closure_operand(kind, y)
                dx.copy_(put(torch, x))
                dy.copy_(put(torch, yk))
                if kind == "freq":
                    cv.set_filter(dy)
                dd.zero_()
                cv()
                ctx.synchronize()
                want = R.impulse_closure_want64(kind, x, d) if (cls == "impulse" and kind != "freq") else None
                note(n, cls, R.assert_closure(dd.cpu().numpy(), kind, x, yk, (kind, n, cls, d), k=k, want64=want))
        finally:
            cv.close()


@pytest.mark.parametrize("n", FUSED + TWO_STEP + BLUESTEIN, ids=lambda v: "n%d" % v)
def test_lag_of_a_delayed_copy(torch, ctx, n):
    """cross_correlate(a, a delayed by d) and then peak_lag: the lag of the float64 correlation, which is the lag the
    delay implies, -d folded above n // 2 -- for n // 2 itself (it stays positive), n // 2 + 1, and odd n."""
    a = rand_c64(60 + n, n)
    da, db, dd = put(torch, a), torch.zeros(n, dtype=torch.complex64, device="cuda"), torch.zeros(n, dtype=torch.complex64, device="cuda")
    cv = ctx.cross_correlate(dd, da, db)
    try:
        for d in (0, 1, -1, n // 2, n // 2 + 1, -(n // 2)):
            b = R.rotate(a, d)
            db.copy_(put(torch, b))
            cv()
            R.assert_lag(ctx.peak_lag(dd), R.closure_want64("xcorr", a, b), n, d, (n, d))
    finally:
        cv.close()


def run_fresh(torch, ctx, kind, x, yk):
    dx, dy, dd = put(torch, x), put(torch, yk), torch.zeros(len(x), dtype=torch.complex64, device="cuda")
    cv = make_closure(ctx, kind, dd, dx, dy)
    cv()
    ctx.synchronize()
    cv.close()
    return dd.cpu().numpy()


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("n", [3, 256, 1000, 65536], ids=lambda v: "n%d" % v)
def test_closure_reads_its_buffers_when_it_runs(torch, ctx, n, kind):
    """Two runs of one closure, its input buffers rewritten in between: the second run is the second input's result,
    the bits a closure made for that input gives."""
    x1, y1 = rand_c64(70 + n, n), R.closure_operand(kind, rand_c64(71 + n, n))
    x2, y2 = rand_c64(72 + n, n), R.closure_operand(kind, rand_c64(73 + n, n))
    dx, dy, dd = put(torch, x1), put(torch, y1), torch.zeros(n, dtype=torch.complex64, device="cuda")
    cv = make_closure(ctx, kind, dd, dx, dy)
    cv()
    first = dd.clone()
    dx.copy_(put(torch, x2))
    if kind == "freq":  # (the filter was taken when the closure was made: only x is read again)
        y2 = y1
    else:
        dy.copy_(put(torch, y2))
    cv()
    ctx.synchronize()
    cv.close()
    assert bits_equal(first.cpu().numpy(), run_fresh(torch, ctx, kind, x1, y1)), (kind, n, "first run")
    got = dd.cpu().numpy()
    assert bits_equal(got, run_fresh(torch, ctx, kind, x2, y2)), (kind, n, "second run")
    R.assert_closure(got, kind, x2, y2, (kind, n, "second run"), k=CLOSURE_K.get(R.closure_family(n), FFT_K))


@pytest.mark.parametrize("n", [256, 4096, 1000], ids=lambda v: "n%d" % v)
def test_set_filter_changes_the_next_run_only(hz, torch, ctx, n):
    """No wait between the first run, the copy of its output, set_filter and the second run: the copy still holds the
    first filter's result (set_filter is ordered behind earlier runs), the second run has the second filter's."""
    x = rand_c64(80 + n, n)
    h1, h2 = R.closure_operand("freq", rand_c64(81 + n, n)), R.closure_operand("freq", R.closure_inputs(n)[1][2])
    dx, dh, dd = put(torch, x), put(torch, h1), torch.zeros(n, dtype=torch.complex64, device="cuda")
    dh2 = put(torch, h2)
    cv = ctx.convolve_freq(dd, dx, dh)
    cv()
    keep = dd.clone()
    cv.set_filter(dh2)
    cv()
    ctx.synchronize()
    k = CLOSURE_K.get(R.closure_family(n), FFT_K)
    assert bits_equal(keep.cpu().numpy(), run_fresh(torch, ctx, "freq", x, h1)), n
    R.assert_closure(keep.cpu().numpy(), "freq", x, h1, (n, "first filter"), k=k)
    assert bits_equal(dd.cpu().numpy(), run_fresh(torch, ctx, "freq", x, h2)), n
    R.assert_closure(dd.cpu().numpy(), "freq", x, h2, (n, "second filter"), k=k)
    with pytest.raises(hz.ErrLengthMismatch):
        cv.set_filter(dh2[:n - 1])
    with pytest.raises(hz.ErrLengthMismatch):
        cv.set_filter(torch.zeros(n + 1, dtype=torch.complex64, device="cuda"))
    cv()
    ctx.synchronize()
    assert bits_equal(dd.cpu().numpy(), run_fresh(torch, ctx, "freq", x, h2)), (n, "a refused set_filter changed the filter")
    cv.close()


def test_closure_refusals(hz, torch, ctx):
    n = 64
    dx, dy, dd = (torch.zeros(n, dtype=torch.complex64, device="cuda") for _ in range(3))
    for kind in ("convolve", "xcorr"):
        cv = make_closure(ctx, kind, dd, dx, dy)
        with pytest.raises(hz.ErrInvalidArgument):
            cv.set_filter(dy)
        cv.close()
    for mode in (-1, 2, 7):
        out = ctypes.c_void_p()
        rc = hz.lib.hzsdr_convolve_create(ctx._h, dd.data_ptr(), n, dx.data_ptr(), n, dy.data_ptr(), n, mode, ctypes.byref(out))
        assert rc == hz.ErrInvalidArgument.status and not out.value, mode
    assert hz.lib.hzsdr_conv_exec(None) == hz.ErrInvalidArgument.status


@pytest.mark.parametrize("n", FUSED, ids=lambda v: "n%d" % v)
def test_convolve_freq_is_one_block_of_convolution_blocks(torch, ctx, n):
    """Both go through conv_blocks_device with one block: the same bits."""
    x, h = rand_c64(90 + n, n), R.closure_operand("freq", rand_c64(91 + n, n))
    dx, dh, out = put(torch, x), put(torch, h), torch.zeros(n, dtype=torch.complex64, device="cuda")
    assert ctx.convolution_blocks(out, dx, dh) == n
    ctx.synchronize()
    assert bits_equal(out.cpu().numpy(), run_fresh(torch, ctx, "freq", x, h)), n


@pytest.mark.parametrize("n", [2, 64, 1024, 65536, 1000], ids=lambda v: "n%d" % v)
def test_closures_host_context_same_bits(torch, ctx, host, n):
    """One length per family, HOST buffers: the bits of the DEVICE run, and the inputs untouched."""
    for kind in R.KINDS:
        x, yk = rand_c64(95 + n, n), R.closure_operand(kind, rand_c64(96 + n, n))
        kx, ky = x.copy(), yk.copy()
        dst = np.zeros(n, np.complex64)
        cv = make_closure(host, kind, dst, x, yk)
        cv()
        cv.close()
        assert bits_equal(dst, run_fresh(torch, ctx, kind, x, yk)), (kind, n)
        assert bits_equal(x, kx) and bits_equal(yk, ky), (kind, n)


# ---- K. the glue ----------------------------------------------------------------------------------------------------------

DELAYS = [0, 5, -9, 130]


def delayed_channels(n):
    base = rand_c64(97, n + 1000)
    return [base[500 - d:500 - d + n].copy() for d in DELAYS]


@pytest.mark.parametrize("n", [4096, 4099], ids=lambda v: "n%d" % v)
def test_check_alignment_four_readers(host, n):
    K = importlib.import_module("go-sdr_amd.kerberos")
    St = importlib.import_module("go-sdr_amd.stream")
    chans = delayed_channels(n)
    want = [0] + [R.peak_lag(R.closure_want64("xcorr", chans[0], c).astype(np.complex64)) for c in chans[1:]]
    assert want == [-d for d in DELAYS]
    for quirk in (False, True):
        readers = [St.BufferReader(c, 2_400_000) for c in chans]
        bufs = [np.zeros(n, np.complex64) for _ in chans]
        lags = K.check_alignment(host, readers, bufs, reference_quirk=quirk)
        assert lags == ([0] + [want[1]] * 3 if quirk else want), (n, quirk)
        for b, c in zip(bufs, chans):
            assert bits_equal(b, c)


def test_phase_offsets_four_readers(host):
    K = importlib.import_module("go-sdr_amd.kerberos")
    St = importlib.import_module("go-sdr_amd.stream")
    n = 4096
    a = rand_c64(98, n)
    chans = [a]
    for k, ang in enumerate((0.7, -2.1, 3.0)):
        y = (a.astype(np.complex128) * np.exp(1j * ang)).astype(np.complex64)
        chans.append(y + (np.float32(0.01) * rand_c64(99 + k, n).view(np.float32)).view(np.complex64))
    offs = K.phase_offsets(host, [St.BufferReader(c, 2_400_000) for c in chans], n=n)
    assert offs.dtype == np.complex64 and len(offs) == 4
    for j in (1, 2, 3):
        mean = R.mean_phase_exact(chans[0], chans[j])
        assert abs(offs[j] - complex(math.cos(mean), math.sin(mean))) <= 1e-6, j
    assert abs(mean - (-3.0)) < 1e-2  # (the last pair: the sign of the rotation it cancels)
    assert abs(offs[0] - complex(math.cos(1 / n), math.sin(1 / n))) <= 1e-6  # the reference's phases[0] = 1

"""The int8 matrix FIR (csrc/hz_firmm.h, csrc/hz_firmm2.h) BIT FOR BIT against exact integer sums (tests/firmm_ref.py,
itself held to the planner headers and to the float64 oracle by tests/test_firmm_ref_cpu.py).

The headers promise "exact integer arithmetic on the quantised taps, one float32 rounding".  Chains without an
elementwise stage, i8 and u8 sources, 8192 outputs per call:
  * the persistent-pass kernel (forms P8: per-plane loop at 1017 .. 1024 taps, P8pair: pair loop, P16) must return
    RN32(2^-S (sum_k q[k] b[m D - k] + dc)) on every output that is not a fix-up output -- every bit of every digit
    plane, every carry of the balanced digits and both ends of the plane-0 window are then visible: a wrong byte of
    the lowest plane is 2^-30 of the largest tap, far below every tolerance of the other FIR tests;
  * the chunk form (C8: FIR_IMPL_MATRIX_CHUNKS, C32, and whatever the persistent passes refuse) forms its low pair of
    planes in float32: it must lie in firmm_ref.chunk_form_interval, which is a single float32 for >= 90 % of the parts;
  * which kernel ran is asserted at every eligibility edge (16 taps, the per-plane loop's 1017 .. 1024, the last tap
    count of the persistent passes at either factor and the next one, int32_combine_ok's bound from both sides).
Fix-up outputs -- the outputs at a stream start whose window crosses it, rounded up to the planner's tile -- are
float64 sums over the UNQUANTISED taps (both kernels' tasks): exact too where the filter is dyadic (families A, B, C
under i8: EVERY output is compared), held to the oracle with assert_fir_close otherwise, and counted.  (Family E found
the persistent passes' tasks summing in float32 chains, 3.9e-7 from the oracle in relative L2 under a boxcar and a
constant input; they sum in float64 since.)

Families (firmm_ref.py): A one digit plane at a time, B digit carries, C the plane-0 window, D tap read-out by
impulses around every pass / chunk / call boundary, E boxcars on int32_combine_ok's bound, F general filters."""
import importlib

import numpy as np
import pytest

import firmm_ref as R
from util import assert_fir_close, rand_i8, rand_u8, zeros

pytestmark = pytest.mark.gpu

SENTINEL = np.complex64(7 + 7j)  # what an output holds before its call: an output nobody wrote fails the comparison


@pytest.fixture(scope="module")
def hz():
    return importlib.import_module("go-sdr_amd")


@pytest.fixture(scope="module")
def dev(hz):
    import torch
    c = hz.Context(0, hz.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


@pytest.fixture(scope="module")
def host(hz):
    c = hz.Context(0, hz.MEM_HOST)
    yield c
    c.close()


def run_stream(hz, ctx, device, form, fmt, taps, x, calls=None, batch=None):
    """The stream x through one chain of kernel form `form`.  calls: [(first output, end output)] per call (default: one
    call); batch: (buffers, after) -- the whole stream as ONE call over that many equal buffers.
    -> (outputs, [(path, kernel) per call])."""
    f = R.FORMS[form]
    D = f["D"]
    n_out = len(x) // D
    ch = ctx.chain(hz.FMT_U8 if fmt == "u8" else hz.FMT_I8, 20_000_000)
    ch.fir_options(hz.FIR_IMPL_MATRIX_CHUNKS if f["chunks"] else hz.FIR_IMPL_AUTO, 0, f["loop"])
    ch.fir_decimate(taps, D)
    if device:
        import torch
        xin = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        out = torch.full((n_out,), complex(SENTINEL), dtype=torch.complex64, device="cuda")
        torch.cuda.synchronize()
    else:
        xin, out = np.ascontiguousarray(x), np.full(n_out, SENTINEL, np.complex64)
    ran = []
    if batch:
        k, after = batch
        each = n_out // k
        assert each * k == n_out
        if after:
            ch.pipeline(True)
        got = ch.run_batch([xin[j * each * D:(j + 1) * each * D] for j in range(k)], [out[j * each:(j + 1) * each] for j in range(k)], after=after)
        assert got == (each * D, each)
        ran.append((ch.last_fir_path(), ch.last_fir_kernel()))
    else:
        for a, b in calls or [(0, n_out)]:
            assert ch.run(xin[a * D:b * D], out[a:b]) == ((b - a) * D, b - a)
            ran.append((ch.last_fir_path(), ch.last_fir_kernel()))
    ctx.synchronize()
    res = out.cpu().numpy() if device else out
    ch.close()
    return res, ran


def oracle_outputs(orc, x, taps, D):
    xc = zeros("c64", len(x))
    orc.convert(xc, x)
    want = zeros("c64", len(x) // D)
    orc.par_fir_decimate_f64(want, xc, taps, D)
    return want, float(np.abs(xc).max())


def check(hz, orc, got, ran, form, fmt, taps, x, what, starts=(0,), transform=(), combine=None):
    """`got` against the exact reference.  starts: the outputs at which a stream (re)starts for the matrix path -- 0, and
    the first output of a matrix call behind a call on the transform kernels; transform: [(a, b)] output ranges of calls
    the transform kernels ran (held to the oracle only); combine: int32_combine_ok where the test knows it (family E)."""
    D = R.FORMS[form]["D"]
    nt, n_out = len(taps), len(x) // D
    passes = R.takes_passes(form, taps, fmt, combine)
    kernel = hz.FIR_KERNEL_MATRIX_PASSES if passes else hz.FIR_KERNEL_MATRIX_CHUNKS
    matrix_calls = [r for r in ran if r[0] == hz.FIR_PATH_MATRIX]
    assert len(matrix_calls) == len(ran) - len(transform), (what, ran)
    assert all(k == kernel for _, k in matrix_calls), (what, "expected kernel", kernel, ran)
    S, q = R.shift_of(taps, fmt), R.quantise(taps, fmt)
    dc = R.dc_of(q, fmt)
    ex = R.exact_outputs(q, dc, R.signed_bytes(x, fmt), D, planes=not passes)
    # the outputs that leave the exact comparison: per stream start, ceil((ntaps - 1) / D) rounded up to the planner's
    # tile (8 outputs on the persistent passes, 16 on the chunk form) -- and none at all when the filter is dyadic
    exactly = np.ones(n_out, bool)
    fix = 0 if R.dyadic(taps, fmt) else R.fixup_outputs(nt, D, 8 if passes else 16)
    for s in starts:
        exactly[s:s + fix] = False
    for a, b in transform:
        exactly[a:b] = False
    left_out = int((~exactly).sum()) - sum(b - a for a, b in transform)
    window = -(-(nt - 1) // D)
    assert left_out <= len(starts) * (window + (7 if passes else 15)), (what, left_out)
    if window % 16 == 0:
        assert left_out <= len(starts) * window, (what, left_out)  # (128 of 8192 at 1024 taps and D = 8, 192 at 1536)
    g = np.ascontiguousarray(got).view(np.float32).reshape(-1, 2)
    if passes:
        want = R.rn32_complex(ex, S, dc).view(np.float32).reshape(-1, 2)
        bad = (g.view(np.int32) != want.view(np.int32)) & exactly[:, None]
        if bad.any():
            m, part = (int(v) for v in np.argwhere(bad)[0])
            raise AssertionError("%s: %d of %d parts are not RN32(exact); the first: output %d part %d, got %r, exact %r (%d units of 2^-%d)"
                                 % (what, int(bad.sum()), 2 * int(exactly.sum()), m, part, g[m, part], want[m, part],
                                    int((ex.re, ex.im)[part][m]), S))
    else:
        same = 0
        for part in (0, 1):
            lo, hi = R.chunk_form_interval(ex.planes[part], dc[part], S)
            bad = ~((lo <= g[:, part]) & (g[:, part] <= hi)) & exactly
            if bad.any():
                m = int(np.flatnonzero(bad)[0])
                raise AssertionError("%s: %d outputs outside the chunk form's interval; the first: output %d part %d, got %r, interval [%r, %r]"
                                     % (what, int(bad.sum()), m, part, g[m, part], lo[m], hi[m]))
            same += int(((lo == hi) & exactly).sum())
        assert same >= 0.9 * 2 * int(exactly.sum()), (what, "the interval is a single float for", same, "parts of", 2 * int(exactly.sum()))
    if not exactly.all():
        want, xmax = oracle_outputs(orc, x, taps, D)
        assert_fir_close(got[~exactly], want[~exactly], taps, xmax, (what, "fix-up / transform outputs"))


# ---- A: one digit plane at a time, at every tap count of the eligibility sweep ------------------------------------

@pytest.mark.parametrize("form,ntaps", R.SWEEP)
def test_one_digit_plane_at_a_time(hz, dev, orc, form, ntaps):
    """Family A: every tap but the anchor lives in ONE digit plane and the anchor reads zeros, so every output is a small
    integer of that plane's unit and a single wrong digit byte anywhere changes it."""
    D = R.FORMS[form]["D"]
    for d in range(4):
        for k0 in (0, 1):
            taps, x = R.family_a(ntaps, d, k0, 100 + d), R.signal_a(R.N_OUT * D, D, k0, 200 + d)
            got, ran = run_stream(hz, dev, True, form, "i8", taps, x)
            check(hz, orc, got, ran, form, "i8", taps, x, ("A", form, ntaps, d, k0))


# ---- B: the balanced digits' carries -----------------------------------------------------------------------------------

@pytest.mark.parametrize("imag", [False, True])
@pytest.mark.parametrize("form,ntaps", [("P8", 1024), ("P8", 17), ("P8pair", 1024), ("P16", 1024), ("C8", 1024), ("C32", 1024)])
def test_digit_carries(hz, dev, orc, form, ntaps, imag):
    """Family B: the coefficients at which a balanced digit carries (+-127 .. +-129, +-32639 .. 32896, 127 W, 127 W + 1,
    -128 W, -128 W - 1, 2^23 - 1, 2^23, 2^29, 2^30 - 64), read out by impulses."""
    D = R.FORMS[form]["D"]
    x = R.d_signal("i8", ntaps, D)
    for v in R.CARRY_VALUES:
        taps = R.family_b(ntaps, v, imag)
        got, ran = run_stream(hz, dev, True, form, "i8", taps, x)
        check(hz, orc, got, ran, form, "i8", taps, x, ("B", form, ntaps, v, imag))


# ---- C: the plane-0 window --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cold", [127 * R.W, 127 * R.W - 1])
@pytest.mark.parametrize("form", list(R.FORMS))
def test_plane0_window(hz, dev, orc, form, cold):
    """Family C: ONE tap with a top digit (127 W + 1, or a complex tap with cold parts and a hot modulus) among cold ones,
    next to either end of the filter and in the middle; a window one pair short drops 2^24 x from an output."""
    D = R.FORMS[form]["D"]
    x = rand_i8(31, R.N_OUT * D)
    filters = [(k, m, R.family_c(1024, k, m, cold=cold)) for k in R.hot_positions(1024) for m in (False, True)]
    filters.append((512, "modulus", R.family_c(1024, 512, modulus=True, cold=cold)))
    for k, m, taps in filters:
        got, ran = run_stream(hz, dev, True, form, "i8", taps, x)
        check(hz, orc, got, ran, form, "i8", taps, x, ("C", form, cold, k, m))


# ---- D: tap read-out by impulses ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["i8", "u8"])
@pytest.mark.parametrize("form,ntaps", [("P8", 1024), ("P8", 17), ("P8pair", 1024), ("P16", 1024), ("C8", 1024), ("C8", 1536), ("C32", 1024), ("C32", 17)])
def test_tap_read_out_by_impulses(hz, dev, orc, form, ntaps, fmt):
    """Family D: general complex taps over twenty binades; single nonzero samples at least ntaps + 16 D apart, on every
    residue mod 16 and just before, at and after every pass and chunk boundary: an output IS one tap times one byte."""
    D = R.FORMS[form]["D"]
    taps, x = R.family_d(ntaps, 40 + ntaps), R.d_signal(fmt, ntaps, D)
    got, ran = run_stream(hz, dev, True, form, fmt, taps, x)
    check(hz, orc, got, ran, form, fmt, taps, x, ("D", form, ntaps, fmt))


@pytest.mark.parametrize("fmt", ["i8", "u8"])
@pytest.mark.parametrize("form", list(R.FORMS))
def test_three_ragged_calls(hz, dev, orc, form, fmt):
    """Three calls with cuts on the 64 D grid, impulses around the cuts: the windows of a call's first outputs reach into
    the previous call's raw bytes.  Only the stream's own start has fix-up outputs."""
    D = R.FORMS[form]["D"]
    cuts = R.ragged_cuts()
    taps, x = R.family_d(1024, 77), R.d_signal(fmt, 1024, D, cuts)
    got, ran = run_stream(hz, dev, True, form, fmt, taps, x, calls=list(zip(cuts[:-1], cuts[1:])))
    check(hz, orc, got, ran, form, fmt, taps, x, ("ragged D", form, fmt))
    x = (rand_i8 if fmt == "i8" else rand_u8)(78, cuts[-1] * D)
    got, ran = run_stream(hz, dev, True, form, fmt, taps, x, calls=list(zip(cuts[:-1], cuts[1:])))
    check(hz, orc, got, ran, form, fmt, taps, x, ("ragged white", form, fmt))


# ---- E: the int32 sum of the two top planes at its limit --------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["i8", "u8"])
@pytest.mark.parametrize("kind", ["real", "diag"])
def test_int32_top_pair_sum_at_its_limit(hz, dev, orc, kind, fmt):
    """Family E: a real and a 45-degree 1024-tap boxcar at the largest float32 amplitude int32_combine_ok accepts (the
    persistent passes must take it, and stay exact under the inputs that line all signs up) and at the next float32
    (the chunk form must take it)."""
    e = R.family_e(kind, fmt)
    for name, x in R.signals_e(fmt, R.N_OUT * 8).items():
        for which, form in (("accepted", "P8"), ("accepted", "P8pair"), ("accepted", "C8"), ("refused", "P8")):
            got, ran = run_stream(hz, dev, True, form, fmt, e[which], x)
            want = hz.FIR_KERNEL_MATRIX_PASSES if (which, form) in (("accepted", "P8"), ("accepted", "P8pair")) else hz.FIR_KERNEL_MATRIX_CHUNKS
            assert ran == [(hz.FIR_PATH_MATRIX, want)], (kind, fmt, which, form, ran)
            check(hz, orc, got, ran, form, fmt, e[which], x, ("E", kind, fmt, which, form, name), combine=which == "accepted")


# ---- F: general filters -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["i8", "u8"])
@pytest.mark.parametrize("form,name", [(form, name) for form in R.FORMS for name in R.F_ON[form]])
def test_general_filters(hz, dev, orc, form, name, fmt):
    """Family F: the bench's low-pass, a floor under it (every tap has a top digit), the peak at either end, random
    complex filters -- under white bytes, the constant extremes and the alternating extremes."""
    D = R.FORMS[form]["D"]
    taps = R.family_f()[name]
    for sname, x in R.signals_f(fmt, R.N_OUT * D).items():
        got, ran = run_stream(hz, dev, True, form, fmt, taps, x)
        check(hz, orc, got, ran, form, fmt, taps, x, ("F", form, name, fmt, sname))


# ---- streams ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["i8", "u8"])
@pytest.mark.parametrize("form", ["P8", "C8"])
def test_host_context(hz, host, orc, form, fmt):
    """HOST space once (every other case runs on device buffers): the bench filter under white bytes."""
    D = R.FORMS[form]["D"]
    taps, x = R.family_f()["bench"], (rand_i8 if fmt == "i8" else rand_u8)(91, R.N_OUT * D)
    got, ran = run_stream(hz, host, False, form, fmt, taps, x)
    check(hz, orc, got, ran, form, fmt, taps, x, ("host", form, fmt))


@pytest.mark.parametrize("after", [False, True])
@pytest.mark.parametrize("form", ["P8", "P16"])
def test_call_over_two_buffers(hz, dev, orc, form, after):
    """hzsdr_chain_run_batch over two buffers of 8192 outputs, plain and overlapped: the second buffer's first windows
    reach back into the first buffer.  A family-A filter per digit plane and the bench filter
    under white u8 bytes."""
    D = R.FORMS[form]["D"]
    n = 2 * R.N_OUT * D
    for d in range(4):
        taps, x = R.family_a(1024, d, d & 1, 100 + d), R.signal_a(n, D, d & 1, 300 + d)
        got, ran = run_stream(hz, dev, True, form, "i8", taps, x, batch=(2, after))
        check(hz, orc, got, ran, form, "i8", taps, x, ("batch A", form, after, d))
    taps, x = R.family_f()["bench"], rand_u8(92, n)
    got, ran = run_stream(hz, dev, True, form, "u8", taps, x, batch=(2, after))
    check(hz, orc, got, ran, form, "u8", taps, x, ("batch bench", form, after))


@pytest.mark.parametrize("form", ["P8", "P16", "C8"])
def test_matrix_transform_matrix(hz, dev, orc, form):
    """A matrix call, a call of 1000 outputs (too short: the transform kernels), a matrix call, on a dyadic filter: the
    float history the transform call leaves is exact for dyadic data, so the fix-up outputs at the third call's start
    are exact and BOTH matrix calls are compared on every output; the transform call's outputs are held to the oracle."""
    D = R.FORMS[form]["D"]
    a, b = R.N_OUT, R.N_OUT + 1000
    calls = [(0, a), (a, b), (b, b + R.N_OUT)]
    # (plane 0: the taps beside the anchor are of its size, so the oracle's relative bound means something for the
    # transform call; the anchor reads zeros all the same)
    taps, x = R.family_a(1024, 0, 1, 100), R.signal_a((b + R.N_OUT) * D, D, 1, 500)
    got, ran = run_stream(hz, dev, True, form, "i8", taps, x, calls=calls)
    assert [p for p, _ in ran] == [hz.FIR_PATH_MATRIX, hz.FIR_PATH_TRANSFORM, hz.FIR_PATH_MATRIX], ran
    check(hz, orc, got, ran, form, "i8", taps, x, ("matrix, transform, matrix", form), starts=(0, b), transform=[(a, b)])

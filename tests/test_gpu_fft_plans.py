"""FFT plans per bin, per transform and across workgroup boundaries (through the C ABI, device context).

What the older FFT tests of tests/test_gpu_parity.py cannot see: they run two or three transforms per plan (one partly
filled workgroup of the LDS kernels, never a second one, never a launch that ends on a workgroup boundary), never more
transforms than one piece of Bluestein's batch loop holds, and they score a transform of random input by ONE relative-L2
number against 3e-7 log2 N + 1e-7 -- a bound that a single wrong twiddle-table entry passes at every size
(tests/test_fft_checker_cpu.py).

The bar (tests/util.py, assert_fft_close): with want64 the float64 transform of the float32 input as stored (analytic for
impulses), and the yardstick a single-precision transform of the same input (scipy's complex64 pocketfft; for a length
that is not a power of two a float32 Bluestein over it, the algorithm the kernels implement),

    m(kernel) <= K * max(m(yardstick), 2**-23)    for m in (max_bin, rel_l2),    K = 4 for every kernel family,

max_bin = max_k |got_k - want_k| / max_k |want_k|.  An honest textbook float32 transform with the kernels' split
twiddle form measures <= 1.7 there; one table entry off by 1e-5 measures 23 ... 57.

Sections:  B  structured inputs per bin, every dispatch of fft_device, forward and backward
           C  batches either side of every workgroup boundary into guarded slices (plans and convolution_blocks);
              plans on c64 sub-slices one sample off 16-byte alignment
           D  a transform's bits do not depend on its neighbours, on NaN / Inf beside it, on the memory space, or on
              how often the plan runs
           E  Bluestein past the first piece of its batch loop (plans and convolution_blocks)
           F  a two-step batch beyond the device's grid height is refused when the plan is made

Observed worst ratio kernel / max(yardstick, 2^-23), max_bin | rel_l2, over sections B, C and E on an MI355X
(forward and backward; printed when the module ends, `pytest -s`):

    family                            random        impulse       tone_on_bin   tone_off_bin  dc            alternating
    radix-4 core (4 ... 128)          1.36 | 0.88   1.00 | 0.54   0.21 | 0.40   0.81 | 0.85   0.00 | 0.00   0.00 | 0.00
    radix-16 core (256 ... 8192)      1.59 | 1.08   1.43 | 0.97   0.99 | 1.23   1.38 | 1.33   0.00 | 0.00   0.00 | 0.00
    two-step N1 x N2 (2^14 ... 2^24)  1.42 | 1.13   1.75 | 1.60   1.00 | 1.50........................................................................................................................................................................................1.36 | 1.29   0.00 | 0.00   0.00 | 0.00
    Bluestein (any other length)      1.95 | 1.49   1.77 | 1.66   2.03 | 1.50   2.30 | 1.56   1.11 | 1.36   2.17 | 1.44
    K = 4 for every family: none needs a factor of its own.

In the two-step lengths the XCD-contiguous tile order of fft2_tile applies when a launch's tile count is a multiple of
eight.  A transform has 4 column tiles at 2^14, 8 at 2^15 and a multiple of 8 from 2^16 on, so only 2^14 with an odd
batch takes the other branch; D runs every length with a batch of 3 and of 8."""
import ctypes
import importlib
import re

import numpy as np
import pytest

from util import (SENT, Guarded, assert_fft_close, assert_fft_rows_close, bits_equal, fft_inputs, fft_want64, rand_c64,
                  zeros)

pytestmark = pytest.mark.gpu

POW2_LDS = [4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192]
POW2_TWO_STEP = [1 << 14, 1 << 15, 1 << 16, 1 << 17, 1 << 18, 1 << 20, 1 << 22, 1 << 24]  # every N1 x N2 of two_step_n1
ANY = [12, 1000, 1536, 4099, 3 << 15, 100_003, (1 << 20) + 7]
PIECE = 1 << 25  # fft_bluestein walks a batch in pieces of max(1, 2^25 / M) transforms


def xpb(n):
    """Transforms per workgroup of the plan kernels: fft_xpb (hz_fft.h) below 256, fv::xpb (hz_fftv.h) from there."""
    return {4: 64, 8: 32, 16: 16, 32: 8, 64: 4, 128: 2, 256: 4, 512: 2}.get(n, 1)


def family(n):
    if n & (n - 1):
        return "bluestein"
    return "radix-4" if n < 256 else ("radix-16" if n <= 8192 else "two-step")


def chirp_m(n):
    m = 1
    while m < 2 * n - 1:
        m <<= 1
    return m


RATIOS = {}  # (family, input class) -> [worst max_bin ratio, worst rel_l2 ratio]


def note(n, cls, ratio):
    r = RATIOS.setdefault((family(n), cls), [0.0, 0.0])
    r[0], r[1] = max(r[0], ratio[0]), max(r[1], ratio[1])


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


@pytest.fixture(scope="module")
def host(hz):
    c = hz.Context(0, hz.MEM_HOST)
    yield c
    c.close()


def plan_of(hz, ctx, src, dst, fwd, batch):
    """A plan that reads `src` and writes `dst` in either direction (forward: iq -> frequency)."""
    return ctx.fft_plan(src, dst, hz.FFT_FORWARD, batch=batch) if fwd else ctx.fft_plan(dst, src, hz.FFT_BACKWARD, batch=batch)


def run(hz, torch, ctx, x, n, fwd):
    """x: batch * n samples (numpy) -> the device plan's output (numpy)."""
    src = torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).cuda()
    dst = torch.zeros_like(src)
    p = plan_of(hz, ctx, src, dst, fwd, src.shape[0] // n)
    p.transform()
    ctx.synchronize()
    p.close()
    return dst.cpu().numpy()


def gauss(seed, count):
    rng = np.random.default_rng(seed)
    x = np.empty(count, np.complex64)
    v = x.view(np.float32)
    v[:] = rng.standard_normal(2 * count, dtype=np.float32)
    return x


DIRS = [(True, "forward"), (False, "backward")]


@pytest.fixture(scope="module", autouse=True)
def report_ratios():
    """Prints what the module measured (`pytest -s`): the table of the docstring and of DESIGN.md section 4."""
    yield
    for (fam, cls), (mb, l2) in sorted(RATIOS.items()):
        print("\nRATIO %-10s %-12s max_bin %5.2f  rel_l2 %5.2f" % (fam, cls, mb, l2), end="")


# ---- B. structured inputs, per bin -----------------------------------------------------------------------------------

@pytest.mark.parametrize("n", POW2_LDS + POW2_TWO_STEP + ANY)
def test_structured_inputs_per_bin(hz, torch, ctx, n):
    """Every input of util.fft_inputs as one transform of ONE batched plan, each checked on its own against float64
    (impulses: the analytic exp(-+2 pi i p k / N), every twiddle product of every pass a visible unit-magnitude bin).
    From 2^22 on: random, two impulses and one tone; at 2^24 without the tone, which costs the host a float64
    transform of its own where an impulse costs none (the module has a quarter of the older GPU suite's wall time to
    live in).  The backward expectation of an input without an analytic one is
    the forward one read backwards, ifft(x) N [k] = fft(x) [-k mod N]: one float64 transform per input."""
    ins = fft_inputs(n, few=n >= (1 << 22))
    if n >= (1 << 24):
        ins = [i for i in ins if i[0] != "tone_off_bin"]
    x = np.concatenate([i[1] for i in ins])
    wants = [i[2] if i[2] is not None else fft_want64(i[1], True) for i in ins]
    for fwd, dname in DIRS:
        got = run(hz, torch, ctx, x, n, fwd).reshape(len(ins), n)
        for j, (cls, xi, _, wb) in enumerate(ins):
            want = wants[j] if fwd else (wb if wb is not None else np.roll(wants[j][::-1], 1))
            note(n, cls.split("@")[0], assert_fft_close(got[j], xi, want, fwd, "n=%d %s %s" % (n, dname, cls)))


# ---- C. workgroup boundaries and guard bands -------------------------------------------------------------------------

def boundary_batches(x):
    return sorted({b for b in (1, x - 1, x, x + 1, 2 * x + 1, 1000 * x + max(1, x // 2)) if b > 0})


def sampled(batch, x):
    """All of a small batch; of a large one the first, the last, the first and last of the last workgroup, every 97th."""
    if batch <= 4 * x + 4:
        return list(range(batch))
    last_wg = (batch - 1) // x * x
    return sorted(set(range(0, batch, 97)) | {0, 1, x - 1, x, last_wg - 1, last_wg, batch - 1})


def no_sentinel_left(values, what):
    left = np.flatnonzero(np.ascontiguousarray(values).view(np.uint32) == 0xA5A5A5A5)
    assert left.size == 0, (what, "output words never written", left.size, "first in sample", int(left[0]) // 2)


@pytest.mark.parametrize("n", [4, 8, 16, 32, 64, 128, 256, 512, 1024, 8192])
def test_plan_batches_either_side_of_a_workgroup(hz, torch, ctx, n):
    """Batches of 1, XPB - 1, XPB, XPB + 1, 2 XPB + 1 and 1000 XPB + max(1, XPB / 2) transforms of distinct data (one
    seeded stream, a transform's data follows from its index) into a sentinel-filled guarded slice: a dead sub-region
    that stores shows in the guard, a live one that does not leaves sentinel words, two that are swapped or overlap in
    LDS fail the value check."""
    X = xpb(n)
    for batch in boundary_batches(X):
        x = gauss(n * 1_000_003 + batch, n * batch)
        pick = sampled(batch, X)
        xs = x.reshape(batch, n)[pick]
        for fwd, dname in DIRS:
            what = "n=%d batch=%d %s" % (n, batch, dname)
            src = torch.from_numpy(x).cuda()
            dst = Guarded(torch, "c64", n * batch, 0)
            p = plan_of(hz, ctx, src, dst.t, fwd, batch)
            p.transform()
            ctx.synchronize()
            p.close()
            dst.check(None, what)
            got = dst.values()
            no_sentinel_left(got, what)
            assert bits_equal(src.cpu().numpy(), x), (what, "the input was written")
            note(n, "random", assert_fft_rows_close(got.reshape(batch, n)[pick], xs, fwd, what + " transforms %s..." % pick[:8]))


def _lowpass_bins(n):
    t = np.arange(n) - (n - 1) / 2
    h = np.sinc(t / 8) / 8 * np.hamming(n)
    return np.fft.fft(h.astype(np.complex128) / n).astype(np.complex64)


def _rel_l2(got, want):
    want = want.astype(np.complex128)
    return float(np.linalg.norm(got.astype(np.complex128) - want) / max(np.linalg.norm(want), 1e-30))


def check_conv_blocks(torch, ctx, orc, flen, nblk, pick, seed):
    """convolution_blocks over nblk whole blocks and half a block, into a guarded sentinel-filled slice: the sampled
    blocks against the oracle at relative L2 <= 2e-6 each, the partial block's output and the guards untouched."""
    what = "flen=%d blocks=%d" % (flen, nblk)
    n = nblk * flen + flen // 2
    x = gauss(seed, n)
    H = _lowpass_bins(flen)
    out = Guarded(torch, "c64", n, 0)
    assert ctx.convolution_blocks(out.t, torch.from_numpy(x).cuda(), torch.from_numpy(H).cuda()) == nblk * flen, what
    ctx.synchronize()
    out.check(None, what)
    got = out.values()
    no_sentinel_left(got[:nblk * flen], what)
    assert (got[nblk * flen:].view(np.uint8) == SENT).all(), (what, "the partial block was written")
    xs = np.concatenate([x[b * flen:(b + 1) * flen] for b in pick])
    want = zeros("c64", len(xs))
    assert orc.convolution_reader(want, xs, H) == len(xs)
    for i, b in enumerate(pick):
        assert _rel_l2(got[b * flen:(b + 1) * flen], want[i * flen:(i + 1) * flen]) < 2e-6, (what, "block", b)


@pytest.mark.parametrize("flen", [4, 8, 16, 32, 64, 128])
def test_convolution_blocks_either_side_of_a_workgroup(torch, ctx, orc, flen):
    """conv_blocks_kernel (blocks shorter than 256) packs fft_xpb blocks into a workgroup like the plan kernel: the
    same block counts."""
    X = xpb(flen)
    for nblk in boundary_batches(X):
        check_conv_blocks(torch, ctx, orc, flen, nblk, sampled(nblk, X), flen * 7919 + nblk)


@pytest.mark.parametrize("n,batch", [(64, 5), (1024, 3), (1 << 16, 2), (1000, 3)])
def test_plan_on_sub_slices_one_sample_off_alignment(hz, torch, ctx, n, batch):
    """What a Go caller's buf[1:] hands over: both buffers 8 bytes past 16-byte alignment (the packed-math kernels move
    8-byte elements; nothing may assume more)."""
    x = rand_c64(n + 17, n * batch)
    for fwd, dname in DIRS:
        what = "n=%d %s off=1" % (n, dname)
        src, dst = Guarded(torch, "c64", n * batch, 1, x), Guarded(torch, "c64", n * batch, 1)
        assert src.t.data_ptr() % 16 == 8 and dst.t.data_ptr() % 16 == 8
        p = plan_of(hz, ctx, src.t, dst.t, fwd, batch)
        p.transform()
        ctx.synchronize()
        p.close()
        src.check(x, what + " input")
        dst.check(None, what)
        no_sentinel_left(dst.values(), what)
        assert_fft_rows_close(dst.values().reshape(batch, n), x.reshape(batch, n), fwd, what)


# ---- D. a transform does not depend on its neighbours ----------------------------------------------------------------

def poisoned(n, seed):
    x = rand_c64(seed, n)
    x[0] = complex(float("nan"), 1.0)
    x[n // 2] = complex(float("inf"), -1.0)
    x[n - 1] = complex(1e30, 1e30)
    return x


def neighbour_case(hz, torch, ctx, n, batch, fwd, singles="all"):
    what = "n=%d batch=%d %s" % (n, batch, "forward" if fwd else "backward")
    x = gauss(n * 31 + batch, n * batch).reshape(batch, n)
    bad = {batch // 2} | ({1} if xpb(n) > 1 and batch > 2 else set())
    for j in bad:
        x[j] = poisoned(n, j)
    src = torch.from_numpy(x.reshape(-1)).cuda()
    dst = torch.zeros_like(src)
    p = plan_of(hz, ctx, src, dst, fwd, batch)
    p.transform()
    ctx.synchronize()
    got = dst.cpu().numpy().reshape(batch, n)
    dst.fill_(7.0)
    p.transform()
    ctx.synchronize()
    assert bits_equal(dst.cpu().numpy().reshape(batch, n), got), (what, "a second transform() gives other bytes")
    p.close()
    finite = np.isfinite(got.view(np.float32)).all(axis=1)
    for b in range(batch):
        assert finite[b] != (b in bad), (what, "transform", b, "finite" if finite[b] else "not finite", "poisoned:", sorted(bad))
    one_in, one_out = torch.zeros(n, dtype=torch.complex64, device="cuda"), torch.zeros(n, dtype=torch.complex64, device="cuda")
    p1 = plan_of(hz, ctx, one_in, one_out, fwd, 1)
    for b in (range(batch) if singles == "all" else singles):
        if b in bad:
            continue
        one_in.copy_(src[b * n:(b + 1) * n])
        p1.transform()
        ctx.synchronize()
        alone = one_out.cpu().numpy()
        if not bits_equal(alone, got[b]):
            d = np.flatnonzero(alone.view(np.uint64) != got[b].view(np.uint64))
            raise AssertionError("%s: transform %d differs from the same data through a batch = 1 plan in %d of %d bins, "
                                 "the first at %d" % (what, b, d.size, n, d[0]))
    p1.close()


@pytest.mark.parametrize("n", [16, 128, 256, 4096, 8192, 1 << 14, 1 << 16, 1 << 18, 1 << 21, 12, 1000])
def test_transform_is_bit_identical_beside_any_neighbours(hz, torch, ctx, n):
    """Transform b of a batch == the same data through a batch = 1 plan, bit for bit, with a transform of NaN, +Inf and
    1e30 mid-batch (and, where a workgroup holds several transforms, inside a workgroup of live ones): every index
    expression -- sub, blockIdx, the tile permutation, by as the batch index, Bluestein's b * m / b * n."""
    X = xpb(n)
    batches = (3, 8) if n >= (1 << 14) else ((X + 3, 4 * X) if X > 1 else (3, 8))
    for batch in batches:
        for fwd, _ in DIRS:
            neighbour_case(hz, torch, ctx, n, batch, fwd)


def test_bluestein_pieces_are_bit_identical_to_single_transforms(hz, torch, ctx):
    """n = 4099 (M = 2^14, pieces of 2048 transforms): batches that end one short of, on and past a piece boundary; the
    transforms around the boundary, the first and the last against batch = 1 plans."""
    per = PIECE // chirp_m(4099)
    for batch in (per - 1, per, per + 5):
        ones = sorted({0, 2, per - 3, per - 2, per - 1, per, per + 1, batch - 1} & set(range(batch)))
        for fwd, _ in DIRS:
            neighbour_case(hz, torch, ctx, 4099, batch, fwd, singles=ones)


@pytest.mark.parametrize("n", [64, 4096, 1 << 16, 1000])
def test_host_and_device_memory_spaces_agree_bitwise(hz, torch, ctx, host, n):
    batch = 5
    x = rand_c64(n + 3, n * batch)
    x[2 * n:3 * n] = poisoned(n, 9)
    for fwd, dname in DIRS:
        out = np.zeros(n * batch, np.complex64)
        p = plan_of(hz, host, x.copy(), out, fwd, batch)
        p.transform()
        p.close()
        assert bits_equal(out, run(hz, torch, ctx, x, n, fwd)), (n, dname)


# ---- E. Bluestein past the first piece -------------------------------------------------------------------------------

@pytest.mark.parametrize("n,batch", [(12, (1 << 20) + 3), (4099, 2048 + 5), (3 << 15, 130), ((1 << 20) + 7, 9)])
def test_bluestein_batches_longer_than_a_piece(hz, torch, ctx, n, batch):
    """fft_bluestein's second trip (b0 += per, x = in + b0 * n, the pieces' shared scratch): the transforms either side
    of every piece boundary, the first and the last (n = 12: every 4099th as well) against float64."""
    per = max(1, PIECE // chirp_m(n))
    assert batch > per
    pick = {0, batch - 1} | {b + d for b in range(per, batch, per) for d in (-1, 0)}
    if n == 12:
        pick |= set(range(0, batch, 4099))
    pick = sorted(pick)
    x = gauss(n, n * batch)
    xs = x.reshape(batch, n)[pick]
    for fwd, dname in DIRS:
        got = run(hz, torch, ctx, x, n, fwd).reshape(batch, n)[pick]
        note(n, "random", assert_fft_rows_close(got, xs, fwd, "n=%d batch=%d %s transforms %s..." % (n, batch, dname, pick[:8])))


def test_convolution_blocks_of_a_chirp_length_longer_than_a_piece(torch, ctx, orc):
    """conv_blocks_generic_fmt at a filter of 1000 bins (M = 2048, pieces of 16384 blocks) over 16384 + 7 blocks and
    half a block."""
    per = PIECE // chirp_m(1000)
    nblk = per + 7
    check_conv_blocks(torch, ctx, orc, 1000, nblk, [0, 1, per - 2, per - 1, per, per + 1, nblk - 2, nblk - 1], 1000)


# ---- F. the grid's height --------------------------------------------------------------------------------------------

def test_two_step_batch_beyond_the_grid_height_is_refused(hz, torch, ctx):
    """The two-step kernels carry the batch in gridDim.y.  A plan whose batch exceeds the device's limit is refused
    with INVALID_ARGUMENT when it is made -- over small dummy buffers, which plan creation does not touch; no transform
    of that size is run.  Lengths whose kernels carry the batch in gridDim.x, or in pieces, take the same batch."""
    dummy = torch.zeros(64, dtype=torch.complex64, device="cuda")

    def make(n, batch):
        h = ctypes.c_void_p()
        ctx._ck(hz.lib.hzsdr_fft_plan_batch(ctx._h, dummy.data_ptr(), dummy.data_ptr(), n, batch, hz.FFT_FORWARD, ctypes.byref(h)))
        hz.lib.hzsdr_fft_free(h)

    with pytest.raises(hz.ErrInvalidArgument) as e:
        make(1 << 14, 1 << 31)
    limit = int(re.search(r"grid height, (\d+)", str(e.value)).group(1))
    assert 1024 <= limit < (1 << 31), limit
    for n in (1 << 14, 1 << 16, 1 << 20, 1 << 24):
        with pytest.raises(hz.ErrInvalidArgument):
            make(n, limit + 1)
    make(8192, limit + 1)
    make(4099, limit + 1)

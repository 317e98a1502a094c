"""The per-plane matrix loop that re-uses its tile windows (csrc/hz_firmm2.h, kReuse: the tiles interleaved over the
column blocks, one B fragment read per step pair, the epilogue's exchange through LDS -- hzsdr_chain_fir_options'
loop_form 10) against the per-plane loop it replaces (loop_form 9: four B reads per pair, v_permlane16_swap in the
epilogue) and against the pair loop (loop_form 8).  The integer sums are exact in all three and the float64 combination
and the mixer run the same operations in the same order on the same lanes, so the outputs must agree BIT FOR BIT: on
the bench's filter, a filter whose plane-0 window is every pair, filters that peak at the first and the last tap, u8
and i8, calls over 1, 4 and 8 buffers plain and overlapped, the clock's 2 pi wrap inside a call, a second call that
continues the stream -- at 2^15 samples per call (4096 outputs: the matrix form's minimum, eight passes) and 2^17.

And against tests/firmm_ref.py's exact integer sums under impulses: one per row 0 .. 79 of a pass image and per half
of the row -- both ends of the register rotation and the first two pairs' four-fragment reads, so every (tile, pair)
fragment of the loop is read out as taps."""
import importlib

import numpy as np
import pytest

import firmm_ref as R
from util import rand_i8, rand_u8

pytestmark = pytest.mark.gpu

TAU = 6.283185307179586476925286766559
PAIR, KEPT, REUSE = 8, 9, 10  # hzsdr_chain_fir_options' loop_form
D, FS = 8, 20_000_000
SIZES = [1 << 15, 1 << 17]


@pytest.fixture(scope="module")
def hz():
    return importlib.import_module("go-sdr_amd")


FILTERS = {
    # the bench's filter: plane 0 nonzero on the middle pairs only
    "bench": lambda: R.lowpass(1024, 1 / 16).astype(np.complex64),
    # a floor under the sinc: every tap has a nonzero top digit, the window is every pair
    "floor": lambda: (R.lowpass(1024, 1 / 16) + 0.05).astype(np.complex64),
    # the peak at the first / the last tap: the window at an edge of the pairs
    "peak_first": lambda: (np.exp(-np.arange(1024) / 40.0) * np.exp(0.7j * np.arange(1024))).astype(np.complex64),
    "peak_last": lambda: (np.exp(-np.arange(1024)[::-1] / 40.0) * np.exp(-0.4j * np.arange(1024))).astype(np.complex64),
}

_cache = {}


def run_stream(hz, loop_form, fmt, name, batches, piped, ts0, n, seed=5):
    """The outputs of one stream of sum(batches) buffers of n samples, `batches[i]` buffers per call, and the kernel each
    call ran.  Kept per argument tuple: the kept loops' outputs are computed once."""
    key = (loop_form, fmt, name, tuple(batches), piped, ts0, n, seed)
    if key in _cache:
        return _cache[key]
    import torch
    total = sum(batches)
    x = (rand_u8 if fmt == "u8" else rand_i8)(seed, n * total)
    xs = [torch.from_numpy(x[j * n:(j + 1) * n]).cuda() for j in range(total)]
    ctx = hz.Context(0, hz.MEM_DEVICE, stream=torch.cuda.Stream().cuda_stream)
    ch = ctx.chain(hz.FMT_U8 if fmt == "u8" else hz.FMT_I8, FS).shift(-FS / 8).fir_options(0, 0, loop_form).fir_decimate(FILTERS[name](), D)
    if piped:
        ch.pipeline(True)
    ch.set_time(ts0)
    ys = [torch.zeros(n // D, dtype=torch.complex64, device="cuda") for _ in range(total)]
    torch.cuda.synchronize()
    j, kernels = 0, []
    for k in batches:
        if k == 1 and not piped:
            assert ch.run(xs[j], ys[j]) == (n, n // D)
        else:
            assert ch.run_batch(xs[j:j + k], ys[j:j + k], after=piped) == (n, n // D)
        kernels.append(ch.last_fir_kernel())
        j += k
    ctx.synchronize()
    out = torch.cat(ys)
    ch.close(), ctx.close()
    _cache[key] = (out, kernels)
    return _cache[key]


def assert_same_bits(hz, args, matrix_calls="all"):
    """loop_form 10 against 9 and 8 on the stream `args`: torch.equal on the raw bits."""
    import torch
    new, k_new = run_stream(hz, REUSE, **args)
    if matrix_calls == "all":
        assert all(k == hz.FIR_KERNEL_MATRIX_PASSES for k in k_new), (args, k_new)
    else:
        assert sum(k == hz.FIR_KERNEL_MATRIX_PASSES for k in k_new) >= matrix_calls, (args, k_new)
    for other in (KEPT, PAIR):
        ref, k_ref = run_stream(hz, other, **args)
        assert k_ref == k_new, (args, other, k_ref, k_new)
        a, b = torch.view_as_real(new).view(torch.int32), torch.view_as_real(ref).view(torch.int32)
        assert a.shape == b.shape
        if not torch.equal(a, b):
            bad = (a != b).any(dim=1).nonzero().flatten()
            raise AssertionError("%s: loop_form %d differs from loop_form %d in %d of %d outputs; the first: output %d (pass %d, tile %d, output %d of the tile)"
                                 % (args, REUSE, other, bad.numel(), a.shape[0], int(bad[0]), int(bad[0]) % (args["n"] // D) // 512,
                                    int(bad[0]) % 512 // 8, int(bad[0]) % 8))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("fmt", ["u8", "i8"])
@pytest.mark.parametrize("name", list(FILTERS))
def test_reuse_loop_equals_kept_loops(hz, name, fmt, n):
    """Two single calls: the stream's start (fix-up tasks, the edge landing) and a call that continues it."""
    assert_same_bits(hz, dict(fmt=fmt, name=name, batches=[1, 1], piped=False, ts0=1.0, n=n))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("piped", [False, True])
def test_reuse_loop_batched(hz, piped, n):
    """Calls over 1, 4 and 8 buffers, plain and overlapped (after=True), each continuing the stream."""
    assert_same_bits(hz, dict(fmt="u8", name="bench", batches=[1, 4, 8, 1], piped=piped, ts0=1.0, n=n))


@pytest.mark.parametrize("n,matrix_calls", [(1 << 15, 1), (1 << 17, 1), (1 << 18, "all")])
def test_reuse_loop_across_the_wrap(hz, n, matrix_calls):
    """The clock's 2 pi wrap inside the second call: binades that double from one sample up, short runs as fix-up tasks,
    several tables per call.  (Whether the call with the wrap keeps the matrix path is the planner's choice by its share
    of fix-up outputs: it does at 2^18 samples, and the calls around it always do.)"""
    ts0 = TAU - 1.5 * n / FS
    assert_same_bits(hz, dict(fmt="u8", name="bench", batches=[1, 1, 1], piped=False, ts0=ts0, n=n), matrix_calls)
    assert_same_bits(hz, dict(fmt="i8", name="peak_first", batches=[1, 1, 1], piped=False, ts0=ts0, n=n), matrix_calls)


def test_default_is_one_of_the_per_plane_loops(hz):
    import torch
    args = dict(fmt="u8", name="bench", batches=[1, 1], piped=False, ts0=1.0, n=1 << 15)
    assert torch.equal(torch.view_as_real(run_stream(hz, 0, **args)[0]).view(torch.int32), torch.view_as_real(run_stream(hz, KEPT, **args)[0]).view(torch.int32))


# ---- every row and half of a pass image, read out as taps ------------------------------------------------------------------

def impulse_signal(fmt, n):
    """Zeros (u8: byte 128) and 160 single samples: impulse k = 2 row + half sits in row `row`, half `half` of the image of
    pass 2 + k % 28 -- sample 4096 pass - 1024 + 64 row + 32 half + (7 k) % 32."""
    x = np.zeros((n, 2), np.int8) if fmt == "i8" else np.full((n, 2), 128, np.uint8)
    pos = []
    for k in range(160):
        row, half = k // 2, k % 2
        p = 4096 * (2 + k % 28) - 1024 + 64 * row + 32 * half + (7 * k) % 32
        assert 0 <= p < n and p not in pos
        pos.append(p)
        v = (1 + k % 100, -(1 + k % 50))
        x[p] = v if fmt == "i8" else (128 + v[0], 128 + v[1])
    return x, pos


@pytest.mark.parametrize("loop_form", [REUSE, KEPT])
@pytest.mark.parametrize("fmt", ["i8", "u8"])
def test_image_rows_read_out_by_impulses(hz, fmt, loop_form):
    """A chain without an elementwise stage returns RN32(2^-S (sum q[k] b[m D - k] + dc)): general complex taps over
    twenty binades, one impulse per image row and half -- an output near an impulse is a few taps times one byte each."""
    import torch
    n = 1 << 17
    taps = R.family_d(1024, 77)
    x, pos = impulse_signal(fmt, n)
    ctx = hz.Context(0, hz.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    ch = ctx.chain(hz.FMT_U8 if fmt == "u8" else hz.FMT_I8, FS).fir_options(0, 0, loop_form).fir_decimate(taps, D)
    out = torch.full((n // D,), 7 + 7j, dtype=torch.complex64, device="cuda")
    assert ch.run(torch.from_numpy(x).cuda(), out) == (n, n // D)
    ctx.synchronize()
    assert ch.last_fir_kernel() == hz.FIR_KERNEL_MATRIX_PASSES
    got = out.cpu().numpy()
    ch.close(), ctx.close()
    S, q = R.shift_of(taps, fmt), R.quantise(taps, fmt)
    dc = R.dc_of(q, fmt)
    ex = R.exact_outputs(q, dc, R.signed_bytes(x, fmt), D, planes=False)
    want = R.rn32_complex(ex, S, dc)
    fix = R.fixup_outputs(1024, D, 8)  # (the stream's first outputs: the fix-up tasks' float64 sums, no impulse there)
    assert pos[0] // D > fix + 128
    g, w = got.view(np.int32).reshape(-1, 2)[fix:], want.view(np.int32).reshape(-1, 2)[fix:]
    bad = np.flatnonzero((g != w).any(axis=1)) + fix
    assert bad.size == 0, "loop_form %d %s: %d outputs are not RN32(exact); the first: output %d (pass %d, tile %d)" % (
        loop_form, fmt, bad.size, int(bad[0]), int(bad[0]) // 512, int(bad[0]) % 512 // 8)
    # (and the impulses did reach outputs: every one of them moves at least its own 128 outputs' worth of taps)
    assert int((ex.re != 0).sum() + (ex.im != 0).sum()) > 160 * 64

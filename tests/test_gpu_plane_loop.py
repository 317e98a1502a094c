"""The persistent-pass kernel's per-plane matrix loop (csrc/hz_firmm2.h, kPlane: one digit plane per
v_mfma_i32_16x16x64_i8 fragment, plane 0 only on the step pairs of the geometry's window, hz_firmm2_plan.h
plane0_window) against the pair loop it replaces (two planes per v_mfma_i32_32x32x32_i8 fragment, kept as
hzsdr_chain_fir_options' loop_form 8): the integer sums are exact either way and the float64 combination runs
the same operations in the same order, so the two must agree BIT FOR BIT -- on the benchmarked filter, on
filters whose window covers every pair or touches the first or the last pair, u8 and i8 sources, across clock
boundaries and the 2 pi wrap, in single calls and in calls over several buffers, plain and overlapped."""
import importlib

import numpy as np
import pytest

from util import rand_i8, rand_u8

pytestmark = pytest.mark.gpu

TAU = 6.283185307179586476925286766559
PAIR_LOOP = 8  # hzsdr_chain_fir_options' loop_form: the pair loop


@pytest.fixture(scope="module")
def hz():
    return importlib.import_module("go-sdr_amd")


def lowpass(ntaps, cutoff):
    k = np.arange(ntaps) - (ntaps - 1) / 2
    return (2 * cutoff * np.sinc(2 * cutoff * k) * np.hamming(ntaps)).astype(np.float32)


FILTERS = {
    # the bench's filter: plane 0 nonzero on the middle pairs only
    "bench": lambda: lowpass(1024, 1 / 16).astype(np.complex64),
    # a floor under the sinc: every tap has a nonzero top digit, the window is every pair
    "floor": lambda: (lowpass(1024, 1 / 16) + 0.05).astype(np.complex64),
    # the peak at the first / the last tap: the window at an edge of the pairs
    "peak_first": lambda: (np.exp(-np.arange(1024) / 40.0) * np.exp(0.7j * np.arange(1024))).astype(np.complex64),
    "peak_last": lambda: (np.exp(-np.arange(1024)[::-1] / 40.0) * np.exp(-0.4j * np.arange(1024))).astype(np.complex64),
    # 1017 taps: the same 17-group window, the taps not a multiple of the tile
    "bench_1017": lambda: lowpass(1017, 1 / 16).astype(np.complex64),
}


def run_stream(hz, loop_form, fmt, taps, batches, piped, ts0, n, shift_frac=-1 / 8, seed=5):
    """The outputs of one stream of sum(batches) buffers of n samples, `batches[i]` buffers per call."""
    import torch
    fs, D = 20_000_000, 8
    total = sum(batches)
    x = (rand_u8 if fmt == "u8" else rand_i8)(seed, n * total)
    xs = [torch.from_numpy(x[j * n:(j + 1) * n]).cuda() for j in range(total)]
    ctx = hz.Context(0, hz.MEM_DEVICE, stream=torch.cuda.Stream().cuda_stream)
    ch = ctx.chain(hz.FMT_U8 if fmt == "u8" else hz.FMT_I8, fs).shift(shift_frac * fs).fir_options(0, 0, loop_form).fir_decimate(taps, D)
    if piped:
        ch.pipeline(True)
    ch.set_time(ts0)
    ys = [torch.zeros(n // D, dtype=torch.complex64, device="cuda") for _ in range(total)]
    torch.cuda.synchronize()
    j = 0
    for k in batches:
        if k == 1 and not piped:
            assert ch.run(xs[j], ys[j]) == (n, n // D)
        else:
            assert ch.run_batch(xs[j:j + k], ys[j:j + k], after=piped) == (n, n // D)
        assert ch.last_fir_kernel() == hz.FIR_KERNEL_MATRIX_PASSES
        j += k
    ctx.synchronize()
    out = np.concatenate([y.cpu().numpy() for y in ys])
    ch.close(), ctx.close()
    return out


def assert_same_bits(a, b, what):
    ai, bi = a.view(np.int32), b.view(np.int32)
    assert ai.shape == bi.shape
    bad = int((ai != bi).sum())
    assert bad == 0, "%s: the per-plane loop differs from the pair loop in %d of %d floats" % (what, bad, ai.size)


@pytest.mark.parametrize("name", list(FILTERS))
@pytest.mark.parametrize("fmt", ["u8", "i8"])
def test_plane_loop_equals_pair_loop(hz, name, fmt):
    """Single calls across the 2 pi wrap (ts0 a little under 2 pi: the clock's binades and the wrap's short runs)."""
    taps = FILTERS[name]()
    args = dict(fmt=fmt, taps=taps, batches=[1] * 6, piped=False, ts0=TAU - 0.05, n=1 << 18)
    assert_same_bits(run_stream(hz, 0, **args), run_stream(hz, PAIR_LOOP, **args), "%s %s" % (name, fmt))


@pytest.mark.parametrize("piped", [False, True])
@pytest.mark.parametrize("batches", [[1, 4, 8], [8, 4, 1]])
def test_plane_loop_equals_pair_loop_batched(hz, piped, batches):
    """Calls over 1, 4 and 8 buffers, plain and overlapped, the wrap inside the stream."""
    taps = FILTERS["bench"]()
    args = dict(fmt="u8", taps=taps, batches=batches, piped=piped, ts0=TAU - 0.3, n=1 << 18)
    assert_same_bits(run_stream(hz, 0, **args), run_stream(hz, PAIR_LOOP, **args), "batches %s piped %s" % (batches, piped))


@pytest.mark.parametrize("shift_frac", [0.0, 0.137, -0.31])
def test_plane_loop_other_shifts(hz, shift_frac):
    """Other modulations of the taps (the table of every clock run differs; the window is the chain's)."""
    taps = FILTERS["peak_first"]()
    args = dict(fmt="u8", taps=taps, batches=[1, 4], piped=False, ts0=1.0, n=1 << 18, shift_frac=shift_frac)
    assert_same_bits(run_stream(hz, 0, **args), run_stream(hz, PAIR_LOOP, **args), "shift %g" % shift_frac)

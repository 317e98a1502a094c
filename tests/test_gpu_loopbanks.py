"""What the four loop banks (IIR, symbol timing, carrier recovery, AGC) do alike around their kernels, once for all of
them: plan, position, state and set_state, reset, the `with` block, close, and a closed object's answers.  Each bank at
R = 1 and R = 3 on a DEVICE context, real rows where the bank has them, one push of 300 samples (past the 256-sample tile
edge).  Nothing here is compared numerically: tests/test_gpu_{iir,symsync,carrier,agc}.py do that."""
import importlib

import numpy as np
import pytest

import agc_ref
import carrier_ref
import iir_ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N = 300
ROWS = (1, 3)


@pytest.fixture(scope="module")
def hz():
    return importlib.import_module("go-sdr_amd")


@pytest.fixture(scope="module")
def ctx(hz):
    c = hz.Context(0, hz.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


# bank -> (make(hz, ctx, rows), complex rows?, the state's shape behind the rows, the state's dtype).  The shared
# parameters are the reference modules' own: agc_ref.LOUD, carrier_ref.gains, iir_ref.decay_section; the symbol-timing
# ones are 5 samples per symbol with the package's loop gains, as tests/test_gpu_symsync.py has them.
BANKS = {
    "iir": (lambda hz, ctx, r: ctx.iir_bank(hz.IIR_REAL_F32, iir_ref.decay_section(), rows=r), False, (1, 2), np.float32),
    "symsync": (lambda hz, ctx, r: ctx.symbol_sync(hz.SYMSYNC_REAL_F32, np.array([5.0, 0.01, *hz.loop_gains(5.0)], np.float32), rows=r),
                False, (8,), np.float32),
    "carrier": (lambda hz, ctx, r: ctx.carrier_loop(hz.CARRIER_QPSK, np.array([*carrier_ref.gains(0.02), 0.001, -0.01, 0.01], np.float32), rows=r),
                True, (2,), np.uint32),
    "agc": (lambda hz, ctx, r: ctx.agc(hz.AGC_REAL_F32, agc_ref.LOUD, rows=r), False, (), np.float32),
}


def samples(r, cplx):
    rng = np.random.default_rng(11 + r)
    shape = (N,) if r == 1 else (r, N)
    x = rng.uniform(-1.0, 1.0, shape).astype(np.float32)
    if cplx:
        x = (x + 1j * rng.uniform(-1.0, 1.0, shape)).astype(np.complex64)
    return torch.from_numpy(x).cuda()


def words(z):
    return np.ascontiguousarray(z).view(np.uint32)


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", list(BANKS))
def test_loop_bank_contract(hz, ctx, name, rows):
    make, cplx, tail, dtype = BANKS[name]
    x = samples(rows, cplx)
    fresh = make(hz, ctx, rows)
    with make(hz, ctx, rows) as bank:
        plan = bank.plan()
        assert isinstance(plan, tuple) and len(plan) == 3 and plan[0] == 1 and plan[1] == 256, plan
        assert bank.position() == 0
        z0, p0 = bank.state()
        assert p0 == 0 and z0.shape == (rows,) + tail and z0.dtype == dtype
        bank.push(x)
        assert bank.position() == N
        z, p = bank.state()
        assert p == N and z.shape == (rows,) + tail and z.dtype == dtype
        assert not np.array_equal(words(z), words(z0)), "the push left the state as it was: nothing below is shown"

        # the state goes back in as it came out, the position with it
        bank.set_state(z0, 0)
        bank.set_state(*bank.state())
        bank.set_state(z, p)
        z1, p1 = bank.state()
        assert p1 == N and np.array_equal(words(z1), words(z))

        # a state of another shape is refused and changes nothing
        for bad in (np.zeros((rows + 1,) + tail, dtype), np.zeros((rows,) + tail + (3,), dtype)):
            with pytest.raises(hz.ErrInvalidArgument):
                bank.set_state(bad, 7)
        z1, p1 = bank.state()
        assert p1 == N and np.array_equal(words(z1), words(z))

        bank.reset()
        assert bank.position() == 0
        z2, p2 = bank.state()
        zf, pf = fresh.state()
        assert p2 == 0 and pf == 0 and np.array_equal(words(z2), words(zf)) and np.array_equal(words(z2), words(z0))
        assert bank._h
    assert not bank._h, "leaving the with block closes the object"
    bank.close()
    bank.close()
    fresh.close()
    fresh.close()
    for closed in (bank, fresh):
        for call in (closed.plan, closed.position, closed.state, lambda: closed.push(x), closed.reset):
            with pytest.raises(hz.ErrInvalidArgument):
                call()

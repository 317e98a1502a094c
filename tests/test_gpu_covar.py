"""The covariance bank and the beam scan (include/hzsdr_covar.h) on the GPU: every format and shape BIT FOR BIT against
the outputs of tests/host/covar_ref.cpp (the host program over the headers the kernels evaluate) and, within the bounds
derived in tests/covar_ref.py, against the independent float64 restatement; two cases that settle the order inside the
matrix instruction and one that settles the tree; bit for bit across cuts, entries, pitches, memory spaces, runs,
sub-arrays and permutations; state and errors; the scan; direction finding end to end; the C++ layer.  Every run is
three blocks and an odd remainder, pushed whole and cut inside a segment and inside a group of four, then flushed."""
import importlib
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import covar_ref as ref
from conftest import ROOT
from util import FMT, rand_c64, rand_i8, rand_i16, rand_u8

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BUILD = os.path.join(ROOT, "build", "covar_gpu")
RAND = {"c64": rand_c64, "u8": rand_u8, "i8": rand_i8, "i16": rand_i16}
FREQ = 433.92e6
LAMBDA = 299792458.0 / FREQ
GRID = np.arange(-90, 91)


@pytest.fixture(scope="module")
def hz():
    return importlib.import_module("go-sdr_amd")


@pytest.fixture(scope="module")
def cv():
    return importlib.import_module("go-sdr_amd.covar")


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


def raw_rows(fmt, n_ch, n, seed):
    return np.stack([RAND[fmt](seed * 100 + i, n) for i in range(n_ch)])


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def as_c64(ctx, rows):
    """hzsdr_convert of device rows to complex64, as numpy (N, n)"""
    if rows.dtype == torch.complex64:
        return rows.cpu().numpy()
    out = torch.empty(rows.shape[:2], dtype=torch.complex64, device=rows.device)
    for i in range(rows.shape[0]):
        assert ctx.convert(out[i], rows[i]) == rows.shape[1]
    torch.cuda.synchronize()
    return out.cpu().numpy()


def host(y):
    if isinstance(y, torch.Tensor):
        torch.cuda.synchronize()
        return y.cpu().numpy()
    return y


def run(bank, rows, cuts=(), check_state=True):
    """push rows whole or cut at `cuts`, then flush -> (blocks, N, N) numpy; the counts are checked after every push"""
    n, b = rows.shape[1], bank.block
    edges = [0] + list(cuts) + [n]
    out = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        want = hi // b - lo // b
        if check_state:
            assert bank.blocks_for(hi - lo) == want
        y = bank.push(rows[:, lo:hi])
        assert y.shape[0] == want
        if check_state:
            assert bank.pending() == (hi, hi // b, hi % b)
        out.append(host(y))
    tail = host(bank.flush())
    assert tail.shape[0] == int(n % b > 0) and bank.pending() == (0, 0, 0)
    return np.concatenate(out + [tail])


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def first_difference(got, want):
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    bad = np.argwhere(g.reshape(-1) != w.reshape(-1))
    at = int(bad[0][0])
    return f"{bad.shape[0]} of {w.size} components differ, the first at {at}: {got.reshape(-1)[at // 2]!r} for {want.reshape(-1)[at // 2]!r}"


# ---- 1. bit for bit against the host program, and within the bound of float64 -----------------------------------------

@pytest.fixture(scope="module")
def table(hz, ctx):
    """every shape and format: the device's matrices (whole and cut), the converted rows, the host program's matrices --
    computed once and left unchanged"""
    runs = {}
    for fmt in ref.FORMATS:
        for n_ch, b in ref.SHAPES:
            rows = dev(raw_rows(fmt, n_ch, ref.stream_length(b), 7 * n_ch + b))
            with ctx.covariance(FMT[fmt], n_ch, b) as bank:
                seg, group, form = bank.plan()
                assert (seg, group) == (256, 8) and form == (hz.COVAR_FORM_ONE_TILE if n_ch <= 8 else hz.COVAR_FORM_THREE_TILES)
                whole = run(bank, rows)
                cut = run(bank, rows, ref.cuts(b))
            runs[fmt, n_ch, b] = (whole, cut, as_c64(ctx, rows))
    keys = list(runs)
    want = ref.exact(BUILD, [(b, runs[k][2], ref.cuts(b)) for k in keys for b in [k[2]]])
    return {k: runs[k] + (w,) for k, w in zip(keys, want)}


@pytest.mark.parametrize("fmt", ref.FORMATS)
def test_bits_and_bound(table, fmt):
    worst = 0.0
    for n_ch, b in ref.SHAPES:
        whole, cut, x, want = table[fmt, n_ch, b]
        assert whole.shape == (4 if b > 1 else 3, n_ch, n_ch)
        assert same(whole, want), f"N={n_ch} B={b} {fmt}, pushed whole: " + first_difference(whole, want)
        assert same(cut, want), f"N={n_ch} B={b} {fmt}, cut at {ref.cuts(b)}: " + first_difference(cut, want)
        w64, bound = ref.covariance(x, b), ref.bank_bound(x, b)
        err = np.maximum(np.abs(whole.real - w64.real), np.abs(whole.imag - w64.imag))
        ratio = float((err / bound).max())
        worst = max(worst, ratio)
        print(f"N={n_ch} B={b} {fmt}: error / bound = {ratio:.4f}")
        assert ratio <= 1.0
        assert np.array_equal(whole, whole.conj().transpose(0, 2, 1))
        assert not np.ascontiguousarray(np.diagonal(whole, axis1=1, axis2=2).imag).view(np.uint32).any()
    print(f"{fmt}: worst error / bound {worst:.4f}")


# ---- 2. the order inside the matrix instruction, and the tree --------------------------------------------------------

def order_case(slots, swap, seed0):
    """float32 values a[k], b[k] on the first `slots` snapshots for which the ascending fused chain, the chain with the
    snapshots `swap` exchanged and the unfused sum give three different float32 values (exact arithmetic)"""
    for seed in range(seed0, seed0 + 1000):
        rng = np.random.default_rng(seed)
        a = (rng.integers(1 << 22, 1 << 23, slots) * rng.choice([-1, 1], slots)).astype(np.float32) / np.float32(1 << 23)
        b = (rng.integers(1 << 22, 1 << 23, slots) * rng.choice([-1, 1], slots)).astype(np.float32) / np.float32(1 << 23)
        pairs = [(Fraction(float(u)), Fraction(float(v))) for u, v in zip(a, b)]
        other = list(pairs)
        other[swap[0]], other[swap[1]] = other[swap[1]], other[swap[0]]
        fused, swapped, unfused = ref.fused_chain(pairs), ref.fused_chain(other), ref.unfused_chain(pairs)
        if len({fused, swapped, unfused}) == 3:
            return a, b, float(fused), float(swapped), float(unfused)
    raise AssertionError("no such input found")


@pytest.mark.parametrize("slots,swap", [(4, (1, 2)), (8, (3, 4))], ids=["inside one step", "across two steps"])
def test_mfma_term_order(ctx, slots, swap):
    """R[0][1].re = G[0][2] + G[1][3] with purely real rows: G[1][3] is +0 and the sum exact, so the entry IS the chain
    over a[k] b[k], k ascending"""
    a, b, fused, swapped, unfused = order_case(slots, swap, 17)
    x = np.zeros((2, 300), np.complex64)
    x[0, :slots], x[1, :slots] = a, b
    with ctx.covariance(FMT["c64"], 2, 300) as bank:
        r = host(bank.push(dev(x)))
    got = float(r[0, 0, 1].real)
    print(f"gpu {got!r}: ascending fused {fused!r}, slots {swap} exchanged {swapped!r}, unfused {unfused!r}")
    assert got == fused and got != swapped and got != unfused
    assert r[0, 0, 1].imag == 0 and r[0, 1, 0].real == np.float32(fused)


def test_tree_not_a_running_sum(ctx):
    x = np.zeros((2, 1024), np.complex64)
    x[0, 0], x[0, 256], x[0, 512], x[0, 768] = 4096, 1, 1, 1
    with ctx.covariance(FMT["c64"], 2, 1024) as bank:
        r = host(bank.push(dev(x)))
        assert r[0, 0, 0] == np.complex64(16777218.0), "a left-to-right sum of the partials gives 16777216"
        # the same block resumed after every segment
        r2 = np.concatenate([host(bank.push(dev(x[:, k:k + 256]))) for k in range(0, 1024, 256)])
    assert same(r, r2)


# ---- 3. invariance, all bit for bit ---------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["c64", "u8"])
def test_entries_spaces_pitches_runs(hz, ctx, hctx, table, fmt):
    n_ch, b = 9, 768
    want = table[fmt, n_ch, b][0]
    raw = raw_rows(fmt, n_ch, ref.stream_length(b), 7 * n_ch + b)
    n = raw.shape[1]
    with ctx.covariance(FMT[fmt], n_ch, b) as bank:
        # a second run
        assert same(run(bank, dev(raw)), want)
        # the pointer entry: N separate buffers
        chans = [dev(raw[i]) for i in range(n_ch)]
        got = host(bank.push(chans))
        assert same(np.concatenate([got, host(bank.flush())]), want)
        # a wider input pitch
        wide = torch.zeros((n_ch, n + 37) + tuple(raw.shape[2:]), dtype=chans[0].dtype, device="cuda")
        wide[:, :n] = dev(raw)
        assert same(run(bank, wide[:, :n]), want)
        # a wider output pitch: the values behind N^2 stay
        out = torch.full((3, n_ch * n_ch + 5), 7 - 3j, dtype=torch.complex64, device="cuda")
        got = host(bank.push(dev(raw), out=out))
        bank.reset()
        assert got.shape == (3, n_ch * n_ch + 5) and same(got[:, :n_ch * n_ch].reshape(3, n_ch, n_ch), want[:3])
        assert (got[:, n_ch * n_ch:] == np.complex64(7 - 3j)).all()
        # one block per push against many
        edges = [0, b, 2 * b, 3 * b, n]
        one = [host(bank.push(dev(raw[:, lo:hi]))) for lo, hi in zip(edges[:-1], edges[1:])]
        assert [y.shape[0] for y in one] == [1, 1, 1, 0]
        assert same(np.concatenate(one + [host(bank.flush())]), want)
    # a HOST context, both entries
    with hctx.covariance(FMT[fmt], n_ch, b) as bank:
        assert same(run(bank, raw, ref.cuts(b)), want)
        got = bank.push([np.ascontiguousarray(raw[i]) for i in range(n_ch)])
        assert same(np.concatenate([got, bank.flush()]), want)
        out = np.full((3, n_ch * n_ch + 2), 1 + 1j, np.complex64)
        got = bank.push(raw, out=out)
        assert same(got[:, :n_ch * n_ch].reshape(3, n_ch, n_ch), want[:3]) and (out[:, n_ch * n_ch:] == np.complex64(1 + 1j)).all()


@pytest.mark.parametrize("n_ch,b", ref.CARRY_SHAPES)
def test_carried_state(ctx, hctx, n_ch, b):
    """tests/covar_ref.py, CARRY_SHAPES: the second push resumes the open block at one finished segment, closes it and
    leaves a new open block of one finished segment -- two workgroups of one launch on the same level of the stack --, the
    third does the same at two, and the flush closes a block of exactly two segments with nothing left to compute.  Bit
    for bit the whole push, and the host program"""
    raw = raw_rows("i16", n_ch, ref.carry_length(b), 31 * n_ch + b)
    rows = dev(raw)
    with ctx.covariance(FMT["i16"], n_ch, b) as bank:
        whole = run(bank, rows)
        for _ in range(3):  # (the race this guards against was one of timing)
            cut = run(bank, rows, ref.carry_cuts(b))
            assert same(cut, whole), f"N={n_ch} B={b}: " + first_difference(cut, whole)
    with hctx.covariance(FMT["i16"], n_ch, b) as bank:
        assert same(run(bank, raw, ref.carry_cuts(b)), whole)
    (want,) = ref.exact(BUILD, [(b, as_c64(ctx, rows), ref.carry_cuts(b))])
    assert whole.shape == (3, n_ch, n_ch) and same(whole, want), first_difference(whole, want)


def test_sub_array_and_permutation(ctx, table):
    fmt, b = "u8", 1539
    want = table[fmt, 16, b][0]
    raw = raw_rows(fmt, 16, ref.stream_length(b), 7 * 16 + b)
    with ctx.covariance(FMT[fmt], 4, b) as bank:
        corner = run(bank, dev(raw[:4]), [5, 700])
    assert same(corner, want[:, :4, :4])
    perm = np.array([3, 0, 15, 7, 8, 2, 9, 1, 4, 5, 6, 10, 11, 12, 13, 14])
    with ctx.covariance(FMT[fmt], 16, b) as bank:
        permuted = run(bank, dev(raw[perm]))
    assert same(permuted, want[:, perm][:, :, perm])
    with ctx.covariance(FMT[fmt], 9, b) as bank:
        assert same(run(bank, dev(raw[:9])), want[:, :9, :9])


# ---- 4. state and errors ------------------------------------------------------------------------------------------

def test_state_and_errors(hz, ctx):
    raw = dev(raw_rows("u8", 3, 2500, 3))
    with ctx.covariance(FMT["u8"], 3, 1000) as bank:
        assert bank.flush().shape[0] == 0 and bank.pending() == (0, 0, 0)  # nothing pushed: nothing written
        first = host(bank.push(raw[:, :1700]))
        assert first.shape[0] == 1 and bank.pending() == (1700, 1, 700)
        state = bank.pending()
        with pytest.raises(hz.ErrDstTooSmall):
            bank.push(raw[:, :2000], out=torch.empty((1, 3, 3), dtype=torch.complex64, device="cuda"))
        with pytest.raises(hz.ErrDstTooSmall):
            lib_push_narrow_out(hz, bank, raw)
        assert bank.pending() == state
        got = C_push_bad_stride(hz, bank, raw)
        assert got == hz._capi.ERR_INVALID_ARGUMENT and bank.pending() == state
        with pytest.raises(hz.ErrInvalidArgument):
            lib_push_null_row(hz, bank, raw)
        assert bank.pending() == state
        # the state is unchanged: the stream goes on as if nothing had happened
        rest = host(bank.push(raw[:, 1700:]))
        tail = host(bank.flush())
        bank.reset()
        assert bank.pending() == (0, 0, 0)
        again = run(bank, raw)
        assert same(np.concatenate([first, rest, tail]), again)
        # reset drops the open block
        bank.push(raw[:, :900])
        bank.reset()
        assert bank.flush().shape[0] == 0
    for n_ch, b in ((1, 16), (17, 16), (4, 0), (4, (1 << 24) + 1)):
        with pytest.raises(hz.ErrInvalidArgument):
            ctx.covariance(FMT["u8"], n_ch, b)
    with pytest.raises(hz.ErrSampleFormatUnknown):
        ctx.covariance(9, 4, 16)
    for g in (0, 65537):
        with pytest.raises(hz.ErrInvalidArgument):
            ctx.beam_scan(np.zeros((g, 4), np.complex64))


def C_push_bad_stride(hz, bank, raw):
    """in_stride below n_in through the C entry"""
    import ctypes as C
    got = C.c_size_t(0)
    out = torch.empty((4, 3, 3), dtype=torch.complex64, device="cuda")
    return hz.lib.hzsdr_covar_push(bank._h, raw.data_ptr(), 100, 99, out.data_ptr(), 4, 9, C.byref(got))


def lib_push_narrow_out(hz, bank, raw):
    """two blocks with an out_stride below N^2"""
    import ctypes as C
    got = C.c_size_t(0)
    out = torch.empty((4, 3, 3), dtype=torch.complex64, device="cuda")
    bank.ctx._ck(hz.lib.hzsdr_covar_push(bank._h, raw.data_ptr(), 2000, 2500, out.data_ptr(), 4, 8, C.byref(got)))


def lib_push_null_row(hz, bank, raw):
    import ctypes as C
    got = C.c_size_t(0)
    arr = (C.c_void_p * 3)(raw[0].data_ptr(), None, raw[2].data_ptr())
    out = torch.empty((4, 3, 3), dtype=torch.complex64, device="cuda")
    bank.ctx._ck(hz.lib.hzsdr_covar_push_channels(bank._h, arr, 100, out.data_ptr(), 4, 9, C.byref(got)))


# ---- 5. the scan --------------------------------------------------------------------------------------------------

def test_scan_bits_and_bound(ctx, hctx):
    rng = np.random.default_rng(23)
    cases, got = [], []
    for n_ch in (2, 4, 9, 16):
        for g in (1, 181, 4099):
            for mats in (1, 5):
                q = (rng.standard_normal((mats, n_ch, n_ch)) + 1j * rng.standard_normal((mats, n_ch, n_ch))).astype(np.complex64)
                w = (rng.standard_normal((g, n_ch)) + 1j * rng.standard_normal((g, n_ch))).astype(np.complex64)
                with ctx.beam_scan(w) as scan:
                    p = host(scan.run(dev(q)))
                    assert same(host(scan.run(dev(q[0]))), p[0])
                if g == 181:
                    with hctx.beam_scan(w) as scan:
                        assert same(scan.run(q), p)
                cases.append((q, w))
                got.append(p)
    worst = 0.0
    for (q, w), p, want in zip(cases, got, ref.exact_scan(BUILD, cases)):
        assert same(p, want), f"N={q.shape[1]} G={w.shape[0]} matrices={q.shape[0]}: " + str(np.argwhere(p != want)[:3])
        worst = max(worst, float((np.abs(p - ref.scan(q, w)) / ref.scan_bound(q, w)).max()))
    print(f"worst scan error / bound: {worst:.4f}")
    assert worst <= 1.0


def test_scan_of_r_is_the_beams_power(hz, cv, ctx):
    """p(R, w) against sum |y|^2 of Context.beamform's output, within the bank's bound carried through w plus the
    scan's"""
    n_ch, n = 5, 3000
    rows = dev(raw_rows("u8", n_ch, n, 41))
    d = np.arange(n_ch) * LAMBDA / 2
    w = cv.steering_weights(FREQ, [-60, -7.5, 0, 33, 90], d)
    with ctx.covariance(FMT["u8"], n_ch, n) as bank, ctx.beam_scan(w) as scan:
        r = bank.push(rows)
        p = host(scan.run(r))[0]
        r = host(r)
    x = as_c64(ctx, rows)
    bank_part = np.einsum("gi,ij,gj->g", np.abs(w), np.sqrt(2) * ref.bank_bound(x, n)[0], np.abs(w))
    bound = bank_part + ref.scan_bound(r, w)[0]
    for k in range(w.shape[0]):
        y = torch.empty(n, dtype=torch.complex64, device="cuda")
        ctx.beamform(y, [rows[i] for i in range(n_ch)], w[k])
        power = float((np.abs(host(y).astype(np.complex128)) ** 2).sum())
        print(f"angle {k}: scan {p[k]!r}, beam {power!r}, difference / bound {abs(p[k] - power) / bound[k]:.4f}")
        assert abs(p[k] - power) <= bound[k]


# ---- 6. direction finding end to end ------------------------------------------------------------------------------

def scene(hz, n_el, fmt, seed, sources, n=4096):
    """line array at half-wavelength spacing, independent complex Gaussian sources (angle, amplitude), noise 0.02 per
    component; the array's response to a bearing is the conjugate of the weights that steer to it"""
    rng = np.random.default_rng(seed)
    d = np.arange(n_el) * LAMBDA / 2
    x = np.zeros((n_el, n), np.complex128)
    for ang, amp in sources:
        s = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)
        x += amp * np.conj(hz.beamform_angles(FREQ, float(ang), d)).astype(np.complex128)[:, None] * s[None, :]
    x += 0.02 * (rng.standard_normal((n_el, n)) + 1j * rng.standard_normal((n_el, n)))
    if fmt == "u8":
        return np.clip(np.rint(np.stack([x.real, x.imag], -1) * 127.5 + 127.5), 0, 255).astype(np.uint8), d
    return x.astype(np.complex64), d


@pytest.mark.parametrize("fmt", ["c64", "u8"])
@pytest.mark.parametrize("n_el", [4, 5, 8])
def test_direction_finding(hz, cv, ctx, n_el, fmt):
    truth = [-20, 35]
    raw, d = scene(hz, n_el, fmt, 1000 * n_el, ((-20, 0.25), (35, 0.2)))
    with ctx.covariance(FMT[fmt], n_el, 4096) as bank, ctx.beam_scan(cv.steering_weights(FREQ, GRID, d)) as scan:
        (r,) = bank.push(dev(raw))
        for name, p in (("music", cv.music(scan, r, sources=2)), ("capon", cv.capon(scan, r))):
            found = sorted(int(v) for v in GRID[cv.peaks(p, 2)])
            print(f"{n_el} elements, {fmt}, {name}: {found}")
            assert len(found) == 2 and all(abs(f - t) <= 1 for f, t in zip(found, truth)), name
        raw1, _ = scene(hz, n_el, fmt, 1000 * n_el + 1, ((35, 0.25),))
        (r1,) = bank.push(dev(raw1))
        (found,) = GRID[cv.peaks(cv.bartlett(scan, r1), 1)]
        assert abs(int(found) - 35) <= 1
        assert np.allclose(bank.normalise(host(r1)), host(r1) / 4096)


def test_stream_covariance_blocks(hz, hctx):
    st = importlib.import_module("go-sdr_amd.stream")
    raw = raw_rows("u8", 4, 5000, 77)
    with hctx.covariance(FMT["u8"], 4, 2048) as bank:
        want = run(bank, raw)
        readers = [st.BufferReader(np.ascontiguousarray(raw[i]), 2_000_000) for i in range(4)]
        got = np.concatenate(list(st.covariance_blocks(readers, bank, block=1500)))
    assert same(got, want) and got.shape == (3, 4, 4)


# ---- 7. the C++ layer ----------------------------------------------------------------------------------------------

def test_cxx_covar(hz):
    """tests/cxx/test_covar.cpp (hzsdr::array::Covariance and ::Scan of go-sdr_amd/cxx/hzsdr.hpp) built with g++ and run."""
    exe = os.path.join(BUILD, "test_covar_cxx")
    os.makedirs(BUILD, exist_ok=True)
    lib_dir = os.path.join(ROOT, "go-sdr_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + ROOT, os.path.join(ROOT, "tests", "cxx", "test_covar.cpp"),
                           "-L" + lib_dir, "-lhzsdr_hip", "-L/opt/rocm/lib", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    env = dict(os.environ, LD_LIBRARY_PATH=lib_dir + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "covar-cxx ok" in p.stdout

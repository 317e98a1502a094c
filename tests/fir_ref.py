"""The transform form of the FIR-decimate terminal (fir_run in csrc/hz_chain_fir.hip, fir_decimate_kernel16 and
fir_synth_kernel16 in csrc/hz_chain_dev.h) restated in numpy: the overlap-save geometry, which kernel form a chain
takes, the clock runs of a call, which blocks may mix late and which the host lists as reference-order blocks, the map
from workgroup to block, a case finder for every class of that list, a float64 reference, the single-precision
yardstick, the per-block checker, and filters and inputs that make every tap and every bin count.  numpy and scipy only
(the clock runs come from the library's pure-host hzsdr_nco_segments): no GPU.  tests/test_fir_ref_cpu.py holds all of
it to a brute-force walk and shows that every planted fault fails the checker; tests/test_chain_fir_plan.py holds the
geometry and the list to the library's own header; tests/test_gpu_fir_blocks.py runs the kernels against it.

Geometry, dispatch, late flags and list are a RESTATEMENT BY READING, not something measured: the tests use them to
size their calls and to prove that their cases reach every form and class.  If the launch code changes, this changes
with it.

The forms fir_run can reach, (N, FOLD):  FOLD = D when D is 2, 4, 8 or 16, N >= 1024 and N / D >= 256, else 0 (the full
backward transform in the analysis kernel); the polyphase analysis for every fold at N <= 4096; N = 256 and 512 (only
through fir_options' nfft_min) hold 4 and 2 blocks per workgroup and never mix late:

    N      256  512  1024     2048        4096           8192
    FOLD   0    0    0 2 4    0 2 4 8     0 2 4 8 16     0 2 4 8 16        (19 forms)

The bar (assert_fir_blocks): for EVERY overlap-save block b of every call, the outputs [b hop / D, (b + 1) hop / D),

    m_b(kernel) <= K * max(m_b(yardstick), 2**-23)    for m in (max_sample, l2),    K = util.FFT_K = 4,

max_sample the block's largest sample error and l2 its L2 error, both over sum|h| * max|x|; the yardstick the same
overlap-save block in complex64 (conv_ref.yardstick_blocks: scipy's complex64 transforms, a complex64 product)."""
import numpy as np

import conv_ref as cr
from util import FFT_FLOOR, FFT_K, rand_c64, rand_i8, rand_i16, rand_u8, zeros

SENT32 = cr.SENT32
MAX_SLOW = 96  # kMaxSlowBlocks
MAX_RUNS = 32  # kNcoMaxSegs: more runs travel as a device table, and the call stays on the reference order
CLASSES = ("none", "1-4", "5-64", "65-96", "given_up")
TAU = 2.0 * np.pi


# ---- geometry and dispatch, restated -------------------------------------------------------------------------------------

class Geom:
    """hzsdr_chain_fir_decimate's block: nfft (N), off, hop for (ntaps, D, nfft_min)."""

    def __init__(self, ntaps, D, nfft_min=0):
        nfft = 1024
        if D in (2, 4, 8, 16):
            nfft = max(1024, 256 * D)
        if nfft_min:
            nfft = nfft_min
        if nfft < 256 or nfft > 8192 or nfft & (nfft - 1):
            nfft = 1024
        while nfft < 4 * ntaps and nfft < 8192:
            nfft <<= 1
        self.ntaps, self.D, self.N = ntaps, D, nfft
        self.off = -(-(ntaps - 1) // D) * D
        self.ok = not self.off + D > nfft  # (the refusal: too many taps for the 8192-point block)
        self.hop = (nfft - self.off) // D * D if self.ok else 0

    def nblocks(self, n):
        return -(-n // self.hop)

    def p0(self, b):
        return b * self.hop - self.off

    def __repr__(self):
        return "Geom(ntaps=%d, D=%d, N=%d, off=%d, hop=%d)" % (self.ntaps, self.D, self.N, self.off, self.hop)


def xpb(n):
    """fv::xpb: overlap-save blocks one workgroup of the analysis kernel holds."""
    return max(64, n // 16) // (n // 16)


def form(g):
    """fir_run's dispatch -> (N, FOLD, poly, late_capable, blocks per workgroup)."""
    fold = g.D if g.D in (2, 4, 8, 16) and xpb(g.N) == 1 and 256 <= g.N // g.D <= 8192 else 0
    poly = g.N in (1024, 2048, 4096) and fold != 0
    return g.N, fold, poly, xpb(g.N) == 1, xpb(g.N)


FORMS = [(256, 0), (512, 0)] + [(n, f) for n in (1024, 2048, 4096, 8192) for f in (0, 2, 4, 8, 16) if f == 0 or n // f >= 256]


# ---- clock runs, late blocks, the slow list -------------------------------------------------------------------------------

def clock_runs(hz, rate, ts0, n):
    """The exactly-linear runs of the Shift clock over a call of n samples from ts0: [(first, count, t0, step)]
    (hzsdr_nco_segments, pure host).  A chain without a Shift has no clock: pass rate = 0 -> []."""
    if not rate or n == 0:
        return []
    return hz.nco_segments(rate, ts0, n, 128)[0]


def run_bounds(runs, n):
    """-> (first, end) per run; no clock: one run over the call."""
    if not runs:
        return [(0, n)]
    return [(r[0], runs[i + 1][0] if i + 1 < len(runs) else n) for i, r in enumerate(runs)]


def run_filters(g, runs, n, in_order=False):
    """late_filters: which runs have a modulated spectrum.  None: the call does not run the LATE kernels at all (the
    reference order was asked for, blocks share a workgroup, more than 32 runs, or no run long enough)."""
    if in_order or not form(g)[3]:
        return None
    if not runs:
        return [True]
    if len(runs) > MAX_RUNS:
        return None
    has = [end - first >= 2 * g.N for first, end in run_bounds(runs, n)]
    return has if any(has) else None


def late_flags(g, runs, n, has):
    """late_block, the device's definition, per block: the span [p0, p0 + N) inside [0, n - off] and inside ONE run that
    has a filter."""
    nb = g.nblocks(n)
    if has is None:
        return [False] * nb
    firsts = [f for f, _ in run_bounds(runs, n)]
    out = []
    for b in range(nb):
        p0 = g.p0(b)
        if p0 < 0 or p0 + g.N + g.off > n:
            out.append(False)
            continue
        lo = max(i for i, f in enumerate(firsts) if f <= p0)
        hi = max(i for i, f in enumerate(firsts) if f <= p0 + g.N - 1)
        out.append(lo == hi and has[lo])
    return out


def slow_list(g, runs, n, has):
    """slow_blocks_plan (csrc/hz_chain_fir_plan.h) -> (list, class).  has None: no LATE kernel, no list."""
    if has is None:
        return [], "none"
    N, hop, off, nb = g.N, g.hop, g.off, g.nblocks(n)
    v = []

    def add_range(lo, hi):
        lo, hi = max(lo, 0), min(hi, nb - 1)
        b = lo
        while b <= hi and len(v) <= MAX_SLOW:
            v.append(b)
            b += 1

    def touching(s_lo, s_hi):
        lo = s_lo + off - N
        add_range(0 if lo < 0 else lo // hop + 1, (s_hi + off) // hop)

    if off > 0:
        add_range(0, (off - 1) // hop)
    add_range((n - N) // hop + 1 if n >= N else 0, nb - 1)
    for r, (first, end) in enumerate(run_bounds(runs, n)):
        if not has[r]:
            touching(first, end - 1)
        elif r > 0:
            touching(first - 1, first)
        if len(v) > MAX_SLOW:
            return [], "given_up"
    v = sorted(set(v))
    if len(v) > MAX_SLOW:
        return [], "given_up"
    return v, slow_class(len(v))


def slow_class(count):
    return "none" if count == 0 else "1-4" if count <= 4 else "5-64" if count <= 64 else "65-96"


def rest_of(g, n, lst):
    return g.nblocks(n) - len(lst)


def grid_of(g, n, lst, late):
    """fir_grid: workgroups of the analysis kernel."""
    if not late:
        return -(-g.nblocks(n) // xpb(g.N))
    return len(lst) + 8 * (-(-rest_of(g, n, lst) // 8))


def nth_unlisted(lst, c):
    """The c-th block not in the ascending list, the three ways the kernel finds it (they have to agree)."""
    if not lst:
        return c
    if len(lst) <= 4:  # the scalar scan
        for e in lst:
            if e <= c:
                c += 1
        return c
    lanes = range(64)  # two entries per lane and a ballot: c + #{i : L[i] - i <= c}
    k = sum(1 for l in lanes if l < len(lst) and lst[l] - l <= c) + sum(1 for l in lanes if l + 64 < len(lst) and lst[l + 64] - (l + 64) <= c)
    return c + k


def block_of_workgroup(g, n, lst, i):
    """The LATE analysis kernel's block of workgroup i (None: the workgroup leaves at once): the list first, then
    c = (i % 8) * chunk + i / 8 over the rest, then the c-th block not in the list."""
    if i < len(lst):
        return lst[i]
    rest = rest_of(g, n, lst)
    chunk = -(-rest // 8)
    j = i - len(lst)
    c = (j % 8) * chunk + j // 8
    if j // 8 >= chunk or c >= rest:
        return None
    return nth_unlisted(lst, c)


def plan_call(hz, g, rate, ts0, n, in_order=False):
    """Everything the tests assert about one call -> dict(runs, has, late, slow, cls, rest)."""
    runs = clock_runs(hz, rate, ts0, n)
    has = run_filters(g, runs, n, in_order)
    lst, cls = slow_list(g, runs, n, has)
    return dict(runs=runs, has=has, late=late_flags(g, runs, n, has), slow=lst, cls=cls, rest=rest_of(g, n, lst))


# ---- the case finder -----------------------------------------------------------------------------------------------------

def edge_start(hz, rate, edge, s, n=None):
    """The clock start that puts the run boundary at `edge` seconds (a binade edge 0.5, 1, 2, 4, or TAU for the wrap) on
    sample s of a call: the first run that begins at or behind the edge begins at sample s (after tests/
    test_gpu_conv_blocks.wrap_start, corrected by what hzsdr_nco_segments then says)."""
    n = s + 8 if n is None else n
    ts0 = edge - (s + 0.5) / rate
    for _ in range(8):
        runs = clock_runs(hz, rate, ts0, n)
        if edge == TAU:
            at = [r[0] for i, r in enumerate(runs) if i and r[2] < runs[i - 1][2]]
        else:
            at = [r[0] for i, r in enumerate(runs) if i and r[2] >= edge > runs[i - 1][2]]
        assert at, (rate, edge, s, "the edge is not inside the call")
        if at[0] == s:
            return ts0
        ts0 += (at[0] - s) / rate
    raise AssertionError((rate, edge, s, "no start puts the edge there"))


DS = {0: (3, 5, 1), 2: (2,), 4: (4,), 8: (8,), 16: (16,)}


def geom_for(N, fold, ntaps=None, D=None):
    """A chain that takes form (N, fold): D (a fold's own, else 3 unless given), ntaps (default: an odd count just
    above N / 8, so that N is the library's own choice where it can be) -> (Geom, nfft_min)."""
    D = (fold if fold else 1 if ntaps == 1 else 3) if D is None else D
    ntaps = N // 8 + 7 if ntaps is None else ntaps
    for nmin in (0, N):
        g = Geom(ntaps, D, nmin)
        if g.ok and form(g)[:2] == (N, fold):
            return g, nmin
    raise AssertionError((N, fold, ntaps, D, "not reachable"))


# (what a slow-list case is built from: a tap count and a scenario of the clock)
SCENARIOS = ("plain", "edge", "two_edges", "wrap")


def scenario_start(hz, scenario, g, n):
    """-> (rate, ts0) for a call of n samples; AssertionError where the scenario does not fit the call."""
    if scenario == "plain":
        return 0, 0.0
    if scenario == "edge":  # the binade edge at 1 s in the middle of the call
        return 2_400_000, edge_start(hz, 2_400_000, 1.0, n // 2 + 1, n)
    if scenario == "two_edges":  # 1 s and 2 s inside the call: the run between them is `rate` samples, with a filter
        rate = -(-max(4 * g.N + 2 * g.hop, n // 2 + 1) // 1000) * 1000
        first = (n - rate) // 2
        assert 0 < first < rate // 2, "the run in front of 1 s begins behind 0.5 s"
        return rate, edge_start(hz, rate, 1.0, first, n)
    return 2_400_000, edge_start(hz, 2_400_000, TAU, n // 3, n)  # the 2 pi wrap a third into the call


def recipes(N, cls):
    """(ntaps, scenario) to try for a class, the cheapest call first.  Few taps: hop ~ 7 N / 8, a boundary lists 2 or 3
    blocks; 7808 taps at 8192 points: hop 384, the stream's edges alone list 41 blocks and every boundary 22."""
    few, many = N // 8 + 7, 7808
    if cls == "none":
        return [(1, "plain")]
    if cls == "1-4":
        return [(few, "plain")]
    if cls == "5-64":
        return [(many, "plain"), (many, "edge")] if N == 8192 else [(few, "wrap")]
    if N != 8192:
        return []
    return [(many, "two_edges")] if cls == "65-96" else [(many, "wrap"), (many, "two_edges")]


def find_case(hz, N, fold, cls, residue=None, rest_below=None, D=None):
    """-> dict(g, nfft_min, rate, ts0, n, plan, scenario) of a call on form (N, fold) whose slow list has class `cls` and
    whose rest = nblocks - len(list) is `residue` mod 8 (or below `rest_below`); None where no such call exists (see
    reachable).  The smallest call of the class's recipes, in whole blocks or ending half a hop into the last."""
    for ntaps, scenario in recipes(N, cls):
        g, nmin = geom_for(N, fold, ntaps, D)
        for nb in range(2, 400):
            for n in (nb * g.hop, nb * g.hop - g.hop // 2 // g.D * g.D):
                if n > 160_000 or (scenario != "plain" and n < 5 * g.N):
                    continue
                try:
                    rate, ts0 = scenario_start(hz, scenario, g, n)
                except AssertionError:
                    continue
                runs = clock_runs(hz, rate, ts0, n)
                has = run_filters(g, runs, n)
                if has is None:
                    continue
                lst, c = slow_list(g, runs, n, has)
                rest = rest_of(g, n, lst)
                if c != cls or (residue is not None and (rest % 8 != residue or rest == 0)) or (rest_below is not None and not 0 < rest < rest_below):
                    continue
                return dict(g=g, nfft_min=nmin, rate=rate, ts0=ts0, n=n, plan=plan_call(hz, g, rate, ts0, n), scenario=scenario)
    return None


def reachable(N, cls):
    """Which (N, class) pairs exist at all.  A list above a dozen entries needs a hop that is small beside N, and
    ntaps <= N / 4 below N = 8192 (the library doubles N until 4 ntaps fit): there hop >= 3 N / 4, a boundary puts at
    most 3 blocks on the list and the short runs behind a 2 pi wrap (together < 4 N samples) at most 7 -- 65 entries
    are out of reach, and so is the give-up.  At 8192 points up to 8185 taps fit and every class exists."""
    return N == 8192 or cls in ("none", "1-4", "5-64")


# ---- filters (never a low-pass: its edge taps and stop-band bins are 1e-4 of the passband) ----------------------------------

def graded_taps(ntaps, seed):
    """Seeded white complex taps: every tap and every bin has a gain of its own."""
    return rand_c64(seed, ntaps)


def delay_taps(ntaps, k0):
    h = np.zeros(ntaps, np.complex64)
    h[k0] = 1.0
    return h


def ends_taps(ntaps):
    """h[0] = 1, h[ntaps - 1] = 1j, the rest 0 (one tap: 1)."""
    h = np.zeros(ntaps, np.complex64)
    h[0] = 1.0
    if ntaps > 1:
        h[ntaps - 1] = 1j
    return h


def delay_places(ntaps):
    return sorted({0, 1, ntaps // 2, ntaps - 2, ntaps - 1} & set(range(ntaps)))


def lowpass_taps(ntaps):
    """What the older tests filter with (tests/test_gpu_latemix.py: taps_for): only for showing what it hides."""
    k = np.arange(ntaps) - (ntaps - 1) / 2
    return (np.sinc(k / 16) / 16 * np.hamming(ntaps) * np.exp(0.3j * k)).astype(np.complex64)


# ---- inputs --------------------------------------------------------------------------------------------------------------

def white(fmt, n, seed):
    return {"c64": rand_c64, "u8": rand_u8, "i8": rand_i8, "i16": rand_i16}[fmt](seed, n)


def impulse_input(fmt, n, places):
    """Zero (u8, which has no zero: 127 / 128, the two codes beside it) but for one sample at each of `places`, of
    amplitude readout.train_amp(fmt, i) (u8: code 255 / 0): behind ends-only taps y[m] reads h[D m - p] out."""
    from readout import train_amp
    from util import DT
    places = [p for p in places if 0 <= p < n]
    if fmt == "c64":
        raw = np.zeros(n, np.complex64)
    else:
        raw = np.zeros((n, 2), DT[fmt])
        if fmt == "u8":
            raw[:, 0], raw[:, 1] = 127, 128
    for i, p in enumerate(places):
        raw[p] = (255, 0) if fmt == "u8" else train_amp(fmt, i % 24)[0]
    return raw


def block_places(g, n, where):
    """One impulse per overlap-save block: sample (where + 7 b) mod hop of block b's hop."""
    return [b * g.hop + (where + 7 * b) % g.hop for b in range(g.nblocks(n))]


def cut_places(cuts):
    """The last sample before every call cut and the first behind it."""
    return sorted({c - 1 for c in cuts if c > 0} | set(cuts))


def stream_of(orc, fmt, raw, stages, rate=0, ts0=0.0):
    """The complex64 stream as stored behind the elementwise stages, by the oracle's bit-exact operators (every Shift
    on the chain's one clock).  stages: ("shift", hz) / ("gain", r) / ("rotate", m) in order."""
    xc = zeros("c64", len(raw))
    if fmt == "c64":
        xc[:] = raw
    else:
        assert orc.convert(xc, np.ascontiguousarray(raw)) == len(raw)
    for kind, v in stages:
        if kind == "shift":
            sh = orc.Shifter(rate)
            sh.ts.value = ts0
            sh(v, xc)
        elif kind == "gain":
            orc.scale(xc, v)
        else:
            orc.rotate(xc, v)
    return xc


# ---- reference and yardstick -----------------------------------------------------------------------------------------------

def want64(xc, h, D, hist=None):
    """y[m] = sum_k h[k] x[D m - k], m < len(xc) // D, in complex128 (a float64 transform-based linear convolution);
    x[-j] = hist[-j], the stream in front of xc (None, or shorter than ntaps - 1: zeros in front)."""
    h = np.asarray(h).astype(np.complex128)
    L = len(h) - 1
    front = np.zeros(L, np.complex128)
    if hist is not None and L:
        t = np.asarray(hist).astype(np.complex128)[-L:]
        front[L - len(t):] = t
    full = np.concatenate([front, np.asarray(xc).astype(np.complex128)])
    m = 1
    while m < len(full) + len(h):
        m <<= 1
    y = np.fft.ifft(np.fft.fft(full, m) * np.fft.fft(h, m))[L:L + len(xc)]
    return np.ascontiguousarray(y[::D][:len(xc) // D])


def want64_direct(xc, h, D, hist=None):
    """The same sums one by one (small cases: what want64 is held to)."""
    h = np.asarray(h).astype(np.complex128)
    L = len(h) - 1
    front = np.zeros(L, np.complex128)
    if hist is not None and L:
        t = np.asarray(hist).astype(np.complex128)[-L:]
        front[L - len(t):] = t
    full = np.concatenate([front, np.asarray(xc).astype(np.complex128)])
    return np.array([np.dot(h, full[D * m + L - np.arange(L + 1)]) for m in range(len(xc) // D)], np.complex128)


def block_rows(g, xc, hist=None):
    """The overlap-save blocks of one call as the kernel stages them -> (nblocks, N) complex64: row b holds the stream
    positions [p0, p0 + N), positions < 0 from `hist` (the `off` samples in front of the call, zeros where there are
    none), positions >= n zero."""
    n = len(xc)
    nb = g.nblocks(n)
    front = np.zeros(g.off, np.complex64)
    if hist is not None and g.off:
        t = np.asarray(hist, np.complex64)[-g.off:]
        front[g.off - len(t):] = t
    full = np.concatenate([front, np.asarray(xc, np.complex64), np.zeros(nb * g.hop + g.N - n, np.complex64)])
    idx = np.arange(nb)[:, None] * g.hop + np.arange(g.N)[None, :]
    return full[idx]


def filter_bins(g, h):
    """FFT_N(h) / N in float64, rounded once to complex64 (filter_spectrum's full layout; conv_ref's convention)."""
    return (np.fft.fft(np.asarray(h).astype(np.complex128), g.N) / g.N).astype(np.complex64)


def pick_outputs(g, y, n):
    """The kept outputs of blocks (nblocks, N): index off + t D, t < hop / D, of every block, the call's n // D."""
    per = g.hop // g.D
    return np.ascontiguousarray(y[:, g.off + g.D * np.arange(per)]).reshape(-1)[:n // g.D]


def yardstick32(g, xc, h, hist=None, H=None, rows=None):
    """The call in single precision, block by block: conv_ref's complex64 overlap-save arithmetic."""
    rows = block_rows(g, xc, hist) if rows is None else rows
    H = filter_bins(g, h) if H is None else H
    return pick_outputs(g, cr.yardstick_blocks(rows.reshape(-1), H, g.N), len(xc))


# ---- the checker ---------------------------------------------------------------------------------------------------------

def block_metrics(g, got, want, scale):
    """-> (max_sample, l2) per overlap-save block of a call's outputs, over `scale` = sum|h| * max|x|."""
    per = g.hop // g.D
    d = np.abs(np.asarray(got).astype(np.complex128) - want)
    nb = -(-len(d) // per)
    pad = np.zeros(nb * per)
    pad[:len(d)] = np.where(np.isnan(d), np.inf, d)
    pad = pad.reshape(nb, per)
    return pad.max(axis=1) / scale, np.sqrt((pad * pad).sum(axis=1)) / scale


def assert_fir_blocks(got, want, yard, h, xmax, g, k=FFT_K, what=""):
    """The bar of the module docstring on EVERY block of one call.  got: the call's n // D outputs; want: want64 of the
    stream; yard: yardstick32 of it; xmax: max|x| of the stream.  NaN or a word of the sentinel pattern fails.
    -> the worst ratios (max_sample, l2); a failure names the worst block and its worst sample."""
    w = np.asarray(want, np.complex128).reshape(-1)
    gt = np.ascontiguousarray(got, np.complex64).reshape(-1)
    assert gt.shape[0] == w.shape[0] == len(yard), (what, "output samples", gt.shape[0], w.shape[0], len(yard))
    if gt.shape[0] == 0:
        return 0.0, 0.0
    per = g.hop // g.D
    left = np.flatnonzero((gt.view(np.uint32).reshape(-1, 2) == SENT32).any(axis=1))
    assert left.size == 0, "%s: %d outputs hold sentinel words (never written), the first %d in block %d" % (
        what, left.size, left[0], left[0] // per)
    scale = float(np.abs(np.asarray(h)).sum()) * max(float(xmax), 1e-30)
    worst = []
    for name, mg, my in zip(("max_sample", "l2"), block_metrics(g, gt, w, scale), block_metrics(g, yard, w, scale)):
        bound = k * np.maximum(my, FFT_FLOOR)
        ratio = mg / np.maximum(my, FFT_FLOOR)
        bad = np.flatnonzero(~(mg <= bound))
        if bad.size:
            b = int(bad[np.argmax(ratio[bad])])
            d = np.abs(gt[b * per:(b + 1) * per].astype(np.complex128) - w[b * per:(b + 1) * per])
            s = int(np.argmax(np.where(np.isnan(d), np.inf, d)))
            raise AssertionError("%s: block %d (%d of %d blocks fail): %s %.3e > %g * max(yardstick %.3e, 2^-23), ratio %.1f, "
                                 "worst output %d: got %s want %s" % (what, b, bad.size, len(mg), name, mg[b], k, my[b], ratio[b],
                                                                     b * per + s, gt[b * per + s], w[b * per + s]))
        worst.append(float(ratio.max()))
    return tuple(worst)


# ---- models of a subtly wrong kernel, on the yardstick's arithmetic -----------------------------------------------------------
# (each takes the call's stream xc, the taps h and the `off` samples in front, and returns the call's outputs)

def fault_last_tap_dropped(g, xc, h, hist):
    h2 = np.array(h, np.complex64)
    h2[-1] = 0
    return yardstick32(g, xc, h2, hist)


def fault_history_late(g, xc, h, hist):
    """The history read one sample late: position p < 0 gets the stream's p - 1."""
    front = np.zeros(g.off + 1, np.complex64)
    if hist is not None:
        t = np.asarray(hist, np.complex64)[-(g.off + 1):]
        front[g.off + 1 - len(t):] = t
    return yardstick32(g, xc, h, front[:g.off])


def fault_stale_history(g, xc, h, hist_two_back):
    """The history of two calls back (a ring of histories advanced once too few)."""
    return yardstick32(g, xc, h, hist_two_back)


def fault_alias_bins_swapped(g, xc, h, hist, k0=3, q1=0, q2=1):
    """Two of the D bins that fold onto output bin k0 of the M = N / D point spectrum exchanged in the filter."""
    M = g.N // g.D
    H = filter_bins(g, h)
    a, b = k0 + M * q1, k0 + M * q2
    H[[a, b]] = H[[b, a]]
    return yardstick32(g, xc, h, hist, H=H)


def fault_block_unwritten(g, xc, h, hist, b):
    y = yardstick32(g, xc, h, hist)
    per = g.hop // g.D
    y[b * per:(b + 1) * per] = np.full(2 * len(y[b * per:(b + 1) * per]), SENT32, np.uint32).view(np.complex64)
    return y


def clock_of(runs, n):
    """ts of every sample of a call from its runs (fma(i, step, t0) is exact: the value is representable)."""
    ts = np.empty(n)
    for (first, end), r in zip(run_bounds(runs, n), runs):
        ts[first:end] = r[2] + np.arange(end - first, dtype=np.float64) * r[3]
    return ts


def late_mixed32(g, raw_c, h, runs, omega, steps_by_block=None):
    """The late mixer's arithmetic for a call whose every block is inside the stream (no history): the CONVERTED samples
    raw_c filtered with the run's modulated taps h[k] exp(-i omega k step), then exp(i omega ts[D m]) at the decimated
    rate, in complex64.  steps_by_block: the step each block's taps are modulated with (default: its own run's)."""
    n = len(raw_c)
    rows = block_rows(g, raw_c)
    bounds = run_bounds(runs, n)
    ts = clock_of(runs, n)
    out = np.zeros((g.nblocks(n), g.hop // g.D), np.complex64)
    k = np.arange(len(h), dtype=np.float64)
    for b in range(g.nblocks(n)):
        mid = min(max(g.p0(b) + g.N // 2, 0), n - 1)
        r = max(i for i, (f, _) in enumerate(bounds) if f <= mid)
        step = runs[r][3] if steps_by_block is None else steps_by_block[b]
        ph = -omega * (k * step)
        hm = np.asarray(h).astype(np.complex128) * (np.cos(ph) + 1j * np.sin(ph))
        y = cr.yardstick_blocks(rows[b], filter_bins(g, hm), g.N)[0]
        pos = b * g.hop + g.D * np.arange(g.hop // g.D)
        t = ts[np.minimum(pos, n - 1)]
        mix = (np.cos(omega * t) + 1j * np.sin(omega * t)).astype(np.complex64)
        out[b] = y[g.off + g.D * np.arange(g.hop // g.D)] * mix
    return out.reshape(-1)[:n // g.D]


# ---- the cases of tests/test_gpu_fir_blocks.py (produced and checked on the CPU by tests/test_fir_ref_cpu.py) -------------------

FMTS = ("c64", "u8", "i8", "i16")
RATE = 2_400_000
SLOW_RATE, SLOW_N = 2_000, 26_000  # a clock so slow that one call from 0 s holds two 2 pi wraps: 40 runs, more than the 32 of the inline table
SHIFT_GAIN = (("shift", 3.1e5), ("gain", 0.5))
ROTATE = (("rotate", 0.6 - 0.8j),)


FORM_FMTS = {(1024, 0): ("c64",), (2048, 0): ("u8",), (4096, 0): ("i8",), (8192, 0): ("i16",),
             (1024, 2): ("u8",), (2048, 2): ("i8",), (4096, 2): ("i16",), (8192, 2): ("c64",),
             (1024, 4): ("i8",), (2048, 4): ("i16",), (4096, 4): ("c64",), (8192, 4): ("u8",),
             (2048, 8): ("i16", "c64"), (4096, 8): ("u8",), (8192, 8): ("i8",),
             (4096, 16): ("c64", "u8"), (8192, 16): ("i8", "i16")}


def form_cases():
    """Section A: every form with the formats rotated so that each of c64, u8, i8 and i16 meets every fold class and
    the full form -> [dict(N, fold, fmt, g, nfft_min, stages, rate, ts0, n)].  Five blocks and a ragged sixth; a Shift
    and a Gain from 1.3 s (one long clock run) in every other case, a rotation in the rest."""
    out = []
    for i, ((N, fold), fmts) in enumerate(sorted(FORM_FMTS.items())):
        g, nmin = geom_for(N, fold)
        for j, fmt in enumerate(fmts):
            shifted = (i + j) % 2 == 0
            out.append(dict(N=N, fold=fold, fmt=fmt, g=g, nfft_min=nmin, stages=SHIFT_GAIN if shifted else ROTATE,
                            rate=RATE, ts0=1.3 if shifted else 0.0, n=5 * g.hop + g.hop // 3 // g.D * g.D + g.D))
    return out


def small_block_cases():
    """Section A at N = 256 and 512 (through nfft_min): 4 and 2 blocks per workgroup; 1 block, one below a
    workgroup's worth, exactly one, one more, two workgroups' worth and one."""
    out = []
    for N, ntaps, D, fmt in ((256, 50, 3, "u8"), (256, 64, 8, "i8"), (512, 100, 2, "i16"), (512, 120, 5, "c64")):
        g = Geom(ntaps, D, N)
        assert form(g)[:2] == (N, 0)
        x = xpb(N)
        for nb in sorted({1, x - 1, x, x + 1, 2 * x + 1} - {0}):
            out.append(dict(N=N, fold=0, fmt=fmt, g=g, nfft_min=N, stages=SHIFT_GAIN, rate=RATE, ts0=1.3,
                            n=nb * g.hop - (g.hop // 2 // D * D if nb > 1 else 0), blocks=nb))
    return out


# one form per fold class for the call and run edges
EDGE_FORMS = ((1024, 0, "c64", 3), (1024, 2, "u8", 2), (2048, 4, "i16", 4), (2048, 8, "i8", 8), (4096, 16, "c64", 16))


def call_lengths(g):
    """Section B: calls of exactly k hops, a decimation step either side, and around `off`; then the short calls."""
    D, hop, off = g.D, g.hop, g.off
    first = [D, hop - D, hop, hop + D, 2 * hop, 3 * hop] + [v for v in (off - D, off, off + D) if v > 0]
    short = max(D, (off // 3 - D) // D * D)
    assert short < off / 3 or off < 6 * D
    return first, [short] * 7 + [2 * hop + hop // 2 // D * D]


def run_edge_cases(hz):
    """Section C: the binade edge at 1 s on p0 - 1, p0, p0 + 1, p0 + N - 1 and p0 + N of block 4's span (both runs long
    enough for a filter), and on the same five around e = n - off - N, the start of the last span that still lies
    inside the call (n = 9 hop + N puts e on block 9's p0: the last block that may mix late, at equality; the run
    behind an edge there is too short for a filter)."""
    out = []
    for N, fold, fmt, D in ((1024, 0, "c64", 1), (2048, 4, "i16", 4), (4096, 16, "u8", 16), (8192, 0, "i8", 1)):
        g, nmin = geom_for(N, fold, None, D)
        n = 9 * g.hop + N  # block 9 spans [9 hop - off, 9 hop - off + N): the last with p0 + N + off <= n
        e = n - g.off - N
        assert e == g.p0(9) and n % D == 0 and g.p0(4) >= 2 * N
        for name, base in (("middle", g.p0(4)), ("end", e)):
            for d in (-1, 0, 1, N - 1, N):
                s = base + d
                out.append(dict(N=N, fold=fold, fmt=fmt, g=g, nfft_min=nmin, stages=(("shift", 3.1e5),), rate=RATE,
                                ts0=edge_start(hz, RATE, 1.0, s, n), n=n, edge=s, where=(name, d)))
    return out


def slow_cases(hz):
    """Section D: every class of the slow list with rest % 8 in {0, 1, 7}, and one call with rest < 8, the forms and
    formats rotated (65 entries and more, and the give-up, exist at 8192 points only: reachable)."""
    out = []
    small = [(1024, 0), (2048, 8), (4096, 16), (1024, 4), (2048, 2), (4096, 0)]
    big = [(8192, 0), (8192, 2), (8192, 4), (8192, 8), (8192, 16)]
    i = 0
    for cls in CLASSES:
        for residue in (0, 1, 7):
            N, fold = big[i % 5] if cls in ("65-96", "given_up") or (cls == "5-64" and residue != 7) else small[i % 6]
            c = find_case(hz, N, fold, cls, residue)
            assert c is not None, (N, fold, cls, residue)
            c.update(N=N, fold=fold, fmt=FMTS[i % 4], cls=cls, residue=residue,
                     stages=(("shift", 0.13 * c["rate"]),) if c["rate"] else ((("gain", 0.5),) if i % 2 else ()))
            out.append(c)
            i += 1
    c = find_case(hz, 2048, 4, "1-4", rest_below=8)
    c.update(N=2048, fold=4, fmt="i16", cls="1-4", residue=None, stages=(("gain", 0.5),))
    out.append(c)
    return out

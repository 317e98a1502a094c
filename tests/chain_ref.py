"""The chains WITHOUT a FIR or convolution terminal (launch_map and run_fmt in csrc/hz_chain.hip; chain_map_kernel,
chain_decimate_kernel and chain_downsample_kernel in csrc/hz_chain_dev.h) restated for the tests: a bit-defined reference
built from the oracle's separate operations, which vector width launch_map takes for a call, the clock cases that reach
every branch of nco_ts, the programs and inputs of tests/test_gpu_chain_terminals.py, a failure message that names
sample, width, tile, lane and clock run, and models of a subtly wrong kernel.  numpy, the oracle and the library's
pure-host hzsdr_nco_segments: no GPU.  tests/test_chain_ref_cpu.py shows that every width, tail and clock class is
reached and that every planted fault changes at least MIN_SEEN outputs of the very inputs the GPU module compares.

The widths (map_widths) and the tile sizes are a RESTATEMENT BY READING of launch_map, not something measured: the
tests use them to prove that their offsets and lengths reach W = 4, W = 2, W = 1 and every tail.  If the launch code
changes, this changes with it.

Everything here is bit-defined: the reference is the reference's own operation order (convert, then every stage in
turn over the whole buffer, every Shift a closure of its own started at the chain's clock), no comparison takes a
tolerance.  The planted clock faults need a sample's factor from a clock value the oracle's closure never forms; they
use a numpy restatement of the stages (apply_with_clock), which the CPU test holds to the oracle bit for bit."""
import functools

import numpy as np

from util import ES, rand_c64, rand_i8, rand_i16, rand_u8, zeros

TAU = 2.0 * np.pi
B = 32768  # kReaderBlock: Decimate and Downsample work in blocks of their input
MAX_STAGES = 6  # kMaxEw
MAX_RUNS = 32  # kNcoMaxSegs: more runs travel as a device table
MIN_SEEN = 3  # a planted fault counts as seen by an input when it changes this many outputs
FMTS = ("c64", "u8", "i8", "i16")
GEN = {"c64": rand_c64, "u8": rand_u8, "i8": rand_i8, "i16": rand_i16}
SEED = {"c64": 611, "u8": 612, "i8": 613, "i16": 614}
RATE, SHIFT = 20_000_000, 2.5e6
N_MAP = 4099
N_TERM = 3 * B + 1234

# tests/test_gpu_subslices.py::_exhaustive's sixteen c64 values: signed zeros, Inf, NaN, denormals, 1e12
SPECIALS = np.array([complex(1, -1), 0, complex(-0.0, 0.5), complex(1e12, -1e12),
                     complex(float("nan"), float("inf")), complex(-3, 3), complex(0.999999, -0.999999),
                     complex(2.0, -2.0), complex(float("-inf"), -0.0), complex(-0.0, -0.0), complex(0.5, -0.5),
                     complex(-1.0, 1.0), complex(1.0000001, -1.0000001), complex(127.5, -128.5),
                     complex(32767.5, -32768.5), complex(1e-45, -1e-45)], np.complex64)


# ---- programs and inputs -----------------------------------------------------------------------------------------------

ROT, ROT2 = 0.6 - 0.3j, -0.25 + 0.7j  # off both axes
G1, G2 = 0.3, 1.7  # no powers of two: a gain that commutes exactly with its neighbours would hide a wrong order


def programs(f=SHIFT):
    """name -> stages, ("shift", hz) / ("gain", r) / ("rotate", m) in order, for a Shift frequency f."""
    return {
        "empty": (),
        "gain": (("gain", G1),),
        "rotate": (("rotate", ROT),),
        "rotate_one": (("rotate", 1 + 0j),),  # dropped by the library (stream/multiply.go:59-62): the empty program
        "gain_shift": (("gain", G1), ("shift", f)),
        "shift_rotate": (("shift", f), ("rotate", ROT)),
        "shift_gain_gain": (("shift", f), ("gain", G1), ("gain", G2)),
        "shift_shift": (("shift", f), ("shift", -0.37 * f)),
        "six": (("rotate", ROT), ("shift", f), ("gain", G1), ("shift", -0.37 * f), ("rotate", ROT2), ("gain", G2)),
    }


TERMINAL_PROGRAMS = ("empty", "rotate", "shift", "gain_shift_rotate")


def terminal_programs(f=SHIFT):
    return {"empty": (), "rotate": (("rotate", ROT),), "shift": (("shift", f),),
            "gain_shift_rotate": (("gain", G1), ("shift", f), ("rotate", ROT))}


def effective(program):
    """The program the chain holds: rotate(1 + 0j) is dropped when it is added."""
    return tuple((k, v) for k, v in program if not (k == "rotate" and np.complex64(v) == np.complex64(1)))


def has_shift(program):
    return any(k == "shift" for k, _ in program)


@functools.lru_cache(maxsize=None)
def _pool(fmt):
    x = GEN[fmt](SEED[fmt], N_TERM)
    if fmt == "c64":
        x[:16] = SPECIALS
    x.flags.writeable = False
    return x


def inputs(fmt, n, start=0):
    """Samples [start, start + n) of the format's seeded stream (rand_*; c64 led by SPECIALS), read-only."""
    assert start + n <= N_TERM
    return _pool(fmt)[start:start + n]


def minus_zero_block(factor):
    """One block of c64 for Downsample by `factor` (B / factor >= 8 windows): white, but window 1 all (-0, -0), window 3
    all (-0, +0), window 5 all (+0, -0), window 6 all (-0, -0), an Inf in window 2 and a NaN in window 4.  A sum that
    starts at -0 instead of +0 gives -0 where the windows hold nothing but -0."""
    assert B // factor >= 8
    x = rand_c64(699, B)
    w = lambda i: slice(i * factor, (i + 1) * factor)
    x[w(1)] = complex(-0.0, -0.0)
    x[w(3)] = complex(-0.0, 0.0)
    x[w(5)] = complex(0.0, -0.0)
    x[w(6)] = complex(-0.0, -0.0)
    x[2 * factor + factor // 2] = complex(float("inf"), 1.0)
    x[4 * factor + factor // 3] = complex(0.5, float("nan"))
    return x


# ---- the reference -----------------------------------------------------------------------------------------------------

def to_c64(orc, fmt, x):
    xc = zeros("c64", len(x))
    if fmt == "c64":
        xc[:] = x
    elif len(x):
        assert orc.convert(xc, np.ascontiguousarray(x)) == len(x)
    return xc


def apply_stages(orc, xc, stages, rate, ts0):
    """The stages AS GIVEN (nothing dropped) over xc in place, by the oracle -> the clock behind the buffer."""
    ts_end = ts0
    for kind, v in stages:
        if kind == "shift":
            sh = orc.Shifter(rate)
            sh.ts.value = ts0
            if len(xc):
                sh(v, xc)
            ts_end = sh.ts.value
        elif kind == "gain":
            orc.scale(xc, v)
        else:
            orc.rotate(xc, v)
    return ts_end


def want(orc, fmt, x, program, rate, ts0):
    """-> (complex64 stream behind the program, clock behind the call).  orc.convert, then orc.Shifter / orc.scale /
    orc.rotate stage by stage; every Shift stage a Shifter of its own started at ts0 (the chain's one clock)."""
    xc = to_c64(orc, fmt, x)
    return xc, apply_stages(orc, xc, effective(program), rate, ts0)


def want_terminal(orc, term, factor, c64):
    """orc.decimate / orc.downsample per whole 32768-sample block of the stream -> B // factor outputs per block."""
    per = B // factor
    nb = len(c64) // B
    out = zeros("c64", nb * per)
    fn = orc.decimate if term == "decimate" else orc.downsample
    for b in range(nb):
        assert fn(out[b * per:(b + 1) * per], np.ascontiguousarray(c64[b * B:(b + 1) * B]), factor) == per
    return out


# ---- launch_map, restated ------------------------------------------------------------------------------------------------

RAW = {"c64": 8, "u8": 2, "i8": 2, "i16": 4}
assert RAW == ES
TILE = {"exact": 128 * 4 * 2, 4: 256 * 1 * 4, 2: 256 * 2 * 2, 1: 256 * 2 * 1}  # samples a workgroup holds per trip


def is_exact_shape(program):
    kinds = [k for k, _ in effective(program)]
    return kinds == ["shift"] or kinds == ["shift", "gain"]


def map_widths(src_bytes_off, dst_bytes_off, fmt, n, program, ulp1=False):
    """launch_map's choice for a call of n samples whose source sits src_bytes_off bytes and whose destination sits
    dst_bytes_off bytes behind a 32-byte boundary -> [(W, first, count)], W in ("exact", 4, 2, 1).

    RESTATED BY READING csrc/hz_chain.hip: shift_exact_kernel ("exact": two samples per vector) for [Shift] and
    [Shift, Gain] when ulp1 is off and both pointers take two-sample vectors; else chain_map_kernel with W = 4 where
    the source is aligned to four raw samples, the destination to 32 bytes and n >= 4; else W = 2 on two raw samples
    and 16 bytes; what is left (the ragged end, or the whole call) at W = 1, counted from base = done.  A workgroup's
    tile is 256 x U vectors, U = 1 at W = 4 and 2 otherwise (TILE, in samples)."""
    if n == 0:
        return []
    ok = lambda w: src_bytes_off % (RAW[fmt] * w) == 0 and dst_bytes_off % (8 * w) == 0
    out, done = [], 0
    if not ulp1 and is_exact_shape(program) and ok(2) and n >= 2:
        done = n // 2 * 2
        out.append(("exact", 0, done))
    elif ok(4) and n >= 4:
        done = n // 4 * 4
        out.append((4, 0, done))
    elif ok(2) and n >= 2:
        done = n // 2 * 2
        out.append((2, 0, done))
    if done < n:
        out.append((1, done, n - done))
    return out


def place(widths, j):
    """-> (W, tile, lane, slot) of sample j of a call: the workgroup trip, the lane and which of the lane's W samples."""
    for W, first, count in widths:
        if first <= j < first + count:
            w = 2 if W == "exact" else W
            k = j - first
            tile, r = divmod(k, TILE[W])
            threads = 128 if W == "exact" else 256
            return W, tile, (r // w) % threads, r % w
    raise AssertionError((widths, j))


# ---- clock cases ------------------------------------------------------------------------------------------------------

CLASSES = ("1", "2-4", "5-32", ">32")  # nco_ts: one run; its rolled scan; its inline binary search; the device table


def clock_runs(hz, rate, ts0, n):
    """[(first, count, t0, step)] of a call (hzsdr_nco_segments, pure host); no clock or no samples: []."""
    if not rate or n == 0:
        return []
    return hz.nco_segments(rate, ts0, n, 512)[0]


def run_of(runs, j):
    r = 0
    for i, s in enumerate(runs):
        if s[0] <= j:
            r = i
    return r


def class_of(count):
    return "1" if count <= 1 else "2-4" if count <= 4 else "5-32" if count <= MAX_RUNS else ">32"


def classify(hz, rate, ts0, n, tile=1024):
    """-> (runs over the call, most runs inside one `tile`-sample tile, class of the call's count)."""
    runs = clock_runs(hz, rate, ts0, n)
    firsts = np.array([r[0] for r in runs], np.int64)
    most = 0
    for t0 in range(0, n, tile):
        lo = np.searchsorted(firsts, t0, side="right") - 1
        hi = np.searchsorted(firsts, min(t0 + tile, n) - 1, side="right") - 1
        most = max(most, int(hi - lo + 1))
    return len(runs), most, class_of(len(runs))


def clock_cases(hz=None):
    """The named clocks of the map tests -> [dict(name, rate, shift, ts0, n, cls, tile)]: cls the class the call's run
    count has to be in, tile the class of the most runs one 1024-sample tile has to hold (what the map's nco_ts
    sees: its window is the tile's).  hz given: every case is checked against hzsdr_nco_segments here."""
    w = TAU / RATE
    cases = [
        dict(name="one_run", rate=RATE, shift=SHIFT, ts0=1.0, n=N_MAP, cls="1", tile="1"),
        dict(name="boundary_in_tile", rate=RATE, shift=SHIFT, ts0=4 - 500 * w, n=N_MAP, cls="2-4", tile="2-4"),
        dict(name="wrap_late", rate=RATE, shift=SHIFT, ts0=TAU - 600 * w, n=N_MAP, cls="5-32", tile="5-32"),
        dict(name="wrap_first_tile", rate=RATE, shift=SHIFT, ts0=TAU - 100 * w, n=N_MAP, cls="5-32", tile="5-32"),
        # (the wrap on sample 1021: the first tile holds four runs, so nco_ts's rolled SCAN steps over the wrap -- at a
        # binade edge the previous run's line still gives the boundary sample's clock, at the wrap it does not)
        dict(name="wrap_at_tile_end", rate=RATE, shift=SHIFT, ts0=TAU - 1021.5 / RATE, n=N_MAP, cls="5-32", tile="5-32"),
        dict(name="fresh", rate=RATE, shift=SHIFT, ts0=0.0, n=N_MAP, cls="5-32", tile="5-32"),
        # (2.5 MHz at 20 MHz turns by pi / 4 a sample: from 0 s the factor of sample 4096 + k is the factor of sample k,
        # and a tail that counted its clock from 0 would go unseen -- the same start with a shift off that grid)
        dict(name="fresh_off_grid", rate=RATE, shift=2_345_678.9, ts0=0.0, n=N_MAP, cls="5-32", tile="5-32"),
        dict(name="table_short", rate=7, shift=1.5, ts0=0.0, n=300, cls=">32", tile=">32"),
        dict(name="table_long", rate=1000, shift=123.0, ts0=0.0, n=3 * B, cls=">32", tile="5-32"),
        dict(name="wrap_fast", rate=200_000_000, shift=95e6, ts0=TAU - 600 * TAU / 200e6, n=N_MAP, cls="5-32", tile="5-32"),
    ]
    if hz is not None:
        for c in cases:
            count, most, cls = classify(hz, c["rate"], c["ts0"], c["n"])
            assert (cls, class_of(most)) == (c["cls"], c["tile"]), (c["name"], count, most)
    return cases


def clock_lengths(case):
    """The lengths a clock case runs at: 1500 and 4099, or the case's own and one with a three-sample tail."""
    if "lengths" in case:
        return case["lengths"]
    return CLOCK_LENGTHS if case["n"] == N_MAP else (case["n"], case["n"] + 3)


def terminal_clock_cases(hz=None):
    """The clocks of the Decimate / Downsample calls of N_TERM samples (chain_sample's window is the whole call: the
    call's run count picks nco_ts's branch)."""
    cases = [
        dict(name="one_run", rate=RATE, shift=SHIFT, ts0=1.0, cls="1"),
        dict(name="wrap_in_block_1", rate=RATE, shift=SHIFT, ts0=TAU - (B + 5000.5) / RATE, cls="5-32"),
        dict(name="fresh", rate=RATE, shift=SHIFT, ts0=0.0, cls="5-32"),
        dict(name="table", rate=1000, shift=123.0, ts0=0.0, cls=">32"),
    ]
    if hz is not None:
        for c in cases:
            count, _, cls = classify(hz, c["rate"], c["ts0"], N_TERM // B * B)
            assert cls == c["cls"], (c["name"], count)
    return cases


# ---- the failure message -----------------------------------------------------------------------------------------------

def same(a, b):
    """Per sample: the two complex64 streams hold the same bytes."""
    a = np.ascontiguousarray(a, np.complex64).view(np.uint64)
    b = np.ascontiguousarray(b, np.complex64).view(np.uint64)
    return a == b


def first_diff(got, want_, widths, runs):
    """None when the streams agree byte for byte, else a message that names the first differing sample, its W, its
    tile and lane, and its clock run."""
    ne = np.flatnonzero(~same(got, want_))
    if ne.size == 0:
        return None
    j = int(ne[0])
    W, tile, lane, slot = place(widths, j)
    r = run_of(runs, j) if runs else None
    return ("%d of %d samples differ, the first at %d: W = %s, tile %d, lane %d, slot %d, clock run %s of %d (first %s): got %r want %r"
            % (ne.size, len(want_), j, W, tile, lane, slot, r, len(runs), runs[r][0] if runs else None,
               complex(np.asarray(got)[j]), complex(np.asarray(want_)[j])))


def seen(a, b):
    """How many samples a planted fault changes: different bytes, a NaN against a NaN of other bits not counted (a
    NaN's sign and payload are the platform's, not the model's)."""
    a = np.ascontiguousarray(a, np.complex64)
    b = np.ascontiguousarray(b, np.complex64)
    af, bf = a.view(np.float32).reshape(-1, 2), b.view(np.float32).reshape(-1, 2)
    eq = (af.view(np.uint32) == bf.view(np.uint32)) | (np.isnan(af) & np.isnan(bf))
    return int((~eq.all(axis=1)).sum())


# ---- the stages in numpy, with a clock value per sample (for the planted clock faults) -----------------------------------

def cmul(v, m):
    """Go's complex64 product (float64 products and sum, rounded once) of an array with a value or an array."""
    v = np.asarray(v, np.complex64)
    m = np.asarray(m, np.complex64)
    ar, ai = v.real.astype(np.float64), v.imag.astype(np.float64)
    br, bi = m.real.astype(np.float64), m.imag.astype(np.float64)
    out = np.empty(np.broadcast(v, m).shape, np.complex64)
    with np.errstate(all="ignore"):
        out.real = (ar * br - ai * bi).astype(np.float32)
        out.imag = (ar * bi + ai * br).astype(np.float32)
    return out


def factor_of(orc, shift_hz, ts):
    """complex64(math.Sincos((tau shift) ts)) per clock value."""
    s, c = orc.go_sincos((TAU * shift_hz) * np.asarray(ts, np.float64))
    f = np.empty(len(s), np.complex64)
    f.real, f.imag = c.astype(np.float32), s.astype(np.float32)
    return f


def apply_with_clock(orc, xc, stages, ts):
    """The stages over converted samples xc whose clock values are ts, sample by sample -> a new array."""
    v = np.array(xc, np.complex64)
    for kind, val in stages:
        if kind == "shift":
            v = cmul(v, factor_of(orc, val, ts))
        elif kind == "gain":
            with np.errstate(all="ignore"):
                v = (v.view(np.float32) * np.float32(val)).view(np.complex64)
        else:
            v = cmul(v, np.complex64(val))
    return v


def clock_of(orc, rate, ts0, n):
    """The reference's clock value of every sample of a call (the closure adds 1 / rate BEFORE it uses the clock)."""
    sh = orc.Shifter(rate)
    sh.ts.value = ts0
    return sh.ts_sequence(n)


def line_of(run, j):
    """Sample j's clock by a run's line t0 + (j - first) step."""
    return run[2] + (np.asarray(j, np.float64) - float(run[0])) * run[3]


def _with_clock(orc, fmt, x, program, rate, ts0, ts_wrong):
    """want(), but the samples whose clock ts_wrong differs from the true one recomputed with it."""
    out, _ = want(orc, fmt, x, program, rate, ts0)
    idx = np.flatnonzero(ts_wrong != clock_of(orc, rate, ts0, len(x)))
    if idx.size:
        out[idx] = apply_with_clock(orc, to_c64(orc, fmt, x)[idx], effective(program), ts_wrong[idx])
    return out


# ---- planted faults: each returns the output of a subtly wrong kernel ------------------------------------------------------

def swaps(program):
    """The adjacent pairs of the held program that can be exchanged."""
    return list(range(len(effective(program)) - 1))


def fault_stages_swapped(orc, fmt, x, program, rate, ts0, i):
    """Stages i and i + 1 applied in the wrong order."""
    p = list(effective(program))
    p[i], p[i + 1] = p[i + 1], p[i]
    return want(orc, fmt, x, tuple(p), rate, ts0)[0]


def fault_tail_clock_from_zero(orc, fmt, x, program, rate, ts0, widths):
    """The W = 1 tail launched with base = 0: its samples take the clock of the call's first samples."""
    ts = clock_of(orc, rate, ts0, len(x))
    bad = ts.copy()
    for W, first, count in widths:
        if W == 1 and first > 0:
            bad[first:first + count] = ts[:count]
    return _with_clock(orc, fmt, x, program, rate, ts0, bad)


def fault_previous_run_line(orc, hz, fmt, x, program, rate, ts0):
    """A sample's run looked up one too low: every sample behind the first run takes the previous run's line."""
    n = len(x)
    runs = clock_runs(hz, rate, ts0, n)
    bad = clock_of(orc, rate, ts0, n)
    for r in range(1, len(runs)):
        j = np.arange(runs[r][0], runs[r][0] + runs[r][1])
        bad[j] = line_of(runs[r - 1], j)
    return _with_clock(orc, fmt, x, program, rate, ts0, bad)


def fault_tile_first_run(orc, hz, fmt, x, program, rate, ts0, tile=1024):
    """A tile's clock taken from the run of the tile's first sample only (a window that forgets its upper end)."""
    n = len(x)
    runs = clock_runs(hz, rate, ts0, n)
    bad = clock_of(orc, rate, ts0, n)
    for t0 in range(0, n, tile):
        j = np.arange(t0, min(t0 + tile, n))
        bad[j] = line_of(runs[run_of(runs, t0)], j)
    return _with_clock(orc, fmt, x, program, rate, ts0, bad)


def fault_unit_rotate_applied(orc, fmt, x, program, rate, ts0):
    """rotate(1 + 0j) kept as a stage: Go's product by 1 + 0j is not the identity on NaN, Inf and -0."""
    xc = to_c64(orc, fmt, x)
    apply_stages(orc, xc, program, rate, ts0)
    return xc


def fault_pick_off_by_one(c64, factor):
    """Decimate picks the sample behind the one it should (the block's last pick stays inside the block)."""
    per, nb = B // factor, len(c64) // B
    i = np.minimum(np.arange(per) * factor + 1, B - 1)
    return np.concatenate([np.asarray(c64)[b * B + i] for b in range(nb)]) if nb else zeros("c64", 0)


def downsample_np(c64, factor, start=0.0, reverse=False):
    """Downsample in numpy: per window the float32 sum in order from `start`, each component over float32(factor)."""
    per, nb = B // factor, len(c64) // B
    w = np.stack([np.asarray(c64[b * B:b * B + per * factor]).reshape(per, factor) for b in range(nb)]).reshape(nb * per, factor)
    f = np.ascontiguousarray(w).view(np.float32).reshape(nb * per, factor, 2)
    seq = np.concatenate([np.full((nb * per, 1, 2), start, np.float32), f[:, ::-1, :] if reverse else f], axis=1)
    with np.errstate(all="ignore"):  # (add.accumulate: one float32 addition after the other, in order)
        acc = np.add.accumulate(seq, axis=1, dtype=np.float32)[:, -1, :] / np.float32(factor)
    return np.ascontiguousarray(acc).view(np.complex64).reshape(-1)


def fault_sum_from_minus_zero(c64, factor):
    return downsample_np(c64, factor, start=-0.0)


def fault_sum_reversed(c64, factor):
    return downsample_np(c64, factor, reverse=True)


def fault_clock_over_offered(orc, fmt, x2, program, rate, ts0, consumed, offered):
    """A terminal's SECOND call (its samples x2) from a clock that advanced over the `offered` samples of the first
    call instead of the `consumed` ones."""
    t = clock_of(orc, rate, ts0, offered)[-1] if offered else ts0
    return want(orc, fmt, x2, program, rate, float(t))[0]


# ---- the cases of tests/test_gpu_chain_terminals.py ------------------------------------------------------------------------

OFFSETS = ((0, 0), (2, 2), (0, 2), (2, 0), (1, 0), (0, 1))  # (source, destination) in samples
LENGTHS = (0, 1, 2, 3, 4, 5, 6, 7, 1023, 1024, 1025, 1026, 1500, 2051, 4099)  # (6 and 1026: the two-sample tail behind W = 4)
CLOCK_LENGTHS = (1500, 4099)
FACTORS = (1, 2, 3, 10, 4096, 32767, 32768)
CUTS = (1366, 1367, 1366)
# (fault, clock case) pairs that cannot reach MIN_SEEN outputs -> the clock case that stands in for them
REPLACED = {("tail", "fresh"): "fresh_off_grid"}


def sum_reversed_unseen(fmt, program_name, factor):
    """Where a Downsample that summed in reverse gives the same bytes: i8 behind no stage (k / 128: every partial sum is
    exact), c64 behind no stage by 3 (two terms of the white stream add exactly), and c64 by 32767 and 32768 (three
    outputs, the first a NaN either way: the specials lead block 0).  The pairs that stand in: the same format behind
    a rotation, and the integer formats at the same factors."""
    return ((fmt == "i8" and program_name == "empty") or (fmt == "c64" and program_name == "empty" and factor == 3)
            or (fmt == "c64" and factor >= 32767))

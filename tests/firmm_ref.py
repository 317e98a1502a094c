"""The exact reference of the int8 matrix FIR (csrc/hz_firmm.h, csrc/hz_firmm2.h and their planners
hz_firmm_plan.h / hz_firmm2_plan.h) in plain numpy and Python integers -- no GPU, no library.

The contract it restates (chains WITHOUT an elementwise stage: omega = 0, the table is the taps')
    S      = digit_shift(taps, scale)           scale = 1/128 (i8), 1/127.5 (u8)
    q[k]   = llround(ldexp(h[k] * scale, S))    per component, |q| <= 2^30
    q      = ((d0 256 + d1) 256 + d2) 256 + d3  balanced digits, every d in [-128, 127]
    dc     = 0.5 (sum q_re -+ sum q_im)         u8 only: a u8 sample is (byte - 128) + 0.5 (1 + i)
    y[m]   = 2^-S (sum_k q[k] * b[m D - k] + dc)
with a complex integer product and b the signed bytes (u8: byte - 128; samples in front of the stream are b = 0).
Every sum is below 2^30 * 128 * 2 * 1536 < 2^50: exact in int64 and in float64.

tests/test_firmm_ref_cpu.py holds S, q, the digits and dc against the headers themselves (tests/host/firmm_quant.cpp)
and rn32(exact) against the float64 oracle; tests/test_gpu_fir_exact.py holds the kernels against this file.

The families of filters and signals of those two tests are defined here as well, so that both walk the same cases."""
import math
import os
import struct
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCALE = {"i8": 1.0 / 128.0, "u8": 1.0 / 127.5}
W = 65536 + 256 + 1  # 127 W is the largest coefficient whose top digit is zero, -128 W the smallest


# ---- the quantisation ------------------------------------------------------------------------------------------------

def _parts(taps):
    t = np.ascontiguousarray(taps, np.complex64)
    return t.real.astype(np.float64), t.imag.astype(np.float64)


def shift_of(taps, fmt):
    """S of mm::digit_shift: the largest tap modulus times the byte scale lies in [2^(e-1), 2^e), S = 30 - e."""
    re, im = _parts(taps)
    hmax = float(np.hypot(re, im).max()) * SCALE[fmt]
    if not hmax > 0.0:
        return 0
    _, e = math.frexp(hmax)
    return max(-900, min(900, 30 - e))


def _llround(v):
    """C's llround: halves away from zero (|v| <= 2^30 + 1/2 here, v +- 0.5 is exact)."""
    return np.where(v >= 0, np.floor(v + 0.5), np.ceil(v - 0.5)).astype(np.int64)


def quantise(taps, fmt, S=None):
    """-> (q_re, q_im) int64: mm::digit_table's quantised taps of a chain without a Shift stage."""
    re, im = _parts(taps)
    S = shift_of(taps, fmt) if S is None else S
    return _llround(np.ldexp(re * SCALE[fmt], S)), _llround(np.ldexp(im * SCALE[fmt], S))


def digits(q):
    """-> int64 array (4, ...) of q's balanced base-256 digits, [0] the most significant."""
    q = np.asarray(q, np.int64).copy()
    d = np.zeros((4,) + q.shape, np.int64)
    for i in (3, 2, 1, 0):
        r = ((q + 128) & 255) - 128
        d[i] = r
        q = (q - r) >> 8
    assert not q.any(), "a coefficient outside four balanced digits"
    return d


def dc_of(q, fmt):
    """The constant term of a u8 stream in units of 2^-S, (re, im) as floats (half integers: exact)."""
    if fmt != "u8":
        return 0.0, 0.0
    sr, si = int(q[0].sum()), int(q[1].sum())
    return 0.5 * (sr - si), 0.5 * (sr + si)


def signed_bytes(x, fmt):
    """The int64 (re, im) the kernels multiply: i8 bytes as they are, u8 bytes minus 128."""
    a = np.asarray(x)
    b = a.astype(np.int64) - (128 if fmt == "u8" else 0)
    return b[:, 0], b[:, 1]


# ---- the exact sums --------------------------------------------------------------------------------------------------

def _corr(c, b, D, n_out):
    """y[m] = sum_k c[k] b[m D - k] for m < n_out in int64, b[j] = 0 for j < 0: one short convolution per residue of k
    mod D (tap k = D j + r reads b[D (m - j) - r], sample m - j of the stream's branch r)."""
    c = np.asarray(c, np.int64)
    y = np.zeros(n_out, np.int64)
    for r in range(min(D, len(c))):
        cr = c[r::D]
        if not cr.any():
            continue
        br = np.zeros(n_out, np.int64)
        if r == 0:
            br[:] = b[0:D * n_out:D]
        else:
            br[1:] = b[D - r:D * (n_out - 1):D]
        y += np.convolve(br, cr)[:n_out]
    return y


class Exact:
    """re, im: the exact integer sums sum_k q[k] * b[m D - k] (without dc); planes[part][d]: the sum of digit plane d
    alone, so that re = ((planes[0][0] 256 + planes[0][1]) 256 + planes[0][2]) 256 + planes[0][3]."""

    def __init__(self, re, im, planes):
        self.re, self.im, self.planes = re, im, planes


def exact_outputs(q, dc, x_bytes, D, hist=None, planes=True):
    """The exact sums of every output of the stream `x_bytes` = (b_re, b_im) (signed_bytes) under the quantised taps
    q = (q_re, q_im).  `hist`: (b_re, b_im) of samples in front of the stream (None: zeros).  `dc` is not added here (it
    may be a half integer): rn32 and chunk_form_interval take it.

    The table's coefficient of (output part, input part) is  re <- (+q_re, -q_im),  im <- (+q_im, +q_re)  and the
    digits are cut from THAT coefficient (digit_table): digits(-q) is not -digits(q) at the edges of the balanced
    range, so the plane sums use digits(-q_im) where the product has a minus sign."""
    del dc
    qr, qi = (np.asarray(v, np.int64) for v in q)
    br, bi = (np.asarray(v, np.int64) for v in x_bytes)
    n_out = len(br) // D
    lead = 0
    if hist is not None:
        hr, hi = (np.asarray(v, np.int64) for v in hist)
        pad = -len(hr) % D
        br = np.concatenate([np.zeros(pad, np.int64), hr, br])
        bi = np.concatenate([np.zeros(pad, np.int64), hi, bi])
        lead = (len(hr) + pad) // D
    total = lead + n_out
    re = _corr(qr, br, D, total) - _corr(qi, bi, D, total)
    im = _corr(qi, br, D, total) + _corr(qr, bi, D, total)
    pl = None
    if planes:
        dr, dmi, di = digits(qr), digits(-qi), digits(qi)
        pl = [[(_corr(dr[d], br, D, total) + _corr(dmi[d], bi, D, total))[lead:] for d in range(4)],
              [(_corr(di[d], br, D, total) + _corr(dr[d], bi, D, total))[lead:] for d in range(4)]]
        for part, full in ((0, re), (1, im)):
            s = pl[part]
            assert np.array_equal(((s[0] * 256 + s[1]) * 256 + s[2]) * 256 + s[3], full[lead:])
    return Exact(re[lead:], im[lead:], pl)


def rn32(v, S, dc=0.0):
    """The correctly rounded float32 of (v + dc) 2^-S: v + dc is exact in float64 (|v| < 2^50, dc a half integer), the
    power of two is exact, ONE rounding to float32."""
    return np.ldexp(np.asarray(v, np.int64).astype(np.float64) + dc, -S).astype(np.float32)


def rn32_complex(ex, S, dc=(0.0, 0.0)):
    out = np.empty(len(ex.re), np.complex64)
    out.real, out.imag = rn32(ex.re, S, dc[0]), rn32(ex.im, S, dc[1])
    return out


def chunk_form_interval(s, dc, S):
    """-> (lo, hi) float32: the values the chunk form (csrc/hz_firmm.h, HZ_MM_SPLIT_BLOCKS = 0) may give for one output
    part whose four exact plane sums are s = (s0, s1, s2, s3) and whose constant term is dc.

    The epilogue, from the code:
        hi  = fma((double) s0, 256.0, (double) s1)                       exact: |hi| < 2^40
        lof = fmaf((float) s2, 256.0f, (float) s3)                       float32: THE inexact step
        v   = fma(hi, 65536.0, (double) lof) + dc                        exact: integers below 2^53, dc a half integer
        y   = (float) (v * 2^-S)                                         the one rounding of the contract
    so the kernel returns RN32((V + eps + dc) 2^-S) with V the exact sum and eps = lof - (256 s2 + s3).  With u = 2^-24:
        (float) s2 = s2 (1 + a), |a| <= u, and a = 0 when |s2| <= 2^24 (every such integer is a float32); s3 likewise;
        fmaf rounds ONCE: lof = (256 f2 + f3)(1 + c), |c| <= u, and c = 0 when 256 f2 + f3 is a float32 -- certainly
        when it is an integer below 2^24 in magnitude, and when f2 = 0 or f3 = 0 (a float32 times a power of two, or
        plus zero);
        |eps| <= 256 |s2| u + |s3| u + (256 |s2| + |s3|)(1 + u) u < 3 u (256 |s2| + |s3|).
    delta = 3 * 2^-24 * (256 |s2| + |s3|), and delta = 0 when |s2|, |s3| <= 2^24 and (|256 s2 + s3| < 2^24 or s2 = 0 or
    s3 = 0).  RN32 is monotone, so the result lies in [RN32((V + dc - delta) 2^-S), RN32((V + dc + delta) 2^-S)].
    (V + dc -+ delta is formed in float64: V + dc is exact and delta < 2^19, far below float32's ulp of any V where the
    float64 rounding of the sum could matter.)"""
    s0, s1, s2, s3 = (np.asarray(v, np.int64) for v in s)
    V = (((s0 * 256 + s1) * 256 + s2) * 256 + s3).astype(np.float64) + dc
    a2, a3 = np.abs(s2), np.abs(s3)
    exact = (a2 <= 1 << 24) & (a3 <= 1 << 24) & ((np.abs(256 * s2 + s3) < 1 << 24) | (s2 == 0) | (s3 == 0))
    delta = np.where(exact, 0.0, 3.0 * 2.0 ** -24 * (256.0 * a2 + a3))
    return np.ldexp(V - delta, -S).astype(np.float32), np.ldexp(V + delta, -S).astype(np.float32)


def fixup_outputs(ntaps, D, tile=1):
    """Outputs at a stream start whose window crosses it, ceil((ntaps - 1) / D), rounded up to the planner's tile (8
    outputs on the persistent passes, 16 on the chunk form: plan_call / plan_chunks round the first matrix output up
    to it).  They come from the fix-up tasks: float64 over the UNQUANTISED taps."""
    n = -(-(ntaps - 1) // D)
    return -(-n // tile) * tile


# ---- the planner's own arithmetic, restated (held against the headers by tests/test_firmm_ref_cpu.py) ---------------

def mm2_geometry_ok(ntaps, D):
    """The size conditions of mm2_eligible (csrc/hz_chain_fir.hip) over hz_firmm2_plan.h's geometry: the pass image in
    12 pieces per lane, the table in 4 per thread, 160 KB of LDS, the fix-up task's window in 1280 samples."""
    if D not in (8, 16):
        return False
    kT, waves, fix_out = 8, 8, 16
    w0 = (ntaps - 1 + 7) // 8 * 8
    window = w0 + D * (kT - 1) + 1
    gs = D // 2
    ks = ((2 * window + 31) // 32 + gs - 1) // gs * gs
    ne = 2 * (ks + 4) + (D // 8) * (kT - 1) + 1
    tile_bytes = 2 * D * kT
    tiles = 32 * (1 if D >= 16 else 2)
    image = (tiles - 1) * tile_bytes + 32 * ks
    table = ne * 128 + 16 + 128
    plane = D == 8 and ks == 68
    slot = ((image // tile_bytes + 1) * (tile_bytes + (32 if plane else 16)) + 255) // 256 * 256
    task = ((2 * ntaps + D * (fix_out - 1)) * 8 + 255) // 256 * 256
    lds = 2 * ((table + 255) // 256 * 256) + 512 + waves * slot + task
    return image <= 12 * 64 * 16 and table <= 4 * 64 * waves * 16 and lds <= 160 * 1024 and ntaps + D * (fix_out - 1) <= 1280


def mm2_last_taps(D):
    """The largest tap count the persistent passes take at decimation D (mm2_geometry_ok is monotone up to there)."""
    n = 16
    while mm2_geometry_ok(n + 1, D):
        n += 1
    assert not any(mm2_geometry_ok(k, D) for k in range(n + 1, n + 64))
    return n


# ---- the header itself: tests/host/firmm_quant.cpp -----------------------------------------------------------------

_HOST = {}


def host_program():
    """Builds tests/host/firmm_quant.cpp once per process (g++, the HIP-free headers) -> the executable's path."""
    if "exe" not in _HOST:
        d = tempfile.TemporaryDirectory(prefix="firmm_quant_")
        exe = os.path.join(d.name, "firmm_quant")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"),
                               os.path.join(ROOT, "tests", "host", "firmm_quant.cpp"), "-o", exe])
        _HOST["dir"], _HOST["exe"] = d, exe
    return _HOST["exe"]


def host_quant(filters, tables=False):
    """filters: [(taps complex64, fmt, D)] -> one dict per filter with the header's S, q_re, q_im, dc, combine_ok,
    geom_ok, p0 = (lo, hi), pairs and (tables=True) the geometry and the digit bytes of both table layouts."""
    exe = host_program()
    with tempfile.TemporaryDirectory(prefix="firmm_taps_") as d:
        path = os.path.join(d, "filters.bin")
        with open(path, "wb") as f:
            for taps, fmt, D in filters:
                t = np.ascontiguousarray(taps, np.complex64)
                f.write(struct.pack("<iii", 1 if fmt == "u8" else 0, D, len(t)))
                f.write(t.tobytes())
        out = subprocess.run([exe, path, "1" if tables else "0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    res, cur = [], None
    for line in out.stdout.splitlines():
        key, _, rest = line.partition(" ")
        if key == "filter":
            cur = {}
            res.append(cur)
        elif key in ("S", "combine_ok", "geom_ok"):
            cur[key] = int(rest)
        elif key == "p0":
            lo, hi, pairs = (int(v) for v in rest.split())
            cur["p0"], cur["pairs"] = (lo, hi), pairs
        elif key == "geom":
            cur["w0"], cur["ks"], cur["ne"], cur["e0"] = (int(v) for v in rest.split())
        elif key == "dc":
            cur["dc"] = tuple(float.fromhex(v) for v in rest.split())
        elif key == "q":
            v = np.array(rest.split(), np.int64)
            cur["q_re"], cur["q_im"] = v[0::2], v[1::2]
        elif key in ("tab1", "tab2"):
            cur[key] = np.frombuffer(bytes.fromhex(rest), np.int8)
    assert len(res) == len(filters)
    return res


def table_digit_bytes(h, qr, qi, v2):
    """The digit bytes digit_table must hold for the quantised taps (qr, qi) in the geometry of host_quant's result
    `h`, as int8 in the table's own order: F[digit][E][part][16] (v2 False) or T[f][E][part][pl][16], digit = 2 f + pl.
    Byte e of (E, part) is the coefficient of input part e & 1 of tap 8 (E - e0) + w0 - (e >> 1)."""
    ne, e0, w0, nt = h["ne"], h["e0"], h["w0"], len(qr)
    E, pout, e = np.meshgrid(np.arange(ne), np.arange(2), np.arange(16), indexing="ij")
    kap = 8 * (E - e0) + w0 - (e >> 1)
    pin = e & 1
    ok = (kap >= 0) & (kap < nt)
    k = np.where(ok, kap, 0)
    coef = np.where(pout == 0, np.where(pin == 0, qr[k], -qi[k]), np.where(pin == 0, qi[k], qr[k]))
    d = digits(np.where(ok, coef, 0))  # (4, ne, 2, 16)
    if v2:
        d = d.reshape(2, 2, ne, 2, 16).transpose(0, 2, 3, 1, 4)  # [f][pl][E][part] -> [f][E][part][pl]
    return np.ascontiguousarray(d).astype(np.int8).ravel()


def plane0_pairs(h, qr, qi, D):
    """The step pairs of the per-plane loop that read a table entry holding a tap with a nonzero top digit in ANY of
    its four table coefficients (+-q_re, +-q_im), from the Python digits: pair t reads the entries (D / 8) i - kq - 4 t
    + e0, i = 0 .. 7, kq = 0 .. 3; tap k sits in entry e0 + (k - w0 + e) / 8 with e = (w0 - k) mod 8."""
    hot = (digits(qr)[0] != 0) | (digits(-qr)[0] != 0) | (digits(qi)[0] != 0) | (digits(-qi)[0] != 0)
    ent = set()
    for k in np.flatnonzero(hot):
        e = (h["w0"] - int(k)) % 8
        ent.add(h["e0"] + (int(k) - h["w0"] + e) // 8)
    pairs = set()
    for t in range(h["pairs"]):
        if any(((D // 8) * i - kq - 4 * t + h["e0"]) in ent for i in range(8) for kq in range(4)):
            pairs.add(t)
    return pairs


def combine_edge(unit, fmt, lo, hi):
    """The last float32 amplitude c in [lo, hi] whose boxcar c * unit (1024 taps) int32_combine_ok accepts, and the
    next float32 above it, by bisection over the float32 bit patterns through the host program.  lo must be accepted,
    hi refused and both on one digit shift S (then the planner's bound grows with c)."""
    def ask(c):
        r = host_quant([(np.full(1024, c * unit, np.complex64), fmt, 8)])[0]
        return r["combine_ok"], r["S"]
    a, b = (int(np.float32(v).view(np.int32)) for v in (lo, hi))
    (oka, sa), (okb, sb) = ask(np.float32(lo)), ask(np.float32(hi))
    assert oka == 1 and okb == 0 and sa == sb, (oka, okb, sa, sb)
    while b - a > 1:
        m = (a + b) // 2
        ok, s = ask(np.int32(m).view(np.float32))
        assert s == sa
        a, b = (m, b) if ok else (a, m)
    return np.int32(a).view(np.float32), np.int32(b).view(np.float32)


# ---- the filter families ---------------------------------------------------------------------------------------------
# "Dyadic": h * scale * 2^S is an integer for every tap.  i8 and S = 30: q = h 2^23, so h = q / 2^23 (a float32 as long
# as q has 24 significant bits).

def from_q(q_re, q_im=None):
    """The complex64 taps whose i8 quantisation at S = 30 is exactly (q_re, q_im)."""
    q_re = np.asarray(q_re, np.int64)
    q_im = np.zeros_like(q_re) if q_im is None else np.asarray(q_im, np.int64)
    t = (q_re.astype(np.float64) + 1j * q_im.astype(np.float64)) / float(1 << 23)
    t32 = t.astype(np.complex64)
    assert np.array_equal(t32.astype(np.complex128), t), "a coefficient with more than 24 significant bits"
    return t32


ANCHOR_A = 1 << 29         # hmax * scale = 1/2, exactly on a power of two: S = 30
ANCHOR_B = (1 << 30) - 64  # the largest |q| a float32 tap reaches


def family_a(ntaps, d, k0, seed):
    """One plane at a time: the anchor 2^29 at tap k0, every other tap r 256^(3 - d) in both parts, r random in
    [-128, 127] (plane 0: in [-22, 22] -- the anchor stays the largest modulus, 22 sqrt(2) < 32, and S = 30)."""
    r = np.random.default_rng(seed)
    lo, hi = (-22, 23) if d == 0 else (-128, 128)
    qr = r.integers(lo, hi, ntaps) * 256 ** (3 - d)
    qi = r.integers(lo, hi, ntaps) * 256 ** (3 - d)
    qr[k0], qi[k0] = ANCHOR_A, 0
    return from_q(qr, qi)


def signal_a(n, D, k0, seed):
    """Random i8 bytes, zero on the samples the anchor tap reads (n = -k0 mod D): it contributes nothing."""
    from util import rand_i8
    x = rand_i8(seed, n).copy()
    x[(-k0) % D::D] = 0
    return x


CARRY_VALUES = [127, -127, 128, -128, 129, -129, 32639, -32639, 32640, -32640, 32896, -32896, 127 * W, 127 * W + 1,
                -128 * W, -128 * W - 1, (1 << 23) - 1, 1 << 23, 1 << 29, ANCHOR_B]


def family_b(ntaps, value, imag=False):
    """Digit carries: `value` at taps 0 and ntaps - 1 and at one tap of each residue mod 8, zeros elsewhere, the anchor
    2^30 - 64 (real) near the middle.  imag: the values go to the imaginary parts (the table's -q_im coefficients)."""
    q = np.zeros(ntaps, np.int64)
    at = sorted({0, ntaps - 1} | {r + 8 * ((37 * r + 1) % (ntaps // 8)) for r in range(8)})
    q[at] = value
    a = np.zeros(ntaps, np.int64)
    mid = next(k for k in range(ntaps // 2, ntaps) if k not in at)
    a[mid] = ANCHOR_B
    return from_q(a, q) if imag else from_q(a + q)


def family_c(ntaps, k_hot, mirror=False, modulus=False, cold=127 * W):
    """The plane-0 window: the anchor at tap 0, `cold` (127 W: top digit 0) on every eighth tap, ONE hot tap 127 W + 1
    at k_hot.  mirror: the same filter reversed (anchor at ntaps - 1).  modulus: the hot tap is complex with cold
    components and a hot modulus instead.  cold = 127 W - 1 is cold by plane0_window's own threshold as well (127 W
    itself is above it, m <= 127 W - 1: the header is careful by one unit), so the window is then as narrow as the
    two hot taps allow and an off-by-one at either of its ends drops 2^24 x from an output."""
    qr, qi = np.zeros(ntaps, np.int64), np.zeros(ntaps, np.int64)
    qr[0::8] = cold
    if modulus:
        qr[k_hot], qi[k_hot] = 127 * W - 5, 1 << 20  # |q| = 8 421 245 > 127 W, both components cold
    else:
        qr[k_hot] = 127 * W + 1
    qr[0], qi[0] = ANCHOR_A, 0
    if mirror:
        qr, qi = qr[::-1].copy(), qi[::-1].copy()
    return from_q(qr, qi)


def hot_positions(ntaps):
    return sorted({7, 8, ntaps // 2, ntaps - 9, ntaps - 1})


def family_d(ntaps, seed):
    """General complex float32 taps with magnitudes spread over 2^-20 .. 1."""
    r = np.random.default_rng(seed)
    mag = np.exp2(-20.0 * r.random(ntaps))
    mag[int(r.integers(0, ntaps))] = 1.0
    return (mag * np.exp(2j * np.pi * r.random(ntaps))).astype(np.complex64)


def impulse_marks(D, n_out, cuts=()):
    """The output indices whose neighbourhood the impulses visit: every pass boundary (512 outputs at D = 8, 256 at D =
    16), which holds every chunk boundary (2048 / 1024 / 512 outputs at D = 8 / 16 / 32), and the call cuts."""
    step = 256 if D == 16 else 512
    return sorted(set(range(step, n_out, step)) | set(cuts))


def impulse_positions(ntaps, D, n, marks):
    """Sample positions at least ntaps + 16 D apart and at least that far into the stream, ascending: mark j (an output
    index) is visited at its sample D m - 1, D m or D m + 1 in turn, and the room between two marks goes to positions
    that walk the residues mod 16."""
    gap = ntaps + 16 * D
    targets = sorted(m * D + (-1, 0, 1)[j % 3] for j, m in enumerate(sorted(marks)))
    pos, res, p = [], 0, gap
    for t in targets + [n + gap]:
        while True:
            q = p + (res - p) % 16
            if q + gap > t or q >= n:
                break
            pos.append(q)
            res, p = (res + 1) % 16, q + gap
        if p <= t < n:
            pos.append(t)
            p = t + gap
    return pos


def dyadic(taps, fmt):
    """h * scale * 2^S is an integer for every tap: the fix-up tasks' float64 sums over the unquantised taps are then the
    quantised sums, exactly (i8 only: a u8 sample is not an integer multiple of the scale)."""
    re, im = _parts(taps)
    S = shift_of(taps, fmt)
    v = np.concatenate([np.ldexp(re * SCALE[fmt], S), np.ldexp(im * SCALE[fmt], S)])
    return fmt == "i8" and bool(np.all(v == np.floor(v)))


def signal_d(fmt, n, pos):
    """i8: zeros with single samples (1, 0), (-128, 0), (0, 127), (1, -128) ...; u8: byte 128 with single bytes 0 / 255."""
    if fmt == "i8":
        x = np.zeros((n, 2), np.int8)
        vals = [(1, 0), (-128, 0), (0, 127), (1, -128), (127, 127), (0, 1), (-128, -128)]
    else:
        x = np.full((n, 2), 128, np.uint8)
        vals = [(0, 128), (255, 128), (128, 0), (128, 255), (0, 255), (255, 0)]
    for j, p in enumerate(pos):
        x[p] = vals[j % len(vals)]
    return x


def lowpass(ntaps, cutoff):
    k = np.arange(ntaps) - (ntaps - 1) / 2
    return (2 * cutoff * np.sinc(2 * cutoff * k) * np.hamming(ntaps)).astype(np.float32)


def family_f():
    """General filters: the bench's, the floor / peak_first / peak_last shapes of tests/test_gpu_plane_loop.py (same
    formulas), three seeded random complex ones (tap counts around the per-plane loop's 1017 .. 1024 window)."""
    f = {
        "bench": lowpass(1024, 1 / 16).astype(np.complex64),
        "floor": (lowpass(1024, 1 / 16) + 0.05).astype(np.complex64),
        "peak_first": (np.exp(-np.arange(1024) / 40.0) * np.exp(0.7j * np.arange(1024))).astype(np.complex64),
        "peak_last": (np.exp(-np.arange(1024)[::-1] / 40.0) * np.exp(-0.4j * np.arange(1024))).astype(np.complex64),
    }
    for seed, nt in ((1, 1024), (2, 1017), (3, 200)):
        r = np.random.default_rng(9000 + seed)
        f["random%d" % seed] = ((r.standard_normal(nt) + 1j * r.standard_normal(nt)) * np.exp2(-8.0 * r.random(nt))).astype(np.complex64)
    return f


def signals_f(fmt, n, seed=11):
    """White bytes, the constant extremes, the alternating pattern -128, 127, -128, ... (u8: 0, 255, ...)."""
    from util import rand_i8, rand_u8
    lo, hi = (-128, 127) if fmt == "i8" else (0, 255)
    dt = np.int8 if fmt == "i8" else np.uint8
    alt = np.empty((n, 2), dt)
    alt[0::2, 0], alt[1::2, 0] = lo, hi
    alt[0::2, 1], alt[1::2, 1] = hi, lo
    return {
        "white": (rand_i8 if fmt == "i8" else rand_u8)(seed, n),
        "all_lo": np.full((n, 2), lo, dt),
        "all_hi": np.full((n, 2), hi, dt),
        "alternating": alt,
    }


def signals_e(fmt, n, seed=12):
    """The inputs that line all signs up under a boxcar, and one white input."""
    from util import filled, rand_i8, rand_u8
    lo, hi = (-128, 127) if fmt == "i8" else (0, 255)
    return {
        "lo_lo": filled(fmt, n, (lo, lo)),
        "lo_hi": filled(fmt, n, (lo, hi)),
        "hi_lo": filled(fmt, n, (hi, lo)),
        "white": (rand_i8 if fmt == "i8" else rand_u8)(seed, n),
    }


# the ends of the bisections of family E: (accepted, refused) amplitudes on ONE digit shift -- |h| scale 2^S runs from
# 2^29 at the first to just under 2^30 at the second, the planner's bound crosses 2^31 near 2^29.5
EDGE_RANGES = {
    ("real", "i8"): (2.0 ** -10, np.nextafter(np.float32(2.0 ** -9), np.float32(0))),
    ("real", "u8"): (2.0 ** -10, 127.0 * 2.0 ** -16),
    ("diag", "i8"): (0.70711 * 2.0 ** -10, 0.7071 * 2.0 ** -9),
    ("diag", "u8"): (0.70711 * 2.0 ** -10, 0.70 * 2.0 ** -9),
}
EDGE_UNIT = {"real": 1.0 + 0.0j, "diag": 1.0 + 1.0j}


def family_e(kind, fmt):
    """-> {"accepted": taps, "refused": taps}: 1024-tap boxcars c * unit at the last amplitude int32_combine_ok accepts
    and at the next float32."""
    key = ("E", kind, fmt)
    if key not in _HOST:
        lo, hi = EDGE_RANGES[(kind, fmt)]
        a, b = combine_edge(EDGE_UNIT[kind], fmt, lo, hi)
        _HOST[key] = {"accepted": np.full(1024, a * EDGE_UNIT[kind], np.complex64), "refused": np.full(1024, b * EDGE_UNIT[kind], np.complex64)}
    return _HOST[key]


def combine_ok(taps, fmt):
    """mm::int32_combine_ok restated (np.sum adds in another order than the header: equal to it away from the bound only
    -- family E, ON the bound, asks the host program)."""
    re, im = _parts(taps)
    total = float(np.hypot(re, im).sum())
    return 128.0 * (1.4142135623730951 * total * SCALE[fmt] * 2.0 ** (shift_of(taps, fmt) - 16) + 2.0 * len(re)) < 2147483648.0


# ---- the cases both tests walk ---------------------------------------------------------------------------------------
# A kernel form: decimation, hzsdr_chain_fir_options' implementation and loop form, the planner's tile.
FORMS = {
    "P8": dict(D=8, chunks=False, loop=0),      # persistent passes, per-plane loop at 1017 .. 1024 taps
    "P8pair": dict(D=8, chunks=False, loop=8),  # persistent passes, pair loop
    "P16": dict(D=16, chunks=False, loop=0),
    "C8": dict(D=8, chunks=True, loop=0),       # FIR_IMPL_MATRIX_CHUNKS
    "C32": dict(D=32, chunks=False, loop=0),    # no persistent passes at this factor
}
N_OUT = 8192
LAST8, LAST16 = 1156, 1040  # mm2_last_taps(8), mm2_last_taps(16): tests/test_firmm_ref_cpu.py holds both to the header
# every eligibility edge: the matrix form's 16, the per-plane loop's window 1017 .. 1024, the persistent passes' last
# tap count and the next one at either factor
SWEEP = [("P8", 16), ("P8", 17), ("P8", 1017), ("P8", 1024), ("P8", LAST8), ("P8", LAST8 + 1), ("P8pair", 17), ("P8pair", 1024),
         ("P16", 16), ("P16", 1017), ("P16", 1024), ("P16", LAST16), ("P16", LAST16 + 1), ("C8", 16), ("C8", 1024), ("C8", 1536),
         ("C32", 17), ("C32", 1024)]


def takes_passes(form, taps, fmt, combine=None):
    """Does this chain run the persistent-pass kernel (else: the chunk form)?"""
    f = FORMS[form]
    ok = combine_ok(taps, fmt) if combine is None else combine
    return (not f["chunks"]) and mm2_geometry_ok(len(taps), f["D"]) and ok


def ragged_cuts():
    """The output cuts of a stream in three ragged calls: on the 64-output grid (samples: 64 D), off every pass and chunk
    boundary, every call at least the 4096 outputs the matrix form asks for -- so this stream is 13 248 outputs long."""
    a = 4096 + 64 * 3
    b = a + 4096 + 64 * 5
    return [0, a, b, b + 4096 + 64 * 7]


def d_signal(fmt, ntaps, D, cuts=None):
    n_out = cuts[-1] if cuts else N_OUT
    marks = impulse_marks(D, n_out, cuts[1:-1] if cuts else ())
    return signal_d(fmt, n_out * D, impulse_positions(ntaps, D, n_out * D, marks))


def chunk_form_cases(family):
    """(id, fmt, D, taps, signal) of every single-call case of one family of tests/test_gpu_fir_exact.py that the chunk
    form runs: the CPU test asserts on them that the interval is a single float32 for at least 90 % of the parts."""
    return [c for c in _chunk_form_cases(family) if c[0][0] == family]


def _chunk_form_cases(family):
    from util import rand_i8
    out = []
    if family == "E":
        for kind in ("real", "diag"):
            for fmt in ("i8", "u8"):
                e = family_e(kind, fmt)
                for which in ("accepted", "refused"):
                    for sname, x in signals_e(fmt, N_OUT * 8).items():
                        out.append(("E-%s-%s-%s-%s" % (kind, fmt, which, sname), fmt, 8, e[which], x))
        return out
    for form, nt in SWEEP:
        D = FORMS[form]["D"]
        for d in range(4):
            t = family_a(nt, d, d & 1, 100 + d)
            if not takes_passes(form, t, "i8"):
                out.append(("A-%s-%d-d%d" % (form, nt, d), "i8", D, t, signal_a(N_OUT * D, D, d & 1, 200 + d)))
    for form in ("C8", "C32"):
        D = FORMS[form]["D"]
        for v in CARRY_VALUES:
            for imag in (False, True):
                out.append(("B-%s-%d-%d" % (form, v, imag), "i8", D, family_b(1024, v, imag), d_signal("i8", 1024, D)))
        for cold in (127 * W, 127 * W - 1):
            for k in hot_positions(1024):
                for mirror in (False, True):
                    out.append(("C-%s-%d-%d-%d" % (form, cold, k, mirror), "i8", D, family_c(1024, k, mirror, cold=cold), rand_i8(31, N_OUT * D)))
            out.append(("C-%s-%d-modulus" % (form, cold), "i8", D, family_c(1024, 512, modulus=True, cold=cold), rand_i8(31, N_OUT * D)))
        for fmt in ("i8", "u8"):
            for nt in ((1024, 1536) if form == "C8" else (1024, 17)):
                out.append(("D-%s-%s-%d" % (form, fmt, nt), fmt, D, family_d(nt, 40 + nt), d_signal(fmt, nt, D)))
            for name in F_ON[form]:
                t = family_f()[name]
                for sname, x in signals_f(fmt, N_OUT * D).items():
                    out.append(("F-%s-%s-%s-%s" % (form, name, fmt, sname), fmt, D, t, x))
    return out


# family F: which filters each form runs (P8: all of them)
F_ON = {
    "P8": ["bench", "floor", "peak_first", "peak_last", "random1", "random2", "random3"],
    "P8pair": ["bench", "floor"],
    "P16": ["bench", "peak_first", "random2"],
    "C8": ["bench", "peak_last", "random1"],
    "C32": ["bench", "random3"],
}

"""The exact reference of the int8 matrix FIR (tests/firmm_ref.py) held to what it restates, without a GPU:
  * its S, quantised taps, balanced digits, constant term, plane-0 pairs and size conditions against the planner
    headers themselves (tests/host/firmm_quant.cpp over csrc/hz_firmm_plan.h and hz_firmm2_plan.h), on every filter
    family of tests/test_gpu_fir_exact.py and on 200 seeded random float32 filters -- the reference is then the
    library's contract, not an invention of the tests;
  * rn32(exact sums) against the float64 direct-form oracle BIT FOR BIT on the dyadic families (where the oracle is
    itself exact): the convention y[m] = sum h[k] x[m D - k] and the i8 conversion b / 128 come from an independent
    implementation;
  * the chunk form's interval (chunk_form_interval) is a single float32 for at least 90 % of the parts of every case
    the GPU test holds to it, so it cannot hide a defect;
  * every family-E boxcar lies on the side of int32_combine_ok its name says, one float32 apart."""
import numpy as np
import pytest

import firmm_ref as R
from util import rand_i8, zeros


def all_filters():
    """(name, taps, fmt, D) of every family, at the tap counts the GPU test uses."""
    out = []
    for form, nt in R.SWEEP:
        D = R.FORMS[form]["D"]
        for d in range(4):
            out.append(("A-%d-d%d" % (nt, d), R.family_a(nt, d, d & 1, 100 + d), "i8", D))
    for nt, D in ((1024, 8), (1024, 16), (1024, 32), (17, 8)):
        for v in R.CARRY_VALUES:
            for imag in (False, True):
                out.append(("B-%d-%d-%d" % (nt, v, imag), R.family_b(nt, v, imag), "i8", D))
    for D in (8, 16, 32):
        for cold in (127 * R.W, 127 * R.W - 1):
            for k in R.hot_positions(1024):
                for mirror in (False, True):
                    out.append(("C-%d-%d-%d" % (cold, k, mirror), R.family_c(1024, k, mirror, cold=cold), "i8", D))
            out.append(("C-%d-modulus" % cold, R.family_c(1024, 512, modulus=True, cold=cold), "i8", D))
    for fmt in ("i8", "u8"):
        for nt, D in ((17, 8), (1024, 8), (1024, 16), (1536, 8), (1024, 32), (17, 32)):
            out.append(("D-%d" % nt, R.family_d(nt, 40 + nt), fmt, D))
        for name, t in R.family_f().items():
            for D in (8, 16, 32):
                out.append(("F-" + name, t, fmt, D))
        for kind in ("real", "diag"):
            for which, t in R.family_e(kind, fmt).items():
                out.append(("E-%s-%s" % (kind, which), t, fmt, 8))
    return out


def random_filters(count=200):
    r = np.random.default_rng(20260)
    out = []
    for i in range(count):
        nt = int(r.integers(16, 1537))
        kind = i % 4
        if kind == 0:
            t = r.standard_normal(nt) + 1j * r.standard_normal(nt)
        elif kind == 1:  # magnitudes over many binades
            t = np.exp2(-24.0 * r.random(nt)) * np.exp(2j * np.pi * r.random(nt))
        elif kind == 2:  # real, a random overall scale (S anywhere)
            t = r.standard_normal(nt) * np.exp2(float(r.integers(-40, 40))) + 0j
        else:            # coefficients around the digit carries, at a random power-of-two scale
            q = r.choice(np.array(R.CARRY_VALUES), nt) + r.integers(-2, 3, nt)
            t = (q + 1j * r.permutation(q)) * np.exp2(float(r.integers(-30, -10)))
        out.append(("random-%d" % i, t.astype(np.complex64), ("i8", "u8")[i & 1], (8, 16, 32)[i % 3]))
    return out


def check_against_header(cases):
    got = R.host_quant([(t, fmt, D) for _, t, fmt, D in cases], tables=True)
    for (name, t, fmt, D), h in zip(cases, got):
        what = (name, fmt, D, len(t))
        assert R.shift_of(t, fmt) == h["S"], what
        qr, qi = R.quantise(t, fmt)
        assert np.array_equal(qr, h["q_re"]) and np.array_equal(qi, h["q_im"]), what
        assert max(np.abs(qr).max(), np.abs(qi).max()) <= 1 << 30, what
        assert R.dc_of((qr, qi), fmt) == h["dc"], what
        for v2, key in ((False, "tab1"), (True, "tab2")):
            assert np.array_equal(R.table_digit_bytes(h, qr, qi, v2), h[key]), what + (key,)
        assert R.mm2_geometry_ok(len(t), D) == bool(h["geom_ok"]), what
        if D in (8, 16):
            # every pair that reads a tap with a nonzero top digit lies inside the header's window
            pairs = R.plane0_pairs(h, qr, qi, D)
            lo, hi = h["p0"]
            assert all(lo <= p < hi for p in pairs), what + (h["p0"], sorted(pairs))
    return got


def test_python_quantisation_equals_the_headers_on_every_family():
    cases = all_filters()
    got = check_against_header(cases)
    for (name, t, fmt, D), h in zip(cases, got):
        if not name.startswith("E-"):  # (family E sits ON the bound: the host program decides there)
            assert R.combine_ok(t, fmt) == bool(h["combine_ok"]), (name, fmt)
        if name[0] in "ABC":
            assert h["S"] == 30 and R.dyadic(t, fmt), name
    # the digit carries are what they are meant to be: 127 W + 1 has a top digit although |q| < 2^23
    assert R.digits(np.array([127 * R.W, 127 * R.W + 1, -128 * R.W, -128 * R.W - 1]))[0].tolist() == [0, 1, 0, -1]
    assert 127 * R.W + 1 < 1 << 23
    # family C with cold = 127 W - 1: the window is NARROWER than all pairs (an off-by-one at its ends has a tap to lose)
    h = R.host_quant([(R.family_c(1024, 512, cold=127 * R.W - 1), "i8", 8)])[0]
    assert 0 < h["p0"][1] - h["p0"][0] < h["pairs"], h["p0"]


def test_python_quantisation_equals_the_headers_on_random_filters():
    check_against_header(random_filters(200))


def test_last_tap_counts_of_the_persistent_passes():
    assert (R.mm2_last_taps(8), R.mm2_last_taps(16)) == (R.LAST8, R.LAST16)
    t = {n: np.ones(n, np.complex64) for n in (R.LAST8, R.LAST8 + 1, R.LAST16, R.LAST16 + 1)}
    got = R.host_quant([(t[R.LAST8], "i8", 8), (t[R.LAST8 + 1], "i8", 8), (t[R.LAST16], "i8", 16), (t[R.LAST16 + 1], "i8", 16)])
    assert [h["geom_ok"] for h in got] == [1, 0, 1, 0]


@pytest.mark.parametrize("D", [8, 16, 32])
def test_exact_reference_equals_the_oracle_on_dyadic_filters(orc, D):
    """Families A, B and C under i8: the oracle's float64 sums of (q / 2^23) (b / 128) are exact, so its float32 output
    is RN32 of the exact sum -- on EVERY output, the first ones (window across the stream start) included."""
    n_out = 1024
    n = n_out * D
    filters = [("A-%d-d%d-k%d" % (nt, d, k0), R.family_a(nt, d, k0, 300 + d), R.signal_a(n, D, k0, 400 + d))
               for nt in (16, 17, 1024) for d in range(4) for k0 in (0, 1)]
    white = rand_i8(55, n)
    filters += [("B-%d-%d" % (v, imag), R.family_b(200, v, imag), white) for v in R.CARRY_VALUES for imag in (False, True)]
    filters += [("C-%d" % k, R.family_c(1024, k, mirror=bool(k & 1)), white) for k in R.hot_positions(1024)]
    filters.append(("C-modulus", R.family_c(1024, 512, modulus=True), white))
    for name, taps, x in filters:
        assert R.dyadic(taps, "i8"), name
        S, q = R.shift_of(taps, "i8"), R.quantise(taps, "i8")
        assert S == 30
        xc = zeros("c64", n)
        orc.convert(xc, x)
        want = zeros("c64", n_out)
        orc.par_fir_decimate_f64(want, xc, taps, D)
        ex = R.exact_outputs(q, (0.0, 0.0), R.signed_bytes(x, "i8"), D)
        got = R.rn32_complex(ex, S)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (name, D)
        # a stream cut in two: the second half with the first as its history gives the same sums
        b = R.signed_bytes(x, "i8")
        cut = (n // 2) // D * D - 3 * D
        tail = R.exact_outputs(q, (0.0, 0.0), (b[0][cut:], b[1][cut:]), D, hist=(b[0][:cut], b[1][:cut]), planes=False)
        assert np.array_equal(tail.re, ex.re[cut // D:]) and np.array_equal(tail.im, ex.im[cut // D:]), name


def test_family_a_outputs_are_small_integers():
    """The anchor reads zeros only, so an output is a sum of at most 2 * ntaps products r 256^(3 - d) b: below 2^24 units
    of 256^(3 - d), exact in float32 -- ONE wrong digit byte anywhere changes an output by at least one such unit."""
    for d in range(4):
        for k0 in (0, 1):
            taps, x = R.family_a(1024, d, k0, 100 + d), R.signal_a(R.N_OUT * 8, 8, k0, 200 + d)
            ex = R.exact_outputs(R.quantise(taps, "i8"), (0.0, 0.0), R.signed_bytes(x, "i8"), 8)
            unit = 256 ** (3 - d)
            for v in (ex.re, ex.im):
                assert not (v % unit).any() and np.abs(v // unit).max() < 1 << 24
                assert np.array_equal(R.rn32(v, 30).astype(np.float64) * 2.0 ** 30, v.astype(np.float64))
            # every polyphase branch of the taps has nonzero taps besides the anchor
            q = R.quantise(taps, "i8")
            assert all((q[0][r::8] != 0).sum() > 1 for r in range(8))


def test_impulse_signals_visit_every_boundary_and_residue():
    for fmt in ("i8", "u8"):
        for nt, D, cuts in ((1024, 8, None), (1536, 8, None), (17, 8, None), (1024, 16, None), (1024, 32, None), (1024, 8, R.ragged_cuts())):
            n_out = cuts[-1] if cuts else R.N_OUT
            marks = R.impulse_marks(D, n_out, cuts[1:-1] if cuts else ())
            pos = np.array(R.impulse_positions(nt, D, n_out * D, marks))
            assert pos.min() >= nt + 16 * D and np.diff(pos).min() >= nt + 16 * D
            assert set(pos % 16) == set(range(16)), (nt, D)
            # every mark has an impulse at D m - 1, D m or D m + 1, and the three offsets all occur
            near = [int(np.abs(pos - m * D).min()) for m in marks if m * D >= 2 * (nt + 16 * D)]
            assert max(near) <= 1, (nt, D, near)
            offs = {int(p - m * D) for m in marks for p in pos if abs(p - m * D) <= 1}
            assert offs == {-1, 0, 1}
            x = R.d_signal(fmt, nt, D, cuts)
            rest = 128 if fmt == "u8" else 0
            assert int((x != rest).any(axis=1).sum()) == len(pos)


def test_family_e_lies_on_the_side_its_name_says():
    for kind in ("real", "diag"):
        for fmt in ("i8", "u8"):
            e = R.family_e(kind, fmt)
            got = R.host_quant([(e["accepted"], fmt, 8), (e["refused"], fmt, 8)])
            assert [h["combine_ok"] for h in got] == [1, 0], (kind, fmt)
            assert got[0]["S"] == got[1]["S"]
            a, b = e["accepted"][0], e["refused"][0]
            assert np.nextafter(a.real, np.float32(1)) == b.real and (kind == "real" or a.imag == a.real and b.imag == b.real)
            # the accepted one keeps the int32 sum of the two top planes for the inputs that line all signs up
            qr, qi = R.quantise(e["accepted"], fmt)
            A = lambda q: (R.digits(q)[0] * 256 + R.digits(q)[1])
            worst = 128 * int(np.abs(A(qr)).sum() + max(np.abs(A(qi)).sum(), np.abs(A(-qi)).sum()))
            assert worst < 1 << 31, (kind, fmt, worst)


@pytest.mark.parametrize("family", list("ABCDEF"))
def test_chunk_form_interval_is_mostly_a_single_float(family):
    """For the reference alone: on every case the GPU test holds to the interval, lo == hi for at least 90 % of the parts
    it compares (the fix-up outputs of the non-dyadic filters left out, as there)."""
    worst = (2.0, "")
    cases = [c for c in R.chunk_form_cases(family)]
    assert cases
    for name, fmt, D, taps, x in cases:
        S, q = R.shift_of(taps, fmt), R.quantise(taps, fmt)
        dc = R.dc_of(q, fmt)
        ex = R.exact_outputs(q, dc, R.signed_bytes(x, fmt), D)
        first = 0 if R.dyadic(taps, fmt) else R.fixup_outputs(len(taps), D, 16)
        same = total = 0
        for part in (0, 1):
            lo, hi = R.chunk_form_interval(ex.planes[part], dc[part], S)
            want = R.rn32(ex.re if part == 0 else ex.im, S, dc[part])
            assert np.all(lo[first:] <= want[first:]) and np.all(want[first:] <= hi[first:]), name
            same += int((lo[first:] == hi[first:]).sum())
            total += len(lo) - first
        share = same / total
        assert share >= 0.9, (name, share)
        worst = min(worst, (share, name))
    print("smallest share of single-float intervals: %.4f (%s)" % worst)

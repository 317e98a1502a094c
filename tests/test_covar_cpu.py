"""The covariance bank's and the beam scan's contract (include/hzsdr_covar.h) without a GPU: the bit-exact host program
tests/host/covar_ref.cpp, whose two evaluations -- directly from the contract, and through the kernels' tile and tree
indexing with the stream cut into pushes -- agree bit for bit (the program's exit status), against the independent
float64 restatement of tests/covar_ref.py within the derived bounds, over every listed shape and format; the exact
consequences of the arithmetic (Hermitian, +0 diagonal, sub-arrays, permutations); the tree's definition; the scan."""
import importlib
import os
from fractions import Fraction

import numpy as np
import pytest

import covar_ref as ref
from conftest import ROOT
from util import rand_c64, rand_i8, rand_i16, rand_u8

BUILD = os.path.join(ROOT, "build", "covar_cpu")
RAND = {"c64": rand_c64, "u8": rand_u8, "i8": rand_i8, "i16": rand_i16}


def rows_of(fmt, n_ch, n, seed):
    """N independent rows of n raw samples -> converted (N, n) complex64"""
    raw = np.stack([RAND[fmt](seed * 100 + i, n) for i in range(n_ch)])
    return ref.converted(fmt, raw)


@pytest.fixture(scope="module")
def streams(orc):
    """(fmt, N, B) -> converted rows of three blocks and the odd remainder"""
    return {(fmt, n_ch, b): rows_of(fmt, n_ch, ref.stream_length(b), 7 * n_ch + b) for fmt in ref.FORMATS for n_ch, b in ref.SHAPES}


@pytest.fixture(scope="module")
def exact(streams):
    """every shape and format through the host program, cut into pushes: computed once"""
    keys = list(streams)
    return dict(zip(keys, ref.exact(BUILD, [(b, streams[fmt, n_ch, b], ref.cuts(b)) for fmt, n_ch, b in keys])))


def test_two_restatements_agree_and_hold_the_bound(streams, exact):
    """(the program exits with a failure where its two evaluations differ: `exact` ran it)"""
    worst = 0.0
    for (fmt, n_ch, b), x in streams.items():
        got = exact[fmt, n_ch, b]
        want, bound = ref.covariance(x, b), ref.bank_bound(x, b)
        assert got.shape == want.shape == (4 if b > 1 else 3, n_ch, n_ch)
        err = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag))
        ratio = float((err / bound).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"N={n_ch} B={b} {fmt}: error / bound = {ratio}"
    print(f"worst error / bound over {len(streams)} runs: {worst:.4f}")


def test_hermitian_and_diagonal_exactly(exact):
    for key, r in exact.items():
        assert np.array_equal(r.real, r.real.transpose(0, 2, 1)), key
        assert np.array_equal(r.imag, -r.imag.transpose(0, 2, 1)), key
        d = np.ascontiguousarray(np.diagonal(r, axis1=1, axis2=2).imag)
        assert not d.view(np.uint32).any(), f"{key}: a diagonal entry's imaginary part is not +0"


def test_sub_array_and_permutation(streams):
    """an entry depends on its two channels only: the 4 x 4 corner of 16 channels is the 4-channel bank, and permuted
    rows give the permuted matrix"""
    x = streams["u8", 16, 1539]
    perm = np.array([3, 0, 15, 7, 8, 2, 9, 1, 4, 5, 6, 10, 11, 12, 13, 14])
    full, corner, permuted = ref.exact(BUILD, [(1539, x, []), (1539, x[:4], [5, 700]), (1539, x[perm], [])])
    assert full[:, :4, :4].tobytes() == np.ascontiguousarray(corner).tobytes()
    assert np.ascontiguousarray(full[:, perm][:, :, perm]).tobytes() == permuted.tobytes()


def test_carried_state(orc):
    """a push that resumes the open block, closes it and leaves a new open block on the same level of the stack, and a
    flush that only collapses (tests/covar_ref.py, CARRY_SHAPES): the program's two evaluations agree (its exit status),
    and cutting changes no bit"""
    streams = [rows_of("i16", n_ch, ref.carry_length(b), 31 * n_ch + b) for n_ch, b in ref.CARRY_SHAPES]
    cases = [(b, x, cut) for (n_ch, b), x in zip(ref.CARRY_SHAPES, streams) for cut in (ref.carry_cuts(b), [])]
    got = ref.exact(BUILD, cases)
    for k, (n_ch, b) in enumerate(ref.CARRY_SHAPES):
        assert got[2 * k].shape == (3, n_ch, n_ch) and got[2 * k].tobytes() == got[2 * k + 1].tobytes()
        err = np.maximum(np.abs(got[2 * k].real - ref.covariance(streams[k], b).real), np.abs(got[2 * k].imag - ref.covariance(streams[k], b).imag))
        assert (err <= ref.bank_bound(streams[k], b)).all()


def test_tree_is_not_a_running_sum():
    """the issue's case: partials 2^24, 1, 1, 1 -> 16777218 by the tree, 16777216 left to right"""
    g = [np.float32(4096.0 * 4096.0)] + [np.float32(1.0)] * 3
    assert ref.tree_sum(g) == np.float32(16777218.0)
    left = np.float32(0)
    for v in g:
        left = np.float32(left + v)
    assert left == np.float32(16777216.0)
    x = np.zeros((2, 4 * 256), np.complex64)
    x[0, 0], x[0, 256], x[0, 512], x[0, 768] = 4096, 1, 1, 1
    (r,) = ref.exact(BUILD, [(1024, x, [])])
    assert r[0, 0, 0] == np.complex64(16777218.0)
    assert ref.tree_shape(0, 7) == (((0, 1), (2, 3)), ((4, 5), 6)) and ref.tree_shape(0, 5) == (((0, 1), (2, 3)), 4)


def test_round_f32_is_float32():
    rng = np.random.default_rng(3)
    for v in rng.standard_normal(200) * 10.0 ** rng.integers(-6, 6, 200):
        assert ref.round_f32(Fraction(float(v))) == Fraction(float(np.float32(v)))
    assert ref.round_f32(Fraction(2 ** 24 + 1)) == 2 ** 24 and ref.round_f32(Fraction(2 ** 24 + 3)) == 2 ** 24 + 4


def test_scan_restatement():
    rng = np.random.default_rng(11)
    cases = []
    for n_ch in (2, 4, 9, 16):
        for g in (1, 181):
            q = (rng.standard_normal((3, n_ch, n_ch)) + 1j * rng.standard_normal((3, n_ch, n_ch))).astype(np.complex64)
            w = (rng.standard_normal((g, n_ch)) + 1j * rng.standard_normal((g, n_ch))).astype(np.complex64)
            cases.append((q, w))
    worst = 0.0
    for (q, w), p in zip(cases, ref.exact_scan(BUILD, cases)):
        ratio = float((np.abs(p - ref.scan(q, w)) / ref.scan_bound(q, w)).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"N={q.shape[1]} G={w.shape[0]}: scan error / bound = {ratio}"
    print(f"worst scan error / bound: {worst:.4f}")
    # a Hermitian matrix gives a real quadratic form: the scan of R is the beam's power
    x = rows_of("c64", 4, 999, 5)
    r = ref.covariance(x, 999).astype(np.complex64)
    w = cases[2][1][:7]
    y = w.astype(np.complex128) @ x.astype(np.complex128)
    assert np.allclose(ref.scan(r, w)[0], (np.abs(y) ** 2).sum(axis=1), rtol=1e-5)


def test_header_and_python_layer_declare_the_same_entries():
    capi = importlib.import_module("go-sdr_amd._capi")
    import re
    text = open(os.path.join(ROOT, "include", "hzsdr_covar.h")).read()
    declared = set(re.findall(r"^int (hzsdr_(?:covar|scan)_\w+)\(", text, re.M))
    assert declared == set(capi.COVAR_SIGNATURES) and len(declared) == 12
    for name in declared:
        assert hasattr(capi.lib, name)

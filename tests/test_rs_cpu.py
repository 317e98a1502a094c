"""The Reed-Solomon decoder bank (include/hzsdr_rs.h) without a GPU: the numpy helpers of go-sdr_amd/rs.py against known
answers, the numpy restatement tests/rs_ref.py (linear algebra) against the definition itself (every codeword of the
k = 1 codes tried), and the host program tests/host/rs_ref.cpp (csrc/hz_rs_math.h: Berlekamp-Massey, Chien, Forney)
against both -- exactly, verdicts and miscorrections beyond t included."""
import importlib
import os

import numpy as np
import pytest

import rs_ref as ref
from conftest import ROOT

BUILD = os.path.join(ROOT, "build")


@pytest.fixture(scope="module")
def hz():
    return importlib.import_module("go-sdr_amd")


def words_with_errors(code, count, seed):
    """`count` words: codewords with 0 ... nroots symbol errors in turn, then words of random bytes"""
    n, nroots = code[4], code[3]
    k = n - nroots
    out = []
    for w in range(count):
        word = ref.encode(code, ref.random_bytes(k, seed * 7919 + w))
        errs = w % (nroots + 2)
        if errs > nroots:
            word = ref.random_bytes(n, seed * 104729 + w)
        else:
            where = np.argsort(ref.splitmix64(seed * 31 + w, n), kind="stable")[:errs]
            word[where] ^= (ref.random_bytes(errs, seed * 17 + w) | 1).astype(np.uint8)
        out.append(word)
    return np.stack(out)


def test_known_answers(hz):
    assert hz.ccsds_randomizer(8).tolist() == [0xFF, 0x48, 0x0E, 0xC0, 0x9A, 0x0D, 0x70, 0xBC]
    assert np.array_equal(hz.ccsds_randomizer(300)[255:], hz.ccsds_randomizer(45))  # the period: 255 bits, so 255 bytes
    to_dual, from_dual = hz.ccsds_dual_basis()
    assert to_dual[:8].tolist() == [0x00, 0x7B, 0xAF, 0xD4, 0x99, 0xE2, 0x36, 0x4D]
    assert from_dual[:8].tolist() == [0x00, 0xCC, 0xAC, 0x60, 0x79, 0xB5, 0xD5, 0x19]
    assert np.array_equal(from_dual[to_dual], np.arange(256)) and np.array_equal(to_dual[from_dual], np.arange(256))
    assert (hz.CCSDS_RS_255_223, hz.CCSDS_RS_255_239, hz.DVB_RS_204_188) == (ref.CCSDS_223, ref.CCSDS_239, ref.DVB)


@pytest.mark.parametrize("code", [ref.CCSDS_223, ref.CCSDS_239, ref.DVB, *ref.K1_CODES])
def test_encode_has_zero_syndromes(hz, code):
    k = code[4] - code[3]
    data = ref.random_bytes(3 * k, 5).reshape(3, k)
    words = hz.rs_encode(code, data)
    assert words.shape == (3, code[4]) and np.array_equal(words[:, :k], data)
    assert not ref.syndromes(code, words).any()
    assert np.array_equal(words[1], ref.encode(code, data[1]))
    g = hz.rs_generator(code)
    assert g.shape == (code[3] + 1,) and g[0] == 1
    assert not ref.syndromes((*code[:4], code[3] + 1), g).any()  # the generator is a codeword of the shortest code
    two = hz.interleave_codewords(words[:2])
    assert np.array_equal(two[0::2], words[0]) and np.array_equal(two[1::2], words[1])


@pytest.mark.parametrize("code", ref.K1_CODES)
def test_numpy_and_program_against_every_codeword(code):
    """a few thousand words with 0 ... nroots errors and random words: both restatements say what the search says"""
    words = words_with_errors(code, 3000, code[3])
    q = ref.Config(code)
    (data, info), = ref.exact(BUILD, [(q, words[None], None)])
    verdicts = set()
    for w, word in enumerate(words):
        want, e = ref.nearest_word(code, word)
        got, ge = ref.decode_word(code, word)
        assert ge == e and np.array_equal(got, want), (code, w)
        assert int(info[0, w]) == (e | 1 << 31 if e != ref.FAILED else 1 << 16), (code, w)
        assert np.array_equal(data[0, w], want[:q.k]), (code, w)
        verdicts.add(e)
    assert verdicts == set(range(code[3] // 2 + 1)) | {ref.FAILED}


@pytest.mark.parametrize("code,I", [(ref.CCSDS_223, 2), (ref.CCSDS_239, 1), (ref.DVB, 3), ((0x11D, 1, 7, 64, 255), 1), ((0x187, 112, 11, 7, 40), 8)])
def test_numpy_against_program_full_size(hz, code, I):
    """frames of I codewords with 0, 1, t - 1, t, t + 1, nroots errors and garbage, through the dual basis and the randomiser"""
    to_dual, from_dual = hz.ccsds_dual_basis()
    q = ref.Config(code, I, in_map=from_dual, out_map=to_dual, scramble=hz.ccsds_randomizer(255))
    t, n = q.t, q.n
    frames, planted = [], []
    for f, errs in enumerate([0, 1, t - 1, t, t + 1, code[3], -1]):
        frame, _ = ref.clean_frame(q, 100 * I + f)
        if errs < 0:
            frame = ref.random_bytes(q.F, f)
        for i in range(I if errs > 0 else 0):
            where = np.argsort(ref.splitmix64(f * 64 + i, n), kind="stable")[:errs]
            frame = ref.hurt(q, frame, i, where, ref.random_bytes(errs, f + i) | 1)
        frames.append(frame)
        planted.append(errs)
    frames = np.stack(frames)[None]
    want_d, want_i = ref.decode_block(q, frames)
    (got_d, got_i), = ref.exact(BUILD, [(q, frames, None)])
    assert np.array_equal(got_i, want_i) and np.array_equal(got_d, want_d)
    for f, errs in enumerate(planted):
        if 0 <= errs <= t:
            assert int(want_i[0, f]) == (I * errs | 1 << 31), (f, errs)
        elif errs == t + 1:
            assert int(want_i[0, f]) >> 31 == 0


def test_configurations_by_the_plan():
    sets = [(p, 0, 1, 2, 3, 1, 0) for p in range(0x100, 0x200)]
    primitive = [s[0] for s, (ok, _, _) in zip(sets, ref.check(BUILD, sets)) if ok]
    assert len(primitive) == 16 and 0x187 in primitive and 0x11D in primitive and 0x11B not in primitive  # phi(255) / 8
    good = (0x187, 112, 11, 32, 255, 4, 255)
    edits = {0: [0x87, 0x387, 0x11B, 0x100], 1: [255], 2: [0, 3, 5, 17, 51, 255], 3: [0, 1, 65], 4: [32, 256], 5: [0, 9], 6: [2041]}
    bad = [tuple(v if i == j else x for j, x in enumerate(good)) for i, vs in edits.items() for v in vs]
    fine = [good, (0x11D, 254, 254, 64, 65, 8, 2040), (0x11D, 0, 1, 2, 3, 1, 0), (0x187, 0, 2, 3, 255, 1, 1)]
    got = ref.check(BUILD, bad + fine)
    assert [g[0] for g in got] == [False] * len(bad) + [True] * len(fine)
    assert got[len(bad)][1:] == (223, 16) and got[len(bad) + 1][1:] == (1, 32) and got[len(bad) + 3][1:] == (252, 1)

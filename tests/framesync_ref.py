"""The independent restatement of the frame sync bank's definition (include/hzsdr_framesync.h) in numpy, the stream
makers of its tests, and the runner of the host program tests/host/framesync_ref.cpp (the bytes the device must produce).

The numpy restatement is written from the header's text: it takes a row's WHOLE stream, decides every float, evaluates
every window position by position over the whole bit array -- no ring, no tiles, no state between pushes -- walks the
candidates through the hold-off, and only then deals the frames to the pushes by the bit that completes them."""
import os
import struct
import subprocess

import numpy as np

from util import splitmix64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL_F32, C64 = 32, 1
FORM_COMPLEX, FORM_DIBIT, FORM_DIFF = 1, 2, 4
MAX_ROWS, MAX_WORD, MAX_PAYLOAD, MAX_HYP = 8192, 64, 8192, 4


class Config:
    """a bank's configuration, as hzsdr_framesync_create takes it"""

    def __init__(self, W, words, P, B=1, cplx=False, mask=None, thr=0, maps=None, diff=0, holdoff=None):
        self.W, self.P, self.B, self.cplx, self.thr, self.diff = int(W), int(P), int(B), bool(cplx), int(thr), int(diff)
        self.words = [int(w) for w in np.atleast_1d(words)]
        self.maps = [0] * len(self.words) if maps is None else [int(m) for m in maps]
        self.mask = (1 << self.W) - 1 if mask is None else int(mask)
        self.holdoff = (self.W + self.P) // max(self.B, 1) if holdoff is None else int(holdoff)
        self.K, self.FB = self.W + self.P - 1, (self.P + 7) // 8
        self.HB = (self.K + 7) // 8

    @property
    def kind(self):
        return C64 if self.cplx else REAL_F32

    def create_args(self):
        """(word_bits, words, maps, payload_bits) and the keywords of Context.frame_sync"""
        return (self.W, self.words, self.maps, self.P), dict(bits_per_symbol=self.B, mask=self.mask, thr=self.thr, diff=self.diff, holdoff=self.holdoff)


def accepted(q):
    """the header's validation, restated"""
    if q.B not in (1, 2) or (q.B == 2 and not q.cplx):
        return False
    if not (q.B <= q.W <= 64 and q.W % q.B == 0 and q.B <= q.P <= 8192 and q.P % q.B == 0 and 1 <= len(q.words) <= 4):
        return False
    if q.mask == 0 or q.mask >> q.W or not 0 <= q.thr < bin(q.mask).count("1") or q.diff not in (0, 1, 2) or (q.diff and q.B == 2):
        return False
    if not 1 <= q.holdoff <= 2 ** 31:
        return False
    return all(0 <= w < 1 << q.W for w in q.words) and all(0 <= m < (4 if q.B == 2 else 2) for m in q.maps)


def floats_of(x, q):
    """the floats a row is decided from, as uint32 bit patterns: a real row's, a complex row's Re (B = 1) or re, im, ... (B = 2)"""
    v = np.ascontiguousarray(x)
    if q.cplx:
        f = v.view(np.float32).reshape(-1, 2)
        f = f.reshape(-1) if q.B == 2 else f[:, 0]
    else:
        f = v
    return np.ascontiguousarray(f, np.float32).view(np.uint32)


def map_bits(bits, m, B):
    """payload bits through map m"""
    bits = np.asarray(bits, np.uint8)
    if B == 1:
        return bits ^ np.uint8(m & 1)
    b0, b1 = bits[0::2].copy(), bits[1::2].copy()
    for _ in range(m % 4):
        b0, b1 = b1, b0 ^ 1
    out = np.empty_like(bits)
    out[0::2], out[1::2] = b0, b1
    return out


def word_bits(word, W):
    """the W bits of a word, first received first"""
    return np.array([(int(word) >> (W - 1 - k)) & 1 for k in range(W)], np.uint8)


def rotated_words(word, W):
    """[the word as received under x i^q, q = 0 ... 3]: the word through the inverse of map q (sync_hypotheses, restated)"""
    return [int("".join(str(b) for b in map_bits(word_bits(word, W), (4 - q) % 4, 2)), 2) for q in range(4)]


def brute(q, pushes, cap):
    """One row.  pushes: the row's symbols per push (each the symbols that push CONSUMES: real float32 or complex64
    arrays) -> ([per push (frames uint8 (k, FB), positions, info, count)], state (position, hold, history bytes, last))
    by the definition, over the whole stream at once; k = min(count, cap)."""
    f = np.concatenate([floats_of(p, q) for p in pushes]) if pushes else np.zeros(0, np.uint32)
    d = ((f >> np.uint32(31)) ^ np.uint32(1)).astype(np.uint8)
    prev = np.concatenate([[0], d])[:len(d)].astype(np.uint8)
    b = d if q.diff == 0 else (d ^ prev if q.diff == 1 else d ^ prev ^ 1)
    total = len(b)
    ends = np.cumsum([len(floats_of(p, q)) for p in pushes])  # the bits delivered behind each push
    wb = [word_bits(w, q.W) for w in q.words]
    mb = word_bits(q.mask, q.W).astype(bool)
    out = [[] for _ in pushes]
    hold = 0
    for e in range(q.W - 1, total - q.P):
        if (e + 1) % q.B:
            continue
        win = b[e - q.W + 1:e + 1]
        dist = [int(((win != w) & mb).sum()) for w in wb]
        best = min(dist)
        if best > q.thr:
            continue
        h = dist.index(best)
        s = (e + 1) // q.B
        if s < hold:
            continue
        hold = s + q.holdoff
        payload = map_bits(b[e + 1:e + 1 + q.P], q.maps[h], q.B)
        k = int(np.searchsorted(ends, e + q.P, side="right"))  # the push that delivers bit e + P
        out[k].append((np.packbits(payload), s, best | (h << 8)))
    res = []
    for fr in out:
        keep = fr[:cap]
        res.append((np.array([x[0] for x in keep], np.uint8).reshape(len(keep), q.FB), np.array([x[1] for x in keep], np.uint64),
                    np.array([x[2] for x in keep], np.uint32), len(fr)))
    hist = np.zeros(q.K, np.uint8)
    take = min(q.K, total)
    if take:
        hist[q.K - take:] = b[total - take:]
    return res, (total // q.B, hold, np.packbits(hist), int(d[-1]) if total else 0)


# ---- the streams -------------------------------------------------------------------------------------

def random_bits(n, seed):
    return (splitmix64(seed, n) >> np.uint64(63)).astype(np.uint8)


def soft(bits, seed, q, rotate=0):
    """soft symbols that decide `bits` (B = 1: one per bit; B = 2: one complex per dibit, b0 on Re and b1 on Im): +-
    magnitudes in [0.25, 1.25); a complex row's other component (B = 1) is noise; rotate: times i^rotate (B = 2)"""
    bits = np.asarray(bits, np.uint8)
    z = splitmix64(seed ^ 0x5EED, 2 * len(bits) + 2)
    mag = (z[:len(bits)] >> np.uint64(40)).astype(np.float64) / float(1 << 24) + 0.25
    v = ((bits.astype(np.float64) * 2.0 - 1.0) * mag).astype(np.float32)
    if not q.cplx:
        return v
    if q.B == 1:
        im = ((z[len(bits):2 * len(bits)] >> np.uint64(40)).astype(np.float64) / float(1 << 23) - 1.0).astype(np.float32)
        return (v + 1j * im).astype(np.complex64)
    x = v.view(np.complex64).copy()
    for _ in range(rotate % 4):
        x = (-x.imag + 1j * x.real).astype(np.complex64)  # times i, exactly
    return x


def plant(bits, at, word, W, payload):
    """the word's W bits at bit `at` of `bits` and the payload behind them, in place"""
    bits[at:at + W] = word_bits(word, W)
    bits[at + W:at + W + len(payload)] = payload
    return bits


def encode_diff(bits, diff):
    """the raw decisions d whose differential decoding (d[-1] = 0) gives `bits`"""
    if diff == 0:
        return np.asarray(bits, np.uint8).copy()
    d, prev = np.empty(len(bits), np.uint8), 0
    for i, b in enumerate(bits):
        prev = d[i] = (int(b) ^ prev) if diff == 1 else (int(b) ^ prev ^ 1)
    return d


# ---- the program -------------------------------------------------------------------------------------

_EXE = {}


def build_exact(build_dir):
    """g++ -O2 of tests/host/framesync_ref.cpp -> the program's path (built once per directory)"""
    if build_dir not in _EXE:
        os.makedirs(build_dir, exist_ok=True)
        exe = os.path.join(build_dir, "framesync_ref")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"),
                               os.path.join(ROOT, "tests", "host", "framesync_ref.cpp"), "-o", exe])
        _EXE[build_dir] = exe
    return _EXE[build_dir]


def _head(q, has_state, pushes):
    words, maps = (q.words + [0] * 4)[:4], (q.maps + [0] * 4)[:4]
    return struct.pack("<9i", int(q.cplx), q.B, q.W, q.thr, len(q.words), q.P, q.diff, int(has_state), pushes) + \
        struct.pack("<6Q4I", q.mask, q.holdoff, *words, *maps)


def exact(build_dir, cases):
    """cases: [(config, pushes, cap)] or [(config, pushes, cap, state)] -> [([per push (frames (R, cap, FB), positions
    (R, cap), info (R, cap), counts (R,))], state)] by the program.  pushes: a list of x or (x, counts); x is float32 or
    complex64 (R, n) (or (n,) for one row); counts uint32 (R,).  state: (positions, holds, history (R, HB), last)."""
    exe = build_exact(build_dir)
    src, dst = os.path.join(build_dir, "framesync_cases.bin"), os.path.join(build_dir, "framesync_out.bin")
    shapes = []
    with open(src, "wb") as f:
        for case in cases:
            q, pushes, cap = case[0], case[1], int(case[2])
            state = case[3] if len(case) > 3 else None
            first = pushes[0][0] if isinstance(pushes[0], tuple) else pushes[0]
            R = 1 if np.asarray(first).ndim == 1 else np.asarray(first).shape[0]
            f.write(_head(q, state is not None, len(pushes)))
            f.write(struct.pack("<qq", R, cap))
            if state is not None:
                p, h, y, d = state
                f.write(np.ascontiguousarray(p, np.uint64).tobytes() + np.ascontiguousarray(h, np.uint64).tobytes())
                y = np.ascontiguousarray(y, np.uint8)
                assert y.shape == (R, q.HB)
                f.write(y.tobytes() + np.ascontiguousarray(d, np.uint8).tobytes())
            for p in pushes:
                x, c = p if isinstance(p, tuple) else (p, None)
                x = np.ascontiguousarray(np.asarray(x).reshape(R, -1))
                assert x.dtype == (np.complex64 if q.cplx else np.float32)
                f.write(struct.pack("<qi", x.shape[1], int(c is not None)))
                if c is not None:
                    f.write(np.ascontiguousarray(c, np.uint32).tobytes())
                f.write(x.tobytes())
            shapes.append((q, R, cap, len(pushes)))
    subprocess.check_call([exe, "run", src, dst])
    out, raw, off = [], open(dst, "rb").read(), 0

    def take(dtype, shape):
        nonlocal off
        count = int(np.prod(shape))
        a = np.frombuffer(raw, dtype, count, off).copy().reshape(shape)
        off += a.nbytes
        return a
    for q, R, cap, pushes in shapes:
        per = [(take(np.uint8, (R, cap, q.FB)), take(np.uint64, (R, cap)), take(np.uint32, (R, cap)), take(np.uint32, (R,))) for _ in range(pushes)]
        state = (take(np.uint64, (R,)), take(np.uint64, (R,)), take(np.uint8, (R, q.HB)), take(np.uint8, (R,)))
        out.append((per, state))
    assert off == len(raw)
    os.remove(src), os.remove(dst)
    return out


def check(build_dir, configs):
    """[config] -> [accepted] by csrc/hz_framesync_plan.h"""
    exe = build_exact(build_dir)
    src, dst = os.path.join(build_dir, "framesync_sets.bin"), os.path.join(build_dir, "framesync_checked.bin")
    with open(src, "wb") as f:
        for q in configs:
            f.write(_head(q, False, 0))
    subprocess.check_call([exe, "check", src, dst])
    got = np.fromfile(dst, np.int32)
    os.remove(src), os.remove(dst)
    assert len(got) == len(configs)
    return [bool(v) for v in got]


def consumed(pushes, row, R):
    """what row `row` consumes of each push of exact()'s form: the list brute() takes"""
    out = []
    for p in pushes:
        x, c = p if isinstance(p, tuple) else (p, None)
        x = np.asarray(x).reshape(R, -1)
        n = x.shape[1] if c is None else min(int(c[row]), x.shape[1])
        out.append(x[row, :n])
    return out


def same_as_brute(q, pushes, cap, got):
    """the program's (or the device's) results of one record against brute(), row by row -> the frames found in all"""
    per, state = got
    R = per[0][3].shape[0] if per else state[0].shape[0]
    found = 0
    for r in range(R):
        want, (pos, hold, hist, last) = brute(q, consumed(pushes, r, R), cap)
        for k, ((fr, ps, inf, cnt), (wf, wp, wi, wc)) in enumerate(zip(per, want)):
            assert int(cnt[r]) == wc, (r, k, int(cnt[r]), wc)
            m = min(wc, cap)
            assert np.array_equal(fr[r, :m], wf) and np.array_equal(ps[r, :m], wp) and np.array_equal(inf[r, :m], wi), (r, k)
            found += wc
        assert int(state[0][r]) == pos and int(state[1][r]) == hold and np.array_equal(state[2][r], hist), r
        if q.diff:
            assert int(state[3][r]) == last, r
    return found

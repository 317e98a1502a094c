"""The independent restatement of the soft frame bank's definition (include/hzsdr_softframe.h) in numpy, the helpers of
its tests, and the runner of the host program tests/host/softframe_ref.cpp (the bytes the device must produce).

The numpy restatement is written from the header's text and shaped unlike the C++: it concatenates a row's WHOLE stream
of decision floats, takes every (s, h) ever emitted, slices stream[s * B : s * B + P] and applies the map on uint32
views.  It knows no pushes, no history and no window."""
import os
import struct
import subprocess

import numpy as np

import framesync_ref as fsr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL_F32, C64 = 32, 1
SERVED, OUTSIDE, NO_HYPOTHESIS = 0, 1, 2
FORM_COMPLEX, FORM_DIBIT = 1, 2
QNAN, SIGN, SENT = 0x7FC00000, 0x80000000, 0xA5A5A5A5
THREADS = 256


class Config:
    """a bank's configuration, as hzsdr_softframe_create takes it"""

    def __init__(self, P, B=1, cplx=False, maps=(0,)):
        self.P, self.B, self.cplx, self.maps = int(P), int(B), bool(cplx), [int(m) for m in maps]

    @property
    def kind(self):
        return C64 if self.cplx else REAL_F32

    @property
    def Ps(self):
        return self.P // self.B

    @property
    def HF(self):
        return self.P - self.B

    @property
    def step(self):
        return THREADS * self.B


def of_framesync(fq):
    """the configuration beside a framesync_ref.Config"""
    return Config(fq.P, fq.B, fq.cplx, fq.maps)


def accepted(q):
    """the header's validation, restated"""
    if q.B not in (1, 2) or (q.B == 2 and not q.cplx):
        return False
    if not (q.B <= q.P <= 8192 and q.P % q.B == 0 and 1 <= len(q.maps) <= 4):
        return False
    return all(0 <= m < (4 if q.B == 2 else 2) for m in q.maps)


# ---- the definition, over whole streams ---------------------------------------------------------------------

def mapped(q, floats, m):
    """P decision floats (uint32) through map m"""
    v = np.array(floats, np.uint32)
    if q.B == 1:
        return v ^ np.uint32(SIGN if m & 1 else 0)
    x0, x1 = v[0::2].copy(), v[1::2].copy()
    for _ in range(m % 4):
        x0, x1 = x1, x0 ^ np.uint32(SIGN)
    out = np.empty_like(v)
    out[0::2], out[1::2] = x0, x1
    return out


def frame(q, stream, s, h):
    """the frame at symbol s under hypothesis h out of a row's whole stream of decision floats (uint32)"""
    lo = int(s) * q.B
    assert lo + q.P <= len(stream)
    return mapped(q, stream[lo:lo + q.P], q.maps[h])


def row_stream(q, pushes, row, R):
    """a row's whole stream of decision floats (uint32): what it consumes of every push, concatenated"""
    parts = [fsr.floats_of(x, q) for x in fsr.consumed([(p[0], p[1]) if p[1] is not None else p[0] for p in pushes], row, R)]
    return np.concatenate(parts) if parts else np.zeros(0, np.uint32)


def same_as_whole_stream(q, pushes, cap, per, R):
    """every SERVED frame of the program's (or the device's) pushes against the whole-stream restatement -> frames compared"""
    seen = 0
    for r in range(R):
        stream = row_stream(q, pushes, r, R)
        for (x, ic, got, pos, info), (y, status) in zip(pushes, per):
            for f in range(min(int(got[r]), cap)):
                if int(status[r, f]) != SERVED:
                    continue
                want = frame(q, stream, pos[r, f], (int(info[r, f]) >> 8) & 0xFF)
                assert np.array_equal(y[r, f], want), (r, f)
                seen += 1
    return seen


def signs_are_the_packed_bits(soft, packed, P):
    """the equivalence of the header: bit k of the frame sync bank's frame is 1 iff the sign bit of float k is clear"""
    bits = np.unpackbits(np.asarray(packed, np.uint8), axis=-1)[..., :P]
    return np.array_equal(bits, ((np.asarray(soft).view(np.uint32) >> np.uint32(31)) ^ np.uint32(1)).astype(np.uint8))


# ---- streams --------------------------------------------------------------------------------------------------

WORD32 = 0x1ACFFC1D


def sync_config(P, form, W=32, word=WORD32):
    """a framesync_ref.Config with a clean 32-bit word and thr 0 for `form`: "real" (maps 0 and 1: the word and its
    complement), "re" (complex rows, B = 1, map 0) or "dibit" (complex rows, B = 2, the four rotations)"""
    if form == "real":
        return fsr.Config(W, [word, word ^ ((1 << W) - 1)], P, maps=[0, 1])
    if form == "re":
        return fsr.Config(W, [word], P, cplx=True)
    return fsr.Config(W, fsr.rotated_words(word, W), P, B=2, cplx=True, maps=[0, 1, 2, 3])


def make_stream(fq, nframes, gap, seed, turn=0, special=False, lead=None):
    """one row: `nframes` frames (the word, P random payload bits) `gap` symbols apart behind `lead` symbols, as soft
    symbols; turn: the hypothesis the row is received under (B = 1: 1 = inverted; B = 2: times i^turn).  special: some
    payload floats become NaNs with payload bits, zeros and infinities OF THE SAME SIGN, so the decisions stay."""
    W, P, B = fq.W, fq.P, fq.B
    lead = (7 + seed % 5) if lead is None else lead
    per = (W + P) // B + gap
    bits = fsr.random_bits((lead + nframes * per + 3) * B, seed)
    pay = []
    for f in range(nframes):
        at = (lead + f * per) * B
        fsr.plant(bits, at, WORD32, W, fsr.random_bits(P, seed * 1000 + f))
        pay.append(at + W)
    if B == 1:
        x = fsr.soft(bits ^ np.uint8(turn & 1), seed, fq)
    else:
        x = fsr.soft(bits, seed, fq, rotate=turn)
    if special:
        u = np.ascontiguousarray(x).view(np.uint32).copy()
        step = 2 if (fq.cplx and B == 1) else 1
        kinds = (0x7FC12345, 0x7F800001, 0, 0x7F800000, 0x7FFFFFFF)
        for f, at in enumerate(pay):
            for j, k in enumerate(range(at + (f % 3), at + P, max(1, P // 7))):
                u[k * step] = (u[k * step] & np.uint32(SIGN)) | np.uint32(kinds[(f + j) % len(kinds)])
        x = u.view(x.dtype)
    return x


def make_rows(fq, R, nframes, gap, seed, special=False):
    """(R, n) rows of make_stream, every row under another hypothesis and with its frames elsewhere"""
    H = len(fq.words)
    rows = [make_stream(fq, nframes, gap, seed + r, turn=r % H, special=special, lead=5 + 3 * r) for r in range(R)]
    n = max(len(x) for x in rows)
    out = np.ones((R, n), rows[0].dtype)  # (a quiet tail: +1)
    for r, x in enumerate(rows):
        out[r, :len(x)] = x
    return out


# ---- pushes ---------------------------------------------------------------------------------------------------

def cut(x, sizes):
    """x (R, n) or (n,) cut along its last axis into pieces of `sizes` (the rest last; 0 gives an empty push)"""
    out, at = [], 0
    for s in sizes:
        out.append(x[..., at:at + s])
        at += s
    if at < x.shape[-1]:
        out.append(x[..., at:])
    return out


def with_frames(build_dir, fq, pieces, cap, in_counts=None):
    """the pieces of a stream (each (R, n) or (n,); in_counts: None or one uint32 (R,) or None per piece) -> soft pushes
    [(x, in_counts, got, positions, info)] and the hard frames per push, found by tests/host/framesync_ref.cpp"""
    ic = in_counts or [None] * len(pieces)
    ((per, _),) = fsr.exact(build_dir, [(fq, [p if c is None else (p, c) for p, c in zip(pieces, ic)], cap)])
    pushes = [(p, c, got, pos, info) for (p, c), (_, pos, info, got) in zip(zip(pieces, ic), per)]
    return pushes, [fr for fr, _, _, _ in per]


# ---- the program ------------------------------------------------------------------------------------------------

_EXE = {}


def build_exact(build_dir):
    """g++ -O2 of tests/host/softframe_ref.cpp -> the program's path (built once per directory)"""
    if build_dir not in _EXE:
        os.makedirs(build_dir, exist_ok=True)
        exe = os.path.join(build_dir, "softframe_ref")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"),
                               os.path.join(ROOT, "tests", "host", "softframe_ref.cpp"), "-o", exe])
        _EXE[build_dir] = exe
    return _EXE[build_dir]


def _head(q, has_state, pushes):
    maps = (q.maps + [0] * 4)[:4]
    return struct.pack("<10i", int(q.cplx), q.B, q.P, len(q.maps), *maps, int(has_state), pushes)


def exact(build_dir, cases):
    """cases: [(config, pushes, cap)] or [(config, pushes, cap, state)] -> [([per push (floats uint32 (R, cap, P), status
    (R, cap))], (positions (R,), history uint32 (R, HF)))] by the program.  pushes: [(x, in_counts, got, positions, info)]
    with x float32 or complex64 (R, n) (or (n,) for one row); state: (positions, history (R, HF) float32 or uint32).
    Slots from min(got, cap) up are SENT."""
    exe = build_exact(build_dir)
    src, dst = os.path.join(build_dir, "softframe_cases.bin"), os.path.join(build_dir, "softframe_out.bin")
    shapes = []
    with open(src, "wb") as f:
        for case in cases:
            q, pushes, cap = case[0], case[1], int(case[2])
            state = case[3] if len(case) > 3 else None
            R = 1 if np.asarray(pushes[0][0]).ndim == 1 else np.asarray(pushes[0][0]).shape[0]
            f.write(_head(q, state is not None, len(pushes)) + struct.pack("<qq", R, cap))
            if state is not None:
                y = np.ascontiguousarray(state[1]).view(np.uint32)
                assert y.shape == (R, q.HF)
                f.write(np.ascontiguousarray(state[0], np.uint64).tobytes() + y.tobytes())
            for x, ic, got, pos, info in pushes:
                x = np.ascontiguousarray(np.asarray(x).reshape(R, -1))
                assert x.dtype == (np.complex64 if q.cplx else np.float32)
                f.write(struct.pack("<qi", x.shape[1], int(ic is not None)))
                if ic is not None:
                    f.write(np.ascontiguousarray(ic, np.uint32).tobytes())
                f.write(x.tobytes())
                if cap:
                    pos, info = np.ascontiguousarray(pos, np.uint64), np.ascontiguousarray(info, np.uint32)
                    assert pos.shape == (R, cap) and info.shape == (R, cap)
                    f.write(np.ascontiguousarray(got, np.uint32).tobytes() + pos.tobytes() + info.tobytes())
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
        per = [(take(np.uint32, (R, cap, q.P)), take(np.uint32, (R, cap))) for _ in range(pushes)]
        out.append((per, (take(np.uint64, (R,)), take(np.uint32, (R, q.HF)))))
    assert off == len(raw)
    os.remove(src), os.remove(dst)
    return out


def check(build_dir, configs):
    """[config] -> [accepted] by csrc/hz_softframe_plan.h"""
    exe = build_exact(build_dir)
    src, dst = os.path.join(build_dir, "softframe_sets.bin"), os.path.join(build_dir, "softframe_checked.bin")
    with open(src, "wb") as f:
        for q in configs:
            f.write(_head(q, False, 0))
    subprocess.check_call([exe, "check", src, dst])
    got = np.fromfile(dst, np.int32)
    os.remove(src), os.remove(dst)
    assert len(got) == len(configs)
    return [bool(v) for v in got]

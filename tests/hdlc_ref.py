"""The independent restatements of the HDLC deframer bank's definition (include/hzsdr_hdlc.h), the helpers of its tests,
and the runner of the host program tests/host/hdlc_ref.cpp (the bytes the device must produce).

brute(): numpy over the whole stream at once -- the events as vectorised 8-bit window tests, the spans between
consecutive flags, the stuffed bits of a span as one vectorised 6-bit test -- with no ring, no tiles, no state and no
span limit (that Lmax loses nothing is thereby checked too).  It takes planted faults, so that the tests can show that
they would notice.
textbook(): the decoder of the books, one bit at a time: a ones counter that drops the 0 behind five 1s, a flag closes a
frame and opens the next, seven 1s abort.  It knows nothing of windows, events or spans; its FCS check recomputes the FCS
over the bytes in front and compares it with the bytes behind."""
import os
import struct
import subprocess

import numpy as np

from util import splitmix64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL_F32, C64 = 32, 1
MAX_ROWS, MAX_BYTES = 8192, 1024
EVENT_ABORT, EVENT_FLAG = 0, 1
FORM_COMPLEX, FORM_DIFF, FORM_FCS16, FORM_FCS32, FORM_MSB_FIRST, FORM_KEEP_BAD = 1, 4, 8, 16, 32, 64
CHUNK_TILES = 16
FLAG = np.array([0, 1, 1, 1, 1, 1, 1, 0], np.uint8)
ABORT = np.array([0, 1, 1, 1, 1, 1, 1, 1], np.uint8)
POLY = {16: 0x8408, 32: 0xEDB88320}
GOOD = {16: 0xF0B8, 32: 0xDEBB20E3}


class Config:
    """a bank's configuration, as hzsdr_hdlc_create takes it"""

    def __init__(self, diff=0, fcs=16, min_bytes=None, max_bytes=64, msb_first=0, keep_bad=0, cplx=False):
        self.diff, self.fcs, self.max_bytes, self.cplx = int(diff), int(fcs), int(max_bytes), bool(cplx)
        self.min_bytes = self.fcs // 8 + 1 if min_bytes is None else int(min_bytes)
        self.msb_first, self.keep_bad = int(msb_first), int(keep_bad)

    kind = property(lambda s: C64 if s.cplx else REAL_F32)
    FB = property(lambda s: s.max_bytes)
    Lmax = property(lambda s: 8 * s.max_bytes + 8 * s.max_bytes // 5)
    K = property(lambda s: s.Lmax + 8)
    HB = property(lambda s: (s.K + 7) // 8)

    def create_kw(self):
        return dict(diff=self.diff, fcs=self.fcs, min_bytes=self.min_bytes, max_bytes=self.max_bytes, msb_first=self.msb_first, keep_bad=self.keep_bad)

    def accepted(self):
        """check_config of csrc/hz_hdlc_plan.h, restated"""
        return (self.diff in (0, 1, 2) and self.fcs in (0, 16, 32) and 1 <= self.min_bytes <= self.max_bytes <= MAX_BYTES and
                self.min_bytes > self.fcs // 8 and self.msb_first in (0, 1) and self.keep_bad in (0, 1))


# ---- the definition, whole arrays -------------------------------------------------------------------

def floats_of(x):
    """the float32 bit patterns that decide: a real row's floats, a complex row's real parts"""
    x = np.asarray(x)
    if np.iscomplexobj(x):
        return np.ascontiguousarray(x, np.complex64).view(np.float32).reshape(-1, 2)[:, 0].copy().view(np.uint32)
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def decided_bits(f, diff):
    """float bit patterns -> (b, d): the stream's bits and the raw decisions"""
    d = ((f >> np.uint32(31)) ^ np.uint32(1)).astype(np.uint8)
    prev = np.concatenate([[0], d])[:len(d)].astype(np.uint8)
    return (d if diff == 0 else (d ^ prev if diff == 1 else d ^ prev ^ 1)), d


def fcs_register(bits, fcs):
    c, poly = (1 << fcs) - 1, POLY[fcs]
    for b in bits:
        c = (c >> 1) ^ (poly if (c ^ int(b)) & 1 else 0)
    return c


def find_events(b, fault=None):
    """[(position, kind)] ascending, behind the abort at -1"""
    padded = np.concatenate([np.zeros(7, np.uint8), b])
    if len(b) == 0:
        return [(-1, EVENT_ABORT)]
    win = np.lib.stride_tricks.sliding_window_view(padded, 8)
    flags = np.flatnonzero((win == FLAG).all(axis=1))
    aborts = np.flatnonzero((win == ABORT).all(axis=1))
    if fault == "abort":
        aborts = aborts[:0]
    ev = sorted([(int(i), EVENT_FLAG) for i in flags] + [(int(i), EVENT_ABORT) for i in aborts])
    if fault == "shared":
        ev = [e for k, e in enumerate(ev) if not (k and e[1] == EVENT_FLAG and ev[k - 1][1] == EVENT_FLAG and e[0] - ev[k - 1][0] == 7)]
    return [(-1, EVENT_ABORT)] + ev


def unstuff(span, fault=None):
    s = np.concatenate([np.zeros(5, np.uint8), span])
    ones = s[0:len(span)] & s[1:len(span) + 1] & s[2:len(span) + 2] & s[3:len(span) + 3] & s[4:len(span) + 4]
    if fault == "boundary":  # every 64-bit word of the span on its own
        idx = np.arange(len(span)) % 64
        ones = ones & (idx >= 5)
    return span[~((span == 0) & (ones == 1))]


def frames_of(b, q, fault=None):
    """[(e2, bytes, position, good)] of the whole stream, emitted ones only, ascending"""
    out = []
    ev = find_events(b, fault)
    for (e1, k1), (e2, k2) in zip(ev, ev[1:]):
        if k1 != EVENT_FLAG or k2 != EVENT_FLAG or e2 - e1 <= 8:
            continue
        bits = unstuff(b[e1 + 1:e2 - 7], fault)
        u = len(bits)
        if u % 8 or not q.min_bytes <= u // 8 <= q.max_bytes:
            continue
        good = 1
        if q.fcs:
            good = int(fcs_register(bits, q.fcs) == (GOOD[q.fcs] ^ (1 if fault == "residue" else 0)))
        if not good and not q.keep_bad:
            continue
        out.append((e2, np.packbits(bits, bitorder="big" if q.msb_first else "little").tobytes(), e1 + 1, good))
    return out, ev[-1]


def brute(q, pushes, cap, fault=None):
    """One row.  pushes: the row's symbols per push (each the symbols that push CONSUMES) -> ([per push ([bytes],
    positions, info, count)], state (position, event, kind, history bytes, last)) by the definition, over the whole
    stream at once; the lists hold min(count, cap) entries."""
    f = np.concatenate([floats_of(p) for p in pushes]) if pushes else np.zeros(0, np.uint32)
    b, d = decided_bits(f, q.diff)
    total = len(b)
    ends = np.cumsum([len(floats_of(p)) for p in pushes])
    found, last_ev = frames_of(b, q, fault)
    out = [[] for _ in pushes]
    for e2, data, pos, good in found:
        out[int(np.searchsorted(ends, e2, side="right"))].append((data, pos, len(data) | (good << 31)))
    res = []
    for fr in out:
        keep = fr[:cap]
        res.append(([x[0] for x in keep], np.array([x[1] for x in keep], np.uint64), np.array([x[2] for x in keep], np.uint32), len(fr)))
    hist = np.zeros(q.K, np.uint8)
    take = min(q.K, total)
    if take:
        hist[q.K - take:] = b[total - take:]
    return res, (total, last_ev[0] + 1, last_ev[1], np.packbits(hist), int(d[-1]) if total else 0)


# ---- the decoder of the books -----------------------------------------------------------------------

def crc_bytes(data, fcs):
    c = (1 << fcs) - 1
    for byte in data:
        c ^= byte
        for _ in range(8):
            c = (c >> 1) ^ (POLY[fcs] if c & 1 else 0)
    return c ^ ((1 << fcs) - 1)


def textbook(b, q):
    """the stream's bits -> [(bytes, position, good)], least significant bit first only"""
    assert not q.msb_first
    out, buf, ones, open_, start = [], [], 0, False, 0
    for i, bit in enumerate(np.asarray(b, np.uint8).tolist()):
        if bit:
            ones += 1
            if ones == 7:
                open_ = False  # abort
            elif ones < 6 and open_:
                buf.append(1)
            continue
        run, ones = ones, 0
        if run == 5:
            continue  # a stuffed 0
        if run == 6:  # a flag: the 0 and the five 1s in front of its sixth went into the frame
            if open_:
                body = buf[:max(0, len(buf) - 6)]
                if len(body) % 8 == 0 and q.min_bytes <= len(body) // 8 <= q.max_bytes:
                    data = np.packbits(np.array(body, np.uint8), bitorder="little").tobytes()
                    n = q.fcs // 8
                    good = 1 if not q.fcs else int(crc_bytes(data[:len(data) - n], q.fcs) == int.from_bytes(data[len(data) - n:], "little"))
                    if good or q.keep_bad:
                        out.append((data, start, good))
            open_, buf, start = True, [], i + 1
            continue
        if run >= 7:
            continue  # behind an abort: nothing is open
        if open_:
            buf.append(0)
    return out


# ---- the streams ------------------------------------------------------------------------------------

def random_bits(n, seed):
    return (splitmix64(seed, n) >> np.uint64(63)).astype(np.uint8)


def random_bytes(n, seed):
    return (splitmix64(seed ^ 0xB17E5, n) >> np.uint64(56)).astype(np.uint8).tobytes()


def soft(d, seed, cplx=False):
    """soft symbols that decide the raw decisions d: +- magnitudes in [0.25, 1.25); a complex row's Im is noise"""
    d = np.asarray(d, np.uint8)
    z = splitmix64(seed ^ 0x5EED, 2 * len(d) + 2)
    mag = (z[:len(d)] >> np.uint64(40)).astype(np.float64) / float(1 << 24) + 0.25
    v = ((d.astype(np.float64) * 2.0 - 1.0) * mag).astype(np.float32)
    if not cplx:
        return v
    im = ((z[len(d):2 * len(d)] >> np.uint64(40)).astype(np.float64) / float(1 << 23) - 1.0).astype(np.float32)
    return (v + 1j * im).astype(np.complex64)


def line(bits, diff):
    """the raw decisions d whose differential decoding (d[-1] = 0) gives `bits`, one step at a time"""
    if diff == 0:
        return np.asarray(bits, np.uint8).copy()
    d, prev = np.empty(len(bits), np.uint8), 0
    for i, b in enumerate(np.asarray(bits, np.uint8).tolist()):
        prev = d[i] = (b ^ prev) if diff == 1 else (b ^ prev ^ 1)
    return d


def stuffed(bits):
    out, ones = [], 0
    for b in np.asarray(bits, np.uint8).tolist():
        out.append(b)
        ones = ones + 1 if b else 0
        if ones == 5:
            out.append(0)
            ones = 0
    return np.array(out, np.uint8)


def frame_bits(payload, fcs, msb_first=False):
    """payload bytes -> the frame's bits with the FCS behind them, unstuffed (the encoder, restated)"""
    bits = np.unpackbits(np.frombuffer(bytes(payload), np.uint8), bitorder="big" if msb_first else "little")
    if fcs:
        c = fcs_register(bits, fcs) ^ ((1 << fcs) - 1)
        bits = np.concatenate([bits, np.array([(c >> k) & 1 for k in range(fcs)], np.uint8)])
    return bits


# ---- the program ------------------------------------------------------------------------------------

_EXE = {}


def build_exact(build_dir):
    """g++ -O2 of tests/host/hdlc_ref.cpp -> the program's path (built once per directory)"""
    if build_dir not in _EXE:
        os.makedirs(build_dir, exist_ok=True)
        exe = os.path.join(build_dir, "hdlc_ref")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"),
                               os.path.join(ROOT, "tests", "host", "hdlc_ref.cpp"), "-o", exe])
        _EXE[build_dir] = exe
    return _EXE[build_dir]


def _head(q, has_state, pushes):
    return struct.pack("<9i", int(q.cplx), q.diff, q.fcs, q.min_bytes, q.max_bytes, q.msb_first, q.keep_bad, int(has_state), pushes)


def exact(build_dir, cases):
    """cases: [(config, pushes, cap)] or [(config, pushes, cap, state)] -> [([per push (frames (R, cap, max_bytes),
    positions (R, cap), info (R, cap), counts (R,))], state)] by the program.  pushes: a list of x or (x, counts); x is
    float32 or complex64 (R, n) (or (n,) for one row); counts uint32 (R,).  state: (positions, events, kinds, history
    (R, HB), last)."""
    exe = build_exact(build_dir)
    src, dst = os.path.join(build_dir, "hdlc_cases.bin"), os.path.join(build_dir, "hdlc_out.bin")
    shapes = []
    with open(src, "wb") as f:
        for case in cases:
            q, pushes, cap = case[0], case[1], int(case[2])
            state = case[3] if len(case) > 3 else None
            first = pushes[0][0] if isinstance(pushes[0], tuple) else pushes[0]
            R = 1 if np.asarray(first).ndim == 1 else np.asarray(first).shape[0]
            f.write(_head(q, state is not None, len(pushes)))
            f.write(struct.pack("<2q", R, cap))
            if state is not None:
                p, e, k, y, d = state
                f.write(np.ascontiguousarray(p, np.uint64).tobytes() + np.ascontiguousarray(e, np.uint64).tobytes() +
                        np.ascontiguousarray(k, np.uint8).tobytes() + np.ascontiguousarray(y, np.uint8).tobytes() + np.ascontiguousarray(d, np.uint8).tobytes())
            for pu in pushes:
                x, cnt = pu if isinstance(pu, tuple) else (pu, None)
                x = np.asarray(x)
                assert x.dtype == (np.complex64 if q.cplx else np.float32), x.dtype
                x = x.reshape(R, -1)
                f.write(struct.pack("<qi", x.shape[1], int(cnt is not None)))
                if cnt is not None:
                    f.write(np.ascontiguousarray(cnt, np.uint32).tobytes())
                f.write(np.ascontiguousarray(x).tobytes())
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
        state = (take(np.uint64, (R,)), take(np.uint64, (R,)), take(np.uint8, (R,)), take(np.uint8, (R, q.HB)), take(np.uint8, (R,)))
        out.append((per, state))
    assert off == len(raw)
    os.remove(src), os.remove(dst)
    return out


def accepted_by_program(build_dir, configs):
    """[config] -> [accepted] by csrc/hz_hdlc_plan.h"""
    exe = build_exact(build_dir)
    src, dst = os.path.join(build_dir, "hdlc_sets.bin"), os.path.join(build_dir, "hdlc_checked.bin")
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
        n = x.shape[1] if c is None else min(int(np.asarray(c).reshape(-1)[row]), x.shape[1])
        out.append(x[row, :n])
    return out


def stored(per, row):
    """[(bytes, position, good)] of everything the program (or the bank) stored for `row`, over the pushes"""
    out = []
    for fr, ps, inf, cnt in per:
        for k in range(min(int(cnt[row]), fr.shape[1])):
            i = int(inf[row, k])
            out.append((bytes(fr[row, k, :i & 0x7FFFFFFF]), int(ps[row, k]), i >> 31))
    return out


def agree(q, pushes, cap, per, state, R, fault=None):
    """the program's results against brute(), row by row; -> the first difference, or None"""
    for r in range(R):
        res, st = brute(q, consumed(pushes, r, R), cap, fault)
        for k, (datas, pos, inf, count) in enumerate(res):
            fr, ps, info, cnt = per[k]
            if int(cnt[r]) != count:
                return f"row {r} push {k}: count {int(cnt[r])} != {count}"
            for s, data in enumerate(datas):
                if bytes(fr[r, s, :len(data)]) != data or fr[r, s, len(data):].any() or int(ps[r, s]) != int(pos[s]) or int(info[r, s]) != int(inf[s]):
                    return f"row {r} push {k} slot {s}"
            if fr[r, len(datas):].any() or ps[r, len(datas):].any() or info[r, len(datas):].any():
                return f"row {r} push {k}: slots behind the count"
        got = (int(state[0][r]), int(state[1][r]), int(state[2][r]), state[3][r], int(state[4][r]))
        if got[:3] != st[:3] or not np.array_equal(got[3], st[3]) or got[4] != st[4]:
            return f"row {r}: state {got[:3]} {got[4]} != {st[:3]} {st[4]}"
    return None

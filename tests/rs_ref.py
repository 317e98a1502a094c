"""The Reed-Solomon decoder bank (include/hzsdr_rs.h) restated in numpy, written independently of csrc/hz_rs_math.h: no
Berlekamp-Massey, no Chien search, no Forney.  decode_word is Peterson-Gorenstein-Zierler: the number of errors is the
rank of the t x t matrix of syndromes, the locator comes from one linear solve, its roots from trying every one of the
n positions, the error values from a second linear solve, and the answer stands only if it reproduces ALL nroots
syndromes -- which is the definition: a codeword within t positions of the received word.  nearest_word is the
definition itself for k = 1: all 256 codewords tried.  exact() runs the host program tests/host/rs_ref.cpp."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CCSDS_223 = (0x187, 112, 11, 32, 255)
CCSDS_239 = (0x187, 120, 11, 16, 255)
DVB = (0x11D, 0, 1, 16, 204)
K1_CODES = ((0x187, 112, 11, 4, 5), (0x187, 112, 11, 3, 5), (0x11D, 0, 1, 5, 6))
FAILED = -1


def splitmix64(seed, n):
    """n uint64 of the splitmix64 sequence from `seed`"""
    with np.errstate(over="ignore"):
        z = (np.uint64(seed & (2 ** 64 - 1)) + np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def random_bytes(n, seed):
    return (splitmix64(seed, n) >> np.uint64(56)).astype(np.uint8)


class Field:
    _made = {}

    def __new__(cls, gfpoly):
        if gfpoly not in cls._made:
            f = super().__new__(cls)
            f.exp, f.log, x = np.zeros(510, np.int64), np.zeros(256, np.int64), 1
            for i in range(255):
                f.exp[i], f.log[x] = x, i
                x = (x << 1) ^ (gfpoly if x & 0x80 else 0)
            assert x == 1 and len(set(f.exp[:255].tolist())) == 255, "not primitive"
            f.exp[255:] = f.exp[:255]
            cls._made[gfpoly] = f
        return cls._made[gfpoly]

    def mul(self, a, b):
        a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
        return np.where((a != 0) & (b != 0), self.exp[self.log[a] + self.log[b]], 0)

    def inv(self, a):
        assert a != 0
        return int(self.exp[255 - self.log[a]])

    def pow_alpha(self, e):
        return int(self.exp[e % 255])

    def solve(self, M, y):
        """x with M x = y over the field, M square -> (x, True), or (None, False) when M is singular"""
        M, y = np.array(M, np.int64), np.array(y, np.int64)
        m = len(y)
        A = np.concatenate([M, y[:, None]], axis=1)
        for c in range(m):
            piv = next((r for r in range(c, m) if A[r, c]), None)
            if piv is None:
                return None, False
            A[[c, piv]] = A[[piv, c]]
            A[c] = self.mul(A[c], self.inv(int(A[c, c])))
            rows = np.nonzero(A[:, c])[0]
            rows = rows[rows != c]
            A[rows] ^= self.mul(A[rows, c][:, None], A[c][None, :])
        return A[:, m], True

    def rank(self, M):
        A = np.array(M, np.int64)
        rank = 0
        for c in range(A.shape[1]):
            piv = next((r for r in range(rank, A.shape[0]) if A[r, c]), None)
            if piv is None:
                continue
            A[[rank, piv]] = A[[piv, rank]]
            A[rank] = self.mul(A[rank], self.inv(int(A[rank, c])))
            rows = np.nonzero(A[:, c])[0]
            rows = rows[rows != rank]
            A[rows] ^= self.mul(A[rows, c][:, None], A[rank][None, :])
            rank += 1
        return rank


def syndromes(code, words):
    """words (..., n) -> (..., nroots): S_j = c(alpha^(prim (fcr + j))), symbol p the coefficient of x^(n-1-p)"""
    gfpoly, fcr, prim, nroots, n = code
    F = Field(gfpoly)
    words = np.asarray(words, np.int64)
    pw = np.array([[F.pow_alpha(prim * (fcr + j) * (n - 1 - p)) for p in range(n)] for j in range(nroots)], np.int64)
    return np.bitwise_xor.reduce(F.mul(words[..., None, :], pw), axis=-1)


def encode(code, data):
    """data (k,) -> the codeword (n,): the remainder of data(x) x^nroots by the generator, by long division"""
    gfpoly, fcr, prim, nroots, n = code
    F = Field(gfpoly)
    g = [1]
    for j in range(nroots):
        root = F.pow_alpha(prim * (fcr + j))
        g = [a ^ b for a, b in zip(g + [0], [0] + [int(F.mul(x, root)) for x in g])]
    rem = [int(v) for v in data] + [0] * nroots
    for p in range(n - nroots):
        lead = rem[p]
        if lead:
            for i in range(1, nroots + 1):
                rem[p + i] ^= int(F.mul(lead, g[i]))
    return np.array([int(v) for v in data] + rem[n - nroots:], np.uint8)


def decode_word(code, word):
    """word (n,) -> (corrected word, e) or (word, FAILED): bounded distance, by linear algebra"""
    gfpoly, fcr, prim, nroots, n = code
    F, t = Field(gfpoly), nroots // 2
    word = np.asarray(word, np.uint8)
    S = syndromes(code, word)
    if not S.any():
        return word.copy(), 0
    nu = F.rank([[S[i + j] for j in range(t)] for i in range(t)])
    if nu == 0:
        return word.copy(), FAILED
    # Lambda(z) = 1 + l_1 z + ... + l_nu z^nu with S_{r} + l_1 S_{r-1} + ... + l_nu S_{r-nu} = 0, r = nu ... 2 nu - 1
    lam, ok = F.solve([[S[r - i] for i in range(1, nu + 1)] for r in range(nu, 2 * nu)], [S[r] for r in range(nu, 2 * nu)])
    if not ok:
        return word.copy(), FAILED
    where = []
    for p in range(n):
        zl = -prim * (n - 1 - p)  # z = 1 / X_p
        val = 1
        for i in range(1, nu + 1):
            val ^= int(F.mul(lam[i - 1], F.pow_alpha(zl * i)))
        if val == 0:
            where.append(p)
    if len(where) != nu:
        return word.copy(), FAILED
    # S_j = sum_i e_i X_i^(fcr + j): nu equations for the values, the rest to hold the answer to
    X = [[F.pow_alpha(prim * (n - 1 - p) * (fcr + j)) for p in where] for j in range(nroots)]
    e, ok = F.solve(X[:nu], S[:nu])
    if not ok or not e.all():
        return word.copy(), FAILED
    if not np.array_equal(np.bitwise_xor.reduce(F.mul(np.array(X, np.int64), e[None, :]), axis=1), S):
        return word.copy(), FAILED
    fixed = word.copy()
    fixed[where] ^= e.astype(np.uint8)
    return fixed, nu


_WORDS = {}


def nearest_word(code, word):
    """the definition for k = 1 or 2: every codeword tried -> (the codeword within t positions, its distance) or
    (word, FAILED).  (The code is linear: all 256^k codewords are the sums of multiples of the k unit words' codewords.)"""
    k = code[4] - code[3]
    assert 1 <= k <= 2
    if code not in _WORDS:
        F, all_ = Field(code[0]), np.zeros((1, code[4]), np.int64)
        for i in range(k):
            unit = encode(code, np.eye(k, dtype=np.uint8)[i]).astype(np.int64)
            all_ = (all_[:, None, :] ^ F.mul(np.arange(256)[:, None], unit[None, :])[None, :, :]).reshape(-1, code[4])
        _WORDS[code] = all_.astype(np.uint8)
        assert len(np.unique(_WORDS[code], axis=0)) == 256 ** k
    word = np.asarray(word, np.uint8)
    dist = (_WORDS[code] != word[None, :]).sum(axis=1)
    best = int(dist.argmin())
    if dist[best] <= code[3] // 2:
        assert (dist == dist[best]).sum() == 1
        return _WORDS[code][best].copy(), int(dist[best])
    return word.copy(), FAILED


class Config:
    def __init__(self, code, I=1, in_map=None, out_map=None, scramble=None):
        self.code, self.I = tuple(int(v) for v in code), int(I)
        self.in_map = None if in_map is None else np.asarray(in_map, np.uint8)
        self.out_map = None if out_map is None else np.asarray(out_map, np.uint8)
        self.scramble = None if scramble is None else np.asarray(scramble, np.uint8).reshape(-1)
        self.nroots, self.n = self.code[3], self.code[4]
        self.k, self.t = self.n - self.nroots, self.nroots // 2
        self.F, self.IK = self.I * self.n, self.I * self.k

    def create_args(self):
        return (self.code,), dict(interleave=self.I, in_map=self.in_map, out_map=self.out_map, scramble=self.scramble)

    def prepare(self, frame):
        """a frame as sent (F,) -> the received symbols"""
        b = np.asarray(frame, np.uint8).copy()
        if self.scramble is not None:
            b ^= np.resize(self.scramble, self.F)
        return b if self.in_map is None else self.in_map[b]

    def unprepare(self, symbols):
        """symbols (F,) -> the frame a sender whose maps are the inverse of in_map would transmit"""
        b = np.asarray(symbols, np.uint8)
        if self.in_map is not None:
            back = np.zeros(256, np.uint8)
            back[self.in_map] = np.arange(256, dtype=np.uint8)
            b = back[b]
        if self.scramble is not None:
            b = b ^ np.resize(self.scramble, self.F)
        return b


def decode_frame(q, frame, word_decoder=decode_word):
    """one frame (F,) -> (data (I k,), info)"""
    v = q.prepare(frame)
    E = nfail = 0
    for i in range(q.I):
        fixed, e = word_decoder(q.code, v[i::q.I])
        if e == FAILED:
            nfail += 1
        else:
            E += e
            v[i::q.I] = fixed
    d = v[:q.IK]
    return (d if q.out_map is None else q.out_map[d]), E | nfail << 16 | (0 if nfail else 1 << 31)


def decode_block(q, frames, counts=None):
    """frames (R, cap, F) -> (data (R, cap, I k), info (R, cap)); slots from a row's count up are zero"""
    R, cap, _ = frames.shape
    data, info = np.zeros((R, cap, q.IK), np.uint8), np.zeros((R, cap), np.uint32)
    for r in range(R):
        for f in range(cap if counts is None else min(int(counts[r]), cap)):
            data[r, f], info[r, f] = decode_frame(q, frames[r, f])
    return data, info


def clean_frame(q, seed):
    """(frame as sent (F,), data symbols (I, k)): random data, encoded, interleaved, unprepared"""
    data = random_bytes(q.I * q.k, seed).reshape(q.I, q.k)
    sym = np.zeros(q.F, np.uint8)
    for i in range(q.I):
        sym[i::q.I] = encode(q.code, data[i])
    return q.unprepare(sym), data


def hurt(q, frame, i, positions, values):
    """errors of `values` added to the symbols `positions` of codeword i (in the symbol domain, before the maps)"""
    sym = q.prepare(frame)
    for p, v in zip(positions, values):
        sym[i + int(p) * q.I] ^= np.uint8(v)
    return q.unprepare(sym)


# ---- the program ---------------------------------------------------------------------------------------

_EXE = {}


def build_exact(build_dir):
    """g++ -O2 of tests/host/rs_ref.cpp -> the program's path (built once per directory)"""
    if build_dir not in _EXE:
        os.makedirs(build_dir, exist_ok=True)
        exe = os.path.join(build_dir, "rs_ref")
        mine = f"{exe}.{os.getpid()}"  # (test workers may build side by side: each links under a name of its own, then moves it into place)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"), os.path.join(ROOT, "tests", "host", "rs_ref.cpp"),
                               "-o", mine])
        os.replace(mine, exe)
        _EXE[build_dir] = exe
    return _EXE[build_dir]


def _head(q, maps=True):
    slen = 0 if q.scramble is None else len(q.scramble)
    h = struct.pack("<7I", *q.code, q.I, slen)
    if not maps:
        return h
    h += struct.pack("<2I", int(q.in_map is not None), int(q.out_map is not None))
    for m in (q.in_map, q.out_map, q.scramble):
        if m is not None:
            h += np.ascontiguousarray(m, np.uint8).tobytes()
    return h


def exact(build_dir, cases):
    """cases: [(config, frames (R, cap, F), counts uint32 (R,) or None)] -> [(data (R, cap, I k), info (R, cap))] by the
    program; slots from a row's count up are zero"""
    exe = build_exact(build_dir)
    src, dst = os.path.join(build_dir, f"rs_cases_{os.getpid()}.bin"), os.path.join(build_dir, f"rs_out_{os.getpid()}.bin")
    shapes = []
    with open(src, "wb") as f:
        for q, frames, counts in cases:
            frames = np.ascontiguousarray(frames)
            R, cap, width = frames.shape
            assert frames.dtype == np.uint8 and width == q.F
            f.write(_head(q) + struct.pack("<qqi", R, cap, int(counts is not None)))
            if counts is not None:
                f.write(np.ascontiguousarray(counts, np.uint32).tobytes())
            f.write(frames.tobytes())
            shapes.append((q, R, cap))
    subprocess.check_call([exe, "run", src, dst])
    out, raw, off = [], open(dst, "rb").read(), 0
    for q, R, cap in shapes:
        data = np.frombuffer(raw, np.uint8, R * cap * q.IK, off).copy().reshape(R, cap, q.IK)
        off += data.nbytes
        info = np.frombuffer(raw, np.uint32, R * cap, off).copy().reshape(R, cap)
        off += info.nbytes
        out.append((data, info))
    assert off == len(raw)
    os.remove(src), os.remove(dst)
    return out


def check(build_dir, sets):
    """[(gfpoly, fcr, prim, nroots, n, interleave, scramble_len)] -> [(accepted, k, t)] by csrc/hz_rs_plan.h"""
    exe = build_exact(build_dir)
    src, dst = os.path.join(build_dir, f"rs_sets_{os.getpid()}.bin"), os.path.join(build_dir, f"rs_checked_{os.getpid()}.bin")
    with open(src, "wb") as f:
        for s in sets:
            f.write(struct.pack("<7I", *s))
    subprocess.check_call([exe, "check", src, dst])
    got = np.fromfile(dst, np.uint32).reshape(-1, 3)
    os.remove(src), os.remove(dst)
    assert len(got) == len(sets)
    return [(bool(a), int(k), int(t)) for a, k, t in got]

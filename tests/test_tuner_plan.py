"""The tuner bank's host arithmetic (csrc/hz_tuner_plan.h) built with AddressSanitizer + UndefinedBehaviorSanitizer and
checked against Python's big integers (tests/host/tuner_plan.cpp, a stand-alone program): counts, the relative index,
the held samples and the flush count of random pushes from stream positions up to 2^62 -- a 2^32 crossing among them,
which no GPU test can push --; the running phase words of random (w, D, push lengths); the window base of random tiles
and chunks; the tile geometry and the chunking of every (D, Q), those of the GPU tests by name.  The same program
checks, with no expectation needed, the LDS request against the budget, both layouts as bijections, the kernel's stepped
slot against the layout and the banks of every B-operand read."""
import os
import random
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPAN_MAX = 1 << 62  # dp::kSpanMax
BUDGET = 66 * 1024
M32 = (1 << 32) - 1
# (D, Q) -> (T, chunks) the planner must choose, from the budget by hand: a plane is D * J floats with J = ceil(((T - 1) D +
# cq) / D) (made odd where that fits) padded to 16 modulo 32, and two planes stay within 16896 floats
GRID = {(256, 1024): (32, 4), (255, 1023): (32, 3), (1, 1): (128, 1), (64, 513): (64, 1), (1, 1024): (128, 1), (16, 129): (128, 1),
        (5, 64): (128, 1), (3, 7): (128, 1), (2, 33): (128, 1), (1, 16): (128, 1), (1, 2): (128, 1), (128, 1024): (32, 1), (200, 1024): (32, 1)}


def plane(d, j):
    p = d * j
    return p + (48 - p % 32) % 32


def columns(d, window):
    j = -(-window // d)
    for c in (j | 1, j):
        if 2 * plane(d, c) <= BUDGET // 4:
            return c
    return 0


def geometry(d, q):
    """the planner's choice, restated: -> (T, cq, chunks, J)"""
    qp = q + q % 2
    for t in (128, 64, 32):
        j = columns(d, (t - 1) * d + qp)
        if j:
            return t, qp, 1, j
    cq = qp
    while not columns(d, 31 * d + cq):
        cq -= 2
    return 32, cq, -(-qp // cq), columns(d, 31 * d + cq)


def cases(seed, streams):
    rng = random.Random(seed)
    lines = []
    for c in range(streams):
        down = rng.choice([1, 2, 5, 255, 256, rng.randint(1, 256)])
        q = rng.choice([1, 2, 16, 1023, 1024, rng.randint(1, 1024)])
        n = [0, (1 << 32) - rng.randint(0, 5), rng.randrange(1 << 40), rng.randrange(1 << 62)][c % 4]
        m = -(-n // down)
        rel = m * down - n
        assert 0 <= rel < down
        lines.append(f"C {down} {q} {n} {m} {rel}")
        w = rng.choice([0, 1, 1 << 31, M32, 1 << 21, 1 << 10, rng.randrange(1 << 32)])
        word = (w * down * m) & M32
        lines.append(f"W {w} {down} {(w * down) & M32} {word}")
        for _ in range(12):
            k = rng.choice([0, 1, 1, rng.randint(0, 9), rng.randint(0, 5000), rng.randrange(1 << 33), rng.randrange(1 << 52), rng.randrange(1 << 63)])
            count = max(0, -(-(k - rel) // down))
            ok = count * down < SPAN_MAX and n + k < (1 << 64) and m + count < (1 << 64)
            if ok and count:
                t, cq, chunks, _ = geometry(down, q)
                last = (count - 1) // t
                for tile in {0, last, rng.randint(0, last)}:
                    for chunk in {0, chunks - 1}:
                        # window sample 0: the tile's first output at the chunk's last q
                        lo = rel + tile * t * down - (chunk * cq + cq - 1)
                        lines.append(f"B {t} {cq} {tile} {chunk} {lo + (1 << 62)}")
            if ok:
                n, m = n + k, m + count
                rel = m * down - n
                assert 0 <= rel < down and m == -(-n // down)
                flush = max(0, -(-(n - 1 + q) // down) - m) if n else 0
                lines.append(f"P {k} 1 {count} {n} {m} {rel} {min(n, q - 1)} {flush}")
                word = (w * down * m) & M32  # (the exact product, reduced: what the running word must equal)
                lines.append(f"A {count} {word}")
            else:
                lines.append(f"P {k} 0 0 0 0 0 0 0")
    return "\n".join(lines) + "\n"


def test_tuner_plan_under_asan_ubsan():
    with tempfile.TemporaryDirectory() as d:
        exe, data = os.path.join(d, "tuner_plan"), os.path.join(d, "cases.txt")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"), os.path.join(ROOT, "tests", "host", "tuner_plan.cpp"),
                               "-o", exe])
        text = cases(20261018, 400)
        assert text.count("\nP") > 4000 and text.count("\nB") > 4000 and text.count("\nA") > 3000 and "\nP 0 1" in text
        assert any(line.startswith("P") and line.split()[2] == "0" for line in text.splitlines()), "no push too long for the counts"
        text += "".join(f"G 7 {down} {q}\n" for down, q in GRID)
        with open(data, "w") as f:
            f.write(text)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe, data], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        assert out.returncode == 0, out.stdout[-4000:]
        assert "tuner_plan ok" in out.stdout, out.stdout[-2000:]
    lines = out.stdout.splitlines()
    (largest,) = [tuple(int(v) for v in s.split(":")[1].split()) for s in lines if s.startswith("largest lds:")]
    print("largest LDS request (D, Q, bytes):", largest)
    assert largest[2] <= BUDGET
    (chunked,) = [int(s.split(":")[1]) for s in lines if s.startswith("chunked:")]
    print("chunked (D, Q) pairs:", chunked)
    assert chunked > 0
    forms = {(down, q): (t, rows, cq, chunks, window, j, pl, nbytes, row_tiles) for k, down, q, t, rows, cq, chunks, window, j, pl, nbytes, row_tiles
             in ([int(v) for v in s.split(":")[1].split()] for s in lines if s.startswith("form:"))}
    for shape, (tile, nchunks) in GRID.items():
        down, q = shape
        t, rows, cq, chunks, window, j, pl, nbytes, row_tiles = forms[shape]
        assert (t, cq, chunks, j) == geometry(down, q), shape
        assert (t, chunks) == (tile, nchunks), f"{shape}: T {t}, {chunks} chunk(s)"
        assert rows * t == 128 * 32 and window == (t - 1) * down + cq and pl == plane(down, j) and nbytes == 8 * pl <= BUDGET
        assert chunks * cq >= q and (chunks - 1) * cq < q + q % 2 and row_tiles == 2
    assert {f[0] for f in forms.values()} == {128, 64, 32}

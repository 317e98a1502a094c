"""The demodulator's host arithmetic (csrc/hz_demod_plan.h) built with AddressSanitizer + UndefinedBehaviorSanitizer and
checked against Python's big integers (tests/host/demod_plan.cpp): counts, the relative index, the held samples and the
flush count of random pushes from stream positions up to 2^62 -- a 2^32 crossing among them, which no GPU test can
push -- and the window of random tiles.  The same program checks the LDS request of every (Q, D) against the budget,
the stepped slot against the layout, and counts the lanes per bank of each 32-lane half of every read, for every
D <= 64: 1 for odd D, at most 2 for even D (DESIGN.md section 4 has the table it prints)."""
import os
import random
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPAN_MAX = 1 << 62  # dp::kSpanMax
TILES = (128, 256, 512, 1024)
BUDGET = 66 * 1024
# (Q, D) of the GPU tests' list with the planner's tiles (tests/test_gpu_demod.py)
GPU_SHAPES = {(1, 1): 1024, (7, 3): 1024, (33, 1): 1024, (64, 5): 1024, (256, 8): 1024, (129, 64): 256, (1024, 64): 128, (1024, 1): 1024,
              (600, 20): 512}


def cases(seed, streams):
    rng = random.Random(seed)
    lines = []
    for c in range(streams):
        down = rng.choice([1, 2, 5, 63, 64, rng.randint(1, 64)])
        q = rng.choice([1, 2, 16, 1024, rng.randint(1, 1024)])
        # a position: N samples consumed, every output with m D < N written
        n = [0, (1 << 32) - rng.randint(0, 5), rng.randrange(1 << 40), rng.randrange(1 << 62)][c % 4]
        m = -(-n // down)
        rel = m * down - n
        assert 0 <= rel < down
        lines.append(f"C {down} {q} {n} {m} {rel}")
        for _ in range(12):
            k = rng.choice([0, 1, 1, rng.randint(0, 9), rng.randint(0, 5000), rng.randrange(1 << 33), rng.randrange(1 << 52), rng.randrange(1 << 63)])
            count = max(0, -(-(k - rel) // down))
            ok = count * down < SPAN_MAX and n + k < (1 << 64) and m + count < (1 << 64)
            if ok and count:
                for tile_outputs in TILES:
                    last = (count - 1) // tile_outputs
                    for tile in {0, last, rng.randint(0, last)}:
                        i0 = rel + tile * tile_outputs * down
                        lines.append(f"T {tile_outputs} {tile} {i0} {i0} {i0 + (tile_outputs - 1) * down + (q - 1)}")
            if ok:
                n, m = n + k, m + count
                rel = m * down - n
                assert 0 <= rel < down and m == -(-n // down)
                flush = max(0, -(-(n - 1 + q) // down) - m) if n else 0
                lines.append(f"P {k} 1 {count} {n} {m} {rel} {min(n, q)} {flush}")
            else:
                lines.append(f"P {k} 0 0 0 0 0 0 0")
    return "\n".join(lines) + "\n"


def test_demod_plan_under_asan_ubsan():
    with tempfile.TemporaryDirectory() as d:
        exe, data = os.path.join(d, "demod_plan"), os.path.join(d, "cases.txt")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"), os.path.join(ROOT, "tests", "host", "demod_plan.cpp"),
                               "-o", exe])
        text = cases(20261018, 400)
        assert text.count("\nP") > 4000 and text.count("\nT") > 4000 and "\nP 0 1" in text
        assert any(line.startswith("P") and line.split()[2] == "0" for line in text.splitlines()), "no push too long for the counts"
        text += "".join(f"G {down} {q}\n" for q, down in GPU_SHAPES)
        with open(data, "w") as f:
            f.write(text)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe, data], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-4000:]
        assert "demod_plan ok" in out.stdout, out.stdout[-2000:]
    lines = out.stdout.splitlines()
    # the lanes per bank: every D reported, 1 for odd D and at most 2 for even D
    banks = dict(tuple(int(v) for v in s.split(":")[1].split()) for s in lines if s.startswith("banks:"))
    print("lanes per bank, by D:", banks)
    assert sorted(banks) == list(range(1, 65))
    assert all(banks[d] == 1 for d in range(1, 65, 2)) and all(banks[d] <= 2 for d in range(2, 65, 2))
    # the largest LDS request over every (Q, D), inside the budget
    (largest,) = [tuple(int(v) for v in s.split(":")[1].split()) for s in lines if s.startswith("largest lds:")]
    print("largest LDS request (D, Q, bytes):", largest)
    assert largest[2] <= BUDGET
    # the GPU tests' shapes take the tiles their list names, every tile size among them
    forms = {(q, down): (t, half, window, j, nbytes) for down, q, t, half, window, j, nbytes in
             ([int(v) for v in s.split(":")[1].split()] for s in lines if s.startswith("form:"))}
    for shape, tile in GPU_SHAPES.items():
        t, half, window, j, nbytes = forms[shape]
        assert t == tile and half == (tile == 128) and window == (tile - 1) * shape[1] + shape[0] and nbytes == 4 * shape[1] * j <= BUDGET
    assert {f[0] for f in forms.values()} == set(TILES)

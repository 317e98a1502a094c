"""The resampler's host arithmetic (csrc/hz_resampler_plan.h) built with AddressSanitizer + UndefinedBehaviorSanitizer
and checked against Python's big integers (tests/host/resampler_plan.cpp): counts, the running phase and relative
index, the held samples and the flush count of random pushes from stream positions up to 2^62 -- a 2^32 crossing
among them, which no GPU test can push -- the window of random tiles, the lanes' (i, phi), and the reciprocal of U
over the whole range the kernel uses.  The same program searches every shape for the largest LDS request and reports
the form of each shape of the GPU tests' accuracy list: the shape the list names as the largest is that maximum, and
the list's tiles are the planner's."""
import os
import random
import subprocess
import tempfile

import readout as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPAN_MAX = 1 << 62  # rs::kSpanMax
TILES = (256, 1024)


def cases(seed, streams):
    rng = random.Random(seed)
    lines = []
    for c in range(streams):
        up, down = rng.choice([1, 2, 3, 160, 147, 1024, rng.randint(1, 1024)]), rng.choice([1, 2, 5, 147, 160, 1024, rng.randint(1, 1024)])
        q = rng.choice([1, 2, 16, 256, rng.randint(1, 256)])
        ntaps = rng.randint((q - 1) * up + 1, min(q * up, 65536)) if (q - 1) * up + 1 <= 65536 else 65536
        q = -(-ntaps // up)
        # a position: N samples consumed, every output with m D < N U written
        n = [0, (1 << 32) - rng.randint(0, 5), rng.randrange(1 << 40), rng.randrange((1 << 62) // up)][c % 4]
        m = -(-n * up // down)
        t = m * down - n * up
        assert 0 <= t < down + up
        lines.append(f"C {up} {down} {q} {ntaps} {n} {m} {t % up} {t // up}")
        for _ in range(12):
            k = rng.choice([0, 1, 1, rng.randint(0, 9), rng.randint(0, 5000), rng.randrange(1 << 33), rng.randrange(1 << 52)])
            count = max(0, -(-(k * up - t) // down))
            ok = count * down < SPAN_MAX and n + k < (1 << 64) and m + count < (1 << 64)
            if ok and count:
                for tile_outputs in TILES:
                    last = (count - 1) // tile_outputs
                    for tile in {0, last, rng.randint(0, last)}:
                        tt = t + tile * tile_outputs * down
                        hi = (tt + (tile_outputs - 1) * down) // up + (q - 1)
                        lines.append(f"T {tile_outputs} {tile} {tt // up} {tt % up} {tt // up} {hi}")
            if ok:
                n, m = n + k, m + count
                t = m * down - n * up
                assert 0 <= t < down + up and m == -(-n * up // down)
                flush = max(0, -(-((n - 1) * up + ntaps) // down) - m) if n else 0
                lines.append(f"P {k} 1 {count} {n} {m} {t % up} {t // up} {min(n, q - 1)} {flush}")
            else:
                lines.append(f"P {k} 0 0 0 0 0 0 0 0")
    return "\n".join(lines) + "\n"


def test_resampler_plan_under_asan_ubsan():
    with tempfile.TemporaryDirectory() as d:
        exe, data = os.path.join(d, "resampler_plan"), os.path.join(d, "cases.txt")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"), os.path.join(ROOT, "tests", "host", "resampler_plan.cpp"),
                               "-o", exe])
        text = cases(20261017, 400)
        assert text.count("\nP") > 4000 and text.count("\nT") > 4000
        text += "".join(f"G {u} {d} {-(-ntaps // u)}\n" for u, d, ntaps, _ in ro.RESAMPLER_SHAPES)
        with open(data, "w") as f:
            f.write(text)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe, data], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-4000:]
        assert "resampler_plan ok" in out.stdout, out.stdout[-2000:]
    lines = out.stdout.splitlines()
    # the largest LDS request among the forms with a window, and the accuracy list's shape that asks for it
    largest = [tuple(int(v) for v in s.split(":")[1].split()) for s in lines if s.startswith("largest lds:")]
    assert largest == [ro.LARGEST_LDS], largest
    u, d, q, window, nbytes = ro.LARGEST_LDS
    assert nbytes > 64 * 1024, "the largest request no longer passes the 64 KiB a launch gets without asking"
    forms = {tuple(v[:3]): v[3:] for v in ([int(t) for t in s.split(":")[1].split()] for s in lines if s.startswith("form:"))}
    mine = [s for s in ro.RESAMPLER_SHAPES if (s[0], s[1], -(-s[2] // s[0])) == (u, d, q)]
    assert len(mine) == 1 and forms[(u, d, q)][5] == nbytes, "the accuracy list lacks the shape of the largest LDS request"
    for up, down, ntaps, tile in ro.RESAMPLER_SHAPES:
        assert forms[(up, down, -(-ntaps // up))][0] == tile, (up, down, ntaps)
    # every reachable (tile, padded, table, direct) combination occurs in the list, by the planner's own report
    combos = {(t, bool(pad), "global" if tg else "uniform" if tu else "lds", bool(direct)) for t, direct, tg, tu, pad, _ in forms.values()}
    assert len(combos) == 11, sorted(combos)

"""The channel bank's host arithmetic (csrc/hz_chanbank_plan.h) built with AddressSanitizer + UndefinedBehaviorSanitizer
(tests/host/chanbank_plan.cpp, a stand-alone program): for every M the tile against the LDS budget, both operand
layouts as bijections, every frame and channel of a tile covered exactly once by the fold's and the product's dealing,
the position map; for random (M, P, D) and random pushes -- up to 2^62 samples, which no GPU test can push -- the counts
against the closed form in 128-bit integers.  The tiles of the GPU tests' shapes by name."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = 66 * 1024


def geometry(m):
    """the planner's choice, restated from the budget by hand: B is 2 Mp (T + 1) floats, A 32 Mp floats per 16-row tile
    -> (T, row_tiles, A in LDS, LDS bytes)"""
    mp = m + m % 2
    t = 64 if 2 * mp * 65 * 4 <= BUDGET else 32
    row_tiles = -(-(-(-2 * m // 16)) // 2) * 2
    b, a = 2 * mp * (t + 1) * 4, row_tiles * 32 * mp * 4
    in_lds = a + b <= BUDGET
    return t, row_tiles, int(in_lds), b + (a if in_lds else 0)


def test_chanbank_plan_under_asan_ubsan():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "chanbank_plan")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"), os.path.join(ROOT, "tests", "host", "chanbank_plan.cpp"),
                               "-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe, "20261018", "4000"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        assert out.returncode == 0, out.stdout[-4000:]
        assert "chanbank_plan ok" in out.stdout, out.stdout[-2000:]
    lines = out.stdout.splitlines()
    (largest,) = [tuple(int(v) for v in s.split(":")[1].split()) for s in lines if s.startswith("largest lds:")]
    print("largest LDS request (M, bytes):", largest)
    assert largest == (255, BUDGET)
    (tiles,) = [tuple(int(v) for v in s.split(":")[1].split()) for s in lines if s.startswith("tiles:")]
    assert tiles == (127, 127), "T = 64 up to M = 128, T = 32 above"
    (in_lds,) = [int(s.split(":")[1]) for s in lines if s.startswith("a in lds:")]
    assert in_lds == sum(geometry(m)[2] for m in range(2, 256)) > 0
    forms = {f[0]: tuple(f[1:]) for f in ([int(v) for v in s.split(":")[1].split()] for s in lines if s.startswith("form:"))}
    assert set(forms) == {2, 3, 7, 8, 12, 16, 17, 64, 100, 128, 255}
    for m, form in forms.items():
        assert form == geometry(m), m
    assert forms[128][0] == 64 and forms[255][0] == 32 and forms[16][2] == 1 and forms[64][2] == 0

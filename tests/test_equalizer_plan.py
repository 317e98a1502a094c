"""The equalizer bank's host arithmetic (csrc/hz_equalizer_plan.h) built with AddressSanitizer +
UndefinedBehaviorSanitizer as a stand-alone program (tests/host/equalizer_plan.cpp): for every N = 1 ... 64, both kinds
and R at the edges of the rows-per-wave steps, Np, G, the segment's pitch and the LDS bytes are what the header's text
gives (recomputed here), inside the family's 66 KiB, and the waves' rows cover the rows exactly once; for every
(G, Np, N, kind) that occurs the distinct addresses per bank in each 32-lane group -- counted from the address maps the
kernel itself uses -- of the walk's reads, the first lanes' output writes, the loader's writes and the storer's reads
are 1; the state's layout; the validation at its edges."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = 66 * 1024
T = 256
R_EDGES = sorted({1, 2, 3, 64, 1000, 8191, 8192} | {1024 * k - 1 + d for k in range(1, 8) for d in (0, 1, 2)})


def expected(rows, taps, cplx):
    """(G, Np, S, lds bytes) from the header's text"""
    lanes = 1
    while lanes < taps:
        lanes *= 2
    g = min(8, 64 // lanes, -(-rows // 1024))
    need = taps - 1 + T
    s = next(v for v in range(need, need + 64) if v % 64 == lanes % 64)
    planes = 2 if cplx else 1
    return g, lanes, s, 4 * (planes * g * s + (planes + 1) * g * (T + 1) + planes * 64)


def test_equalizer_plan_under_asan_ubsan():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "equalizer_plan")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"), os.path.join(ROOT, "tests", "host", "equalizer_plan.cpp"), "-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:]
    assert "equalizer_plan ok" in out.stdout, out.stdout[-2000:]
    lines = out.stdout.splitlines()
    geoms = {tuple(int(v) for v in s.split(":")[1].split()) for s in lines if s.startswith("geom:")}
    assert {g[:3] for g in geoms} == {(r, n, c) for r in R_EDGES for n in range(1, 65) for c in (0, 1)}
    for r, n, c, g, lanes, s, lds in geoms:
        assert (g, lanes, s, lds) == expected(r, n, c), (r, n, c)
        assert lds < BUDGET
    banks = [tuple(int(v) for v in s.split(":")[1].split()) for s in lines if s.startswith("banks:")]
    print("(rows per wave, lanes per row) pairs:", sorted({b[:2] for b in banks}))
    pairs = {(g, lanes) for lanes in (1, 2, 4, 8, 16, 32, 64) for g in range(1, min(8, 64 // lanes) + 1)}
    assert {b[:2] for b in banks} == pairs
    assert {b[:4] for b in banks} == {expected(r, n, c)[:2] + (n, 1 + c) for r in R_EDGES for n in range(1, 65) for c in (0, 1)}
    bad = [b for b in banks if b[4:] != (1, 1, 1, 1)]
    assert not bad, f"bank conflicts (G, Np, N, planes, walk, out, load, store): {bad[:5]}"
    (largest,) = [int(s.split(":")[1]) for s in lines if s.startswith("largest lds:")]
    print("largest LDS request:", largest)
    assert largest == max(g[6] for g in geoms) == 4 * (2 * 8 * 264 + 3 * 8 * 257 + 128) < BUDGET

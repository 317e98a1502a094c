"""The AGC bank's host arithmetic (csrc/hz_agc_plan.h) built with AddressSanitizer + UndefinedBehaviorSanitizer as a
stand-alone program (tests/host/agc_plan.cpp): for every R = 1 ... 8192 and both kinds the LDS request is at most
3 * 256 * 9 floats (inside the family's 66 KiB) and the waves' rows cover the rows exactly once; for every rows-per-wave
the lanes per bank in each 32-lane group of the loader's and storer's accesses and of the walk's -- counted from the
address maps the kernel itself uses, over all planes, the gain plane included -- are 1; the derivation of iref and the
validation at its edges; 2^20 steps at the extreme accepted sets with the error held at -1 and at +1 keep the gain
finite, above zero and in range."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = 66 * 1024


def test_agc_plan_under_asan_ubsan():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "agc_plan")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"), os.path.join(ROOT, "tests", "host", "agc_plan.cpp"), "-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:]
    assert "agc_plan ok" in out.stdout, out.stdout[-2000:]
    lines = out.stdout.splitlines()
    banks = [tuple(int(v) for v in s.split(":")[1].split()) for s in lines if s.startswith("banks:")]
    print("(rows per wave, planes, lanes per bank of the loader and storer, of the walk):", banks)
    assert {b[:2] for b in banks} == {(g, p) for g in range(1, 9) for p in (2, 3)} and len(banks) == 16
    assert all(b[2:] == (1, 1) for b in banks)
    (largest,) = [int(s.split(":")[1]) for s in lines if s.startswith("largest lds:")]
    print("largest LDS request:", largest)
    assert largest == 3 * 256 * 9 * 4 < BUDGET

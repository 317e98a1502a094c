"""The symbol-timing recovery bank's host arithmetic (csrc/hz_symsync_plan.h) built with AddressSanitizer +
UndefinedBehaviorSanitizer as a stand-alone program (tests/host/symsync_plan.cpp): for every R = 1 ... 8192 and both
kinds the LDS request is under 28 KiB (inside the family's 66 KiB) and the waves' rows cover the rows exactly once; for
every geometry that occurs, the lanes per bank in each 32-lane group of the loader's write, the walk's sample read, the
walk's symbol write and the storer's read -- counted from the address maps the kernel itself uses -- are 1; no strobe
pattern the invariants allow puts more than T / 2 + 1 symbols of a row into a tile; the bound function holds against a
counter denser than any real row, for every small n; the parameters' validation at its edges."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = 66 * 1024


def test_symsync_plan_under_asan_ubsan():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "symsync_plan")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"), os.path.join(ROOT, "tests", "host", "symsync_plan.cpp"), "-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:]
    assert "symsync_plan ok" in out.stdout, out.stdout[-2000:]
    lines = out.stdout.splitlines()
    banks = [tuple(int(v) for v in s.split(":")[1].split()) for s in lines if s.startswith("banks:")]
    print("(rows per wave, planes, lanes per bank of the loader, the walk's read, the walk's write, the storer):", banks)
    # every rows-per-wave from 1 to 8, real and complex
    assert {b[0] for b in banks} == set(range(1, 9)) and {b[1] for b in banks} == {1, 2} and len(banks) == 16
    assert all(b[2:] == (1, 1, 1, 1) for b in banks)
    (largest,) = [int(s.split(":")[1]) for s in lines if s.startswith("largest lds:")]
    print("largest LDS request:", largest)
    assert 0 < largest < 28 * 1024 <= BUDGET

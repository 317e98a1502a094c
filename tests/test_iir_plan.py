"""The IIR bank's host arithmetic (csrc/hz_iir_plan.h) built with AddressSanitizer + UndefinedBehaviorSanitizer as a
stand-alone program (tests/host/iir_plan.cpp): for every R = 1 ... 8192, both kinds (and each sample size) and every S,
the LDS request is inside the budget and the waves' rows cover the rows exactly once; for every geometry that occurs,
the lanes per bank in each 32-lane group of both tile accesses -- counted from the address maps the kernel itself uses
-- are 1."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = 66 * 1024


def test_iir_plan_under_asan_ubsan():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "iir_plan")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"), os.path.join(ROOT, "tests", "host", "iir_plan.cpp"), "-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:]
    assert "iir_plan ok" in out.stdout, out.stdout[-2000:]
    lines = out.stdout.splitlines()
    banks = [tuple(int(v) for v in s.split(":")[1].split()) for s in lines if s.startswith("banks:")]
    print("(rows per wave, steps, planes, lanes per bank of the loader, of the recursion):", banks)
    # every rows-per-wave from 1 to 8, real and complex, four steps per lane
    assert {b[0] for b in banks} == set(range(1, 9)) and {b[1] for b in banks} == {4} and {b[2] for b in banks} == {1, 2}
    assert all(b[3] == 1 and b[4] == 1 for b in banks)
    (largest,) = [int(s.split(":")[1]) for s in lines if s.startswith("largest lds:")]
    print("largest LDS request:", largest)
    assert 0 < largest <= BUDGET

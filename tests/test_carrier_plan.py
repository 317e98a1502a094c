"""The carrier recovery bank's host arithmetic (csrc/hz_carrier_plan.h) built with AddressSanitizer +
UndefinedBehaviorSanitizer as a stand-alone program (tests/host/carrier_plan.cpp): for every R = 1 ... 8192, with and
without the track plane, the LDS request is at most 3 * 256 * 9 floats (inside the family's 66 KiB) and the waves' rows
cover the rows exactly once; for every rows-per-wave, the lanes per bank in each 32-lane group of the loader's write and
the walk's access -- counted from the address maps the kernel itself uses, the track plane included -- are 1; the
derivation of the constants and the validation at its edges; no int32 overflow at the extreme accepted sets with the
error held at +-1 for 2^20 samples, by an int64 evaluation beside the int32 one and by car_step itself."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = 66 * 1024


def test_carrier_plan_under_asan_ubsan():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "carrier_plan")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"), os.path.join(ROOT, "tests", "host", "carrier_plan.cpp"), "-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:]
    assert "carrier_plan ok" in out.stdout, out.stdout[-2000:]
    lines = out.stdout.splitlines()
    banks = [tuple(int(v) for v in s.split(":")[1].split()) for s in lines if s.startswith("banks:")]
    print("(rows per wave, lanes per bank of the loader, the walk, the track's loader, the track's walk):", banks)
    assert {b[0] for b in banks} == set(range(1, 9)) and len(banks) == 8
    assert all(b[1:] == (1, 1, 1, 1) for b in banks)
    (largest,) = [int(s.split(":")[1]) for s in lines if s.startswith("largest lds:")]
    print("largest LDS request:", largest)
    assert largest == 3 * 256 * 9 * 4 < BUDGET

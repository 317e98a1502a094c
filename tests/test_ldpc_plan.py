"""The LDPC decoder bank's host arithmetic (csrc/hz_ldpc_plan.h, csrc/hz_ldpc_math.h) built with AddressSanitizer +
UndefinedBehaviorSanitizer as a stand-alone program (tests/host/ldpc_plan.cpp): forged row pointers, columns at and above
n, repeated and descending columns, degrees 0, 1 and 65, E above its bound and head + N above n over arrays of exactly the
stated lengths -- every one refused with no access outside the arrays; the plan of random admissible codes and of the
codes at the bounds inside the LDS budget it reports; the tables by variable against the tables by check; a frame through
the kernel's own passes and layout inside a buffer of exactly the planned LDS bytes, against a plain decoder."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = 160 * 1024


def test_ldpc_plan_under_asan_ubsan():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "ldpc_plan")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"), os.path.join(ROOT, "tests", "host", "ldpc_plan.cpp"), "-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:]
    assert "ldpc_plan ok" in out.stdout, out.stdout[-2000:]
    (largest,) = [int(s.split(":")[1]) for s in out.stdout.splitlines() if s.startswith("largest lds:")]
    print("largest LDS request:", largest)
    assert largest == 64 + 32768 + 16384 + 65536 <= BUDGET  # n = 16384, E = 65536: the counters, P, q, the messages

"""The demapper bank's host arithmetic (csrc/hz_demap_plan.h, csrc/hz_demap_math.h) built with AddressSanitizer +
UndefinedBehaviorSanitizer as a stand-alone program (tests/host/demap_plan.cpp): forged perm entries at and above S m,
non-finite points and gains over arrays of exactly the stated lengths -- every one refused with no access outside the
arrays; the plan at the bounds (S = 8192 with m = 2, S = 2048 with m = 8, N = 1 and N = 8192) and of random admissible
shapes inside the LDS budget it reports; a call through the kernel's own walk and layout inside buffers of exactly the
planned sizes, with both forms of the minima, against a plain loop; the check of a call at its edges.  Only this
stand-alone program runs under a sanitizer."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = 160 * 1024


def test_demap_plan_under_asan_ubsan():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "demap_plan")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"), os.path.join(ROOT, "tests", "host", "demap_plan.cpp"), "-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:]
    assert "demap_plan ok" in out.stdout, out.stdout[-2000:]
    (largest,) = [int(s.split(":")[1]) for s in out.stdout.splitlines() if s.startswith("largest lds:")]
    print("largest LDS request:", largest)
    assert largest == 16384 * 4 <= BUDGET  # S m = 16384 values of one frame

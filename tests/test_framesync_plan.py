"""The frame sync bank's host arithmetic (csrc/hz_framesync_plan.h, csrc/hz_framesync_math.h) built with AddressSanitizer +
UndefinedBehaviorSanitizer as a stand-alone program (tests/host/framesync_plan.cpp): the ring's geometry for every (W, P)
at the bounds; the ring walked as the kernel walks it, every window and every payload word read back by funnel shifts at
every bit offset 0 ... 63 against a bit-by-bit loop, with pushes of every length modulo 64 and the history re-aligned
behind each; the word reversal and the other word forms against the bit forms; the largest LDS request, 256 words,
against the family's 66 KiB."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = 66 * 1024


def test_framesync_plan_under_asan_ubsan():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "framesync_plan")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"), os.path.join(ROOT, "tests", "host", "framesync_plan.cpp"), "-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:]
    assert "framesync_plan ok" in out.stdout, out.stdout[-2000:]
    (largest,) = [int(s.split(":")[1]) for s in out.stdout.splitlines() if s.startswith("largest lds:")]
    print("largest LDS request:", largest)
    assert largest == 256 * 8 < BUDGET

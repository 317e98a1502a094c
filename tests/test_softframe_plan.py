"""The soft frame bank's index arithmetic (csrc/hz_softframe_plan.h) built with AddressSanitizer +
UndefinedBehaviorSanitizer as a stand-alone program (tests/host/softframe_plan.cpp): the window test at its uint64 edges
(s near 0 with p0 < Kh, s + Ps at p1 and p1 + 1, positions near 2^64) against 128-bit integers; the gather, lane by lane
in both forms, and the carry over buffers of exactly the planned sizes at P = B, P = 8192 and Kh = 0 with pushes shorter
than the history; the maps; every rejected configuration and every refused push."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_softframe_plan_under_asan_ubsan():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "softframe_plan")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"), os.path.join(ROOT, "tests", "host", "softframe_plan.cpp"), "-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:]
    assert "softframe_plan ok" in out.stdout, out.stdout[-2000:]

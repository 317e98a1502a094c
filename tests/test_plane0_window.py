"""The per-plane matrix loop's plane-0 window (csrc/hz_firmm2_plan.h, mm2::plane0_window), built with
AddressSanitizer + UndefinedBehaviorSanitizer and checked against the digit tables themselves
(tests/host/plane0_window.cpp): every nonzero top digit of every clock run's table lies on step pairs inside
the window, for random filters, scales, shifts and modulations and for taps exactly on the bound.  CPU only."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plane0_window_under_asan_ubsan():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "plane0_window")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "host", "plane0_window.cpp"),
                               os.path.join(ROOT, "go-sdr_amd", "csrc", "hz_host.cpp"), "-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe, "300"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-4000:]
        assert "plane0_window ok" in out.stdout, out.stdout[-2000:]

"""The host arithmetic that the bit-ring banks share (csrc/hz_bitring_plan.h) built with AddressSanitizer +
UndefinedBehaviorSanitizer as a stand-alone program (tests/host/bitring_plan.cpp): for every K from 1 to 8192 + 63 the
ring's geometry, the history's bytes there and back from both sides, and the re-alignment of the history behind pushes
of 0, 1, 63, 64, 65 and 64 kChunk - 1, 64 kChunk, 64 kChunk + 1 bits against the plain bit array."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bitring_plan_under_asan_ubsan():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "bitring_plan")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"), os.path.join(ROOT, "tests", "host", "bitring_plan.cpp"), "-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:]
    assert "bitring_plan ok" in out.stdout, out.stdout[-2000:]
    assert "widest ring: 256" in out.stdout, out.stdout[-2000:]

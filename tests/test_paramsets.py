"""The loop banks' parameter-set bookkeeping (csrc/hz_paramsets.h, the HIP-free part of csrc/hz_loopbank.h) built with
AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program (tests/host/paramsets.cpp) over the AGC bank's
check and derivation: one set against R copies of it for R up to 8192, rows of their own, a refused last row, the first
of two refusals, and a holder that a refused call leaves bit for bit as it was."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_paramsets_under_asan_ubsan():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "paramsets")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"), os.path.join(ROOT, "tests", "host", "paramsets.cpp"), "-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:]
    assert "paramsets ok" in out.stdout, out.stdout[-2000:]

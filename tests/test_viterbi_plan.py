"""The Viterbi decoder bank's host arithmetic (csrc/hz_viterbi_plan.h, csrc/hz_viterbi_math.h) built with AddressSanitizer
+ UndefinedBehaviorSanitizer as a stand-alone program (tests/host/viterbi_plan.cpp): the plan for every (K, n,
termination) at the bounds of D and across the edge between the LDS and the scratch form of the decisions; the puncture
index table against a bit-by-bit walk for every pattern length; a wave emulated lane by lane with the kernel's own maps
over buffers of exactly the planned sizes -- metrics by lane exchange, decision words, the chunked traceback, the decoded
words -- against a plain decoder; the CRC's byte table against its bit steps; the largest LDS request against the family's
66 KiB."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = 66 * 1024


def test_viterbi_plan_under_asan_ubsan():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "viterbi_plan")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"), os.path.join(ROOT, "tests", "host", "viterbi_plan.cpp"), "-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:]
    assert "viterbi_plan ok" in out.stdout, out.stdout[-2000:]
    (largest,) = [int(s.split(":")[1]) for s in out.stdout.splitlines() if s.startswith("largest lds:")]
    print("largest LDS request:", largest)
    assert 60 * 1024 < largest <= BUDGET

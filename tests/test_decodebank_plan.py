"""What the decoder banks share on the host (csrc/hz_decodebank_plan.h, csrc/hz_received.h) built with AddressSanitizer +
UndefinedBehaviorSanitizer as a stand-alone program (tests/host/decodebank_plan.cpp): slot_frame against plain division
for every slot under every kind of count; check_call under each bank's Slots, every refusal with its exact message and
code and in its order of precedence; quantise, hard and packed_bit at their special values."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_decodebank_plan_under_asan_ubsan():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "decodebank_plan")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"), os.path.join(ROOT, "tests", "host", "decodebank_plan.cpp"), "-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:]
    assert "decodebank_plan ok" in out.stdout, out.stdout[-2000:]

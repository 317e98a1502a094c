"""The HDLC deframer bank's host arithmetic (csrc/hz_hdlc_plan.h, csrc/hz_hdlc_math.h) built with AddressSanitizer +
UndefinedBehaviorSanitizer as a stand-alone program (tests/host/hdlc_plan.cpp): the validation over every combination of
values around the bounds; the geometry for every max_bytes; the word forms (stuffed mask, bit deletion, the FCS of a
word, the powers table and the modular product) against the bit forms; the history's bytes there and back; and the walk:
random noise and encoded traffic in random cuts through a ring laid out and read as the kernel does it, lane by lane,
every slot index checked, against a bit-serial decoder over the whole stream.  The largest LDS request, a ring of 256
words, a frame buffer of 129 and the FCS's byte table of 1 KiB, against the family's 66 KiB."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = 66 * 1024


def test_hdlc_plan_under_asan_ubsan():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "hdlc_plan")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"), os.path.join(ROOT, "tests", "host", "hdlc_plan.cpp"), "-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:]
    assert "hdlc_plan ok" in out.stdout, out.stdout[-2000:]
    (largest,) = [int(s.split(":")[1]) for s in out.stdout.splitlines() if s.startswith("largest lds:")]
    print("largest LDS request:", largest)
    assert largest == (256 + 129) * 8 + 1024 < BUDGET

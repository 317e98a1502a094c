"""The Reed-Solomon decoder bank's host arithmetic (csrc/hz_rs_plan.h, csrc/hz_rs_math.h) built with AddressSanitizer +
UndefinedBehaviorSanitizer as a stand-alone program (tests/host/rs_plan.cpp): the plan at every bound of nroots, n and
the interleave; the validation of configurations (all 16 primitive polynomials, every prim) and of calls (pitches,
strides, in place, partial overlaps); a workgroup emulated wave by wave and lane by lane with the kernel's own index maps
over buffers of exactly the planned sizes -- the table block, the LDS, the input and output spans -- against the plain
decoder, on clean words, correctable and uncorrectable ones, all 0x00, all 0xFF and random words; the largest LDS
request against what the plan promises (a few KiB, far inside the family's 66 KiB)."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = 66 * 1024


def test_rs_plan_under_asan_ubsan():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "rs_plan")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"), os.path.join(ROOT, "tests", "host", "rs_plan.cpp"), "-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:]
    assert "rs_plan ok" in out.stdout, out.stdout[-2000:]
    (largest,) = [int(s.split(":")[1]) for s in out.stdout.splitlines() if s.startswith("largest lds:")]
    print("largest LDS request:", largest)
    assert 4 * 1024 < largest <= 5 * 1024 <= BUDGET

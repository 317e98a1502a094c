"""What the polyphase banks share on the host (csrc/hz_polyphase_plan.h) built with AddressSanitizer +
UndefinedBehaviorSanitizer as a stand-alone program (tests/host/polyphase_plan.cpp): for random (M, P, D) of the
channelizer's and the channel bank's ranges and random pushes -- 0, 1, L - 1, L, L + D - 1, L + D, up to 2^62 samples and
beyond, which no GPU test can push -- the counts of step against the closed form in 128-bit integers; rot and pos against
the `& (M - 1)` forms for every power-of-two M; the argument check of a create, every refusal alone and the earlier of two;
the synthesis bank's counts of a group below 2^32 at every legal corner."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_polyphase_plan_under_asan_ubsan():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "polyphase_plan")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"), os.path.join(ROOT, "tests", "host", "polyphase_plan.cpp"), "-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe, "20261021", "8000"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-4000:]
    assert "polyphase_plan ok" in out.stdout, out.stdout[-2000:]
    lines = out.stdout.splitlines()
    (pushes,) = [int(s.split(":")[1]) for s in lines if s.startswith("pushes:")]
    (too_long,) = [int(s.split(":")[1]) for s in lines if s.startswith("too long:")]
    assert pushes > 100000 and too_long > 1000, "both sides of the largest push were walked"
    (refusals,) = [tuple(int(v) for v in s.split(":")[1].split()) for s in lines if s.startswith("refusals:")]
    assert refusals[0] == 7 * 13 and refusals[1] > 7 * 13 * 8, "every refusal alone and in pairs, under each rule"
    (largest,) = [int(s.split(":")[1]) for s in lines if s.startswith("largest group total:")]
    print("largest overlap-add of a group:", largest)
    assert largest == (1 << 21) + 31 * 8192 < 1 << 32, "group_frames(M) D + L - D at D = M = 8192, P = 32"

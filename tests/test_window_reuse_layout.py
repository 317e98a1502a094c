"""The window-re-using per-plane matrix loop's index maps (csrc/hz_firmm2_plan.h: reuse_row_offset, reuse_b_offset,
reuse_b_reg, reuse_b_read, xchg_*), built with AddressSanitizer + UndefinedBehaviorSanitizer
(tests/host/window_reuse_layout.cpp): the register rotation simulated from the reads the loop issues holds the right
image row on every pair, block and lane; the LDS bank model gives the conflict-free 4 cycles for each read (8 and more
for two wrong strides) and 8 for the landing's writes; the rows and the LDS budget fit; the epilogue's exchange is a
bijection onto the mixer's lanes and registers.  CPU only."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_window_reuse_layout_under_asan_ubsan():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "window_reuse_layout")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "host", "window_reuse_layout.cpp"), "-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-4000:]
        assert "window_reuse_layout ok" in out.stdout, out.stdout[-2000:]

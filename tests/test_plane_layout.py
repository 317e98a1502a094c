"""The per-plane matrix loop's LDS layouts (csrc/hz_firmm2_plan.h: plane_piece, plane_a_offset, plane_b_offset,
tile_stride), built with AddressSanitizer + UndefinedBehaviorSanitizer (tests/host/plane_layout.cpp): the staging
permutation of the tap table is a bijection, every (plane, entry, part) lies where the loop reads it, an LDS bank
model gives the conflict-free 4 cycles for each of the loop's reads (and 8 for the layouts it had before), and the
largest geometry's LDS fits a compute unit.  CPU only."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plane_layout_under_asan_ubsan():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "plane_layout")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "host", "plane_layout.cpp"), "-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-4000:]
        assert "plane_layout ok" in out.stdout, out.stdout[-2000:]

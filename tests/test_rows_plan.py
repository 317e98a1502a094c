"""The arithmetic of a call's rows (csrc/hz_rows.h, behind Stage::in_rows / out_rows) built with AddressSanitizer +
UndefinedBehaviorSanitizer and checked against Python's big integers (tests/host/rows_plan.cpp, a stand-alone program):
the span (rows - 1) * pitch + count in elements and bytes and the dense size of random (rows, count, pitch, size) --
refused exactly where a product or sum passes 2^64 - 1 --, and the route for every combination of (HOST context, one
row, pitch == count, pinned), with and without elements."""
import itertools
import os
import random
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 1 << 64
NOTHING, DENSE, CALLER, COPY2D = 0, 1, 2, 3


def span_line(rows, count, pitch, size):
    if rows == 0 or count == 0:
        return f"S {rows} {count} {pitch} {size} 1 0 0 0"
    elems = (rows - 1) * pitch + count
    dense = rows * count * size
    # every intermediate the header forms: (rows - 1) * pitch, the sum, the bytes, rows * count, the dense bytes
    if max((rows - 1) * pitch, elems, elems * size, rows * count, dense) >= LIMIT:
        return f"S {rows} {count} {pitch} {size} 0 0 0 0"
    return f"S {rows} {count} {pitch} {size} 1 {elems} {elems * size} {dense}"


def span_cases(seed, n):
    rng = random.Random(seed)
    lines = []

    def draw(bits):
        return rng.choice([0, 1, 2, rng.randrange(1 << bits), (1 << bits) - 1, 1 << bits])

    for i in range(n):
        bits = [(12, 20, 21), (31, 32, 33), (20, 40, 41), (1, 62, 63), (33, 30, 31), (63, 1, 1)][i % 6]
        rows, count = draw(bits[0]), draw(bits[1])
        pitch = rng.choice([count, count + rng.randrange(1 << 10), draw(bits[2])])
        lines.append(span_line(rows, count, pitch, rng.choice([2, 4, 8])))
    # the edge itself: the largest spans that fit and the first that do not
    for size in (2, 4, 8):
        top = (LIMIT - 1) // size
        lines += [span_line(1, top, 0, size), span_line(1, top + 1, 0, size), span_line(2, top // 2, top // 2, size),
                  span_line(2, top // 2 + 1, top // 2 + 1, size), span_line(3, 5, (top - 5) // 2, size), span_line(3, 5, (top - 5) // 2 + 1, size),
                  span_line(1 << 32, 1 << 29, 1 << 29, size), span_line((1 << 32) - 1, 1 << 28, 1 << 28, size)]
    return lines


def route_cases():
    lines = []
    for host, one, dense, pinned in itertools.product((0, 1), repeat=4):
        rows, count = (1 if one else 3), 100
        pitch = count if dense else 128
        want = DENSE if one or dense else CALLER if not host or pinned else COPY2D
        lines.append(f"R {host} {rows} {count} {pitch} {pinned} {want}")
        lines.append(f"K {host} {rows} {count} {pitch} {pinned} {DENSE if one else CALLER if not host or pinned else COPY2D}")
        lines.append(f"R {host} {rows} 0 {pitch} {pinned} {NOTHING}")
        lines.append(f"R {host} 0 {count} {pitch} {pinned} {NOTHING}")
    return lines


def test_rows_plan_under_asan_ubsan():
    spans, routes = span_cases(20261019, 6000), route_cases()
    refused = sum(line.split()[5] == "0" for line in spans)
    assert refused > 500 and len(spans) - refused > 2000, (refused, len(spans))
    assert len(routes) == 64 and {line.split()[-1] for line in routes} == {"0", "1", "2", "3"}
    with tempfile.TemporaryDirectory() as d:
        exe, data = os.path.join(d, "rows_plan"), os.path.join(d, "cases.txt")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"), os.path.join(ROOT, "tests", "host", "rows_plan.cpp"),
                               "-o", exe])
        with open(data, "w") as f:
            f.write("\n".join(spans + routes) + "\n")
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe, data], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-4000:]
    assert f"spans: {len(spans)} routes: {len(routes)}" in out.stdout and "rows_plan ok" in out.stdout, out.stdout[-2000:]

"""The covariance bank's host arithmetic (csrc/hz_covar_plan.h) built with AddressSanitizer + UndefinedBehaviorSanitizer
(tests/host/covar_plan.cpp, a stand-alone program) and checked against Python integers: the counts, the open segment
and the items of random pushes from positions up to 2^62 -- which no GPU test can reach --, the flush of every such
state, the shape of the tree for every segment count up to 2^16 against the recursive definition, the LDS request
against the budget.  The program checks by itself that the items cover a push exactly once and in order, that every node
joins adjacent runs with the earlier one on the left, that a resumed block builds the same tree, and both operand
layouts as bijections."""
import functools
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = 66 * 1024
SEG, GROUP, PITCH = 256, 8, 130
MASK = (1 << 64) - 1


def items(seg0, seg1):
    """items of the segments [seg0, seg1) of a block: singles up to the next multiple of 8, aligned groups, singles"""
    head = min(seg1, -(-seg0 // GROUP) * GROUP) - seg0
    groups = (seg1 - seg0 - head) // GROUP
    return head + groups + (seg1 - seg0 - head - groups * GROUP)


def mix(left, right):
    return ((left * 0x9E3779B97F4A7C15) & MASK) ^ ((right + 0xBF58476D1CE4E5B9 + (left << 7) + (left >> 3)) & MASK)


@functools.lru_cache(maxsize=None)
def shape(n):
    """the hash of T(lo, lo + n): the recursive definition, split at the largest power of two strictly below n"""
    if n == 1:
        return 1
    p = 1
    while p * 2 < n:
        p *= 2
    return mix(shape(p), shape(n - p))


def test_covar_plan_under_asan_ubsan():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "covar_plan")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"), os.path.join(ROOT, "tests", "host", "covar_plan.cpp"),
                               "-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe, "20261018", "1500"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        assert out.returncode == 0, out.stdout[-4000:]
        assert "covar_plan ok" in out.stdout, out.stdout[-2000:]
    lines = out.stdout.splitlines()

    lds = [tuple(int(v) for v in s.split(":")[1].split()) for s in lines if s.startswith("lds:")]
    assert [v[0] for v in lds] == list(range(2, 17))
    for n, nbytes, rows, tiles in lds:
        assert (rows, tiles) == ((16, 1) if n <= 8 else (32, 3)) and nbytes == rows * PITCH * 4 <= BUDGET
    print("largest LDS request (N, bytes):", max(lds, key=lambda v: v[1])[:2])

    pushes = [s for s in lines if s.startswith("push:")]
    assert len(pushes) == 1500
    far = 0
    for s in pushes:
        left, right = s[5:].split("|")
        b, consumed, opened, n = (int(v) for v in left.split())
        written, nconsumed, nblock, nopen, held_in, held_out, v, nitems, keep = (int(v) for v in right.split())
        assert opened == consumed % b
        total = opened + n
        assert written == total // b and nconsumed == consumed + n and nblock == consumed // b + written and nopen == total % b
        assert held_in == opened % SEG and held_out == nopen % SEG and v == held_in + n
        spb = -(-b // SEG)
        if written == 0:
            want, last = items(opened // SEG, nopen // SEG), items(opened // SEG, nopen // SEG)
        else:
            last = items(0, nopen // SEG)
            want = items(opened // SEG, spb) + (written - 1) * items(0, spb) + last
        assert nitems == want and keep == int(last > 0), s
        far += consumed + n > 1 << 61
    assert far > 100, "too few pushes near the end of the range"

    flushes = [s for s in lines if s.startswith("flush:")]
    assert len(flushes) == 1500
    for s in flushes:
        left, right = s[6:].split("|")
        b, opened = (int(v) for v in left.split())
        written, nitems, held_in, nconsumed = (int(v) for v in right.split())
        assert written == int(opened > 0) and nitems == items(opened // SEG, -(-opened // SEG)) and held_in == opened % SEG and nconsumed == 0

    sys.setrecursionlimit(10000)
    trees = [tuple(int(v) for v in s.split(":")[1].split()) for s in lines if s.startswith("tree:")]
    assert [t[0] for t in trees] == list(range(1, (1 << 16) + 1))
    for nseg, h in trees:
        assert h == shape(nseg), f"the tree over {nseg} segments is not the recursive definition's"

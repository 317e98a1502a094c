"""The transform FIR's host arithmetic (csrc/hz_chain_fir_plan.h) built with AddressSanitizer + UndefinedBehaviorSanitizer
(tests/host/chain_fir_plan.cpp, a stand-alone program): random geometries, calls and clock runs against a walk over every
block, and the cases of tests/test_fir_ref_cpu.py -- the geometry sweep, the run boundary swept over a span's and the
call's ends, every run-edge and slow-list case the GPU tests use -- answered by the header and compared with the Python
restatement (tests/fir_ref.py).  The list the GPU cases are sized by is then the library's own, not only a
restatement of it."""
import importlib
import os
import subprocess
import tempfile

import fir_ref as fr
from test_fir_ref_cpu import fake_runs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def slow_line(g, runs, n, has):
    firsts = [r[0] for r in runs]
    return "S %d %d %d %d %d %d %s %s" % (g.N, g.hop, g.off, n, g.nblocks(n), len(firsts), " ".join(map(str, firsts)),
                                           " ".join(str(int(v)) for v in has))


def test_chain_fir_plan_under_asan_ubsan():
    hz = importlib.import_module("go-sdr_amd")
    lines, want = [], []
    for D in (1, 2, 3, 4, 5, 8, 10, 16, 32):
        for ntaps in (1, 2, 30, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 5000, 7808, 8185, 8186, 8192, 8193):
            for nmin in (0, 256, 300, 512, 1024, 2048, 4096, 8192, 16384):
                g = fr.Geom(ntaps, D, nmin)
                lines.append("G %d %d %d" % (ntaps, D, nmin))
                want.append("G %d %d %d %d" % ((g.N, g.off, g.hop, 1) if g.ok else (g.N, 0, 0, 0)))
    calls = []
    for ntaps, D in ((135, 3), (263, 8), (7808, 4), (1031, 1)):
        g = fr.Geom(ntaps, D)
        b_mid = 2 * g.N // g.hop + 3
        n0 = g.p0(b_mid + 2 * g.N // g.hop + 6) + g.N + g.off
        base = g.p0(b_mid)
        sweeps = [(n0, base + d) for d in (-1, 0, 1, g.N - 1, g.N)] + [(n0 + d, base) for d in (-1, 0, 1, g.N - 1, g.N)]
        sweeps += [(n0, n0 - g.off - g.N + d) for d in (-1, 0, 1, g.N - 1, g.N)]
        for n, s in sweeps:
            for firsts in ([0, s], [0, s, s + 2 * g.N], [0, s, s + 100], [0]):
                calls.append((g, fake_runs(firsts), n))
    for c in fr.run_edge_cases(hz) + fr.slow_cases(hz):
        calls.append((c["g"], fr.clock_runs(hz, c["rate"], c["ts0"], c["n"]), c["n"]))
    classes = set()
    for g, runs, n in calls:
        has = fr.run_filters(g, runs, n)
        if has is None:
            continue
        lst, cls = fr.slow_list(g, runs, n, has)
        classes.add(cls)
        lines.append(slow_line(g, runs, n, has))
        want.append(" ".join(["S", str(len(lst))] + [str(b) for b in lst]))
    assert classes == set(fr.CLASSES)
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "chain_fir_plan")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I" + os.path.join(ROOT, "go-sdr_amd", "csrc"), os.path.join(ROOT, "tests", "host", "chain_fir_plan.cpp"),
                               "-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe, "20261020", "20000"], env=env, input="\n".join(lines) + "\n", stdout=subprocess.PIPE,
                             stderr=subprocess.STDOUT, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-4000:]
    got = out.stdout.splitlines()
    assert got[-1] == "chain_fir_plan ok", out.stdout[-2000:]
    assert len(got) == len(want) + 1
    for line, g_, w_ in zip(lines, got, want):
        assert g_ == w_, (line, "the header says", g_, "the restatement", w_)
    print("%d geometries and %d calls agree with the header" % (sum(w.startswith("G") for w in want), sum(w.startswith("S") for w in want)))

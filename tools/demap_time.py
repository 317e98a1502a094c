"""Times the demapper bank (include/hzsdr_demap.h) in us per call, median of --steps after --warmup, and writes the lines
to --out (profiles/demap_time.txt).  The shape is 8192 rows x 4 frames of S = 2048 symbols, and one frame alone for the
latency; the kinds are LLR_F32, C64 with m = 2, 4, 6, 7, 8 (qam_points; psk_points at m = 7) and REAL_F32 with m = 2 (pam_points), each with the
values in their order and under a block_interleaver perm over the same N values.  N = S m where that is at most 8192;
at m = 6, 7 and 8 a frame has 12288, 14336 and 16384 values and a bank needs a perm, so "in order" is there the perm 0 ... 8191
(the first 8192 values kept) and the interleaver permutes those.  Inputs are made on the device and come from HBM over
a rotation of --rotation buffers, each larger than the 256 MiB the last-level cache holds.

The yardstick is the library's own device copy (hzsdr_convert c64 -> c64) of (read + written) / 2 bytes, which reads and
writes as many bytes as the stage.  Per case: us per call, us of the copy, their ratio, Gsymbols/s and GB/s moved.

From m = 7 on the kernel takes a symbol's minima by the two-sided tree (HZSDR_DEMAP_FORM_TREE), below point by point;
--alt-lib names builds of the library with another threshold (make ... EXTRA=-DHZ_DEMAP_TREE_FROM=6: the tree at m = 6
too; =9: point by point everywhere), which child processes time over the cases with m >= 6, and the table states every
time beside the float32 operations per symbol counted from the code: 5 per point (C64) for the distances, the minima of
the form, and 2 per bit for the value.

    python tools/demap_time.py [--steps 20] [--warmup 3] [--rotation 2] [--alt-lib PATH ...] [--out profiles/demap_time.txt]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
hz = importlib.import_module("go-sdr_amd")
from symsync_time import timed  # noqa: E402

S, ROWS, CAP = 2048, 8192, 4
# name -> (kind, m)
CASES = {"llr": (hz.DEMAP_LLR_F32, 1), "c64 m=2": (hz.DEMAP_C64, 2), "c64 m=4": (hz.DEMAP_C64, 4), "c64 m=6": (hz.DEMAP_C64, 6), "c64 m=7": (hz.DEMAP_C64, 7), "c64 m=8": (hz.DEMAP_C64, 8),
         "real m=2": (hz.DEMAP_REAL_F32, 2)}


def minima(m, tree):
    """a symbol's minima in either form (csrc/hz_demap_math.h: naive_minima, tree_minima)"""
    if not tree:
        return m << m
    c = min(m, 5)
    return ((1 << m) >> c) * (3 * (1 << c) - 3 + (m - c))


def operations(kind, m, tree):
    """float32 operations per symbol, counted from the code"""
    if kind == hz.DEMAP_LLR_F32:
        return 1
    return (5 if kind == hz.DEMAP_C64 else 2) * (1 << m) + minima(m, tree) + 2 * m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rotation", type=int, default=2)
    ap.add_argument("--alt-lib", nargs="*", default=[], help="other builds of the library (other HZ_DEMAP_TREE_FROM), timed over the cases with m >= 6")
    ap.add_argument("--only", nargs="*", default=None, help="case names (the child process of --alt-lib)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "demap_time.txt"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = hz.Context(0, hz.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    lines, results = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"median of {args.steps} calls after {args.warmup}; S = {S}; inputs from a rotation of {args.rotation} buffers; "
        f"the copy: hzsdr_convert c64 -> c64 of (read + written) / 2 bytes")
    gen = torch.Generator(device="cuda").manual_seed(5)
    for name, (kind, m) in CASES.items():
        if args.only is not None and name not in args.only:
            continue
        pts = None if kind == hz.DEMAP_LLR_F32 else hz.pam_points(m) if kind == hz.DEMAP_REAL_F32 else hz.qam_points(m) if m % 2 == 0 else hz.psk_points(m)
        L = S * m
        N = min(L, hz.DEMAP_MAX_OUT)
        il = hz.block_interleaver(N // 128 if N >= 8192 else N // 64, 128 if N >= 8192 else 64)
        assert len(il) == N
        W = 2 * S if kind == hz.DEMAP_C64 else S
        for rows, cap in ((1, 1), (ROWS, CAP)):
            rot = args.rotation if rows > 1 else 1
            ins = [torch.randn((rows, cap, W), generator=gen, device="cuda", dtype=torch.float32) * 0.7 for _ in range(rot)]
            out = torch.empty((rows, cap, N), device="cuda", dtype=torch.float32)
            moved = 4 * rows * cap * (W + N)
            copy_us = None
            if rows > 1:
                ncopy = moved // 16
                ca = [torch.empty(ncopy, dtype=torch.complex64, device="cuda") for _ in range(rot)]
                cb = torch.empty(ncopy, dtype=torch.complex64, device="cuda")
                copy_us = round(timed(lambda i: ctx.convert(cb, ca[i % rot]), args.steps, args.warmup), 1)
                del ca, cb
            for order, perm in (("in order", None if L == N else np.arange(N, dtype=np.uint32)), ("interleaved", il)):
                bank = ctx.demapper(kind, pts, S, perm=perm, gain=hz.demap_gain(0.1), rows=rows)
                per_group, threads, frame_lds, form = bank.plan()
                tree = bool(form & hz.DEMAP_FORM_TREE)
                bank.run(ins[0], out=out)
                torch.cuda.synchronize()
                steps = args.steps if rows > 1 else 5 * args.steps
                us = round(timed(lambda i: bank.run(ins[i % rot], out=out), steps, args.warmup), 1)
                bank.close()
                case = {"bank": "demap", "case": name, "kind": kind, "m": m, "S": S, "N": N, "rows": rows, "cap": cap, "order": order, "frames_per_group": per_group,
                        "threads_per_frame": threads, "frame_lds_bytes": frame_lds, "form": form, "tree": tree, "us": us, "copy_us": copy_us,
                        "of_the_copy": None if copy_us is None else round(us / copy_us, 3), "gsymbols_per_s": round(rows * cap * S / us / 1e3, 3),
                        "moved_gbytes_per_s": round(moved / us / 1e3, 1), "operations_per_symbol": operations(kind, m, tree),
                        "minima_per_symbol": 0 if kind == hz.DEMAP_LLR_F32 else minima(m, tree)}
                beside = "" if copy_us is None else f" = {case['of_the_copy']:.3f} of the copy's {copy_us:9.1f} us"
                say(f"demap {name:8s} N={N:5d} {order:11s} frames={rows * cap:6d} (rows {rows} x cap {cap}): {us:10.1f} us{beside}; "
                    f"{case['gsymbols_per_s']:8.3f} Gsymbols/s, {case['moved_gbytes_per_s']:7.1f} GB/s moved; {case['operations_per_symbol']} operations per symbol "
                    f"({'tree' if tree else 'point by point'}: {case['minima_per_symbol']} minima); frames/group={per_group} threads/frame={threads} "
                    f"frame LDS={frame_lds} form={form}")
                results.append(case)
            del ins, out
    ctx.close()
    for lib in args.alt_lib:
        names = [n for n, (k, m) in CASES.items() if m >= 6]
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps", str(args.steps), "--warmup", str(args.warmup), "--rotation", str(args.rotation),
                                "--out", os.devnull, "--only", *names], env=dict(os.environ, HZSDR_LIB=os.path.abspath(lib)), capture_output=True, text=True,
                               timeout=900)
        if child.returncode != 0:
            raise SystemExit("the child process over --alt-lib failed:\n" + child.stdout[-2000:] + child.stderr[-2000:])
        other = json.loads(child.stdout.strip().splitlines()[-1])["demap_time"]
        say(f"another build of the library ({os.path.basename(lib)}), timed by a child process over the same cases; where its form is this build's, the two times show the spread:")
        for o in other:
            (here,) = [c for c in results if c["bank"] == "demap" and (c["case"], c["rows"], c["order"]) == (o["case"], o["rows"], o["order"])]
            word = lambda c: "tree" if c["tree"] else "point by point"
            say(f"demap {o['case']:8s} {o['order']:11s} frames={o['rows'] * o['cap']:6d}: there {word(o):14s} {o['us']:10.1f} us with {o['operations_per_symbol']} operations per symbol "
                f"({o['minima_per_symbol']} minima); here {word(here):14s} {here['us']:10.1f} us with {here['operations_per_symbol']} ({here['minima_per_symbol']} minima)")
        results += [dict(o, bank="demap_other_build:" + os.path.basename(lib)) for o in other]
    if args.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"demap_time": results}))


if __name__ == "__main__":
    main()

"""Times the soft frame bank (include/hzsdr_softframe.h) in us per push, median of --steps after --warmup, and writes the
lines to --out (profiles/softframe_time.txt): one frame alone (one row, cap 1: the latency of the two launches), then
8192 rows x cap 4 at P = 2048, real rows and complex rows at two bits per symbol.  Every row gets n = P / B symbols per
push and four frames that end in the push, 0, 1/4, 1/2 and 3/4 of a payload before its last symbol, so that the gather
reads the history and the input alike; the positions move on with the stream from push to push, as in use.  The inputs
rotate through buffers whose bytes together pass the 256 MB cache by a quarter.

The stage is a copy, so each case stands beside the library's own device copy (hzsdr_convert between equal formats) of
as many bytes as the gather WRITES (rows * cap * P floats).  Per case: us per push, us of the copy, their ratio and the
GB/s written.  The first row's first frame must come back as the stream's floats.

    python tools/softframe_time.py [--steps 100] [--warmup 20] [--out profiles/softframe_time.txt]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
hz = importlib.import_module("go-sdr_amd")
from symsync_time import CACHE, timed  # noqa: E402

P = 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "softframe_time.txt"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    torch.manual_seed(1)
    ctx = hz.Context(0, hz.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    lines, results = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def run(name, kind, B, rows, cap):
        Ps = P // B
        n = Ps
        shape = (n,) if rows == 1 else (rows, n)
        moved_in = rows * n * (8 if B == 2 else 4)
        rot = int(max(2, min(16, -(-(CACHE + CACHE // 4) // moved_in))))
        ins = [torch.randn(shape + ((2,) if kind == hz.FMT_C64 else ()), dtype=torch.float32, device="cuda") for _ in range(rot)]
        xs = [torch.view_as_complex(a) if kind == hz.FMT_C64 else a for a in ins]
        written = rows * cap * P * 4
        src = torch.randn(written // 8, 2, dtype=torch.float32, device="cuda")
        src, dst = torch.view_as_complex(src), torch.empty(written // 8, dtype=torch.complex64, device="cuda")
        copy_us = round(timed(lambda i: ctx.convert(dst, src), args.steps, args.warmup), 1)
        del src, dst
        bank = hz.SoftFrames(ctx, kind, P, [0, 1] if B == 1 else [0, 1, 2, 3], bits_per_symbol=B, rows=rows)
        step, hf, form = bank.plan()
        # frame f of a push ends f / cap of a payload before the push's last symbol; push k consumes [k n, (k + 1) n)
        back = torch.tensor([(f * Ps) // cap for f in range(cap)], dtype=torch.int64, device="cuda")
        info = (torch.arange(rows * cap, dtype=torch.int32, device="cuda").reshape(rows, cap) % (2 if B == 1 else 4)) << 8
        info[0, 0] = 0
        got = torch.full((rows,), cap, dtype=torch.int32, device="cuda")
        calls = args.warmup + args.steps + 2
        pos = [((k + 1) * n - Ps - back).repeat(rows, 1).contiguous() for k in range(calls)]
        soft = torch.zeros((rows, cap, P), dtype=torch.float32, device="cuda")
        status = torch.zeros((rows, cap), dtype=torch.int32, device="cuda")
        done = [0]

        def push(i):
            k = done[0]
            done[0] += 1
            bank.push(xs[k % rot], None, pos[k], info, got, cap, out=(soft, status))

        push(0)
        torch.cuda.synchronize()
        first = ins[0].reshape(rows, -1)[0]
        ok = bool(torch.equal(soft[0, 0].view(torch.int32), first.view(torch.int32))) and int(status[0, 0]) == 0
        us = round(timed(push, args.steps, args.warmup), 1)
        served = int((status == 0).sum())
        bank.close()
        case = {"bank": "softframe", "kind": name, "B": B, "P": P, "rows": rows, "cap": cap, "n": n, "step_floats": step, "history_floats": hf,
                "form": form, "rotation": rot, "written_bytes": written, "us": us, "copy_us": copy_us, "of_the_copy": round(us / copy_us, 3),
                "written_gbytes_per_s": round(written / us / 1e3, 1), "served_last_push": served, "first_frame_right": ok}
        say(f"softframe {name} B={B} P={P} R={rows:5d} cap={cap} n={n}: {us:9.1f} us = {case['of_the_copy']:.3f} of the copy's {copy_us:9.1f} us "
            f"({written} bytes written, {case['written_gbytes_per_s']:.1f} GB/s); rotation {rot}; {served} of {rows * cap} served in the last push; "
            f"first frame right: {ok}")
        results.append(case)

    say(f"gather + carry per push, median of {args.steps} pushes after {args.warmup}; the copy: hzsdr_convert c64 -> c64 of the bytes written")
    run("f32", hz.SYMSYNC_REAL_F32, 1, 1, 1)
    run("c64", hz.FMT_C64, 2, 1, 1)
    run("f32", hz.SYMSYNC_REAL_F32, 1, 8192, 4)
    run("c64", hz.FMT_C64, 2, 8192, 4)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps({"softframe_time": results}))


if __name__ == "__main__":
    main()

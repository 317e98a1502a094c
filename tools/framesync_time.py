"""Times the frame sync bank (include/hzsdr_framesync.h) in us per push, median of --steps after --warmup, from HBM (a
rotation of input buffers whose bytes together pass the 256 MB cache by a quarter: 320 MiB at least): R = 1, 100, 1024
and 8192 rows, real rows (B = 1) and complex rows with B = 2, a 32-bit word with thr = 2 in front of P = 168 and of
P = 8192 payload bits, hits absent (white rows: a false candidate is a matter of 1e-7 per bit) and rare (a frame planted
every 16384 symbols of every row from symbol 64 on, as far as whole frames fit a push).  A push carries 512 MiB of
symbols (4 MiB for R = 1, which is bound by the latency of ONE wave's loads).  Beside every input, in the same run and over the
same bytes, the library's own device copy (hzsdr_convert between equal formats: copy_stream_kernel): the yardstick,
which reads the bytes once AND writes them once, where this stage reads them once and writes almost nothing.

Prints one line per case and one JSON line at the end.

    python tools/framesync_time.py [--steps 200] [--warmup 30] [--rows 1 100 1024 8192]
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

ROWS = (1, 100, 1024, 8192)
WORD, W, THR = 0x1ACFFC1D, 32, 2
PUSH_BYTES, ONE_ROW_BYTES = 512 << 20, 4 << 20
EVERY = 16384  # symbols from one planted frame to the next
CAP = 4


def plant(x, B, P, seed):
    """the word and a payload into every row of the float view x (rows, floats), every EVERY symbols"""
    rng = np.random.default_rng(seed)
    floats = x.shape[-1]
    span = W + P
    vals = np.concatenate([[(WORD >> (W - 1 - k)) & 1 for k in range(W)], rng.integers(0, 2, P)]).astype(np.float32) * 2.0 - 1.0
    vals = torch.from_numpy(vals).cuda()
    starts = list(range(64 * B, floats - span, EVERY * B))
    for at in starts:
        x[..., at:at + span] = vals
    return len(starts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rows", type=int, nargs="+", default=list(ROWS), help="the row counts to time")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    torch.manual_seed(1)
    ctx = hz.Context(0, hz.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    results = []
    for rows in args.rows:
        for kind, name, B, size in ((hz.SYMSYNC_REAL_F32, "f32", 1, 4), (hz.FMT_C64, "c64", 2, 8)):
            n = max(16384, (ONE_ROW_BYTES if rows == 1 else PUSH_BYTES) // (rows * size) // 64 * 64)
            moved = rows * n * size
            rot = max(2, -(-(CACHE + CACHE // 4) // moved))
            shape = (n,) if rows == 1 else (rows, n)
            ins = [torch.randn(shape + ((2,) if B == 2 else ()), dtype=torch.float32, device="cuda") for _ in range(rot)]
            # the yardstick: the library's copy of the same bytes
            flat = [a.view(-1).view(torch.complex64) for a in ins]
            dst = torch.empty_like(flat[0])
            copy_us = round(timed(lambda i: ctx.convert(dst, flat[i % rot]), args.steps, args.warmup), 1)
            del dst
            for hits in ("absent", "rare"):  # (both absent cases first: a planted word stays in the buffers)
                for P in (168, 8192):
                    planted = 0
                    if hits == "rare":
                        for k, a in enumerate(ins):
                            planted = plant(a.view(rows, -1) if rows > 1 else a.view(-1), B, P, 10 * k + P)
                    xs = [torch.view_as_complex(a) if B == 2 else a for a in ins]
                    words, maps = hz.sync_hypotheses(WORD, W, B, "rotate" if B == 2 else "invert")
                    bank = ctx.frame_sync(kind, W, words, maps, P, bits_per_symbol=B, thr=THR, rows=rows)
                    per_wave, tile, ring, form = bank.plan()
                    outs = bank.push(xs[0], None, CAP)
                    t = round(timed(lambda i: bank.push(xs[i % rot], None, CAP, out=outs), args.steps, args.warmup), 1)
                    counts = outs[3].cpu().numpy().view(np.uint32)
                    bank.close()
                    case = {"bank": "framesync", "kind": name, "B": B, "P": P, "hits": hits, "rows": rows, "n": n, "rows_per_wave": per_wave,
                            "ring_words": ring, "form": form, "rotation": rot, "input_bytes": moved, "us": t, "copy_us": copy_us,
                            "of_the_copy": round(t / copy_us, 3), "read_gbytes_per_s": round(moved / t / 1e3, 1),
                            "row_msymbols_per_s": round(n / t, 2), "planted_per_row": planted, "frames_last_push": int(counts.sum()),
                            "most_in_a_row": int(counts.max())}
                    print(f"framesync {name} B={B} P={P:4d} hits {hits:6s} R={rows:5d} n={n:8d} rows/wave={per_wave}: {t:9.1f} us = "
                          f"{case['of_the_copy']:.3f} of the copy's {copy_us:9.1f} us; reads {case['read_gbytes_per_s']:.1f} GB/s, one row "
                          f"{case['row_msymbols_per_s']:.2f} Msymbols/s; rotation {rot}; {planted} planted per row, {case['frames_last_push']} "
                          f"frames in the last push, {case['most_in_a_row']} at most in a row", flush=True)
                    results.append(case)
            del ins, flat, xs
    ctx.close()
    print(json.dumps({"framesync_time": results}))


if __name__ == "__main__":
    main()

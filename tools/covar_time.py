"""Times the covariance bank (include/hzsdr_covar.h) in us per push of 2^22 snapshots per row, median of 30, from HBM (a
rotation of four input blocks past the cache), for N in {4, 8, 16} x {u8, c64} x B in {4096, 2^20}, beside two
yardsticks in the same process:

  copy     the library's own device copy (hzsdr_convert c64 -> c64) over the case's algorithmic bytes -- N * B * sample
           size in, N^2 * 8 out, per block -- as (read + written) / 2 bytes copied.
  peak     the share of the float32 matrix peak (157 TFLOP/s nominal): `of_peak` counts 8 Np^2 B flops per block, Np = 16
           or 32 (the complex products of an Np-channel array); `issued_of_peak` counts what the kernel issues, 2 * 256 *
           tiles flops per snapshot (one accumulator tile up to 8 channels, three above).

Prints one line per case and one JSON line at the end.  No number here is a pass / fail threshold.

    python tools/covar_time.py [--steps 30] [--warmup 10] [--channels 4 8 16] [--blocks 4096 1048576]
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
hz = importlib.import_module("go-sdr_amd")

L = 1 << 22
ROT = 4
PEAK = 157.3e12


def timed(f, steps, warmup):
    for i in range(warmup):
        f(i)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for i, (a, b) in enumerate(ev):
        a.record()
        f(i)
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev])) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--channels", type=int, nargs="*", default=[4, 8, 16])
    ap.add_argument("--blocks", type=int, nargs="*", default=[4096, 1 << 20])
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = hz.Context(0, hz.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device="cuda").manual_seed(1)
    results = []
    for n in args.channels:
        for fmt, code, size in (("u8", hz.FMT_U8, 2), ("c64", hz.FMT_C64, 8)):
            if fmt == "u8":
                bufs = [torch.randint(0, 256, (n, L, 2), dtype=torch.uint8, device="cuda", generator=g) for _ in range(ROT)]
            else:
                bufs = [torch.complex(torch.randn((n, L), device="cuda", generator=g), torch.randn((n, L), device="cuda", generator=g))
                        for _ in range(ROT)]
            for b in args.blocks:
                bank = ctx.covariance(code, n, b)
                blocks = bank.blocks_for(L)
                alg = blocks * (n * b * size + n * n * 8)
                ncopy = alg // 16  # complex64 values copied: (read + written) / 2 bytes
                ca = [torch.empty(ncopy, dtype=torch.complex64, device="cuda") for _ in range(ROT)]
                cb = torch.empty(ncopy, dtype=torch.complex64, device="cuda")
                copy = round(timed(lambda i: ctx.convert(cb, ca[i % ROT]), args.steps, args.warmup), 1)
                del ca, cb
                out = torch.empty((blocks, n, n), dtype=torch.complex64, device="cuda")
                t = round(timed(lambda i: bank.push(bufs[i % ROT], out=out), args.steps, args.warmup), 1)
                seg, group, form = bank.plan()
                bank.close()
                np_, tiles = (16, 1) if n <= 8 else (32, 3)
                flops, issued = 8.0 * np_ * np_ * b * blocks, 2.0 * 256 * tiles * b * blocks
                case = {"fmt": fmt, "n": n, "block": b, "form": form, "us": t, "gsnapshots": round(L / t / 1e3, 2),
                        "gbytes_in": round(n * L * size / t / 1e3, 1), "of_peak": round(flops / (t * 1e-6) / PEAK, 4),
                        "issued_of_peak": round(issued / (t * 1e-6) / PEAK, 4), "copy": copy, "push_over_copy": round(t / copy, 2)}
                print(f"{fmt:3s} N={n:2d} B={b:7d}: {t:9.1f} us per 2^22 snapshots ({case['gsnapshots']} Gsnapshots/s, {case['gbytes_in']} GB/s in), "
                      f"{100 * case['of_peak']:.1f} % of the float32 matrix peak ({100 * case['issued_of_peak']:.1f} % issued); copy of the same "
                      f"bytes {copy} us (the push takes {case['push_over_copy']} x that)", flush=True)
                results.append(case)
                del out
            del bufs
    ctx.close()
    print(json.dumps({"covar_time": results}))


if __name__ == "__main__":
    main()

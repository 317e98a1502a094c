"""Times the channel bank (include/hzsdr_chanbank.h) in us per push of 2^24 input samples, median of 30, from HBM (a
rotation of four input buffers past the cache), for a list of (M, P, D) from u8 and from complex64 samples, beside two
yardsticks in the same process:

  peak     the fraction of the float32 matrix peak the push reaches: 8 M Mp flops per frame, 2^24 / D frames, against
           157 TFLOP/s nominal.
  copy     the library's own device copy (hzsdr_convert c64 -> c64) over the case's algorithmic bytes -- the input once,
           8 M bytes out per frame -- as (read + written) / 2 bytes copied.

Prints one line per case and one JSON line at the end.  No number here is a pass / fail threshold.

    python tools/chanbank_time.py [--steps 30] [--warmup 10] [--shapes 8,8,8 16,8,8 ...] [--layout channels]
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

L = 1 << 24
ROT = 4
SHAPES = ((8, 8, 8), (16, 8, 8), (64, 8, 64), (100, 8, 100), (128, 8, 64), (255, 4, 255))
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
    ap.add_argument("--shapes", nargs="*", default=None, help="M,P,D triples")
    ap.add_argument("--layout", default="channels", choices=["frames", "channels"])
    args = ap.parse_args()
    shapes = SHAPES if not args.shapes else tuple(tuple(int(v) for v in s.split(",")) for s in args.shapes)
    torch.cuda.set_device(0)
    ctx = hz.Context(0, hz.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device="cuda").manual_seed(1)
    inputs = {"u8": (hz.FMT_U8, 2, [torch.randint(0, 256, (L, 2), dtype=torch.uint8, device="cuda", generator=g) for _ in range(ROT)]),
              "c64": (hz.FMT_C64, 8, [torch.complex(torch.randn(L, device="cuda", generator=g), torch.randn(L, device="cuda", generator=g))
                                       for _ in range(ROT)])}
    results = []
    for m, p, d in shapes:
        taps = hz.channelizer_taps(m, p)
        for fmt, (code, size, bufs) in inputs.items():
            bank = ctx.channel_bank(code, m, taps, hop=d, layout=args.layout)
            frames = bank.frames_for(L)
            alg = L * size + 8 * m * frames
            ncopy = alg // 16  # complex64 values copied: (read + written) / 2 bytes
            ca = [torch.empty(ncopy, dtype=torch.complex64, device="cuda") for _ in range(ROT)]
            cb = torch.empty(ncopy, dtype=torch.complex64, device="cuda")
            copy = round(timed(lambda i: ctx.convert(cb, ca[i % ROT]), args.steps, args.warmup), 1)
            del ca, cb
            out = torch.empty((m, frames) if args.layout == "channels" else (frames, m), dtype=torch.complex64, device="cuda")
            # (each push starts a fresh stream: the frames of a 2^24-sample push, no carried state)
            t = round(timed(lambda i: (bank.reset(), bank.push(bufs[i % ROT], out=out)), args.steps, args.warmup), 1)
            tile, rows, form = bank.plan()
            bank.close()
            flops = 8.0 * m * (m + m % 2) * frames
            case = {"fmt": fmt, "m": m, "p": p, "d": d, "layout": args.layout, "tile": tile, "tile_rows": rows, "form": form, "us": t,
                    "gsamples": round(L / t / 1e3, 2), "tflops": round(flops / t / 1e6, 2), "of_peak": round(flops / (t * 1e-6) / PEAK, 4),
                    "copy": copy, "kernel_over_copy": round(t / copy, 2)}
            print(f"{fmt:3s} M={m:3d} P={p:2d} D={d:3d} T={tile}x{rows} form={form}: {t:10.1f} us per 2^24 samples ({case['gsamples']} Gsamples/s), "
                  f"{case['tflops']:6.2f} TFLOP/s = {100 * case['of_peak']:.1f} % of the float32 matrix peak; copy of the same bytes {copy} us "
                  f"(the push takes {case['kernel_over_copy']} x that)", flush=True)
            results.append(case)
            del out
    ctx.close()
    print(json.dumps({"chanbank_time": results}))


if __name__ == "__main__":
    main()

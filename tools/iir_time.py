"""Times the IIR bank (include/hzsdr_iir.h) in us per push, median of --steps, from HBM (a rotation of input and output
buffers whose bytes together pass the 256 MB cache): real float32 rows with R = 1, 100 and 8192, complex64 rows with
R = 256, each with S = 1 and S = 4 sections, beside one yardstick in the same process:

  copy     the library's own device copy (hzsdr_convert c64 -> c64) over the case's bytes, 4 (8) in + 4 (8) out per
           sample, as (read + written) / 2 bytes copied, through a rotation of the same size.

Prints one line per case, with the copy's time as a fraction of the kernel's, the samples per second of one row, and
one JSON line at the end.

    python tools/iir_time.py [--steps 20] [--warmup 5]
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

CACHE = 256 << 20
# (kind, rows, samples per row)
CASES = (("f32", 1, 1 << 20), ("f32", 100, 1 << 17), ("f32", 8192, 1 << 11), ("c64", 256, 1 << 16))
SECTIONS = (1, 4)


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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = hz.Context(0, hz.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device="cuda").manual_seed(1)
    results = []
    for kind, rows, n in CASES:
        cplx = kind == "c64"
        size = 8 if cplx else 4
        moved = 2 * rows * n * size  # bytes read + written
        rot = max(2, min(64, -(-(CACHE + CACHE // 4) // moved)))
        shape = (rows, n) if rows > 1 else (n,)
        ins = [torch.randn(shape, device="cuda", generator=g, dtype=torch.float32) for _ in range(rot)]
        if cplx:
            ins = [torch.complex(a, torch.randn(shape, device="cuda", generator=g, dtype=torch.float32)) for a in ins]
        outs = [torch.empty_like(a) for a in ins]
        ncopy = moved // 16  # complex64 values copied: (read + written) / 2 bytes
        ca = [torch.empty(ncopy, dtype=torch.complex64, device="cuda") for _ in range(rot)]
        cb = [torch.empty(ncopy, dtype=torch.complex64, device="cuda") for _ in range(rot)]
        copy = round(timed(lambda i: ctx.convert(cb[i % rot], ca[i % rot]), args.steps, args.warmup), 1)
        del ca, cb
        for s in SECTIONS:
            sec = np.concatenate([hz.lowpass(3000.0, 0.8, 48e3), hz.dc_block(0.99), hz.notch(5000.0, 6.0, 48e3), hz.deemphasis(75e-6, 48e3)][:s])
            bank = ctx.iir_bank(hz.FMT_C64 if cplx else hz.IIR_REAL_F32, sec, rows=rows)
            per_wave, tile, form = bank.plan()
            # (the stream goes on from push to push: the state is carried, as in use)
            t = round(timed(lambda i: bank.push(ins[i % rot], out=outs[i % rot]), args.steps, args.warmup), 1)
            bank.close()
            case = {"kind": kind, "rows": rows, "n": n, "sections": s, "rows_per_wave": per_wave, "tile": tile, "form": form, "rotation": rot,
                    "rotation_bytes": rot * moved, "us": t, "copy": copy, "copy_over_kernel": round(copy / t, 4),
                    "row_msamples_per_s": round(n / t, 2), "gbytes_per_s": round(moved / t / 1e3, 1)}
            print(f"{kind} R={rows:5d} n={n:8d} S={s} rows/wave={per_wave} T={tile}: {t:10.1f} us, copy of the same bytes {copy:8.1f} us "
                  f"({case['copy_over_kernel']:.3f} of the kernel's time), {case['gbytes_per_s']:7.1f} GB/s, one row {case['row_msamples_per_s']:.1f} Msamples/s; "
                  f"rotation {rot} x {moved >> 20} MiB", flush=True)
            results.append(case)
        del ins, outs
    ctx.close()
    print(json.dumps({"iir_time": results}))


if __name__ == "__main__":
    main()

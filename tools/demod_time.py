"""Times the demodulator bank (include/hzsdr_demod.h) in us per 2^24 input samples, median of 30, from HBM (a rotation
of four input buffers past the cache): FM with (Q, D) = (1, 1), the bare detector, and (64, 5), over 256 rows of 2^16
complex64 samples, beside one yardstick in the same process:

  copy     the library's own device copy (hzsdr_convert c64 -> c64) over the case's algorithmic bytes, 8 in + 4 / D out
           per input sample, as (read + written) / 2 bytes copied.

Prints one line per case, with the copy's time as a fraction of the kernel's, and one JSON line at the end.

    python tools/demod_time.py [--steps 30] [--warmup 10] [--all-modes]
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
ROWS = 256
SHAPES = ((1, 1), (64, 5))
MODES = {"fm": hz.DEMOD_FM, "phase": hz.DEMOD_PHASE, "envelope": hz.DEMOD_ENVELOPE, "power": hz.DEMOD_POWER}


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
    ap.add_argument("--all-modes", action="store_true", help="phase, envelope and power beside FM")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = hz.Context(0, hz.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device="cuda").manual_seed(1)
    bufs = [torch.complex(torch.randn(L, device="cuda", generator=g), torch.randn(L, device="cuda", generator=g)).view(ROWS, L // ROWS)
            for _ in range(ROT)]
    results = []
    for q, down in SHAPES:
        taps = np.hamming(q + 2)[1:-1].astype(np.float32)
        taps /= taps.sum()
        alg = L * 8 + 4 * (L // down)
        ncopy = alg // 16  # complex64 values copied: (read + written) / 2 bytes
        ca = [torch.empty(ncopy, dtype=torch.complex64, device="cuda") for _ in range(ROT)]
        cb = torch.empty(ncopy, dtype=torch.complex64, device="cuda")
        copy = round(timed(lambda i: ctx.convert(cb, ca[i % ROT]), args.steps, args.warmup), 1)
        del ca, cb
        for name, mode in MODES.items():
            if name != "fm" and not args.all_modes:
                continue
            dm = ctx.demodulator(hz.FMT_C64, mode, taps, down, streams=ROWS)
            n = L // ROWS
            out = torch.empty((ROWS, dm.outputs_for(n)), dtype=torch.float32, device="cuda")
            # (each push starts a fresh stream: the outputs of a 2^24-sample push, no carried state)
            t = round(timed(lambda i: (dm.reset(), dm.push(bufs[i % ROT], out=out)), args.steps, args.warmup), 1)
            tile, form = dm.plan()
            dm.close()
            case = {"mode": name, "q": q, "down": down, "rows": ROWS, "tile": tile, "form": form, "bytes_per_sample": round(alg / L, 2),
                    "us": t, "copy": copy, "copy_over_kernel": round(copy / t, 3)}
            print(f"{name:8s} Q={q:4d} D={down:2d} rows={ROWS} T={tile} form={form}: {t:9.1f} us per 2^24 samples, copy of the same bytes "
                  f"{copy} us ({case['bytes_per_sample']} B per sample): the copy takes {case['copy_over_kernel']:.2f} of the kernel's time",
                  flush=True)
            results.append(case)
            del out
    ctx.close()
    print(json.dumps({"demod_time": results}))


if __name__ == "__main__":
    main()

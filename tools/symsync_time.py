"""Times the symbol-timing recovery bank (include/hzsdr_symsync.h) in us per push, median of --steps, from HBM (a
rotation of input and output buffers whose bytes together pass the 256 MB cache): real float32 and complex64 rows with
R = 1, 100 and 8192 at 5 samples per symbol, beside two yardsticks in the same process over the same rows:

  iir      the IIR bank (include/hzsdr_iir.h) with S = 2 sections over the same input buffers: the same shape of kernel
           (one wave per G rows, lane = row, tiles of 256 samples through LDS), a sequential walk of 4 (8 for complex
           rows) dependent fused steps per sample against this bank's longer step;
  copy     the library's own device copy (hzsdr_convert c64 -> c64) over the case's input bytes read and half as many
           written (the symbols), as (read + written) / 2 bytes copied, through a rotation of the same size.

The rows are a raised-cosine symbol stream (every row a rotation of one stream), so that the loop is in lock as in use.
Prints one line per case and one JSON line at the end.

    python tools/symsync_time.py [--steps 20] [--warmup 5]
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
SPS = 5.0
# (kind, rows, samples per row)
CASES = (("f32", 1, 1 << 20), ("f32", 100, 1 << 17), ("f32", 8192, 1 << 11), ("c64", 1, 1 << 20), ("c64", 100, 1 << 17), ("c64", 8192, 1 << 11))


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


def stream(n, cplx, seed):
    """n samples of +-1 (or (+-1 +- i) / sqrt 2) symbols through a raised cosine of roll-off 0.5 at SPS samples per symbol"""
    rng = np.random.default_rng(seed)
    count = int(n / SPS) + 20
    a = 2.0 * rng.integers(0, 2, count) - 1.0
    if cplx:
        a = (a + 1j * (2.0 * rng.integers(0, 2, count) - 1.0)) / np.sqrt(2.0)
    t = (np.arange(n) + 0.3) / SPS + 9.0
    k0 = np.floor(t).astype(np.int64)
    x = np.zeros(n, a.dtype)
    for d in range(-8, 10):
        u = t - (k0 + d)
        den = 1.0 - u * u
        den = np.where(np.abs(den) < 1e-9, 1.0, den)
        x += a[k0 + d] * np.sinc(u) * np.cos(np.pi * 0.5 * u) / den
    return x.astype(np.complex64 if cplx else np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = hz.Context(0, hz.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    params = np.array([SPS, 0.01, *hz.loop_gains(SPS)], np.float32)
    results = []
    for kind, rows, n in CASES:
        cplx = kind == "c64"
        size = 8 if cplx else 4
        read = rows * n * size
        moved = read + read // int(SPS)  # bytes read + symbols written
        bank = ctx.symbol_sync(hz.FMT_C64 if cplx else hz.SYMSYNC_REAL_F32, params, rows=rows)
        per_wave, tile, form = bank.plan()
        bound = bank.max_symbols(n)
        # the rotation by the bytes of this bank's own buffers: an input and a destination of `bound` symbols per row
        # (the IIR bank's destinations below are as large as its inputs: its rotation is larger still)
        rotated = read + rows * bound * size
        rot = max(2, min(96, -(-(CACHE + CACHE // 4) // rotated)))
        assert rot * rotated > CACHE, "the rotation does not pass the cache"
        one = torch.from_numpy(stream(n + rows, cplx, 1)).cuda()
        base = torch.stack([one[r:r + n] for r in range(rows)]) if rows > 1 else one[:n].clone()
        ins = [base.clone() for _ in range(rot)]
        outs = [torch.empty((rows, bound) if rows > 1 else (bound,), dtype=base.dtype, device="cuda") for _ in range(rot)]
        counts = torch.zeros(rows, dtype=torch.int32, device="cuda")
        # (the stream goes on from push to push: the state is carried, as in use)
        t = round(timed(lambda i: bank.push(ins[i % rot], out=outs[i % rot], counts=counts), args.steps, args.warmup), 1)
        symbols = int(counts.max())
        bank.close()
        sec = np.concatenate([hz.lowpass(3000.0, 0.8, 48e3), hz.dc_block(0.99)])
        iir = ctx.iir_bank(hz.FMT_C64 if cplx else hz.IIR_REAL_F32, sec, rows=rows)
        fouts = [torch.empty_like(a) for a in ins]
        ti = round(timed(lambda i: iir.push(ins[i % rot], out=fouts[i % rot]), args.steps, args.warmup), 1)
        iir.close()
        del fouts, outs
        ncopy = max(1, moved // 16)  # complex64 values copied: (read + written) / 2 bytes
        ca = [torch.empty(ncopy, dtype=torch.complex64, device="cuda") for _ in range(rot)]
        cb = [torch.empty(ncopy, dtype=torch.complex64, device="cuda") for _ in range(rot)]
        copy = round(timed(lambda i: ctx.convert(cb[i % rot], ca[i % rot]), args.steps, args.warmup), 1)
        del ca, cb, ins
        case = {"kind": kind, "rows": rows, "n": n, "sps": SPS, "rows_per_wave": per_wave, "tile": tile, "form": form, "rotation": rot, "rotation_bytes": rot * rotated,
                "symbols_per_row": symbols, "bound": bound, "us": t, "iir_s2_us": ti, "copy_us": copy, "over_iir": round(t / ti, 3),
                "copy_over_kernel": round(copy / t, 4), "row_msamples_per_s": round(n / t, 2), "ns_per_sample_and_wave": round(t * 1e3 / n, 2),
                "gbytes_per_s": round(moved / t / 1e3, 1)}
        print(f"{kind} R={rows:5d} n={n:8d} rows/wave={per_wave} T={tile}: {t:10.1f} us ({symbols} symbols per row), IIR S=2 {ti:10.1f} us "
              f"({case['over_iir']:.2f} x), copy {copy:8.1f} us, one row {case['row_msamples_per_s']:.1f} Msamples/s, "
              f"{case['ns_per_sample_and_wave']:.2f} ns per sample of a wave, {case['gbytes_per_s']:7.1f} GB/s; rotation {rot} x {rotated / 2 ** 20:.1f} MiB", flush=True)
        results.append(case)
    ctx.close()
    print(json.dumps({"symsync_time": results}))


if __name__ == "__main__":
    main()

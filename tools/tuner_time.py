"""Times the tuner bank (include/hzsdr_tuner.h) in us per push of 2^24 input samples, median of 30, from HBM (a rotation
of four input buffers past the cache): K = 4, 16, 64 and 256 tuners at (Q, D) = (256, 32) and (1024, 256), u8 and
complex64 samples, beside three yardsticks in the same process:

  peak     the fraction of the float32 matrix peak the push reaches: 8 K Qp flops per output column, 2^24 / D columns,
           against 157 TFLOP/s nominal.
  copy     the library's own device copy (hzsdr_convert c64 -> c64) over the case's algorithmic bytes -- the input once,
           K rows of 8 / D bytes out per input sample -- as (read + written) / 2 bytes copied.
  chains   K separate chain().shift(f).fir_decimate(h, D) objects run one after the other on the same input: what the
           library offered before the bank.

Prints one line per case and one JSON line at the end.  No number here is a pass / fail threshold.

    python tools/tuner_time.py [--steps 30] [--warmup 10] [--no-chains]
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
RATE = 20_000_000
TUNERS = (4, 16, 64, 256)
SHAPES = ((256, 32), (1024, 256))
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


def prototype(q, down):
    """a windowed-sinc low-pass at half the output rate"""
    t = np.arange(q) - (q - 1) / 2
    h = np.sinc(t / down) * np.blackman(q + 2)[1:-1]
    return (h / h.sum()).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-chains", action="store_true", help="skip the K separate chains")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = hz.Context(0, hz.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device="cuda").manual_seed(1)
    inputs = {"c64": (hz.FMT_C64, 8, [torch.complex(torch.randn(L, device="cuda", generator=g), torch.randn(L, device="cuda", generator=g))
                                       for _ in range(ROT)]),
              "u8": (hz.FMT_U8, 2, [torch.randint(0, 256, (L, 2), dtype=torch.uint8, device="cuda", generator=g) for _ in range(ROT)])}
    rng = np.random.default_rng(3)
    results = []
    for q, down in SHAPES:
        taps = prototype(q, down)
        for fmt, (code, size, bufs) in inputs.items():
            for k in TUNERS:
                freqs = rng.uniform(-0.45, 0.45, k) * RATE
                words = [hz.tuner_word(f, RATE) for f in freqs]
                alg = L * size + 8 * k * (L // down)
                ncopy = alg // 16  # complex64 values copied: (read + written) / 2 bytes
                ca = [torch.empty(ncopy, dtype=torch.complex64, device="cuda") for _ in range(ROT)]
                cb = torch.empty(ncopy, dtype=torch.complex64, device="cuda")
                copy = round(timed(lambda i: ctx.convert(cb, ca[i % ROT]), args.steps, args.warmup), 1)
                del ca, cb
                bank = ctx.tuner_bank(code, words, taps, down)
                out = torch.empty((k, bank.outputs_for(L)), dtype=torch.complex64, device="cuda")
                # (each push starts a fresh stream: the outputs of a 2^24-sample push, no carried state)
                t = round(timed(lambda i: (bank.reset(), bank.push(bufs[i % ROT], out=out)), args.steps, args.warmup), 1)
                tile, rows, form = bank.plan()
                bank.close()
                flops = 8.0 * k * (q + q % 2) * (L // down)
                case = {"fmt": fmt, "k": k, "q": q, "down": down, "tile": tile, "tile_rows": rows, "form": form, "us": t,
                        "tflops": round(flops / t / 1e6, 2), "of_peak": round(flops / (t * 1e-6) / PEAK, 4), "copy": copy,
                        "copy_over_kernel": round(copy / t, 3)}
                if not args.no_chains:
                    chains = [ctx.chain(code, RATE).shift(-float(f)).fir_decimate(taps, down) for f in freqs]
                    one = torch.empty(L // down + 8, dtype=torch.complex64, device="cuda")
                    steps = max(3, args.steps // (1 + k // 16))
                    case["chains"] = round(timed(lambda i: [c.run(bufs[i % ROT], one) for c in chains], steps, min(args.warmup, 2)), 1)
                    case["chains_over_kernel"] = round(case["chains"] / t, 2)
                    for c in chains:
                        c.close()
                    del one
                print(f"{fmt:3s} K={k:3d} Q={q:4d} D={down:3d} T={tile}x{rows} form={form}: {t:10.1f} us per push, {case['tflops']:6.2f} TFLOP/s = "
                      f"{100 * case['of_peak']:.1f} % of the float32 matrix peak; copy of the same bytes {copy} us "
                      f"({case['copy_over_kernel']:.3f} of the kernel's time)"
                      + (f"; {k} chains {case['chains']} us ({case['chains_over_kernel']} x)" if "chains" in case else ""), flush=True)
                results.append(case)
                del out
    ctx.close()
    print(json.dumps({"tuner_time": results}))


if __name__ == "__main__":
    main()

"""Times the polyphase synthesis bank (include/hzsdr_synthesizer.h) in us per 2^24 output samples, from HBM (a rotation
of four input buffers), for (M, P, D) in {(256, 8, 256), (256, 8, 128), (1024, 8, 1024), (1024, 8, 512),
(4096, 4, 4096), (4096, 4, 2048)}, c64 and u8 destinations, both input layouts, beside two yardsticks in the same
process:

  copy     the library's own copy (hzsdr_convert c64 -> c64) over the case's algorithmic bytes,
           8 M per frame read + D sizeof(dst sample) per frame written, as (read + written) / 2 bytes copied;
  unfused  a transposing copy for the channel-major layout, hzsdr_fft_plan_batch backward, the tap product and
           overlap-add in torch (one gather, product and add per hop-sized piece of the prototype), and hzsdr_convert
           for the u8 destination.

Prints one line per case and one JSON line at the end.

    python tools/synthesizer_time.py [--steps 30] [--warmup 10]
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

N_OUT = 1 << 24
ROT = 4


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
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = hz.Context(0, hz.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    gen = torch.Generator(device="cuda").manual_seed(1)
    results = []
    for m, p, hop in ((256, 8, 256), (256, 8, 128), (1024, 8, 1024), (1024, 8, 512), (4096, 4, 4096), (4096, 4, 2048)):
        L = m * p
        F = N_OUT // hop
        # DC-gain-1 taps scaled so that the u8 destination stays in range (a standard deviation of about 0.15)
        taps = (hz.channelizer_taps(m, p).astype(np.float64) * 0.15 * np.sqrt(3.0 * hop)).astype(np.float32)
        td = torch.from_numpy(taps).cuda()
        fm = [torch.complex(torch.rand((F, m), device="cuda", generator=gen) * 2 - 1,
                            torch.rand((F, m), device="cuda", generator=gen) * 2 - 1) for _ in range(ROT)]
        freq = torch.empty(F * m, dtype=torch.complex64, device="cuda")
        w = torch.empty(F * m, dtype=torch.complex64, device="cuda")
        plans = [ctx.fft_plan(w, b.view(-1), hz.FFT_BACKWARD, batch=F) for b in fm] + [ctx.fft_plan(w, freq, hz.FFT_BACKWARD, batch=F)]
        acc = torch.empty((F - 1) * hop + L, dtype=torch.complex64, device="cuda")
        phases = m // hop
        jj = torch.arange(F, device="cuda")
        for layout in ("frames", "channels"):
            bufs = fm if layout == "frames" else [b.T.contiguous() for b in fm]
            for fmt in ("c64", "u8"):
                code = hz.FMT_U8 if fmt == "u8" else hz.FMT_C64
                dsize = 2 if fmt == "u8" else 8
                alg = F * (8 * m + hop * dsize)
                ncopy = alg // 16  # complex64 values copied: (read + written) / 2 bytes
                ca = [torch.empty(ncopy, dtype=torch.complex64, device="cuda") for _ in range(ROT)]
                cb = torch.empty(ncopy, dtype=torch.complex64, device="cuda")
                copy = round(timed(lambda i: ctx.convert(cb, ca[i % ROT]), args.steps, args.warmup), 1)
                del ca, cb
                out = torch.empty((N_OUT, 2), dtype=torch.uint8, device="cuda") if fmt == "u8" else \
                    torch.empty(N_OUT, dtype=torch.complex64, device="cuda")
                sy = ctx.synthesizer(code, m, taps, hop=hop, layout=layout)
                # (each push starts a fresh stream: the 2^24 samples of one push, no carried state)
                fused = round(timed(lambda i: (sy.reset(), sy.push(bufs[i % ROT], out=out)), args.steps, args.warmup), 1)
                sy.close()

                def unfused(i):
                    if layout == "channels":
                        freq.view(F, m).copy_(bufs[i % ROT].T)
                        plans[ROT].transform()
                    else:
                        plans[i % ROT].transform()
                    acc.zero_()
                    wv = w.view(F, phases, hop)
                    rows = acc[:(F - 1) * hop + L].view(-1, hop)
                    for c in range(L // hop):  # piece c of the prototype: frame j lands on hop-block j + c
                        rows[c:c + F] += wv[jj, (jj + c) % phases] * td[c * hop:(c + 1) * hop]
                    if fmt == "u8":
                        ctx.convert(out, acc[:N_OUT])
                    return acc
                slow = round(timed(unfused, max(3, args.steps // 5), max(2, args.warmup // 5)), 1)
                case = {"m": m, "p": p, "hop": hop, "dst": fmt, "layout": layout, "frames": F,
                        "bytes_per_sample": round(alg / N_OUT, 2), "fused": fused, "copy": copy, "unfused": slow,
                        "fused_over_copy": round(fused / copy, 2)}
                print(f"M={m:5d} P={p} hop={hop:5d} {fmt:4s} {layout:8s}: fused {fused:8.1f} us, copy of the same bytes "
                      f"{copy:7.1f} us, unfused {slow:9.1f} us per 2^24 samples ({case['bytes_per_sample']} B per sample)",
                      flush=True)
                results.append(case)
                del out
            del bufs
        for pl in plans:
            pl.close()
        del fm, freq, w, acc
    ctx.close()
    print(json.dumps({"synthesizer_time": results}))


if __name__ == "__main__":
    main()

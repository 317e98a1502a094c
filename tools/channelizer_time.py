"""Times the polyphase channelizer (include/hzsdr_channelizer.h) in us per 2^24 input samples, from HBM (a rotation of
four input buffers), for (M, P) in {(256, 8), (1024, 8), (4096, 4)}, hop in {M, M/2}, u8 and c64 sources, both output
layouts, beside two yardsticks in the same process:

  copy     the library's own copy (hzsdr_convert c64 -> c64) over the case's algorithmic bytes,
           2^24 sizeof(src sample) read + 8 M frames written, as (read + written) / 2 bytes copied;
  unfused  hzsdr_convert, a torch gather of the frames times the taps summed over p (and the rotation's roll),
           hzsdr_fft_plan_batch, and a transposing copy for the channel-major layout.

Prints one line per case and one JSON line at the end.

    python tools/channelizer_time.py [--steps 30] [--warmup 10]
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
    g = torch.Generator(device="cuda").manual_seed(1)
    srcs = {
        "u8": [torch.randint(0, 256, (L, 2), dtype=torch.uint8, device="cuda", generator=g) for _ in range(ROT)],
        "c64": [torch.complex(torch.randn(L, device="cuda", generator=g), torch.randn(L, device="cuda", generator=g))
                for _ in range(ROT)],
    }
    results = []
    for m, p in ((256, 8), (1024, 8), (4096, 4)):
        taps = hz.channelizer_taps(m, p)
        td = torch.from_numpy(taps).cuda().view(p, m)
        for hop in (m, m // 2):
            F = (L - p * m) // hop + 1
            conv = torch.empty(L, dtype=torch.complex64, device="cuda")
            iq = torch.empty(F * m, dtype=torch.complex64, device="cuda")
            freq = torch.empty_like(iq)
            plan = ctx.fft_plan(iq, freq, hz.FFT_FORWARD, batch=F)
            # u_j[r] = v_j[(r - j hop) mod M]
            roll = ((torch.arange(m, device="cuda")[None, :] - (torch.arange(F, device="cuda") * hop)[:, None]) % m)
            for fmt, bufs in srcs.items():
                code = hz.FMT_U8 if fmt == "u8" else hz.FMT_C64
                ssize = 2 if fmt == "u8" else 8
                alg = L * ssize + 8 * m * F
                ncopy = alg // 16  # complex64 values copied: (read + written) / 2 bytes
                ca = [torch.empty(ncopy, dtype=torch.complex64, device="cuda") for _ in range(ROT)]
                cb = torch.empty(ncopy, dtype=torch.complex64, device="cuda")
                copy = round(timed(lambda i: ctx.convert(cb, ca[i % ROT]), args.steps, args.warmup), 1)
                del ca, cb
                for layout in ("frames", "channels"):
                    out = torch.empty((F, m) if layout == "frames" else (m, F), dtype=torch.complex64, device="cuda")
                    ch = ctx.channelizer(code, m, taps, hop=hop, layout=layout)
                    # (each push starts a fresh stream: the frames of a 2^24-sample push, no carried state)
                    fused = round(timed(lambda i: (ch.reset(), ch.push(bufs[i % ROT], out=out)), args.steps, args.warmup), 1)
                    ch.close()

                    def unfused(i):
                        x = bufs[i % ROT]
                        if fmt == "u8":
                            ctx.convert(conv, x)
                            c = conv
                        else:
                            c = x
                        v = (c.as_strided((F, p, m), (hop, m, 1)) * td).sum(1)
                        if hop != m:
                            v = torch.gather(v.view(torch.float64), 1, roll).view(torch.complex64)
                        iq.view(F, m).copy_(v)
                        plan.transform()
                        if layout == "channels":
                            out.copy_(freq.view(F, m).T)
                        return freq
                    slow = round(timed(unfused, max(3, args.steps // 5), max(2, args.warmup // 5)), 1)
                    case = {"m": m, "p": p, "hop": hop, "src": fmt, "layout": layout, "frames": F,
                            "bytes_per_sample": round(alg / L, 2), "fused": fused, "copy": copy, "unfused": slow,
                            "fused_over_copy": round(fused / copy, 2)}
                    print(f"M={m:5d} P={p} hop={hop:5d} {fmt:4s} {layout:8s}: fused {fused:8.1f} us, copy of the same bytes "
                          f"{copy:7.1f} us, unfused {slow:9.1f} us per 2^24 samples ({case['bytes_per_sample']} B per sample)",
                          flush=True)
                    results.append(case)
                    del out
            plan.close()
            del iq, freq, conv, roll
    ctx.close()
    print(json.dumps({"channelizer_time": results}))


if __name__ == "__main__":
    main()

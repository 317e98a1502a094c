"""Times the fused power spectrum (include/hzsdr_spectrum.h) in us per 2^24 input samples, from HBM (a rotation of
four input buffers), for N in {1024, 4096}, hop in {N, N/2}, K = 16, u8 and c64 sources: both kernel forms, the form
auto selects, and the unfused baseline in the same process (hzsdr_convert + hzsdr_fft_plan_batch + torch window,
|X|^2 and sum over K).  Prints one line per case and one JSON line at the end.

    python tools/spectrum_time.py [--steps 50] [--warmup 20]
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
sp = importlib.import_module("go-sdr_amd.spectrum")

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
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = hz.Context(0, hz.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device="cuda").manual_seed(1)
    srcs = {
        "u8": [torch.randint(0, 256, (L, 2), dtype=torch.uint8, device="cuda", generator=g) for _ in range(ROT)],
        "c64": [torch.complex(torch.randn(L, device="cuda", generator=g), torch.randn(L, device="cuda", generator=g))
                for _ in range(ROT)],
    }
    K, results = 16, []
    for n in (1024, 4096):
        w = sp.hann(n)
        wd = torch.from_numpy(w).cuda()
        for hop in (n, n // 2):
            F = (L - n) // hop + 1
            rows = F // K
            out = torch.empty((rows + 1, n), dtype=torch.float32, device="cuda")
            # the unfused baseline's buffers: converted samples, framed + windowed frames, their spectra
            conv = torch.empty(L, dtype=torch.complex64, device="cuda")
            iq = torch.empty(rows * K * n, dtype=torch.complex64, device="cuda")
            freq = torch.empty_like(iq)
            plan = ctx.fft_plan(iq, freq, hz.FFT_FORWARD, batch=rows * K)
            scale = sp.spectrum_scale("power", n, K, w)
            for fmt, bufs in srcs.items():
                code = hz.FMT_U8 if fmt == "u8" else hz.FMT_C64
                case = {"n": n, "hop": hop, "K": K, "src": fmt, "rows": rows}
                for name, form in (("row_walk", hz.SPECTRUM_FORM_ROW_WALK), ("frame_parallel", hz.SPECTRUM_FORM_FRAME_PARALLEL),
                                   ("auto", hz.SPECTRUM_FORM_AUTO)):
                    s = ctx.spectrum(code, n, hop=hop, avg=K, window=w, scale="power")
                    s.options(form)
                    # (each push starts a fresh stream: the rows of a 2^24-sample push, no carried state)
                    case[name] = round(timed(lambda i: (s.reset(), s.push(bufs[i % ROT], out=out)), args.steps, args.warmup), 1)
                    if form == hz.SPECTRUM_FORM_AUTO:
                        case["auto_form"] = "row_walk" if s.last_form() == hz.SPECTRUM_FORM_ROW_WALK else "frame_parallel"
                    s.close()

                def unfused(i):
                    x = bufs[i % ROT]
                    if fmt == "u8":
                        ctx.convert(conv, x)
                        c = conv
                    else:
                        c = x
                    frames = c.as_strided((rows * K, n), (hop, 1))
                    torch.mul(frames, wd, out=iq.view(rows * K, n))
                    plan.transform()
                    p = torch.view_as_real(freq).square().sum(-1)
                    return p.view(rows, K, n).sum(1).mul_(scale)
                case["unfused"] = round(timed(unfused, args.steps, args.warmup), 1)
                case["fused_over_unfused"] = round(min(case["row_walk"], case["frame_parallel"]) / case["unfused"], 3)
                print(f"N={n:5d} hop={hop:5d} K={K} {fmt:4s} rows={rows:5d}: row walk {case['row_walk']:8.1f} us, "
                      f"frame-parallel {case['frame_parallel']:8.1f} us, auto ({case['auto_form']}) {case['auto']:8.1f} us, "
                      f"unfused {case['unfused']:8.1f} us per 2^24 samples", flush=True)
                results.append(case)
            plan.close()
            del iq, freq, conv
    ctx.close()
    print(json.dumps({"spectrum_time": results}))


if __name__ == "__main__":
    main()

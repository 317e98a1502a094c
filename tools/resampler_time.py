"""Times the polyphase resampler (include/hzsdr_resampler.h) in us per 2^24 input samples, median of 30, from HBM (a
rotation of four input buffers), for (U, D, Q) in {(1, 4, 32), (3, 2, 16), (160, 147, 24), (2, 5, 24), (1, 1, 64)},
c64 and u8 sources, one stream of 2^24 samples and 256 rows of 2^16, beside two yardsticks in the same process:

  copy     the library's own copy (hzsdr_convert c64 -> c64) over the case's algorithmic bytes,
           sizeof(src sample) + 8 U / D per input sample, as (read + written) / 2 bytes copied;
  unfused  hzsdr_convert, a zero-stuffed copy of the stream, and torch's conv1d with stride D over its real and
           imaginary parts.  Where the zero-stuffed stream of 2^24 samples would not be reasonable (U above 4) the
           route runs on 2^24 / 64 samples and its time is scaled; the case says so.

Prints one line per case and one JSON line at the end.

    python tools/resampler_time.py [--steps 30] [--warmup 10] [--only-fused]
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
SHAPES = ((1, 4, 32), (3, 2, 16), (160, 147, 24), (2, 5, 24), (1, 1, 64))


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
    ap.add_argument("--only-fused", action="store_true", help="skip the two yardsticks (profiling runs)")
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
    for up, down, q in SHAPES:
        taps = hz.resampler_taps(up, down, q)
        for fmt, bufs in srcs.items():
            code = hz.FMT_U8 if fmt == "u8" else hz.FMT_C64
            ssize = 2 if fmt == "u8" else 8
            alg = L * ssize + 8 * (L * up // down)
            copy = slow = None
            scaled = 1
            if not args.only_fused:
                ncopy = alg // 16  # complex64 values copied: (read + written) / 2 bytes
                ca = [torch.empty(ncopy, dtype=torch.complex64, device="cuda") for _ in range(ROT)]
                cb = torch.empty(ncopy, dtype=torch.complex64, device="cuda")
                copy = round(timed(lambda i: ctx.convert(cb, ca[i % ROT]), args.steps, args.warmup), 1)
                del ca, cb
                # the unfused route: convert, zero-stuff, conv1d with stride D over (re, im) as two rows
                scaled = 1 if up <= 4 else 64
                nu = L // scaled
                conv = torch.empty(nu, dtype=torch.complex64, device="cuda")
                w = torch.from_numpy(taps[::-1].copy()).cuda().view(1, 1, -1)
                stuffed = torch.zeros((2, 1, len(taps) - 1 + nu * up), dtype=torch.float32, device="cuda")

                def unfused(i):
                    x = bufs[i % ROT][:nu]
                    if fmt == "u8":
                        ctx.convert(conv, x)
                        c = conv
                    else:
                        c = x
                    stuffed[:, 0, len(taps) - 1::up] = torch.view_as_real(c).T
                    return torch.nn.functional.conv1d(stuffed, w, stride=down)
                try:
                    slow = round(timed(unfused, max(3, args.steps // 10), 2) * scaled, 1)
                except RuntimeError as e:  # (a route torch cannot run is reported, not hidden)
                    print(f"unfused route failed for U={up} D={down}: {str(e).splitlines()[0]}", flush=True)
                del conv, stuffed, w
            for rows in (1, ROWS):
                n = L // rows
                rs = ctx.resampler(code, up, down, taps, streams=rows)
                count = rs.outputs_for(n)
                out = torch.empty((count,) if rows == 1 else (rows, count), dtype=torch.complex64, device="cuda")
                views = [b if rows == 1 else b.view((rows, n) + tuple(b.shape[1:])) for b in bufs]
                # (each push starts a fresh stream: the outputs of a 2^24-sample push, no carried state)
                fused = round(timed(lambda i: (rs.reset(), rs.push(views[i % ROT], out=out)), args.steps, args.warmup), 1)
                tile, form = rs.plan()
                rs.close()
                case = {"up": up, "down": down, "q": q, "src": fmt, "rows": rows, "tile": tile, "form": form,
                        "bytes_per_sample": round(alg / L, 2), "fused": fused, "copy": copy, "unfused": slow, "unfused_scaled_from": L // scaled,
                        "fused_over_copy": round(fused / copy, 2) if copy else None}
                print(f"U={up:4d} D={down:4d} Q={q:3d} {fmt:4s} rows={rows:4d} T={tile} form={form}: fused {fused:9.1f} us, copy of the same "
                      f"bytes {copy} us, unfused {slow} us{' (scaled from 2^24 / %d samples)' % scaled if scaled > 1 else ''} per 2^24 samples "
                      f"({case['bytes_per_sample']} B per sample)", flush=True)
                results.append(case)
                del out
    ctx.close()
    print(json.dumps({"resampler_time": results}))


if __name__ == "__main__":
    main()

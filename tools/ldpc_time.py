"""Times the LDPC decoder bank (include/hzsdr_ldpc.h) in us per call, median of --steps after --warmup, and writes the
lines to --out (profiles/ldpc_time.txt): the (3, 6) regular code of n = 2048 (rate 1/2, D = 1024, every variable
received) and the (3, 4) regular code of n = 16384 (k = 4096; N = 8192 received, the other half punctured, D = 4096:
the largest frame, its tables read through the cache), each at ONE frame and at 8192 rows x 4 frames, and each at a noise
level where frames converge early and at one where they run to max_iters = 20.  Soft input, scale 16, a = 12, beta = 0.
Every frame is one of 32 noisy copies of the all-zero codeword (BPSK, -1 + sigma * noise): the code is linear and the
decision symmetric, so the work is that of any codeword.  The many-frame inputs are put together on the device.

Per case: us per call, the iterations the frames ran (mean, least, most, from info), us per frame and iteration -- for
one frame the latency of an iteration, for many frames the call over all frames' iterations -- and Gbit/s of decoded data
(frames * D / us), beside the Viterbi bank's 10.7 Gbit/s (K = 7, D = 1024, 65536 frames) from its header, the family's
yardstick.  Beside them, counted from the code: the LDS accesses per edge and iteration.

    python tools/ldpc_time.py [--steps 30] [--warmup 5] [--out profiles/ldpc_time.txt]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
hz = importlib.import_module("go-sdr_amd")
from symsync_time import timed  # noqa: E402

DISTINCT, MAX_ITERS, SCALE = 32, 20, 16.0
VITERBI_GBIT = 10.7
# name -> (n, dv, dc, N, D, sigma early, sigma late)
CODES = {"n2048": (2048, 3, 6, 2048, 1024, 0.6, 1.3), "n16384": (16384, 3, 4, 8192, 4096, 0.45, 1.3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ldpc_time.txt"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = hz.Context(0, hz.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    lines, results = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"median of {args.steps} calls after {args.warmup}; max_iters {MAX_ITERS}, scale {SCALE}, a = 12, beta = 0; the Viterbi bank decodes {VITERBI_GBIT} Gbit/s")
    for name, (n, dv, dc, N, D, early, late) in CODES.items():
        code = hz.regular_code(n, dv, dc, seed=1)
        rng = np.random.default_rng(n)
        for rows, cap in ((1, 1), (8192, 4)):
            bank = ctx.ldpc(hz.LDPC_SOFT_F32, code, received=N, data_bits=D, scale=SCALE, max_iters=MAX_ITERS, norm=12, rows=rows)
            per_group, threads, frame_lds, form = bank.plan()
            for regime, sigma in (("early", early), ("late", late)):
                base = torch.from_numpy((-1.0 + sigma * rng.standard_normal((DISTINCT, N))).astype(np.float32)).cuda()
                pick = (torch.arange(rows * cap, device="cuda") * 7) % DISTINCT
                frames = base[pick].reshape(rows, cap, N).contiguous()
                outs = bank.decode(frames)
                torch.cuda.synchronize()
                info = outs[1].cpu().numpy().view(np.uint32)
                iters, ok = (info >> 16) & 0xFF, info >> 31
                steps = args.steps if rows == 1 else max(3, args.steps // 6)
                us = round(timed(lambda i: bank.decode(frames, out=outs), steps, min(args.warmup, steps)), 1)
                count = rows * cap
                work = float(np.maximum(iters, 1).sum())  # (a frame that leaves at once still makes one check pass)
                case = {"bank": "ldpc", "code": name, "n": n, "m": code.m, "E": code.E, "N": N, "D": D, "frames": count, "rows": rows, "cap": cap,
                        "regime": regime, "sigma": sigma, "frames_per_group": per_group, "threads_per_frame": threads, "frame_lds_bytes": frame_lds,
                        "form": form, "us": us, "iters_mean": round(float(iters.mean()), 2), "iters_min": int(iters.min()), "iters_max": int(iters.max()),
                        "ok_fraction": round(float(ok.mean()), 3), "us_per_frame_iteration": round(us / work, 4),
                        "decoded_gbit_per_s": round(count * D / us / 1e3, 3)}
                say(f"ldpc {name} n={n} m={code.m} E={code.E} N={N} D={D} frames={count:6d} (rows {rows} x cap {cap}) {regime:5s} sigma={sigma}: "
                    f"{us:10.1f} us, iters mean {case['iters_mean']} ({case['iters_min']} ... {case['iters_max']}), ok {case['ok_fraction']}, "
                    f"{case['us_per_frame_iteration']} us per frame and iteration, {case['decoded_gbit_per_s']} Gbit/s decoded "
                    f"({case['decoded_gbit_per_s'] / VITERBI_GBIT:.2f} of the Viterbi bank's); frames/group={per_group} threads/frame={threads} "
                    f"frame LDS={frame_lds} form={form}")
                results.append(case)
            bank.close()
    say("LDS accesses per edge and iteration, counted from hz_ldpc.hip: the check pass reads P[v] and r_e, writes t_e into the message's byte, reads it back "
        "and writes r_e; the variable pass reads r_e: 4 reads and 2 writes of state, messages per edge (int8), one generation of P (int16).  "
        "With the tables in LDS (form 1) col[e] and vedge[k] add 2 reads per edge, row_ptr and vptr 2 reads per check and per variable; "
        "form 2 reads them through the cache.  Per variable the variable pass also reads q[v] and writes P[v].  Summaries per check were not tried.")
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps({"ldpc_time": results}))


if __name__ == "__main__":
    main()

"""Times the AGC bank (include/hzsdr_agc.h) in us per push, median of --steps, from HBM (a rotation of input and output
buffers whose bytes together pass the 256 MB cache by a quarter: 320 MiB at least): R = 1, 100, 256, 512, 1024 and 8192
rows, both kinds, with and without the track, n chosen per R so that a push lasts about a millisecond (found by a first
push of 4096 samples per row), the same n for every case of an R.  Beside them, in the same run and over the same R and
n, the carrier recovery bank's TONE form (timed and rows of tools/carrier_time.py): the yardstick, a row-wave kernel whose
walk is a long chain where this one's is a short one.

The rows are QPSK symbols of 4 samples each at the level 0.2 (every row a rotation of one stream; real rows: its real
part), the loop at ref 1, attack 0.1, decay 0.01, so that it is settled as in use.  Prints one line per case and one JSON
line at the end.

    python tools/agc_time.py [--steps 200] [--warmup 30] [--rows 1 100 256 512 1024 8192]
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
from symsync_time import CACHE, timed  # noqa: E402
from carrier_time import carrier, rotation  # noqa: E402

ROWS = (1, 100, 256, 512, 1024, 8192)
TARGET_US = 1000.0
LEVEL = 0.2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)  # (pushes of a millisecond: a fifth of a second per case)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rows", type=int, nargs="+", default=list(ROWS), help="the row counts to time")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = hz.Context(0, hz.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    params = np.array([1.0, 0.1, 0.01, 1e-4, 1.0, 2.0 ** -10, 2.0 ** 10], np.float32)
    cparams = np.array([*hz.carrier_gains(0.02), 0.0, -0.01, 0.01], np.float32)
    results = []
    for rows in args.rows:
        # n for about a millisecond: a first push of 4096 samples per row, complex rows without the track
        probe = (LEVEL * carrier(4096, hz.CARRIER_QPSK, 1)).astype(np.complex64)
        probe = torch.from_numpy(np.tile(probe, (rows, 1)) if rows > 1 else probe).cuda()
        with ctx.agc(hz.FMT_C64, params, rows=rows) as bank:
            dst = torch.empty_like(probe)
            first = timed(lambda i: bank.push(probe, out=dst), 5, 2)
        n = max(256, int(4096 * TARGET_US / first) // 256 * 256)
        del probe, dst
        qpsk = (LEVEL * carrier(n + rows, hz.CARRIER_QPSK, 1)).astype(np.complex64)
        for kind, name, size in ((hz.AGC_REAL_F32, "f32", 4), (hz.FMT_C64, "c64", 8)):
            one = torch.from_numpy(qpsk if size == 8 else np.ascontiguousarray(qpsk.real)).cuda()
            for track in (False, True):
                moved = rows * n * (2 * size + (4 if track else 0))  # bytes read + written
                rot, ins = rotation(one, rows, n, moved)
                assert rot * moved >= CACHE + CACHE // 4, "the rotation does not pass the cache"
                outs = [torch.empty_like(a) for a in ins]
                trs = [torch.empty(a.shape, dtype=torch.float32, device="cuda") for a in ins] if track else None
                bank = ctx.agc(kind, params, rows=rows)
                per_wave, tile, form = bank.plan()
                # (the stream goes on from push to push: the gain is carried, as in use)
                if track:
                    t = timed(lambda i: bank.push(ins[i % rot], out=outs[i % rot], track=trs[i % rot]), args.steps, args.warmup)
                else:
                    t = timed(lambda i: bank.push(ins[i % rot], out=outs[i % rot]), args.steps, args.warmup)
                gain = float(bank.state()[0].astype(np.float64).mean())
                bank.close()
                del ins, outs, trs
                t = round(t, 1)
                case = {"bank": "agc", "kind": name, "track": track, "rows": rows, "n": n, "rows_per_wave": per_wave, "tile": tile, "form": form,
                        "rotation": rot, "rotation_bytes": rot * moved, "us": t, "row_msamples_per_s": round(n / t, 2),
                        "aggregate_msamples_per_s": round(rows * n / t, 1), "ns_per_sample_and_wave": round(t * 1e3 / n, 2),
                        "gbytes_per_s": round(moved / t / 1e3, 1), "mean_gain": round(gain, 4)}
                print(f"agc {name} track={int(track)} R={rows:5d} n={n:7d} rows/wave={per_wave}: {t:9.1f} us, one row "
                      f"{case['row_msamples_per_s']:.2f} Msamples/s, all rows {case['aggregate_msamples_per_s']:.1f} Msamples/s, "
                      f"{case['ns_per_sample_and_wave']:.2f} ns per sample of a wave, {case['gbytes_per_s']:.1f} GB/s; rotation {rot}; "
                      f"the gains end at {gain:.4f}", flush=True)
                results.append(case)
            del one
        # the carrier recovery bank's TONE form over the same R and n
        one = torch.from_numpy(carrier(n + rows, hz.CARRIER_TONE, 1)).cuda()
        moved = rows * n * 16
        rot, ins = rotation(one, rows, n, moved)
        outs = [torch.empty_like(a) for a in ins]
        bank = ctx.carrier_loop(hz.CARRIER_TONE, cparams, rows=rows)
        t = round(timed(lambda i: bank.push(ins[i % rot], out=outs[i % rot]), args.steps, args.warmup), 1)
        per_wave = bank.plan()[0]
        bank.close()
        del ins, outs, one
        case = {"bank": "carrier", "mode": "tone", "track": False, "rows": rows, "n": n, "rows_per_wave": per_wave, "rotation": rot, "us": t,
                "row_msamples_per_s": round(n / t, 2), "aggregate_msamples_per_s": round(rows * n / t, 1), "ns_per_sample_and_wave": round(t * 1e3 / n, 2)}
        print(f"carrier tone track=0 R={rows:5d} n={n:7d} rows/wave={per_wave}: {t:9.1f} us, one row {case['row_msamples_per_s']:.2f} Msamples/s, "
              f"all rows {case['aggregate_msamples_per_s']:.1f} Msamples/s, {case['ns_per_sample_and_wave']:.2f} ns per sample of a wave; rotation {rot}", flush=True)
        results.append(case)
    ctx.close()
    print(json.dumps({"agc_time": results}))


if __name__ == "__main__":
    main()

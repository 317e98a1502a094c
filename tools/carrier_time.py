"""Times the carrier recovery bank (include/hzsdr_carrier.h) in us per push, median of --steps, from HBM (a rotation of
input and output buffers whose bytes together pass the 256 MB cache): R = 1, 100, 1024 and 8192 complex64 rows, each of
the three detectors, with and without the track, n chosen per R so that a push lasts about a millisecond (found by a
first push of 4096 samples per row), the same n for every case of an R.  Beside them, in the same run and over the same
R and n, the symbol-timing bank's complex rows at 5 samples per symbol (timed and stream of tools/symsync_time.py): the
nearest row-wave kernel.

The rows are a unit-amplitude tone, BPSK or QPSK symbols of 4 samples each, 0.002 cycles per sample off (every row a
rotation of one stream), so that the loop is in lock as in use.  Prints one line per case and one JSON line at the end.

    python tools/carrier_time.py [--steps 200] [--warmup 30] [--rows 1 100 1024 8192]
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
from symsync_time import CACHE, SPS, stream, timed  # noqa: E402

ROWS = (1, 100, 1024, 8192)
OFFSET = 0.002
TARGET_US = 1000.0
NAMES = {hz.CARRIER_TONE: "tone", hz.CARRIER_BPSK: "bpsk", hz.CARRIER_QPSK: "qpsk"}


def carrier(n, mode, seed):
    """n complex64 samples: a tone, or +-1 / (+-1 +- i) / sqrt 2 symbols held for 4 samples, OFFSET cycles per sample off"""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    a = np.ones(n, np.complex128)
    if mode != hz.CARRIER_TONE:
        a = (2.0 * rng.integers(0, 2, n // 4 + 1) - 1.0)[k // 4].astype(np.complex128)
    if mode == hz.CARRIER_QPSK:
        a = (a + 1j * (2.0 * rng.integers(0, 2, n // 4 + 1) - 1.0)[k // 4]) / np.sqrt(2.0)
    return (a * np.exp(2j * np.pi * OFFSET * k + 0.5j)).astype(np.complex64)


def rotation(one, rows, n, per_push_bytes):
    """`rot` copies of the rows (row r: the stream from sample r on), enough of them to pass the cache"""
    rot = max(2, -(-(CACHE + CACHE // 4) // per_push_bytes))
    base = torch.stack([one[r:r + n] for r in range(rows)]) if rows > 1 else one[:n].clone()
    return rot, [base.clone() for _ in range(rot)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)  # (pushes of a millisecond: a fifth of a second per case)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rows", type=int, nargs="+", default=list(ROWS), help="the row counts to time")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = hz.Context(0, hz.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    params = np.array([*hz.carrier_gains(0.02), 0.0, -0.01, 0.01], np.float32)
    sparams = np.array([SPS, 0.01, *hz.loop_gains(SPS)], np.float32)
    results = []
    for rows in args.rows:
        # n for about a millisecond: a first push of 4096 samples per row, QPSK without the track
        probe = carrier(4096, hz.CARRIER_QPSK, 1)
        probe = torch.from_numpy(np.tile(probe, (rows, 1)) if rows > 1 else probe).cuda()
        with ctx.carrier_loop(hz.CARRIER_QPSK, params, rows=rows) as bank:
            dst = torch.empty_like(probe)
            first = timed(lambda i: bank.push(probe, out=dst), 5, 2)
        n = max(256, int(4096 * TARGET_US / first) // 256 * 256)
        del probe, dst
        for mode in (hz.CARRIER_TONE, hz.CARRIER_BPSK, hz.CARRIER_QPSK):
            one = torch.from_numpy(carrier(n + rows, mode, 1)).cuda()
            for track in (False, True):
                moved = rows * n * (16 + (4 if track else 0))  # bytes read + written
                rot, ins = rotation(one, rows, n, moved)
                assert rot * moved > CACHE, "the rotation does not pass the cache"
                outs = [torch.empty_like(a) for a in ins]
                trs = [torch.empty(a.shape, dtype=torch.float32, device="cuda") for a in ins] if track else None
                bank = ctx.carrier_loop(mode, params, rows=rows)
                per_wave, tile, form = bank.plan()
                # (the stream goes on from push to push: the state is carried, as in use)
                if track:
                    t = timed(lambda i: bank.push(ins[i % rot], out=outs[i % rot], track=trs[i % rot]), args.steps, args.warmup)
                else:
                    t = timed(lambda i: bank.push(ins[i % rot], out=outs[i % rot]), args.steps, args.warmup)
                freq = float(bank.state()[0][:, 1].view(np.int32).astype(np.float64).mean() / 2.0 ** 32)
                bank.close()
                del ins, outs, trs
                t = round(t, 1)
                case = {"bank": "carrier", "mode": NAMES[mode], "track": track, "rows": rows, "n": n, "rows_per_wave": per_wave, "tile": tile, "form": form,
                        "rotation": rot, "rotation_bytes": rot * moved, "us": t, "row_msamples_per_s": round(n / t, 2),
                        "aggregate_msamples_per_s": round(rows * n / t, 1), "ns_per_sample_and_wave": round(t * 1e3 / n, 2),
                        "gbytes_per_s": round(moved / t / 1e3, 1), "mean_frequency": round(freq, 6)}
                print(f"carrier {NAMES[mode]} track={int(track)} R={rows:5d} n={n:7d} rows/wave={per_wave}: {t:9.1f} us, one row "
                      f"{case['row_msamples_per_s']:.2f} Msamples/s, all rows {case['aggregate_msamples_per_s']:.1f} Msamples/s, "
                      f"{case['ns_per_sample_and_wave']:.2f} ns per sample of a wave, {case['gbytes_per_s']:.1f} GB/s; rotation {rot}; "
                      f"F ends at {freq:.6f}", flush=True)
                results.append(case)
            del one
        # the symbol-timing bank's complex rows over the same R and n
        one = torch.from_numpy(stream(n + rows, True, 1)).cuda()
        bank = ctx.symbol_sync(hz.FMT_C64, sparams, rows=rows)
        bound = bank.max_symbols(n)
        moved = rows * (n + bound) * 8
        rot, ins = rotation(one, rows, n, moved)
        outs = [torch.empty((rows, bound) if rows > 1 else (bound,), dtype=torch.complex64, device="cuda") for _ in range(rot)]
        counts = torch.zeros(rows, dtype=torch.int32, device="cuda")
        t = round(timed(lambda i: bank.push(ins[i % rot], out=outs[i % rot], counts=counts), args.steps, args.warmup), 1)
        per_wave = bank.plan()[0]
        bank.close()
        del ins, outs, one
        case = {"bank": "symsync", "kind": "c64", "rows": rows, "n": n, "sps": SPS, "rows_per_wave": per_wave, "rotation": rot, "us": t,
                "row_msamples_per_s": round(n / t, 2), "aggregate_msamples_per_s": round(rows * n / t, 1), "ns_per_sample_and_wave": round(t * 1e3 / n, 2)}
        print(f"symsync c64 R={rows:5d} n={n:7d} rows/wave={per_wave}: {t:9.1f} us, one row {case['row_msamples_per_s']:.2f} Msamples/s, "
              f"all rows {case['aggregate_msamples_per_s']:.1f} Msamples/s, {case['ns_per_sample_and_wave']:.2f} ns per sample of a wave; rotation {rot}", flush=True)
        results.append(case)
    ctx.close()
    print(json.dumps({"carrier_time": results}))


if __name__ == "__main__":
    main()

"""Times the equalizer bank (include/hzsdr_equalizer.h) in us per push, median of --steps, from HBM (a rotation of input
and output buffers whose bytes together pass the 256 MB cache by a quarter: 320 MiB at least): R = 1, 64, 1024 and 8192
rows x N = 4, 11, 32 and 64 taps, both kinds, CMA with mu = 0.001 on QPSK symbols through the 4-tap channel of the
tests (real rows: the real part), so that the loop runs settled as in use.  Beside every case, over the same bytes, the
library's own device copy (hzsdr_convert between equal formats): the yardstick.  Prints one line per case and one JSON
line at the end.

    python tools/equalizer_time.py [--steps 40] [--warmup 8] [--rows 1 64 1024 8192] [--taps 4 11 32 64]

The A/B of the lane-exchange forms (HZ_EQ_EXCHANGE of csrc/hz_equalizer.hip: 0 = ds_bpermute, 1 = DPP and lane swaps,
2 = a round trip through the LDS): build one library per form,

    make -C go-sdr_amd/csrc BUILD=../../build/csrc_x0 OUT=../libhzsdr_hip_x0.so EXTRA=-DHZ_EQ_EXCHANGE=0     (and x1, x2)

and run them interleaved on one box, `--rounds` times in turn, every run a fresh process with HZSDR_LIB set:

    python tools/equalizer_time.py --ab go-sdr_amd/libhzsdr_hip_x0.so go-sdr_amd/libhzsdr_hip_x1.so go-sdr_amd/libhzsdr_hip_x2.so

The A/B cases are complex rows, R = 1 and 1024, every N; each run also prints a checksum of its outputs, and the forms
must agree on it (the sum's bits do not depend on the form).
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = (1, 64, 1024, 8192)
TAPS = (4, 11, 32, 64)
CACHE = 256 << 20
CHANNEL = np.array([0.2 - 0.1j, 1.0, 0.45 + 0.3j, -0.2 + 0.15j])


def symbols_of(rows):
    """symbols per row and push: a push of some hundred microseconds at least, the buffers of 8192 rows within reach"""
    return 4096 if rows <= 1024 else 2048


def received(n, seed):
    rng = np.random.default_rng(seed)
    a = ((2.0 * rng.integers(0, 2, n) - 1.0) + 1j * (2.0 * rng.integers(0, 2, n) - 1.0)) / np.sqrt(2.0)
    return (np.convolve(a, CHANNEL)[:n] + 0.02 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


def cases_run(args, ab):
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    hz = importlib.import_module("go-sdr_amd")
    from symsync_time import timed
    torch.cuda.set_device(0)
    ctx = hz.Context(0, hz.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    params = np.array([0.001, 1.0], np.float32)
    results = []
    for rows in args.rows:
        n = symbols_of(rows)
        stream = received(n + rows, 1)
        for taps in args.taps:
            for kind, name, size in ((hz.EQUALIZER_REAL_F32, "f32", 4), (hz.FMT_C64, "c64", 8)):
                if ab and size == 4:
                    continue
                one = torch.from_numpy(stream if size == 8 else np.ascontiguousarray(stream.real)).cuda()
                moved = rows * n * 2 * size  # bytes read + written
                rot = max(2, -(-(CACHE + CACHE // 4) // moved))
                base = torch.stack([one[r:r + n] for r in range(rows)]) if rows > 1 else one[:n].clone()
                ins = [base.clone() for _ in range(rot)]
                outs = [torch.empty_like(a) for a in ins]
                bank = ctx.equalizer(kind, hz.EQUALIZER_CMA, taps, taps // 2, params, rows=rows)
                per_wave, tile, form = bank.plan()
                # the taps converge first: the timed pushes see the settled loop (the stream goes on from push to push)
                for _ in range(3 if ab else 1):
                    bank.push(ins[0], out=outs[0])
                t = round(timed(lambda i: bank.push(ins[i % rot], out=outs[i % rot]), args.steps, args.warmup), 1)
                bank.reset()
                check = zlib.crc32(bank.push(ins[0], out=outs[0]).cpu().numpy().tobytes())
                bank.close()
                flat = [a.reshape(-1).view(torch.complex64) if size == 4 else a.reshape(-1) for a in ins]  # (the same bytes as complex64)
                dst = torch.empty_like(flat[0])
                copy_us = None
                if not ab:
                    copy_us = round(timed(lambda i: ctx.convert(dst, flat[i % rot]), args.steps, args.warmup), 1)
                del ins, outs, flat, dst, base, one
                case = {"kind": name, "rows": rows, "taps": taps, "n": n, "rows_per_wave": per_wave, "tile": tile, "form": form, "rotation": rot,
                        "us": t, "copy_us": copy_us, "of_the_copy": round(t / copy_us, 1) if copy_us else None,
                        "row_msymbols_per_s": round(n / t, 3), "aggregate_msymbols_per_s": round(rows * n / t, 1),
                        "ns_per_symbol_and_wave": round(t * 1e3 / n, 1), "crc": check}
                print(f"equalizer {name} R={rows:5d} N={taps:2d} n={n:5d} rows/wave={per_wave}: {t:9.1f} us, one row {case['row_msymbols_per_s']:.3f} "
                      f"Msymbols/s, all rows {case['aggregate_msymbols_per_s']:.1f} Msymbols/s, {case['ns_per_symbol_and_wave']:.1f} ns per symbol of a wave; "
                      f"the copy of the same bytes {copy_us} us; rotation {rot}", flush=True)
                results.append(case)
    ctx.close()
    print(json.dumps({"equalizer_time": results}))


def ab_run(args):
    """every library in turn, `rounds` times over: a fresh process each, so that no form runs on a warmer chip than another"""
    runs = {lib: [] for lib in args.ab}
    for rnd in range(args.rounds):
        for lib in args.ab:
            env = dict(os.environ, HZSDR_LIB=os.path.abspath(lib))
            cmd = [sys.executable, os.path.abspath(__file__), "--ab-child", "--steps", str(args.steps), "--warmup", str(args.warmup),
                   "--rows", "1", "1024", "--taps", *[str(t) for t in args.taps]]
            out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                print(out.stdout[-2000:], out.stderr[-2000:])
                raise SystemExit(f"{lib}: exit status {out.returncode}")
            runs[lib].append(json.loads(out.stdout.strip().splitlines()[-1])["equalizer_time"])
    first = runs[args.ab[0]][0]
    for k, case in enumerate(first):
        line = f"A/B c64 R={case['rows']:5d} N={case['taps']:2d} n={case['n']}:"
        for lib in args.ab:
            us = [r[k]["us"] for r in runs[lib]]
            same = all(r[k]["crc"] == case["crc"] for r in runs[lib])
            line += f"  {os.path.basename(lib)} {np.median(us):9.1f} us (runs {' '.join(f'{u:.1f}' for u in us)}){'' if same else ' OUTPUTS DIFFER'}"
        print(line, flush=True)
    print(json.dumps({"equalizer_ab": {os.path.basename(lib): runs[lib] for lib in args.ab}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rows", type=int, nargs="+", default=list(ROWS), help="the row counts to time")
    ap.add_argument("--taps", type=int, nargs="+", default=list(TAPS), help="the tap counts to time")
    ap.add_argument("--ab", nargs="+", help="libraries built with different HZ_EQ_EXCHANGE, timed interleaved")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ab-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.ab:
        ab_run(args)
    else:
        cases_run(args, args.ab_child)


if __name__ == "__main__":
    main()

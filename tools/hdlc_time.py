"""Times the HDLC deframer bank (include/hzsdr_hdlc.h) in us per push, median of --steps after --warmup, real rows, fcs 16,
frames of 3 ... 256 bytes, cap 128.  Four loads in one run:
  - negative: all-negative floats, no 1 bit and so no event (one row of 2^20 symbols, and --rows rows of 2^16);
  - random:   random signs, a flag or an abort every 128 bits: the worst case for the event loop;
  - hdlc32:   encoded traffic, 32-byte frames at 50 % duty (a frame, then as many bits of idle flags);
  - hdlc256:  the same with 256-byte frames.
The rows of the two traffic loads are eight encoded streams of different payloads, each rotated by a row's own offset.
A push of 8192 rows carries 2 GiB, eight times the 256 MB cache, so one input buffer per load is from HBM.  One row's
4 MiB stay in the cache, as in tools/framesync_time.py: one wave's latency is what that case measures.
Beside every load, in the same run and over the same rows: the frame sync bank (a 32-bit word, thr 2, 168 payload bits,
what README.md quotes for it) and the library's own device copy of the bytes read (hzsdr_convert between equal formats).

--ab adds what the FCS A/B needs: traffic of 32-byte and of 1024-byte frames through a bank of max_bytes 1024 with fcs 32
and with fcs 0 (the same work less the FCS), 1024 rows.  One form of the FCS for every length is a build of its own
(make EXTRA=-DHZ_HDLC_WALK_BYTES=0 or =1024, csrc/hz_hdlc_plan.h; then HZSDR_LIB=... python tools/hdlc_time.py --ab).

Prints one line per case and one JSON line at the end.

    python tools/hdlc_time.py [--steps 100] [--warmup 10] [--rows 8192] [--ab]
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

WORD, W, THR, P = 0x1ACFFC1D, 32, 2, 168
N_ROWS, N_ONE = 1 << 16, 1 << 20
CAP, VARIANTS = 128, 8


def traffic_bits(n, frame_bytes, fcs, seed):
    """n bits: frames of frame_bytes bytes (FCS included) of random payloads, each followed by as many bits of idle flags"""
    rng = np.random.default_rng(seed)
    parts, have = [], 0
    while have < n + 8:
        payload = rng.integers(0, 256, frame_bytes - fcs // 8, dtype=np.uint8).tobytes()
        frame = hz.hdlc_encode([payload], fcs=fcs)
        idle = hz.hdlc_encode([], flags=max(1, (len(frame) - 16) // 8))
        parts += [frame, idle]
        have += len(frame) + len(idle)
    return np.concatenate(parts)[:n]


def traffic_rows(rows, n, frame_bytes, fcs):
    """(rows, n) float32 on the device: VARIANTS streams, row r the stream r % VARIANTS rotated by 97 r symbols"""
    variants = min(VARIANTS, rows)
    base = np.stack([traffic_bits(n, frame_bytes, fcs, 10 * frame_bytes + v) for v in range(variants)]).astype(np.float32) * 2.0 - 1.0
    base = torch.from_numpy(base).cuda()
    x = torch.empty((rows, n), dtype=torch.float32, device="cuda")
    for r in range(rows):
        x[r] = torch.roll(base[r % variants], 97 * r)
    return x.view(-1) if rows == 1 else x


def load(name, rows, n, fcs=16):
    shape = (n,) if rows == 1 else (rows, n)
    if name == "negative":
        return -torch.rand(shape, dtype=torch.float32, device="cuda") - 0.25
    if name == "random":
        return torch.randn(shape, dtype=torch.float32, device="cuda")
    return traffic_rows(rows, n, int(name[4:]), fcs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rows", type=int, default=8192, help="the rows of the many-row cases")
    ap.add_argument("--ab", action="store_true", help="the loads of the FCS A/B instead")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    torch.manual_seed(1)
    ctx = hz.Context(0, hz.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    results = []
    if args.ab:
        cases = [(name, 1024, N_ROWS, fcs, 1024) for name in ("hdlc32", "hdlc1024") for fcs in (32, 0)]
    else:
        cases = [(name, rows, n, 16, 256) for rows, n in ((1, N_ONE), (args.rows, N_ROWS)) for name in ("negative", "random", "hdlc32", "hdlc256")]
    for name, rows, n, fcs, max_bytes in cases:
        x = load(name, rows, n, 32 if args.ab else fcs)
        moved = rows * n * 4
        bank = ctx.hdlc(hz.SYMSYNC_REAL_F32, fcs=fcs, max_bytes=max_bytes, rows=rows)
        per_wave, tile, ring, form = bank.plan()
        outs = bank.push(x, None, CAP)
        t = round(timed(lambda i: bank.push(x, None, CAP, out=outs), args.steps, args.warmup), 1)
        counts = outs[3].cpu().numpy().view(np.uint32)
        bank.close()
        del outs
        case = {"bank": "hdlc", "load": name, "rows": rows, "n": n, "fcs": fcs, "max_bytes": max_bytes, "rows_per_wave": per_wave, "ring_words": ring,
                "form": form, "input_bytes": moved, "us": t, "row_msymbols_per_s": round(n / t, 2), "read_gbytes_per_s": round(moved / t / 1e3, 1),
                "frames_last_push": int(counts.sum()), "most_in_a_row": int(counts.max())}
        if not args.ab:
            words, maps = hz.sync_hypotheses(WORD, W, 1, "invert")
            fs = ctx.frame_sync(hz.SYMSYNC_REAL_F32, W, words, maps, P, thr=THR, rows=rows)
            fouts = fs.push(x, None, 4)
            case["framesync_us"] = round(timed(lambda i: fs.push(x, None, 4, out=fouts), args.steps, args.warmup), 1)
            fs.close()
            del fouts
            flat = x.view(-1).view(torch.complex64)
            dst = torch.empty_like(flat)
            case["copy_us"] = round(timed(lambda i: ctx.convert(dst, flat), args.steps, args.warmup), 1)
            del dst, flat
            case["of_framesync"] = round(t / case["framesync_us"], 2)
            case["of_the_copy"] = round(t / case["copy_us"], 2)
        print(f"hdlc {name:8s} R={rows:5d} n={n:8d} fcs={fcs:2d} max_bytes={max_bytes:4d}: {t:10.1f} us, one row {case['row_msymbols_per_s']:8.2f} Msymbols/s, reads "
              f"{case['read_gbytes_per_s']:7.1f} GB/s; " +
              (f"frame sync {case['framesync_us']:9.1f} us ({case['of_framesync']:.2f} x), copy {case['copy_us']:9.1f} us ({case['of_the_copy']:.2f} x); " if not args.ab else "") +
              f"{case['frames_last_push']} frames in the last push, {case['most_in_a_row']} at most in a row", flush=True)
        results.append(case)
        del x
    ctx.close()
    print(json.dumps({"hdlc_time": results}))


if __name__ == "__main__":
    main()

"""Times the Viterbi decoder bank (include/hzsdr_viterbi.h) in us per call, median of --steps after --warmup, and writes
the lines to --out (profiles/viterbi_time.txt): the K = 7 rate 1/2 TAIL code with D = 1024 data bits at 1, 64, 1024, 8192
and 65536 frames, hard and soft input, plus K = 9 and K = 5 at 8192 frames.  Frames lie in min(frames, 8192) rows of
frames / rows slots.  The inputs rotate through buffers whose bytes together pass the 256 MB cache by a quarter (at most
16 buffers: the small cases are bound by latency, not by memory).  Every frame is one of 32 coded random data words with
3 % of its channel bits flipped (soft: values of magnitude 20 ... 60, the flipped ones weak); the decoder's work does
not depend on the data.

Per case: us per call, decoded Mbit/s (frames * D / us), and for one frame the cycles per trellis step of one wave -- the
whole call over T, and the slope between D = 1024 and D = 2048, which leaves the launch out; both hold the forward
add-compare-select AND the traceback of a step.  Cycles are counted at --mhz, 2400 by default: the MI355X's nominal
engine clock, which a lone wave holds (tools/clock_watch.py measures the clock under a load).

    python tools/viterbi_time.py [--steps 200] [--warmup 30] [--mhz 2400] [--out profiles/viterbi_time.txt]
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

CODES = {7: (0o171, 0o133), 9: (0o561, 0o753), 5: (0o23, 0o35)}
D, MAX_ROT, DISTINCT = 1024, 16, 32


def frames_for(K, kind, d, count, seed):
    """(frames (rows, cap, FB or N), data bits (DISTINCT, d)) with rows = min(count, 8192)"""
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 2, (DISTINCT, d)).astype(np.uint8)
    code = np.stack([hz.conv_encode(u, K, CODES[K]) for u in data])
    hurt = code ^ (rng.random(code.shape) < 0.03).astype(np.uint8)
    if kind == hz.VITERBI_BITS:
        base = np.packbits(hurt, axis=-1)
    else:
        mag = np.where(hurt == code, rng.uniform(20, 60, code.shape), rng.uniform(1, 10, code.shape))
        base = ((hurt.astype(np.float64) * 2 - 1) * mag).astype(np.float32)
    rows = min(count, 8192)
    cap = count // rows
    pick = np.arange(rows * cap) % DISTINCT
    return base[pick].reshape(rows, cap, -1), data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--mhz", type=float, default=2400.0, help="the clock the cycle counts assume")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "viterbi_time.txt"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = hz.Context(0, hz.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    mhz = args.mhz
    lines, results = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def run(K, kind, name, d, count):
        frames, data = frames_for(K, kind, d, count, 7 * K + count % 1000)
        rows, cap = frames.shape[:2]
        rot = int(min(MAX_ROT, max(2, -(-(CACHE + CACHE // 4) // frames.nbytes))))
        ins = [torch.from_numpy(np.roll(frames, k, axis=0) if rows > 1 else frames).cuda() for k in range(rot)]
        bank = ctx.viterbi(kind, K, CODES[K], d, scale=1.0, rows=rows)
        per_wave, per_lane, dec_bytes, form = bank.plan()
        N, FB, T, DB = bank.sizes()
        outs = bank.decode(ins[0])
        torch.cuda.synchronize()
        got = np.unpackbits(outs[0].cpu().numpy()[0, 0])[:d]
        ok = bool(np.array_equal(got, data[0]))
        us = round(timed(lambda i: bank.decode(ins[i % rot], out=outs), args.steps, args.warmup), 1)
        bank.close()
        case = {"bank": "viterbi", "K": K, "input": name, "D": d, "T": T, "frames": count, "rows": rows, "cap": cap, "frames_per_wave": per_wave,
                "states_per_lane": per_lane, "decision_bytes": dec_bytes, "form": form, "rotation": rot, "us": us,
                "decoded_mbit_per_s": round(count * d / us, 2), "first_frame_decoded": ok}
        say(f"viterbi K={K} {name} D={d} T={T} frames={count:6d} (rows {rows} x cap {cap}) frames/wave={per_wave} states/lane={per_lane} form={form}: "
            f"{us:10.1f} us, {case['decoded_mbit_per_s']:10.2f} Mbit/s decoded; rotation {rot}; first frame decoded: {ok}")
        results.append(case)
        return case

    say(f"cycles at {mhz:.0f} MHz (nominal); median of {args.steps} calls after {args.warmup}")
    for kind, name in ((hz.VITERBI_BITS, "hard"), (hz.VITERBI_SOFT_F32, "soft")):
        one = None
        for count in (1, 64, 1024, 8192, 65536):
            c = run(7, kind, name, D, count)
            one = one or c
        two = run(7, kind, name, 2 * D, 1)
        whole = one["us"] * mhz / one["T"]
        slope = (two["us"] - one["us"]) * mhz / (two["T"] - one["T"])
        say(f"viterbi K=7 {name} one frame, one wave: {whole:.0f} cycles per trellis step over the whole call; {slope:.0f} cycles per step from the slope "
            f"D = {D} -> {2 * D} (forward step and traceback step together, launch left out)")
        results.append({"bank": "viterbi", "K": 7, "input": name, "cycles_per_step_whole_call": round(whole, 1), "cycles_per_step_slope": round(slope, 1)})
        for K in (9, 5):
            run(K, kind, name, D, 8192)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps({"viterbi_time": results}))


if __name__ == "__main__":
    main()

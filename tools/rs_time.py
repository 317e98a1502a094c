"""Times the Reed-Solomon decoder bank (include/hzsdr_rs.h) in us per call, median of --steps after --warmup, and writes
the lines to --out (profiles/rs_time.txt): the CCSDS 255/223 code -- one codeword alone (latency), then 65536 codewords
clean, with t / 2 = 8 and with t = 16 symbol errors each, at I = 1 (65536 frames) and at I = 4 (16384 frames).  Frames lie
in min(frames, 8192) rows of frames / rows slots.  The inputs rotate through buffers whose bytes together pass the
256 MB cache by a quarter (at most 16).  Every codeword is one of 32 encoded random data words with its errors at random
places; the first frame's data must come back.

Per case: us per call and Gbit/s of corrected DATA (codewords * 223 * 8 / us).

--label names the build in the lines: the library is built with the syndrome step's multiply as two table reads in LDS
(the default) or, with `make EXTRA=-DHZ_RS_PRODUCTS`, as eight register-held products; run the tool once per build
(HZSDR_LIB selects the library) and keep both sets of lines.

    python tools/rs_time.py [--steps 100] [--warmup 20] [--label tables] [--out profiles/rs_time.txt] [--append]
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

MAX_ROT, DISTINCT = 16, 32


def frames_for(code, interleave, codewords, errors, seed):
    """(frames (rows, cap, I n), data (DISTINCT, I k)): every frame one of DISTINCT, `errors` wrong symbols per codeword"""
    rng = np.random.default_rng(seed)
    n, k = code[4], code[4] - code[3]
    data = rng.integers(0, 256, (DISTINCT, interleave, k)).astype(np.uint8)
    words = hz.rs_encode(code, data)
    for w in words.reshape(-1, n):
        where = rng.permutation(n)[:errors]
        w[where] ^= rng.integers(1, 256, errors).astype(np.uint8)
    base = hz.interleave_codewords(words)
    count = codewords // interleave
    rows = min(count, 8192)
    cap = count // rows
    return base[np.arange(rows * cap) % DISTINCT].reshape(rows, cap, -1), hz.interleave_codewords(data)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--label", default="tables", help="the syndrome multiply of the library under test")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rs_time.txt"))
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = hz.Context(0, hz.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    code = hz.CCSDS_RS_255_223
    lines, results = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def run(interleave, codewords, errors):
        frames, data = frames_for(code, interleave, codewords, errors, 11 * interleave + errors)
        rows, cap = frames.shape[:2]
        rot = int(min(MAX_ROT, max(2, -(-(CACHE + CACHE // 4) // frames.nbytes))))
        ins = [torch.from_numpy(np.roll(frames, k, axis=0) if rows > 1 else frames).cuda() for k in range(rot)]
        bank = ctx.reed_solomon(code, interleave, rows=rows)
        waves, lds, per_cu, _ = bank.plan()
        outs = bank.decode(ins[0])
        torch.cuda.synchronize()
        info = int(outs[1].cpu().numpy().view(np.uint32)[0, 0])
        ok = bool(np.array_equal(outs[0].cpu().numpy()[0, 0], data[0])) and info == (interleave * errors | 1 << 31)
        us = round(timed(lambda i: bank.decode(ins[i % rot], out=outs), args.steps, args.warmup), 1)
        bank.close()
        case = {"bank": "rs", "multiply": args.label, "interleave": interleave, "codewords": codewords, "errors": errors, "rows": rows, "cap": cap,
                "waves_per_group": waves, "lds_bytes": lds, "groups_per_cu": per_cu, "rotation": rot, "us": us,
                "data_gbit_per_s": round(codewords * 223 * 8 / us / 1e3, 2), "first_frame_corrected": ok}
        say(f"rs 255/223 [{args.label}] I={interleave} codewords={codewords:6d} errors={errors:2d} (rows {rows} x cap {cap}) waves/group={waves} lds={lds} "
            f"groups/CU={per_cu}: {us:10.1f} us, {case['data_gbit_per_s']:9.2f} Gbit/s of data; rotation {rot}; first frame corrected: {ok}")
        results.append(case)

    say(f"syndrome multiply: {args.label}; median of {args.steps} calls after {args.warmup}")
    for errors in (0, 8, 16):
        run(1, 1, errors)
    for interleave in (1, 4):
        for errors in (0, 8, 16):
            run(interleave, 65536, errors)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps({"rs_time": results}))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Interleaved-frame encode / clean decode against the row form of the same codec and codeword
count (ezrs_encode_interleaved / ezrs_decode_interleaved vs ezrs_encode_rows / ezrs_decode).

    python tools/il_bench.py [--ncw 1048576] [--out profiles/il/il_bench.json]

Codecs RS(255,223) (plane-sliced) and RS_CCSDS(255,223) (bit-sliced); geometries depth 4 (fast
path), depth 5 (general path) and one striped frame whose depth is the whole batch.  Device events;
every shape is warmed; interleaved and row-form calls alternate in the same process, `reps`
repeats per figure sized so that each figure has at least 0.5 s of timed work; the figure is the
median, the spread (max - min) / median.  The staged form is timed with the default staging chunk
(EZRS_IL_STAGE_MB, inside the Infinity Cache) and with the whole batch staged in one pass.
GB/s counts the frames' bytes once (ncw * 255)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ezpwd-reed-solomon_amd"))

import torch  # noqa: E402

import ezrs  # noqa: E402

REPS = 5


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / 1e3 / iters          # seconds per call


def figure(fns):
    """fns: name -> callable, timed alternately; returns name -> {median_s, spread, iters}."""
    iters = {}
    for n, f in fns.items():
        f()
        torch.cuda.synchronize()
        t = timed(f, 3)
        iters[n] = max(3, int(0.5 / REPS / t) + 1)
    runs = {n: [] for n in fns}
    for _ in range(REPS):
        for n, f in fns.items():
            runs[n].append(timed(f, iters[n]))
    return {n: {"median_s": statistics.median(v), "spread": (max(v) - min(v)) / statistics.median(v),
                "iters": iters[n]} for n, v in runs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncw", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "il", "il_bench.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    out = {"ncw": args.ncw, "reps": REPS, "device": torch.cuda.get_device_name(0), "results": []}
    for cname, mk in (("RS(255,223)", lambda: ezrs.Codec.rs(255, 223)),
                      ("RS_CCSDS(255,223)", lambda: ezrs.Codec.ccsds(223, True))):
        c = mk()
        g = torch.Generator(device="cuda").manual_seed(1)
        rows = torch.randint(0, 256, (args.ncw, 255), generator=g, device="cuda", dtype=torch.int32).to(torch.uint8)
        c.encode(rows)
        res_r = torch.empty(args.ncw, dtype=torch.int32, device="cuda")
        for gname, depth in (("depth4", 4), ("depth5", 5), ("stripe", args.ncw)):
            F = args.ncw // depth
            ncw = F * depth
            fr = rows[:ncw].view(F, depth, 255).transpose(1, 2).contiguous()     # [F, 255, depth]
            res_i = torch.empty(ncw, dtype=torch.int32, device="cuda")
            rr = rows[:ncw]
            for stage in ("default", "0"):
                if stage == "default":
                    os.environ.pop("EZRS_IL_STAGE_MB", None)
                else:
                    os.environ["EZRS_IL_STAGE_MB"] = stage
                enc = figure({"interleaved": lambda: c.encode_interleaved(fr), "row": lambda: c.encode(rr)})
                dec = figure({"interleaved": lambda: c.decode_interleaved(fr, result=res_i),
                              "row": lambda: c.decode(rr, result=res_r[:ncw])})
                torch.cuda.synchronize()
                assert int((res_i != 0).sum()) == 0 and int((res_r[:ncw] != 0).sum()) == 0
                assert torch.equal(fr.transpose(1, 2).reshape(ncw, 255), rr)
                for op, fg in (("encode", enc), ("decode_clean", dec)):
                    ti, tr = fg["interleaved"]["median_s"], fg["row"]["median_s"]
                    rec = {"codec": cname, "geometry": gname, "depth": depth, "ncw": ncw, "op": op,
                           "staging": "chunked" if stage == "default" else "whole batch",
                           "workspace_bytes": c.interleaved_workspace_bytes(223, depth, F),
                           "t_interleaved_ms": ti * 1e3, "t_row_ms": tr * 1e3, "ratio": ti / tr,
                           "interleaved_GBps": ncw * 255 / ti / 1e9, "row_GBps": ncw * 255 / tr / 1e9,
                           "spread_interleaved": fg["interleaved"]["spread"],
                           "spread_row": fg["row"]["spread"]}
                    out["results"].append(rec)
                    print(json.dumps(rec), flush=True)
            os.environ.pop("EZRS_IL_STAGE_MB", None)
            del fr
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

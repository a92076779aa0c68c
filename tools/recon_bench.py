#!/usr/bin/env python3
"""Shared-erasure reconstruction of a striped frame (Recon.reconstruct, with and without the
per-codeword check) against the staged decode given the same erasures in every codeword
(Codec.decode_interleaved), on the same buffers.

    python tools/recon_bench.py [--gib 1.0] [--out profiles/recon/recon_bench.json]
    python tools/recon_bench.py --ptrs [--gib 1.0] [--out profiles/recon/recon_ptrs_bench.json]

One frame per shape: len + nroots shards of `depth` symbols, symbol stride = depth, sized so that
the frame holds at least --gib GiB (well past the 256 MiB Infinity Cache).  Device events; every
call is warmed; the three calls alternate in the same process, `reps` repeats per figure sized so
that each figure has at least 0.5 s of timed work; the figure is the median, the spread
(max - min) / median.  The lost shards hold garbage before the first call of each kind; repeats
find them already rebuilt, which changes nothing in what either path computes (the staged decode
runs its erasure path on every codeword that carries erasures, the reconstruction never reads the
lost shards).  GB/s counts the frame's bytes once; hbm_fraction counts survivor bytes read + lost
bytes written + result bytes against 8 TB/s.

--ptrs: the pointer form (ezrs_reconstruct_ptrs) against the strided form instead, same shapes and
the same data, every shard of the pointer form an allocation of its own; the calls alternate in the
same process as above.  The pointer form is called through the C ABI with its pointer array built
once, as a C caller has it; ptrs_over_strided is the ratio of the medians.  A third figure,
ptrs_inframe, is the pointer form on pointers to the rows of the strided frame itself: the same
addresses as the strided form, so that the kernels' addressing is compared apart from where the
allocator put the shards."""
import ctypes as C
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
HBM = 8e12

SHAPES = [
    # (name, codec, len, lost)
    ("RS(255,251) len 10, 4 lost", lambda: ezrs.Codec.rs(255, 251), 10, [0, 3, 11, 13]),
    ("RS(255,252) len 17, 3 lost", lambda: ezrs.Codec.rs(255, 252), 17, [2, 9, 18]),
    ("RS(255,223) len 223, 4 lost", lambda: ezrs.Codec.rs(255, 223), 223, [5, 100, 222, 240]),
    ("RS(255,223) len 223, 32 lost", lambda: ezrs.Codec.rs(255, 223), 223, list(range(0, 64, 2))),
    ("RS_CCSDS(255,223) len 223, 4 lost", lambda: ezrs.Codec.ccsds(223, True), 223, [5, 222, 223, 254]),
]


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
        t = timed(f, 2)
        iters[n] = max(2, int(0.5 / REPS / t) + 1)
    runs = {n: [] for n in fns}
    for _ in range(REPS):
        for n, f in fns.items():
            runs[n].append(timed(f, iters[n]))
    return {n: {"median_s": statistics.median(v), "spread": (max(v) - min(v)) / statistics.median(v),
                "iters": iters[n]} for n, v in runs.items()}


def main_ptrs(args):
    L, sp = ezrs.lib(), ezrs._stream_ptr(None)
    out = {"gib": args.gib, "reps": REPS, "device": torch.cuda.get_device_name(0), "results": []}
    for name, mk, length, lost in SHAPES:
        c = mk()
        S, nlost = length + c.nroots, len(lost)
        depth = (int(args.gib * (1 << 30)) // S + 1023) // 1024 * 1024
        g = torch.Generator(device="cuda").manual_seed(1)
        shards = torch.empty((S, depth), dtype=torch.uint8, device="cuda")
        for s in range(length):
            shards[s] = torch.randint(0, 256, (depth,), generator=g, device="cuda", dtype=torch.int32).to(torch.uint8)
        frames = shards[None]
        c.encode_interleaved(frames)
        good = shards[lost].clone()
        own = [shards[s].clone() for s in range(S)]             # every shard an allocation of its own
        arr = (C.c_void_p * S)(*[t.data_ptr() for t in own])
        arr_in = (C.c_void_p * S)(*[shards[s].data_ptr() for s in range(S)])
        plan = c.recon_plan(length, lost)
        res, res_p = (torch.empty(depth, dtype=torch.int32, device="cuda") for _ in range(2))
        rp = C.c_void_p(res_p.data_ptr())
        fns = {"strided": lambda: plan.reconstruct(frames, result=res),
               "ptrs": lambda: L.ezrs_reconstruct_ptrs(plan._h, arr, depth, rp, sp),
               "strided_nocheck": lambda: plan.reconstruct(frames),
               "ptrs_nocheck": lambda: L.ezrs_reconstruct_ptrs(plan._h, arr, depth, None, sp),
               "ptrs_inframe": lambda: L.ezrs_reconstruct_ptrs(plan._h, arr_in, depth, rp, sp),
               "ptrs_inframe_nocheck": lambda: L.ezrs_reconstruct_ptrs(plan._h, arr_in, depth, None, sp)}
        for what, fn in fns.items():                # each path once on garbage
            shards[lost] = 0x5A
            for p in lost:
                own[p].fill_(0x5A)
            r = fn()
            assert r is None or r is res or r == 0, (name, what)
            torch.cuda.synchronize()
            got = torch.stack([own[p] for p in lost]) if what in ("ptrs", "ptrs_nocheck") else shards[lost]
            assert torch.equal(got, good), (name, what)
        assert torch.equal(res, res_p) and bool((res == nlost).all()), name
        fg = figure(fns)
        torch.cuda.synchronize()
        assert torch.equal(torch.stack([own[p] for p in lost]), good), name
        rec = {"shape": name, "len": length, "nroots": c.nroots, "nlost": nlost, "depth": depth,
               "frame_bytes": S * depth}
        for k, v in fg.items():
            rec[f"t_{k}_ms"], rec[f"spread_{k}"] = v["median_s"] * 1e3, v["spread"]
        rec["ptrs_over_strided"] = fg["ptrs"]["median_s"] / fg["strided"]["median_s"]
        rec["ptrs_over_strided_nocheck"] = fg["ptrs_nocheck"]["median_s"] / fg["strided_nocheck"]["median_s"]
        rec["inframe_over_strided"] = fg["ptrs_inframe"]["median_s"] / fg["strided"]["median_s"]
        rec["inframe_over_strided_nocheck"] = (fg["ptrs_inframe_nocheck"]["median_s"] /
                                               fg["strided_nocheck"]["median_s"])
        rec["iters"] = {k: v["iters"] for k, v in fg.items()}
        out["results"].append(rec)
        print(json.dumps(rec), flush=True)
        del shards, frames, good, own, res, res_p, plan, c, fns
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--ptrs", action="store_true", help="the pointer form against the strided form")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", "recon",
                                        "recon_ptrs_bench.json" if args.ptrs else "recon_bench.json")
    torch.cuda.set_device(0)
    if args.ptrs:
        return write(args.out, main_ptrs(args))
    out = {"gib": args.gib, "reps": REPS, "device": torch.cuda.get_device_name(0), "results": []}
    for name, mk, length, lost in SHAPES:
        c = mk()
        S, nlost = length + c.nroots, len(lost)
        depth = (int(args.gib * (1 << 30)) // S + 1023) // 1024 * 1024
        g = torch.Generator(device="cuda").manual_seed(1)
        shards = torch.empty((S, depth), dtype=torch.uint8, device="cuda")
        for s in range(length):
            shards[s] = torch.randint(0, 256, (depth,), generator=g, device="cuda", dtype=torch.int32).to(torch.uint8)
        frames = shards[None]
        c.encode_interleaved(frames)
        good = shards[lost].clone()
        plan = c.recon_plan(length, lost)
        res = torch.empty(depth, dtype=torch.int32, device="cuda")
        res_d = torch.empty(depth, dtype=torch.int32, device="cuda")
        eras = torch.tensor(lost, dtype=torch.int32, device="cuda").repeat(depth, 1).contiguous()
        neras = torch.full((depth,), nlost, dtype=torch.int32, device="cuda")
        # each path once on garbage, checked against the encoded shards
        for what, fn, r in (("recon", lambda: plan.reconstruct(frames, result=res), res),
                            ("recon_nocheck", lambda: plan.reconstruct(frames), None),
                            ("staged_decode", lambda: c.decode_interleaved(frames, eras=eras, neras=neras,
                                                                           result=res_d), res_d)):
            shards[lost] = 0x5A
            fn()
            torch.cuda.synchronize()
            assert torch.equal(shards[lost], good), (name, what)
            # the decode returns 0 for a codeword whose garbage happened to be right (valid as
            # received): a few in 2^24 with three lost symbols
            ok = r is None or bool(((r == nlost) | ((r == 0) if what == "staged_decode" else False)).all())
            assert ok, (name, what)
        fg = figure({"recon": lambda: plan.reconstruct(frames, result=res),
                     "recon_nocheck": lambda: plan.reconstruct(frames),
                     "staged_decode": lambda: c.decode_interleaved(frames, eras=eras, neras=neras, result=res_d)})
        torch.cuda.synchronize()
        assert torch.equal(shards[lost], good), name
        fbytes = S * depth
        t_r, t_n, t_d = (fg[k]["median_s"] for k in ("recon", "recon_nocheck", "staged_decode"))
        rec = {"shape": name, "len": length, "nroots": c.nroots, "nlost": nlost, "depth": depth,
               "frame_bytes": fbytes,
               "t_recon_ms": t_r * 1e3, "t_recon_nocheck_ms": t_n * 1e3, "t_staged_decode_ms": t_d * 1e3,
               "recon_GBps": fbytes / t_r / 1e9, "recon_nocheck_GBps": fbytes / t_n / 1e9,
               "staged_decode_GBps": fbytes / t_d / 1e9,
               "recon_hbm_fraction": (fbytes + 4 * depth) / t_r / HBM,
               "recon_nocheck_hbm_fraction": fbytes / t_n / HBM,
               "staged_over_recon": t_d / t_r, "staged_over_recon_nocheck": t_d / t_n,
               "spread_recon": fg["recon"]["spread"], "spread_recon_nocheck": fg["recon_nocheck"]["spread"],
               "spread_staged_decode": fg["staged_decode"]["spread"],
               "iters": {k: v["iters"] for k, v in fg.items()}}
        out["results"].append(rec)
        print(json.dumps(rec), flush=True)
        del shards, frames, good, eras, neras, res, res_d, plan, c
        torch.cuda.empty_cache()
    write(args.out, out)


def write(path, out):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()

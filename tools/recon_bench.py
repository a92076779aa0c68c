#!/usr/bin/env python3
"""Shared-erasure reconstruction of a striped frame (Recon.reconstruct, with and without the
per-codeword check) against the staged decode given the same erasures in every codeword
(Codec.decode_interleaved), on the same buffers.

    python tools/recon_bench.py [--gib 1.0] [--out profiles/recon/recon_bench.json]
    python tools/recon_bench.py --ptrs [--gib 1.0] [--out profiles/recon/recon_ptrs_bench.json]
    python tools/recon_bench.py --batch [--gib 1.0] [--out profiles/recon/recon_batch_bench.json]
    python tools/recon_bench.py --mixed [--gib 1.0] [--out profiles/recon/recon_mixed_bench.json]

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
allocator put the shards.

--batch: many small stripes under one plan, three ways, alternating in the same process as above.
Per shape and shard size (4 KiB, 64 KiB, 1 MiB) there are nstripes stripes, so many that all shards
together hold at least --gib GiB.  Every shard is a buffer of its own in one pool, placed by a random
permutation, so addresses are monotonic neither in the position nor in the stripe.
  loop     one ezrs_reconstruct_ptrs call per stripe through the C ABI, the host pointer arrays built
           once (the Python loop around the calls adds its own share to each of them)
  batch    one ezrs_reconstruct_ptrs_batch call on the same shards, its table built once by
           ezrs.ptr_table
  strided  one ezrs_reconstruct_interleaved call with nframes = nstripes on a frame tensor of the
           same bytes: the same arithmetic and no pointer fetch
  batch_inframe  the batch call on a table of pointers to the rows of the strided frames
           themselves: the same addresses as the strided call, so that the kernels' addressing is
           compared apart from where the shards lie
batch_over_loop, batch_over_strided and inframe_over_strided are the ratios of the medians.

--mixed: the single-drive rebuild of rotated placement, RS(255,251) shortened to len 10 (14 shards
per stripe), shards of 4 KiB and of 64 KiB, stripe s having lost position s % 14; with and without
`result`.  The shards lie as in --batch; the table of all stripes is resident.  Alternating:
  buckets    what a caller without the mixed call does: 14 ezrs_reconstruct_ptrs_batch calls, one per
             pattern, on 14 compacted tables.  The bucketing, the sub-tables and the per-bucket
             result buffers are built outside the timed region, which favours this way
  mixed      one ezrs_reconstruct_ptrs_mixed call on the resident table, plan_of[s] = s % 14
  batch_one  one ezrs_reconstruct_ptrs_batch call on the resident table under the plan that has lost
             position 0: as many stripes, one plan, the ceiling
  mixed_one  the mixed call with a set of that one plan and plan_of all zero: the same work as
             batch_one, through the directory
  batch_one_again  batch_one a second time in the alternation: how far two timings of the same call
             lie apart in this run
mixed_over_buckets, mixed_over_batch_one, mixed_one_over_batch_one and batch_again_over_batch_one are
the ratios of the medians; the spreads of the figures are next to them."""
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


BATCH_SHAPES = [
    # (name, codec, len, lost, with result)
    ("RS(255,251) len 10, 4 lost", lambda: ezrs.Codec.rs(255, 251), 10, [0, 3, 11, 13], True),
    ("RS(255,223) len 223, 4 lost, no result", lambda: ezrs.Codec.rs(255, 223), 223, [5, 100, 222, 240], False),
]
SHARD_BYTES = [4 << 10, 64 << 10, 1 << 20]


def main_batch(args):
    L, sp = ezrs.lib(), ezrs._stream_ptr(None)
    out = {"gib": args.gib, "reps": REPS, "device": torch.cuda.get_device_name(0), "results": []}
    for name, mk, length, lost, use_result in BATCH_SHAPES:
        for n in SHARD_BYTES:                       # 1-byte symbols
            c = mk()
            S, nlost = length + c.nroots, len(lost)
            ns = max(1, -(-int(args.gib * (1 << 30)) // (S * n)))
            frames = torch.empty((ns, S, n), dtype=torch.uint8, device="cuda")
            g = torch.Generator(device="cuda").manual_seed(1)
            step = max(1, (64 << 20) // (length * n))           # 64 Mi symbols at a time
            for s0 in range(0, ns, step):
                blk = frames[s0:s0 + step, :length]
                blk.copy_(torch.randint(0, 256, blk.shape, generator=g, device="cuda", dtype=torch.uint8))
            c.recon_plan(length, list(range(length, S))).reconstruct(frames)    # the parity
            good = frames[:, lost].clone()
            # the same shards, each a buffer of its own, placed by a random permutation of the slots
            perm = torch.randperm(ns * S, generator=torch.Generator().manual_seed(2))
            pool = torch.empty((ns * S, n), dtype=torch.uint8, device="cuda")
            pool[perm.cuda()] = frames.view(ns * S, n)
            slot = pool.unbind(0)
            pl = perm.view(ns, S).tolist()
            table, n_, align = ezrs.ptr_table([[slot[i] for i in row] for row in pl])
            assert n_ == n and align == 16
            host = table.cpu().numpy()
            rows = [host.ctypes.data + 8 * S * s for s in range(ns)]    # one host pointer array per stripe
            lost_slots = perm.view(ns, S)[:, lost].reshape(-1).cuda()
            table_in = (frames.data_ptr() + torch.arange(ns * S, dtype=torch.int64).view(ns, S) * n).cuda()
            plan = c.recon_plan(length, lost)
            res, res_p = (torch.empty(ns * n, dtype=torch.int32, device="cuda") if use_result else None
                          for _ in range(2))
            rp = res_p.data_ptr() if use_result else 0

            def loop():
                for s in range(ns):
                    L.ezrs_reconstruct_ptrs(plan._h, rows[s], n, rp + 4 * n * s if rp else None, sp)

            fns = {"loop": loop,
                   "batch": lambda: L.ezrs_reconstruct_ptrs_batch(plan._h, table.data_ptr(), S, n, ns, align,
                                                                  rp or None, sp),
                   "strided": lambda: plan.reconstruct(frames, result=res),
                   "batch_inframe": lambda: L.ezrs_reconstruct_ptrs_batch(
                       plan._h, table_in.data_ptr(), S, n, ns, 16, res.data_ptr() if use_result else None, sp)}
            inframe = ("strided", "batch_inframe")
            for what, fn in fns.items():            # each path once on garbage
                frames[:, lost] = 0x5A
                pool[lost_slots] = 0x5A
                if use_result:
                    res.fill_(77)
                    res_p.fill_(77)
                r = fn()
                assert r is None or r is res or r == 0, (name, n, what)
                torch.cuda.synchronize()
                got = frames[:, lost] if what in inframe else pool[lost_slots].view(ns, nlost, n)
                assert torch.equal(got, good), (name, n, what)
                if use_result:
                    assert bool(((res if what in inframe else res_p) == nlost).all()), (name, n, what)
            fg = figure(fns)
            torch.cuda.synchronize()
            assert torch.equal(pool[lost_slots].view(ns, nlost, n), good), (name, n)
            rec = {"shape": name, "len": length, "nroots": c.nroots, "nlost": nlost, "shard_bytes": n,
                   "nstripes": ns, "total_bytes": ns * S * n, "result": use_result}
            for k, v in fg.items():
                rec[f"t_{k}_ms"], rec[f"spread_{k}"] = v["median_s"] * 1e3, v["spread"]
            rec["batch_over_loop"] = fg["batch"]["median_s"] / fg["loop"]["median_s"]
            rec["batch_over_strided"] = fg["batch"]["median_s"] / fg["strided"]["median_s"]
            rec["inframe_over_strided"] = fg["batch_inframe"]["median_s"] / fg["strided"]["median_s"]
            rec["loop_us_per_stripe"] = fg["loop"]["median_s"] / ns * 1e6
            rec["iters"] = {k: v["iters"] for k, v in fg.items()}
            out["results"].append(rec)
            print(json.dumps(rec), flush=True)
            del frames, good, pool, slot, table, table_in, res, res_p, plan, c, fns, lost_slots
            torch.cuda.empty_cache()
    return out


MIXED_SHARD_BYTES = [4 << 10, 64 << 10]


def main_mixed(args):
    L, sp = ezrs.lib(), ezrs._stream_ptr(None)
    out = {"gib": args.gib, "reps": REPS, "device": torch.cuda.get_device_name(0), "results": []}
    name, length = "RS(255,251) len 10, stripe s lost [s % 14]", 10
    for use_result in (True, False):
        for n in MIXED_SHARD_BYTES:                 # 1-byte symbols
            c = ezrs.Codec.rs(255, 251)
            S = length + c.nroots
            ns = max(S, -(-int(args.gib * (1 << 30)) // (S * n)))
            frames = torch.empty((ns, S, n), dtype=torch.uint8, device="cuda")
            g = torch.Generator(device="cuda").manual_seed(1)
            step = max(1, (64 << 20) // (length * n))           # 64 Mi symbols at a time
            for s0 in range(0, ns, step):
                blk = frames[s0:s0 + step, :length]
                blk.copy_(torch.randint(0, 256, blk.shape, generator=g, device="cuda", dtype=torch.uint8))
            c.recon_plan(length, list(range(length, S))).reconstruct(frames)    # the parity
            perm = torch.randperm(ns * S, generator=torch.Generator().manual_seed(2))
            pool = torch.empty((ns * S, n), dtype=torch.uint8, device="cuda")
            pool[perm.cuda()] = frames.view(ns * S, n)
            good = pool.clone()
            del frames
            table = (pool.data_ptr() + perm.view(ns, S) * n).cuda()     # [ns, S] int64, resident
            assert pool.data_ptr() % 16 == 0
            plan_of = (torch.arange(ns, dtype=torch.int32) % S).cuda()
            lost_slots = perm.view(ns, S)[torch.arange(ns), torch.arange(ns) % S].cuda()   # slot of (s, s % S)
            first_slots = perm.view(ns, S)[:, 0].contiguous().cuda()                       # slot of (s, 0)
            plans = [c.recon_plan(length, [k]) for k in range(S)]
            rset, rset1 = ezrs.ReconSet(plans), ezrs.ReconSet(plans[:1])
            zeros = torch.zeros(ns, dtype=torch.int32, device="cuda")
            # the parent's way, prepared: per pattern the compacted table and a result buffer
            sub = [table[k::S].contiguous() for k in range(S)]
            res = torch.empty(ns * n, dtype=torch.int32, device="cuda") if use_result else None
            sub_res = [torch.empty(t.shape[0] * n, dtype=torch.int32, device="cuda") if use_result else None
                       for t in sub]
            rp = res.data_ptr() if use_result else None
            calls = [(plans[k]._h, sub[k].data_ptr(), sub[k].shape[0], sub_res[k].data_ptr() if use_result else None)
                     for k in range(S)]

            def buckets():
                for h, t, nb, r in calls:
                    L.ezrs_reconstruct_ptrs_batch(h, t, S, n, nb, 16, r, sp)

            def batch_one():
                return L.ezrs_reconstruct_ptrs_batch(plans[0]._h, table.data_ptr(), S, n, ns, 16, rp, sp)

            fns = {"buckets": buckets,
                   "mixed": lambda: L.ezrs_reconstruct_ptrs_mixed(rset._h, plan_of.data_ptr(), table.data_ptr(), S, n,
                                                                  ns, 16, rp, sp),
                   "batch_one": batch_one,
                   "mixed_one": lambda: L.ezrs_reconstruct_ptrs_mixed(rset1._h, zeros.data_ptr(), table.data_ptr(), S,
                                                                      n, ns, 16, rp, sp),
                   "batch_one_again": lambda: batch_one()}
            for what, fn in fns.items():            # each path once on garbage
                pool[first_slots if "one" in what else lost_slots] = 0x5A
                if use_result:
                    res.fill_(77)
                    for r in sub_res:
                        r.fill_(77)
                r = fn()
                assert r is None or r == 0, (n, what)
                torch.cuda.synchronize()
                assert torch.equal(pool, good), (n, what)
                if use_result:
                    for r in sub_res if what == "buckets" else [res]:
                        assert bool((r == 1).all()), (n, what)
            fg = figure(fns)
            torch.cuda.synchronize()
            assert torch.equal(pool, good), n
            rec = {"shape": name, "len": length, "nroots": c.nroots, "shard_bytes": n, "nstripes": ns,
                   "total_bytes": ns * S * n, "result": use_result}
            for k, v in fg.items():
                rec[f"t_{k}_ms"], rec[f"spread_{k}"] = v["median_s"] * 1e3, v["spread"]
                rec[f"{k}_GBps"] = ns * S * n / v["median_s"] / 1e9
            med = {k: v["median_s"] for k, v in fg.items()}
            rec["mixed_over_buckets"] = med["mixed"] / med["buckets"]
            rec["mixed_over_batch_one"] = med["mixed"] / med["batch_one"]
            rec["mixed_one_over_batch_one"] = med["mixed_one"] / med["batch_one"]
            rec["batch_again_over_batch_one"] = med["batch_one_again"] / med["batch_one"]
            rec["iters"] = {k: v["iters"] for k, v in fg.items()}
            out["results"].append(rec)
            print(json.dumps(rec), flush=True)
            del good, pool, table, sub, res, sub_res, plans, rset, rset1, c, fns, calls, lost_slots, first_slots
            torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--ptrs", action="store_true", help="the pointer form against the strided form")
    ap.add_argument("--batch", action="store_true", help="many small stripes: loop, batch call, strided call")
    ap.add_argument("--mixed", action="store_true",
                    help="rotated placement: a call per pattern, one mixed call, one single-plan call")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", "recon",
                                        "recon_mixed_bench.json" if args.mixed else
                                        "recon_batch_bench.json" if args.batch else
                                        "recon_ptrs_bench.json" if args.ptrs else "recon_bench.json")
    torch.cuda.set_device(0)
    if args.mixed:
        return write(args.out, main_mixed(args))
    if args.batch:
        return write(args.out, main_batch(args))
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

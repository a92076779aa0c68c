#!/usr/bin/env python3
"""In-place parity update of a striped frame (Update.apply) against the two ways to re-encode the
whole stripe: the all-parity reconstruction (Recon.reconstruct without result, the fastest
re-encode the project has) and the staged Codec.encode_interleaved, on the same buffers.  Neither
comparison shares a kernel with the update.

    python tools/update_bench.py [--gib 1.0] [--out profiles/update/update_bench.json]
    python tools/update_bench.py --ptrs [--gib 1.0] [--out profiles/update/update_ptrs_bench.json]
    python tools/update_bench.py --batch [--gib 1.0] [--out profiles/update/update_batch_bench.json]
    python tools/update_bench.py --mixed [--gib 1.0] [--out profiles/update/update_mixed_bench.json]

One frame per shape: len + nroots shards of `depth` symbols, symbol stride = depth, sized so that
the frame holds at least --gib GiB (well past the 256 MiB Infinity Cache); newsyms is a packed
[nchanged, depth] buffer.  Device events; every call is warmed; the three calls alternate in the
same process, `reps` repeats per figure sized so that each figure has at least 0.5 s of timed work;
the figure is the median, the spread (max - min) / median.  Repeats of the update find the new
symbols already in place (a zero delta), which changes nothing in what it loads, computes or
stores.  GB/s counts the frame's bytes once; hbm_fraction counts the bytes the update must move
(old and new changed symbols and the parity read, changed symbols and parity written) against
8 TB/s.

--ptrs: the pointer form (ezrs_update_ptrs) against the strided form instead, same shapes and the
same data; the pointer form has only the changed shards, the parity shards and the new symbols,
each an allocation of its own.  The calls alternate in the same process as above; the pointer form
is called through the C ABI with its pointer arrays built once, as a C caller has them;
ptrs_over_strided is the ratio of the medians.  A third figure, ptrs_inframe, is the pointer form on
pointers to the rows of the strided frame and of its newsyms: the same addresses as the strided
form, so that the kernels' addressing is compared apart from where the allocator put the shards.

--batch: many small stripes under one plan, three ways, alternating in the same process as above.
Per shape and shard size (4 KiB, 64 KiB, 1 MiB) there are nstripes stripes, so many that all shards
of the stripes together hold at least --gib GiB; on the device, for the pointer forms, are only the
changed shards, the parity shards and the new symbols, each a buffer of its own in one pool, placed by
a random permutation.
  loop     one ezrs_update_ptrs call per stripe through the C ABI, the host pointer arrays built
           once (the Python loop around the calls adds its own share to each of them)
  batch    one ezrs_update_ptrs_batch call on the same shards, its tables built once by
           ezrs.ptr_table
  strided  one ezrs_update_interleaved call with nframes = nstripes on frame tensors of the same
           bytes: the same arithmetic and no pointer fetch
  batch_inframe  the batch call on tables of pointers to the rows of the strided frames and of
           their newsyms: the same addresses as the strided call, so that the kernels' addressing
           is compared apart from where the shards lie
batch_over_loop, batch_over_strided and inframe_over_strided are the ratios of the medians.

--mixed: a flush of small writes in which every stripe has a change set of its own, RS(255,251) at
len 10 with shards of 4 KiB and 64 KiB, so many stripes that the shards the update touches (changed,
parity, new symbols; nothing else is on the device) hold at least --gib GiB, each a buffer of its
own in one pool, placed by a random permutation.  Two mixes, ten plans each, stripe s under plan
s % 10: "one changed" (stripe s changes position s % 10) and "1..5 changed" (stripe s changes
1 + s % 5 positions, (s + 3 i) % 10: five kernel bodies in one launch).  Five calls alternate in
the same process as above:
  buckets    ten ezrs_update_ptrs_batch calls, one per plan, each on its own compacted table and
             new_table; the bucketing and the compacted tables are made once, outside the timed region
  mixed      one ezrs_update_ptrs_mixed call on the resident tables, ten plans
  batch_one  one ezrs_update_ptrs_batch call with every stripe under plan 0 (one changed position),
             on a table that names each stripe's first changed shard at that plan's position: the
             same buffers, and what a call costs that fetches no plan
  mixed_one  the mixed call with a set of that one plan and plan_of all zero, on the same table
  batch_one_again   batch_one a second time: what two timings of the same call differ by
mixed_over_buckets, mixed_one_over_batch_one and batch_again_over_batch_one are the ratios of the
medians.  Not measured: the host's bucketing, plans with large tables."""
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
    # (name, codec, len, changed)
    ("RS(255,251) len 10, 1 changed", lambda: ezrs.Codec.rs(255, 251), 10, [3]),
    ("RS(255,252) len 17, 1 changed", lambda: ezrs.Codec.rs(255, 252), 17, [9]),
    ("RS(255,223) len 223, 1 changed", lambda: ezrs.Codec.rs(255, 223), 223, [100]),
    ("RS(255,223) len 223, 4 changed", lambda: ezrs.Codec.rs(255, 223), 223, [5, 100, 101, 222]),
    ("RS_CCSDS(255,223) len 223, 1 changed", lambda: ezrs.Codec.ccsds(223, True), 223, [100]),
    ("RS(1023,1007) len 100, 1 changed", lambda: ezrs.Codec.rs(1023, 1007), 100, [50]),
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


def rand_rows(rows, depth, w, mask, g):
    """[rows, depth] random symbols of w bytes."""
    dt = torch.uint8 if w == 1 else torch.int16     # 16-bit symbols as int16: the bits are what counts
    out = torch.empty((rows, depth), dtype=dt, device="cuda")
    for s in range(rows):
        out[s] = torch.randint(0, mask + 1, (depth,), generator=g, device="cuda", dtype=torch.int32).to(dt)
    return out


def main_ptrs(args):
    L, sp = ezrs.lib(), ezrs._stream_ptr(None)
    out = {"gib": args.gib, "reps": REPS, "device": torch.cuda.get_device_name(0), "results": []}
    for name, mk, length, changed in SHAPES:
        c = mk()
        w, NR, nchg = c.info.datum_bytes, c.nroots, len(changed)
        S = length + NR
        depth = (int(args.gib * (1 << 30)) // (S * w) + 1023) // 1024 * 1024
        g = torch.Generator(device="cuda").manual_seed(1)
        shards = torch.empty((S, depth), dtype=torch.uint8 if w == 1 else torch.int16, device="cuda")
        shards[:length] = rand_rows(length, depth, w, c.nn, g)
        frames = shards[None]
        parity = list(range(length, S))
        plan = c.update_plan(length, changed)
        c.recon_plan(length, parity).reconstruct(frames)        # the first parity
        newsyms = rand_rows(nchg, depth, w, c.nn, g)[None]
        used = changed + parity
        own = {p: shards[p].clone() for p in used}              # only what the call needs, each its own
        new = [newsyms[0, r].clone() for r in range(nchg)]
        arr = (C.c_void_p * S)(*[own[p].data_ptr() if p in own else None for p in range(S)])
        narr = (C.c_void_p * nchg)(*[t.data_ptr() for t in new])
        arr_in = (C.c_void_p * S)(*[shards[p].data_ptr() if p in own else None for p in range(S)])
        narr_in = (C.c_void_p * nchg)(*[newsyms[0, r].data_ptr() for r in range(nchg)])
        fns = {"strided": lambda: plan.apply(frames, newsyms),
               "ptrs": lambda: L.ezrs_update_ptrs(plan._h, arr, narr, depth, sp),
               "ptrs_inframe": lambda: L.ezrs_update_ptrs(plan._h, arr_in, narr_in, depth, sp)}
        for what, fn in fns.items():                # each path once, a nonzero delta
            assert fn() in (0, None), (name, what)
        torch.cuda.synchronize()
        assert torch.equal(torch.stack([own[p] for p in used]), shards[used]), name
        fg = figure(fns)
        torch.cuda.synchronize()
        assert torch.equal(torch.stack([own[p] for p in used]), shards[used]), name
        rec = {"shape": name, "len": length, "nroots": NR, "nchanged": nchg, "depth": depth,
               "frame_bytes": S * depth * w, "update_bytes_moved": (3 * nchg + 2 * NR) * depth * w}
        for k, v in fg.items():
            rec[f"t_{k}_ms"], rec[f"spread_{k}"] = v["median_s"] * 1e3, v["spread"]
        rec["ptrs_over_strided"] = fg["ptrs"]["median_s"] / fg["strided"]["median_s"]
        rec["inframe_over_strided"] = fg["ptrs_inframe"]["median_s"] / fg["strided"]["median_s"]
        rec["iters"] = {k: v["iters"] for k, v in fg.items()}
        out["results"].append(rec)
        print(json.dumps(rec), flush=True)
        del shards, frames, own, new, newsyms, plan, c, fns
        torch.cuda.empty_cache()
    return out


BATCH_SHAPES = [
    # (name, codec, len, changed)
    ("RS(255,251) len 10, 1 changed", lambda: ezrs.Codec.rs(255, 251), 10, [3]),
    ("RS(255,223) len 223, 1 changed", lambda: ezrs.Codec.rs(255, 223), 223, [100]),
    ("RS(1023,1007) len 100, 1 changed", lambda: ezrs.Codec.rs(1023, 1007), 100, [50]),
]
SHARD_BYTES = [4 << 10, 64 << 10, 1 << 20]


def main_batch(args):
    L, sp = ezrs.lib(), ezrs._stream_ptr(None)
    out = {"gib": args.gib, "reps": REPS, "device": torch.cuda.get_device_name(0), "results": []}
    for name, mk, length, changed in BATCH_SHAPES:
        for sb in SHARD_BYTES:
            c = mk()
            w, NR, nchg = c.info.datum_bytes, c.nroots, len(changed)
            S, n = length + NR, sb // w
            ns = max(1, -(-int(args.gib * (1 << 30)) // (S * sb)))
            dt = torch.uint8 if w == 1 else torch.int16
            g = torch.Generator(device="cuda").manual_seed(1)
            frames = torch.empty((ns, S, n), dtype=dt, device="cuda")
            step = max(1, (64 << 20) // (length * n))           # 64 Mi symbols at a time
            for s0 in range(0, ns, step):
                blk = frames[s0:s0 + step, :length]
                blk.copy_(torch.randint(0, c.nn + 1, blk.shape, generator=g, device="cuda", dtype=torch.int32))
            parity = list(range(length, S))
            c.recon_plan(length, parity).reconstruct(frames)            # the first parity
            newsyms = torch.randint(0, c.nn + 1, (ns, nchg, n), generator=g, device="cuda",
                                    dtype=torch.int32).to(dt)
            used = changed + parity
            U = len(used) + nchg                    # buffers per stripe: changed | parity | new symbols
            perm = torch.randperm(ns * U, generator=torch.Generator().manual_seed(2))
            pool = torch.empty((ns * U, n), dtype=dt, device="cuda")
            pool[perm.cuda()] = torch.cat([frames[:, used], newsyms], dim=1).reshape(ns * U, n)
            orig, frames0 = pool.clone(), frames[:, used].clone()
            slot = pool.unbind(0)
            pl = perm.view(ns, U).tolist()
            at = {p: i for i, p in enumerate(used)}
            table, n_, a1 = ezrs.ptr_table([[slot[row[at[p]]] if p in at else None for p in range(S)]
                                            for row in pl], optional=[p for p in range(S) if p not in at])
            ntable, _, a2 = ezrs.ptr_table([[slot[i] for i in row[len(used):]] for row in pl])
            align = min(a1, a2)
            assert n_ == n and align == 16
            host, nhost = table.cpu().numpy(), ntable.cpu().numpy()
            rows = [(host.ctypes.data + 8 * S * s, nhost.ctypes.data + 8 * nchg * s) for s in range(ns)]
            used_slots = perm.view(ns, U)[:, :len(used)].reshape(-1).cuda()
            table_in = (frames.data_ptr() + torch.arange(ns * S, dtype=torch.int64).view(ns, S) * sb).cuda()
            ntable_in = (newsyms.data_ptr() + torch.arange(ns * nchg, dtype=torch.int64).view(ns, nchg) * sb).cuda()
            plan = c.update_plan(length, changed)

            def loop():
                for a, b in rows:
                    L.ezrs_update_ptrs(plan._h, a, b, n, sp)

            fns = {"loop": loop,
                   "batch": lambda: L.ezrs_update_ptrs_batch(plan._h, table.data_ptr(), S, ntable.data_ptr(), nchg,
                                                             n, ns, align, sp),
                   "strided": lambda: plan.apply(frames, newsyms),
                   "batch_inframe": lambda: L.ezrs_update_ptrs_batch(plan._h, table_in.data_ptr(), S,
                                                                     ntable_in.data_ptr(), nchg, n, ns, 16, sp)}
            inframe = ("strided", "batch_inframe")
            want = None
            for what, fn in fns.items():            # each path once, a nonzero delta, on the same input
                pool.copy_(orig)
                frames[:, used] = frames0
                assert fn() in (0, None), (name, sb, what)
                torch.cuda.synchronize()
                got = frames[:, used].clone() if what in inframe else pool[used_slots].view(ns, len(used), n)
                want = got.clone() if want is None else want
                assert torch.equal(got, want) and not torch.equal(got, frames0), (name, sb, what)
            fg = figure(fns)
            torch.cuda.synchronize()
            assert torch.equal(pool[used_slots].view(ns, len(used), n), want), (name, sb)
            rec = {"shape": name, "len": length, "nroots": NR, "nchanged": nchg, "shard_bytes": sb,
                   "nstripes": ns, "total_bytes": ns * S * sb, "update_bytes_moved": (3 * nchg + 2 * NR) * ns * sb}
            for k, v in fg.items():
                rec[f"t_{k}_ms"], rec[f"spread_{k}"] = v["median_s"] * 1e3, v["spread"]
            rec["batch_over_loop"] = fg["batch"]["median_s"] / fg["loop"]["median_s"]
            rec["batch_over_strided"] = fg["batch"]["median_s"] / fg["strided"]["median_s"]
            rec["inframe_over_strided"] = fg["batch_inframe"]["median_s"] / fg["strided"]["median_s"]
            rec["loop_us_per_stripe"] = fg["loop"]["median_s"] / ns * 1e6
            rec["iters"] = {k: v["iters"] for k, v in fg.items()}
            out["results"].append(rec)
            print(json.dumps(rec), flush=True)
            del frames, newsyms, pool, orig, frames0, slot, table, ntable, table_in, ntable_in, plan, c, fns
            del used_slots, want
            torch.cuda.empty_cache()
    return out


MIXED_SHARD_BYTES = [4 << 10, 64 << 10]
MIXES = [
    # (name, the changed positions of stripe s)
    ("one changed: [s % 10]", lambda s: [s % 10]),
    ("1..5 changed: 1 + s % 5 positions (s + 3 i) % 10", lambda s: [(s + 3 * i) % 10 for i in range(1 + s % 5)]),
]


def main_mixed(args):
    L, sp = ezrs.lib(), ezrs._stream_ptr(None)
    out = {"gib": args.gib, "reps": REPS, "device": torch.cuda.get_device_name(0), "results": []}
    length, NP = 10, 10
    for mix, changed_of in MIXES:
        for n in MIXED_SHARD_BYTES:                 # 1-byte symbols
            c = ezrs.Codec.rs(255, 251)
            NR = c.nroots
            S = length + NR
            lists = [changed_of(k) for k in range(NP)]
            assert all(changed_of(k) == lists[k % NP] for k in range(4 * NP))
            per10 = sum(2 * len(ch) + NR for ch in lists)               # buffers of ten stripes
            ns = max(NP, -(-int(args.gib * (1 << 30)) * NP // (per10 * n)))
            maxchg = max(len(ch) for ch in lists)
            # slots of stripe s: changed [k] | parity [NR] | new symbols [k]
            first, T = [], 0
            for s in range(ns):
                first.append(T)
                T += 2 * len(lists[s % NP]) + NR
            perm = torch.randperm(T, generator=torch.Generator().manual_seed(2)).tolist()
            g = torch.Generator(device="cuda").manual_seed(1)
            pool = torch.empty((T, n), dtype=torch.uint8, device="cuda")
            step = max(1, (256 << 20) // n)
            for t0 in range(0, T, step):
                blk = pool[t0:t0 + step]
                blk.copy_(torch.randint(0, 256, blk.shape, generator=g, device="cuda", dtype=torch.uint8))
            assert pool.data_ptr() % 16 == 0
            base = pool.data_ptr()
            tab = [[0] * S for _ in range(ns)]      # an entry no plan of the stripe uses: NULL
            tab1 = [[0] * S for _ in range(ns)]
            ntab = [[0] * maxchg for _ in range(ns)]
            written = []
            for s in range(ns):
                ch = lists[s % NP]
                k, f = len(ch), first[s]
                for r, p in enumerate(ch):
                    tab[s][p] = base + perm[f + r] * n
                    ntab[s][r] = base + perm[f + k + NR + r] * n
                tab1[s][lists[0][0]] = base + perm[f] * n
                for i in range(NR):
                    tab[s][length + i] = tab1[s][length + i] = base + perm[f + k + i] * n
                written += perm[f:f + k + NR]
            table = torch.tensor(tab, dtype=torch.int64).cuda()
            table_one = torch.tensor(tab1, dtype=torch.int64).cuda()
            ntable = torch.tensor(ntab, dtype=torch.int64).cuda()
            written = torch.tensor(written, dtype=torch.int64).cuda()
            del tab, tab1, ntab
            orig = pool.clone()
            plans = [c.update_plan(length, ch) for ch in lists]
            assert len(lists[0]) == 1
            uset, uset1 = ezrs.UpdateSet(plans), ezrs.UpdateSet(plans[:1])
            plan_of = (torch.arange(ns, dtype=torch.int32) % NP).cuda()
            zeros = torch.zeros(ns, dtype=torch.int32, device="cuda")
            # the parent's way, prepared: per plan the compacted table and new_table
            sub = [(table[k::NP].contiguous(), ntable[k::NP].contiguous()) for k in range(NP)]
            calls = [(plans[k]._h, sub[k][0].data_ptr(), sub[k][1].data_ptr(), sub[k][0].shape[0]) for k in range(NP)]

            def buckets():
                for h, t, nt, nb in calls:
                    L.ezrs_update_ptrs_batch(h, t, S, nt, maxchg, n, nb, 16, sp)

            def batch_one():
                return L.ezrs_update_ptrs_batch(plans[0]._h, table_one.data_ptr(), S, ntable.data_ptr(), maxchg, n,
                                                ns, 16, sp)

            fns = {"buckets": buckets,
                   "mixed": lambda: L.ezrs_update_ptrs_mixed(uset._h, plan_of.data_ptr(), table.data_ptr(), S,
                                                             ntable.data_ptr(), maxchg, n, ns, 16, sp),
                   "batch_one": batch_one,
                   "mixed_one": lambda: L.ezrs_update_ptrs_mixed(uset1._h, zeros.data_ptr(), table_one.data_ptr(), S,
                                                                 ntable.data_ptr(), maxchg, n, ns, 16, sp),
                   "batch_one_again": lambda: batch_one()}
            want = {}
            for what, fn in fns.items():            # each path once, a nonzero delta, on the same input
                pool.copy_(orig)
                r = fn()
                assert r is None or r == 0, (mix, n, what)
                torch.cuda.synchronize()
                got = pool[written]
                kind = "one" if "one" in what else "mix"
                want.setdefault(kind, got)
                assert torch.equal(got, want[kind]) and not torch.equal(got, orig[written]), (mix, n, what)
                del got
            fg = figure(fns)
            torch.cuda.synchronize()
            rec = {"mix": mix, "shape": "RS(255,251) len 10", "len": length, "nroots": NR, "nplans": NP,
                   "shard_bytes": n, "nstripes": ns, "touched_bytes": T * n,
                   "bytes_moved_mixed": sum(3 * len(lists[s % NP]) + 2 * NR for s in range(ns)) * n,
                   "bytes_moved_one": (3 + 2 * NR) * ns * n}
            for k, v in fg.items():
                rec[f"t_{k}_ms"], rec[f"spread_{k}"] = v["median_s"] * 1e3, v["spread"]
            med = {k: v["median_s"] for k, v in fg.items()}
            rec["mixed_GBps_moved"] = rec["bytes_moved_mixed"] / med["mixed"] / 1e9
            rec["batch_one_GBps_moved"] = rec["bytes_moved_one"] / med["batch_one"] / 1e9
            rec["mixed_over_buckets"] = med["mixed"] / med["buckets"]
            rec["mixed_one_over_batch_one"] = med["mixed_one"] / med["batch_one"]
            rec["batch_again_over_batch_one"] = med["batch_one_again"] / med["batch_one"]
            rec["iters"] = {k: v["iters"] for k, v in fg.items()}
            out["results"].append(rec)
            print(json.dumps(rec), flush=True)
            del pool, orig, table, table_one, ntable, written, sub, calls, plans, uset, uset1, c, fns, want
            torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--ptrs", action="store_true", help="the pointer form against the strided form")
    ap.add_argument("--batch", action="store_true", help="many small stripes: loop, batch call, strided call")
    ap.add_argument("--mixed", action="store_true",
                    help="a change set per stripe: a call per plan, one mixed call, one single-plan call")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", "update",
                                        "update_mixed_bench.json" if args.mixed else
                                        "update_batch_bench.json" if args.batch else
                                        "update_ptrs_bench.json" if args.ptrs else "update_bench.json")
    torch.cuda.set_device(0)
    if args.mixed:
        return write(args.out, main_mixed(args))
    if args.batch:
        return write(args.out, main_batch(args))
    if args.ptrs:
        return write(args.out, main_ptrs(args))
    out = {"gib": args.gib, "reps": REPS, "device": torch.cuda.get_device_name(0), "results": []}
    for name, mk, length, changed in SHAPES:
        c = mk()
        w, NR, nchg = c.info.datum_bytes, c.nroots, len(changed)
        S = length + NR
        depth = (int(args.gib * (1 << 30)) // (S * w) + 1023) // 1024 * 1024
        g = torch.Generator(device="cuda").manual_seed(1)
        shards = torch.empty((S, depth), dtype=torch.uint8 if w == 1 else torch.int16, device="cuda")
        shards[:length] = rand_rows(length, depth, w, c.nn, g)
        frames = shards[None]
        parity = list(range(length, S))
        plan = c.update_plan(length, changed)
        reenc = c.recon_plan(length, parity)
        reenc.reconstruct(frames)                   # the first parity
        newsyms = rand_rows(nchg, depth, w, c.nn, g)[None]
        # each path once, checked against the others: the update's parity must be what both
        # re-encodes write on the new data
        old = shards[changed].clone()
        plan.apply(frames, newsyms)
        torch.cuda.synchronize()
        assert torch.equal(shards[changed], newsyms[0]), name
        good = shards[parity].clone()
        for what, fn in (("reencode_recon", lambda: reenc.reconstruct(frames)),
                         ("reencode_staged", lambda: c.encode_interleaved(frames))):
            shards[parity] = 0x5A
            fn()
            torch.cuda.synchronize()
            assert torch.equal(shards[parity], good), (name, what)
        plan.apply(frames, old[None])               # and back: a nonzero delta once more
        reenc.reconstruct(frames)
        torch.cuda.synchronize()
        fg = figure({"update": lambda: plan.apply(frames, newsyms),
                     "reencode_recon": lambda: reenc.reconstruct(frames),
                     "reencode_staged": lambda: c.encode_interleaved(frames)})
        torch.cuda.synchronize()
        assert torch.equal(shards[parity], good), name
        fbytes = S * depth * w
        moved = (3 * nchg + 2 * NR) * depth * w     # old + new read, new written; parity read + written
        t_u, t_r, t_e = (fg[k]["median_s"] for k in ("update", "reencode_recon", "reencode_staged"))
        rec = {"shape": name, "len": length, "nroots": NR, "nchanged": nchg, "depth": depth,
               "frame_bytes": fbytes, "update_bytes_moved": moved,
               "t_update_ms": t_u * 1e3, "t_reencode_recon_ms": t_r * 1e3, "t_reencode_staged_ms": t_e * 1e3,
               "update_GBps": fbytes / t_u / 1e9, "reencode_recon_GBps": fbytes / t_r / 1e9,
               "reencode_staged_GBps": fbytes / t_e / 1e9,
               "update_hbm_fraction": moved / t_u / HBM,
               "recon_over_update": t_r / t_u, "staged_over_update": t_e / t_u,
               "spread_update": fg["update"]["spread"], "spread_reencode_recon": fg["reencode_recon"]["spread"],
               "spread_reencode_staged": fg["reencode_staged"]["spread"],
               "iters": {k: v["iters"] for k, v in fg.items()}}
        out["results"].append(rec)
        print(json.dumps(rec), flush=True)
        del shards, frames, good, old, newsyms, plan, reenc, c
        torch.cuda.empty_cache()
    write(args.out, out)


def write(path, out):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()

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
GB/s counts the frames' bytes once (ncw * 255).

    python tools/il_bench.py --ptrs [--out profiles/il/il_ptrs_bench.json]

The pointer forms of the staged decode (ezrs_decode_ptrs / ezrs_decode_ptrs_batch) against
ezrs_decode_interleaved on the same symbols, same method: see ptrs_main.

    python tools/il_bench.py --select [--out profiles/il/il_select_bench.json]

The scrub with selection (verify, ezrs_select_failed, ezrs_decode_ptrs_select) against
ezrs_decode_ptrs_batch over all stripes, same method: see select_main."""
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


# --ptrs: (name, codec, len, stripes, shard_len, align, one-stripe form)
PTRS_SHAPES = [
    ("RS(255,223) 1 x 1Mi a16", (255, 223), 223, 1, 1 << 20, 16, True),
    ("RS(255,251) 10+4 1024 x 64Ki a16", (255, 251), 10, 1024, 1 << 16, 16, False),
    ("RS(255,251) 10+4 1024 x 64Ki a1", (255, 251), 10, 1024, 1 << 16, 1, False),
    ("RS(255,251) 10+4 64Ki x 256 a16", (255, 251), 10, 1 << 16, 256, 16, False),
]


def ptrs_main(out_path):
    """The pointer forms of the staged decode against ezrs_decode_interleaved on the same symbols
    laid out with sym_stride = shard_len: clean decode and decode with 1 % of the codewords
    corrupted (one symbol each).  The corrupted figure times [put the corruption back, decode] in
    both arms: a decode repairs its input, and the put is the same indexed store of 1 % of the
    codewords' bytes into either layout.  Every shard is a buffer of its own, 16 bytes of gap to the
    next; align 1 puts every shard at an odd address."""
    out = {"reps": REPS, "device": torch.cuda.get_device_name(0), "results": []}
    for name, (n, k), L, F, D, align, one in PTRS_SHAPES:
        c = ezrs.Codec.rs(n, k)
        S, ncw = L + c.nroots, F * D
        g = torch.Generator(device="cuda").manual_seed(2)
        fr = torch.randint(0, 256, (F, S, D), generator=g, device="cuda", dtype=torch.int32).to(torch.uint8)
        c.encode_interleaved(fr)
        pitch, off = D + 16, 0 if align == 16 else 1
        arena = torch.zeros((F, S, pitch), dtype=torch.uint8, device="cuda")
        arena[:, :, off:off + D] = fr
        base = arena.data_ptr() + off
        table = (base + torch.arange(F * S, dtype=torch.int64, device="cuda") * pitch).view(F, S)
        shards = [arena[0, p, off:off + D] for p in range(S)] if one else None
        res_p = torch.empty(ncw, dtype=torch.int32, device="cuda")
        res_s = torch.empty(ncw, dtype=torch.int32, device="cuda")
        # 1 % of the codewords, one wrong symbol each: flat indices into both layouts
        nbad = max(1, ncw // 100)
        kk = torch.randperm(ncw, generator=g, device="cuda")[:nbad]
        pp = torch.randint(0, S, (nbad,), generator=g, device="cuda")
        f, j = kk // D, kk % D
        ix_s, ix_p = (f * S + pp) * D + j, (f * S + pp) * pitch + off + j
        flat_s, flat_p = fr.view(-1), arena.view(-1)
        wrong = flat_s[ix_s] ^ 0x5A

        if one:
            def dec_p():
                c.decode_ptrs(shards, L, result=res_p)
        else:
            def dec_p():
                c.decode_ptrs_batch(table, L, D, align=align, result=res_p)

        def dec_s():
            c.decode_interleaved(fr, result=res_s)

        def bad_p():
            flat_p[ix_p] = wrong
            dec_p()

        def bad_s():
            flat_s[ix_s] = wrong
            dec_s()

        clean = figure({"ptrs": dec_p, "strided": dec_s})
        torch.cuda.synchronize()
        assert int((res_p != 0).sum()) == 0 and int((res_s != 0).sum()) == 0
        bad = figure({"ptrs": bad_p, "strided": bad_s})
        torch.cuda.synchronize()
        assert int(res_p.sum()) == nbad == int(res_s.sum()) and torch.equal(res_p, res_s)
        assert torch.equal(arena[:, :, off:off + D], fr)
        for op, fg in (("decode_clean", clean), ("decode_1pct", bad)):
            tp, ts = fg["ptrs"]["median_s"], fg["strided"]["median_s"]
            rec = {"shape": name, "len": L, "nstripes": F, "shard_len": D, "align": align,
                   "form": "ezrs_decode_ptrs" if one else "ezrs_decode_ptrs_batch", "op": op,
                   "workspace_bytes": c.decode_ptrs_workspace_bytes(L, D, F),
                   "t_ptrs_ms": tp * 1e3, "t_strided_ms": ts * 1e3, "ratio": tp / ts,
                   "ptrs_GBps": ncw * S / tp / 1e9, "strided_GBps": ncw * S / ts / 1e9,
                   "spread_ptrs": fg["ptrs"]["spread"], "spread_strided": fg["strided"]["spread"]}
            out["results"].append(rec)
            print(json.dumps(rec), flush=True)
        del fr, arena, table, shards, res_p, res_s, flat_s, flat_p
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", out_path)


# --select: the fast-path shapes of PTRS_SHAPES and the corrupted fractions
SELECT_SHAPES = [s for s in PTRS_SHAPES if s[5] == 16]
SELECT_FRACTIONS = [1e-2, 1e-4]
CROSSOVER_SHAPE = "RS(255,251) 10+4 1024 x 64Ki a16"


class SelectShape:
    """One shape of --select: the stripes in buffers of their own, the table, and the two scrubs."""

    def __init__(self, name, nk, L, F, D):
        self.name, self.L, self.F, self.D = name, L, F, D
        self.c = c = ezrs.Codec.rs(*nk)
        self.S, self.ncw = S, ncw = L + c.nroots, F * D
        self.g = g = torch.Generator(device="cuda").manual_seed(2)
        self.fr = fr = torch.randint(0, 256, (F, S, D), generator=g, device="cuda", dtype=torch.int32).to(torch.uint8)
        c.encode_interleaved(fr)
        self.pitch = pitch = D + 16
        self.arena = arena = torch.zeros((F, S, pitch), dtype=torch.uint8, device="cuda")
        arena[:, :, :D] = fr
        self.table = (arena.data_ptr() + torch.arange(F * S, dtype=torch.int64, device="cuda") * pitch).view(F, S)
        self.plan = c.recon_plan(L, [])                  # nlost = 0: the verify
        self.ver = torch.empty(ncw, dtype=torch.int32, device="cuda")
        self.res_full = torch.empty(ncw, dtype=torch.int32, device="cuda")
        self.count = torch.empty(1, dtype=torch.int64, device="cuda")

    def measure(self, fraction):
        """One symbol wrong in `fraction` of the codewords: both arms time [put the corruption back,
        scrub]; returns the record."""
        c, L, F, D, S, ncw, g = self.c, self.L, self.F, self.D, self.S, self.ncw, self.g
        nbad = min(ncw, max(1, int(round(ncw * fraction))))
        kk = torch.randperm(ncw, generator=g, device="cuda")[:nbad]
        pp = torch.randint(0, S, (nbad,), generator=g, device="cuda")
        ix = ((kk // D) * S + pp) * self.pitch + kk % D
        flat = self.arena.view(-1)
        wrong = flat[ix] ^ 0x5A
        cap = 2 * nbad
        sel = torch.empty(cap, dtype=torch.int64, device="cuda")
        res_sel = torch.empty(cap, dtype=torch.int32, device="cuda")
        table, ver, count, res_full, plan = self.table, self.ver, self.count, self.res_full, self.plan

        def select():
            flat[ix] = wrong
            plan.reconstruct_ptrs_batch(table, D, align=16, result=ver)
            c.select_failed(ver, cap=cap, sel=sel, count=count)
            c.decode_ptrs_select(table, L, D, sel, count=count, result=res_sel)

        def full():
            flat[ix] = wrong
            c.decode_ptrs_batch(table, L, D, align=16, result=res_full)

        fg = figure({"select": select, "full": full})
        torch.cuda.synchronize()
        assert int(count[0]) == nbad == int(res_full.sum()) and bool((res_sel[:nbad] == 1).all())
        assert bool((res_sel[nbad:] == 0).all()) and torch.equal(sel[:nbad], kk.sort().values)
        assert torch.equal(self.arena[:, :, :D], self.fr)
        ts, tf = fg["select"]["median_s"], fg["full"]["median_s"]
        return {"shape": self.name, "len": L, "nstripes": F, "shard_len": D, "fraction": fraction,
                "corrupted_codewords": nbad, "cap": cap,
                "workspace_bytes_select": c.decode_select_workspace_bytes(L, cap) + c.select_workspace_bytes(ncw),
                "workspace_bytes_full": c.decode_ptrs_workspace_bytes(L, D, F),
                "t_select_ms": ts * 1e3, "t_full_ms": tf * 1e3, "ratio": ts / tf,
                "spread_select": fg["select"]["spread"], "spread_full": fg["full"]["spread"]}


def select_main(out_path):
    """The scrub with selection against the full decode, on the fast-path shapes of --ptrs, one
    symbol corrupted in 1 % and in 0.01 % of the codewords.
      select  verify (reconstruct_ptrs_batch under an nlost = 0 plan, with result) + select_failed +
              decode_ptrs_select with the device count, cap = 2 x the corrupted codewords
      full    decode_ptrs_batch over all stripes (unchanged code)
    Then the corrupted fraction at which both cost the same on the 64 KiB shape, by bisection over
    the fraction (geometric midpoints) to within a factor of 2."""
    out = {"reps": REPS, "device": torch.cuda.get_device_name(0), "results": [], "crossover": None}
    for name, nk, L, F, D, _, _ in SELECT_SHAPES:
        sh = SelectShape(name, nk, L, F, D)
        for fraction in SELECT_FRACTIONS:
            rec = sh.measure(fraction)
            out["results"].append(rec)
            print(json.dumps(rec), flush=True)
        if name == CROSSOVER_SHAPE:
            lo, hi, steps = 1e-4, 0.5, []               # select wins at lo, loses at hi?
            ends = {f: sh.measure(f) for f in (lo, hi)}
            steps += list(ends.values())
            if ends[lo]["ratio"] >= 1 or ends[hi]["ratio"] < 1:
                verdict = "below 1e-4" if ends[lo]["ratio"] >= 1 else "above 0.5"
            else:
                while hi / lo > 2:
                    mid = (lo * hi) ** 0.5
                    rec = sh.measure(mid)
                    steps.append(rec)
                    lo, hi = (mid, hi) if rec["ratio"] < 1 else (lo, mid)
                verdict = "between"
            out["crossover"] = {"shape": name, "verdict": verdict, "fraction_lo": lo, "fraction_hi": hi,
                                "steps": steps}
            print(json.dumps(out["crossover"]), flush=True)
        del sh
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", out_path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncw", type=int, default=1 << 20)
    ap.add_argument("--select", action="store_true",
                    help="the scrub with selection (verify, select_failed, decode_ptrs_select) against the full decode")
    ap.add_argument("--ptrs", action="store_true",
                    help="the pointer forms of the staged decode against the strided form")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    if args.select:
        return select_main(args.out or os.path.join(ROOT, "profiles", "il", "il_select_bench.json"))
    if args.ptrs:
        return ptrs_main(args.out or os.path.join(ROOT, "profiles", "il", "il_ptrs_bench.json"))
    args.out = args.out or os.path.join(ROOT, "profiles", "il", "il_bench.json")
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

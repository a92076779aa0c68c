#!/usr/bin/env python3
"""VALU / scratch / VGPR / occupancy statistics per kernel of a device assembly file (hipcc -S
--cuda-device-only).  The register count, the scratch size and the occupancy are the compiler's own
figures: the `; NumVgprs:`, `; ScratchSize:` and `; Occupancy:` comments it writes after each
function.  Usage: tools/isa_stats.py file.s [substring]"""
import collections
import re
import sys

L = open(sys.argv[1]).read().split('\n')
sub = sys.argv[2] if len(sys.argv) > 2 else ''
starts = [i for i, l in enumerate(L) if re.match(r'^_Z\S+:\s', l)] + [len(L)]
for i, nxt in zip(starts, starts[1:]):
    name = re.match(r'^(_Z\S+):', L[i]).group(1)
    if sub not in name:
        continue
    en = next(j for j in range(i, nxt) if L[j].strip().startswith('.Lfunc_end'))
    c = collections.Counter(re.match(r'\s+(v_\w+)', x).group(1) for x in L[i:en] if re.match(r'\s+v_', x))
    scr = sum('scratch_' in x for x in L[i:en])
    ds = sum(bool(re.match(r'\s+ds_', x)) for x in L[i:en])
    vm = sum(bool(re.match(r'\s+(buffer|global)_', x)) for x in L[i:en])
    rep = {}                                        # the compiler's report, between this function and the next
    for x in L[en:nxt]:
        m = re.match(r'; (NumVgprs|ScratchSize|Occupancy): (\d+)', x)
        if m:
            rep.setdefault(m.group(1), m.group(2))
    print(f"{name[:70]:70s} valu {sum(c.values()):6d} ds {ds:5d} vmem {vm:4d} scratch insts {scr:3d} "
          f"vgpr {rep.get('NumVgprs', '?')} scratch {rep.get('ScratchSize', '?')} occ {rep.get('Occupancy', '?')}")

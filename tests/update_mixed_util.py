"""What the mixed-plan parity update tests (test_update_mixed_gpu.py) add to ptrs_util and
recon_mixed_util: stripes that each change positions of their own, or are skipped.  ONE arena
(ptrs_util.Arena) holds, for every live stripe, the shards at its own plan's changed positions
("s", stripe, position), its parity shards, and its new-symbol buffers ("n", stripe, r); for a
skipped stripe one data shard, one parity shard and one new-symbol buffer that nothing may touch;
and one decoy buffer.  Every table entry that a stripe's own plan does not use points at the decoy:
valid memory with a fixed pattern, so a stray write shows in the arena compare and a stray read that
is used shows as wrong parity, and nothing faults.  The old codewords are recon_mixed_util.rows
(encoded by the oracle, never modified); the expected parity is the oracle's encode of the old stripe
with the changed symbols replaced, computed once per content and shared."""
import numpy as np

from ptrs_util import Arena
from recon_mixed_util import ALIGN, ocodec, rows

PAD, NEW_PAD = 3, 2
DECOY = ("decoy",)


def standard_sets(L):
    """Change sets for len L >= 6: one, two, three and four positions (kept in registers where the
    row block allows it), five (read again per row block), and every data position (the result is a
    fresh encode).  Not ascending."""
    five = [5, 1] + [p for p in (6, 7, 8, 2, 3, 4) if p < L][:3]
    return [[3], [L - 1, 0], [0, 4, 2], [L - 1, 0, 4, 2], five, list(range(L))]


_CONTENT = {}


def _content(spec, L, n, plans, plan_of, seed):
    """(new symbols per live stripe {s: [n, nchanged]}, with bits above the symbol; the re-encoded
    stripes {s: [n, S]}).  Read-only."""
    key = (spec, L, n, tuple(map(tuple, plans)), tuple(plan_of), seed)
    if key not in _CONTENT:
        oc = ocodec(spec)
        old = rows(spec, L, n, len(plan_of))
        dt = old.dtype
        rng = np.random.default_rng(seed + 1000 + n)
        live = [s for s, pi in enumerate(plan_of) if pi < len(plans)]
        new = {s: rng.integers(0, 1 << (8 * dt.itemsize), (n, len(plans[plan_of[s]]))).astype(dt) for s in live}
        enc = old[live].copy().reshape(len(live) * n, old.shape[2])
        for i, s in enumerate(live):
            enc[i * n:(i + 1) * n, plans[plan_of[s]]] = new[s] & dt.type(oc.nn)
        if live:
            oc.encode_batch(enc, L)
        enc = enc.reshape(len(live), n, old.shape[2])
        enc.setflags(write=False)
        for v in new.values():
            v.setflags(write=False)
        _CONTENT[key] = new, {s: enc[i] for i, s in enumerate(live)}
    return _CONTENT[key]


class Stripes:
    """ns = len(plan_of) stripes of shard_len n; stripe s changes plans[plan_of[s]], or is skipped
    when plan_of[s] >= len(plans).  everything: every position of every live stripe has a buffer (and
    the table no decoys at them).  err: {s: [n, nroots]} XOR-ed into the old parity of stripe s, which
    must then stay wrong by as much.

    * ``before``  the arena as the call finds it
    * ``exp``     the arena after the call"""

    def __init__(self, spec, L, plans, plan_of, n, cls="A16", odd=None, everything=False, err=None, seed=3):
        old = rows(spec, L, n, len(plan_of))
        self.ns, self.n, self.S, self.L, self.dt = len(plan_of), n, old.shape[2], L, old.dtype
        self.plans, self.plan_of, self.cls = [list(p) for p in plans], list(plan_of), cls
        self.live = [s for s in range(self.ns) if self.plan_of[s] < len(plans)]
        self.skipped = [s for s in range(self.ns) if s not in self.live]
        self.chg = {s: self.plans[self.plan_of[s]] for s in self.live}
        self.maxchg = max(len(p) for p in self.plans)
        S, par = self.S, list(range(L, self.S))
        sizes = {DECOY: n}
        for s in self.live:
            for p in (range(S) if everything else sorted(set(self.chg[s])) + par):
                sizes[("s", s, p)] = n
            for r in range(len(self.chg[s])):
                sizes[("n", s, r)] = n
        for s in self.skipped:
            sizes[("s", s, 1)] = sizes[("s", s, S - 1)] = sizes[("n", s, 0)] = n
        self.ar = ar = Arena(sizes, self.dt.itemsize, cls, odd, seed)
        new, enc = _content(spec, L, n, self.plans, self.plan_of, seed)
        rng = np.random.default_rng(seed + 200)
        full = 1 << (8 * self.dt.itemsize)
        before = ar.host.copy()
        ar.put(before, DECOY, (np.arange(n) * 37 + 11).astype(self.dt))
        for s in self.skipped:
            for k in (("s", s, 1), ("s", s, S - 1), ("n", s, 0)):
                ar.put(before, k, rng.integers(0, full, n).astype(self.dt))
        exp = before.copy()
        for s in self.live:
            e = np.zeros((n, S - L), self.dt) if err is None or s not in err else err[s]
            for p in range(S):
                if ("s", s, p) not in sizes:
                    continue
                x = e[:, p - L] if p >= L else 0
                ar.put(before, ("s", s, p), old[s, :, p] ^ x)
                ar.put(exp, ("s", s, p), enc[s][:, p] ^ x)
            for r, p in enumerate(self.chg[s]):
                ar.put(before, ("n", s, r), new[s][:, r])
                ar.put(exp, ("n", s, r), new[s][:, r])
                ar.put(exp, ("s", s, p), new[s][:, r])          # the data is stored as given
        self.before, self.exp = before, exp

    def tables(self, torch, dev):
        """(table [ns, S + PAD], new_table [ns, largest nchanged + NEW_PAD], shard_len, align): int64
        device tensors.  Whatever a stripe's own plan does not use, the pads and both rows of a
        skipped stripe included, is the address of the decoy."""
        ar, base = self.ar, dev.data_ptr()
        addr = lambda k: base + ar.off[k]
        tab = np.full((self.ns, self.S + PAD), addr(DECOY), np.int64)
        new = np.full((self.ns, self.maxchg + NEW_PAD), addr(DECOY), np.int64)
        for k in ar.off:
            if k[0] == "s" and k[1] in self.live:
                tab[k[1], k[2]] = addr(k)
            elif k[0] == "n" and k[1] in self.live:
                new[k[1], k[2]] = addr(k)
        return torch.from_numpy(tab).cuda(), torch.from_numpy(new).cuda(), self.n, ALIGN[self.cls](ar.w)

    def plan_tensor(self, torch, dtype=None):
        po = np.array(self.plan_of, np.uint32).view(np.int32)
        t = torch.from_numpy(po).cuda()
        return t if dtype is None else t.view(dtype)

"""What the mixed-plan reconstruction tests (test_recon_mixed_gpu.py) add to ptrs_util: stripes that
each work under a plan of their own, or under none.  All shards of all stripes are carved from ONE
arena (ptrs_util.Arena) with keys (stripe, position); the codewords are encoded by the oracle, once
per geometry, and never modified."""
import numpy as np

import oracle as O
from ptrs_util import Arena

POISON = 0x0DEAD0000BAD0001                        # odd, not even a canonical address: never dereferenced
PAD = 3
ALIGN = {"A16": lambda w: 16, "A4": lambda w: 4, "A1": lambda w: w}


def params(spec):
    kind, n, k = spec
    return O.rs_params(n, k) if kind == "rs" else O.ccsds_params(k, kind == "ccsds")


def codec(spec):
    import ezrs
    kind, n, k = spec
    return ezrs.Codec.rs(n, k) if kind == "rs" else ezrs.Codec.ccsds(k, dual=kind == "ccsds")


_ROWS, _OC = {}, {}


def ocodec(spec):
    if spec not in _OC:
        _OC[spec] = O.Codec(*params(spec))
    return _OC[spec]


def rows(spec, L, n, ns):
    """ns stripes of n oracle-encoded codewords of length L, [ns, n, L + nroots]; read-only."""
    key = (spec, L, n, ns)
    if key not in _ROWS:
        oc = ocodec(spec)
        rng = np.random.default_rng(L * 7919 + n * 31 + ns)
        r = (rng.integers(0, 1 << 16, (ns * n, L + oc.nroots)) & oc.nn).astype(oc.dtype)
        oc.encode_batch(r, L)
        r = r.reshape(ns, n, -1)
        r.setflags(write=False)
        _ROWS[key] = r
    return _ROWS[key]


def standard_plans(L, NR):
    """P0 verify, P1 one data shard, P2 parity and data (not ascending), P3 all parity (encode), P4
    NROOTS lost (nothing left to check), P5 = P1 again."""
    return [[], [1], [L + 1, 0], list(range(L, L + NR)), list(range(NR)), [1]]


class Stripes:
    """ns = len(plan_of) stripes of shard_len n; stripe s works under the loss list
    plans[plan_of[s]], or is skipped when plan_of[s] >= len(plans).  absent: the (stripe, position)
    pairs, lost positions of their stripes, that have no buffer (NULL in the table: not wanted).

    * ``exp``   the arena after a clean call: every buffer of a live stripe holds its shard
    * ``gone``  the arena before it: garbage in the lost buffers of the live stripes; a skipped
                stripe holds garbage at two positions, in both images"""

    def __init__(self, spec, L, plans, plan_of, n, cls="A16", odd=None, absent=(), seed=1):
        self.rows = rows(spec, L, n, len(plan_of))
        self.ns, self.n, self.S, self.dt = len(plan_of), n, self.rows.shape[2], self.rows.dtype
        self.plans, self.plan_of, self.cls = [list(p) for p in plans], list(plan_of), cls
        self.live = [s for s in range(self.ns) if self.plan_of[s] < len(plans)]
        self.lost = {s: self.plans[self.plan_of[s]] for s in self.live}
        absent = set(absent)
        assert all(s in self.lost and p in self.lost[s] for s, p in absent)
        keys = [(s, p) for s in range(self.ns) for p in range(self.S) if (s, p) not in absent]
        self.ar = ar = Arena({k: n for k in keys}, self.dt.itemsize, cls, odd, seed)
        rng = np.random.default_rng(seed + 100)
        junk = lambda: rng.integers(0, 1 << (8 * self.dt.itemsize), n).astype(self.dt)
        self.exp = ar.host.copy()
        for s, p in keys:
            ar.put(self.exp, (s, p), self.rows[s, :, p])
        for s in set(range(self.ns)) - set(self.live):
            for p in (1, self.S - 1):
                ar.put(self.exp, (s, p), junk())
        self.gone = self.exp.copy()
        self.written = [(s, p) for s in self.live for p in self.lost[s] if (s, p) not in absent]
        for k in self.written:
            ar.put(self.gone, k, junk())
        self.optional = sorted({p for s in self.live for p in self.lost[s]})

    def nlost(self, s):
        return len(self.lost[s])

    def survivors(self, s):
        return [p for p in range(self.S) if p not in self.lost[s]]

    def table(self, torch, dev, poisoned=()):
        """(table, shard_len, align) through ezrs.ptr_table, with PAD poison entries per stripe; every
        entry of a skipped stripe, and of the stripes in `poisoned`, is the poison address."""
        import ezrs
        ar = self.ar
        ts = [[ar.tensor(torch, dev, (s, p)) if (s, p) in ar.off else None for p in range(self.S)]
              for s in range(self.ns)]
        tab, n, align = ezrs.ptr_table(ts, optional=self.optional)
        assert tab.shape == (self.ns, self.S) and n == self.n and align == ALIGN[self.cls](ar.w)
        host = np.full((self.ns, self.S + PAD), POISON, np.int64)
        host[:, :self.S] = tab.cpu().numpy()
        for s in set(range(self.ns)) - set(self.live) | set(poisoned):
            host[s] = POISON
        return torch.from_numpy(host).to(tab.device), n, align

    def plan_tensor(self, torch, dtype=None):
        po = np.array(self.plan_of, np.uint32).view(np.int32)
        t = torch.from_numpy(po).cuda()
        return t if dtype is None else t.view(dtype)

    def clean_result(self, fill):
        """result after a clean call on a result prefilled with `fill`."""
        r = np.full((self.ns, self.n), fill, np.int32)
        for s in self.live:
            r[s] = self.nlost(s)
        return r.reshape(-1)

    def corrupt(self, nn):
        """One symbol flipped in every third codeword of every live stripe, at a position that
        survives under that stripe's plan.  Returns (image, hit: the codewords [n] flipped)."""
        ar = self.ar
        rng = np.random.default_rng(self.n + self.ns)
        hit = np.arange(self.n) % 3 == 1
        bad = self.gone.copy()
        for s in self.live:
            surv = self.survivors(s)
            for k in np.nonzero(hit)[0]:
                p = surv[int(rng.integers(0, len(surv)))]
                v = ar.get(bad, (s, p), self.dt)
                v[k] ^= int(rng.integers(1, nn + 1))
                ar.put(bad, (s, p), v)
        return bad, hit

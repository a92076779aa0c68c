"""What the pointer-form decode tests (test_decode_ptrs_gpu.py, test_decode_ptrs_batch_gpu.py)
share.  A case is built on the CPU from the oracle alone: stripes of separate shard buffers carved
from a ptrs_util.Arena (shuffled placement, guard bytes), encoded with the oracle, corrupted as
test_interleaved_gpu._corrupt does, and decoded with the oracle on the de-interleaved rows; `check`
then compares what the device call left behind with that, bit for bit: the whole arena (symbols,
guards, every byte that must not change), the results, the positions of every corrected codeword and
the correction patterns of a subset.  Codewords are numbered stripe-major, k = s * shard_len + j; the
buffer of position p of stripe s has the key (s, p)."""
import numpy as np

import oracle as O
from interleave_util import interleave
from ptrs_util import Arena, download
from test_interleaved_gpu import _codecs, _corrupt, _dev, _host


class Case:
    """spec: ("rs" | "ccsds" | "ccsds_conv", n, k); L: data symbols; D: shard_len; F: stripes."""

    def __init__(self, spec, L, D, F=1, cls="A16", odd=None, with_eras=False, karn=False, seed=0):
        kind, n, k = spec
        params = O.rs_params(n, k) if kind == "rs" else O.ccsds_params(k, kind == "ccsds")
        self.spec, self.L, self.D, self.F, self.karn, self.with_eras = spec, L, D, F, karn, with_eras
        self.oc = oc = O.Codec(*params, karn=karn)
        self.nr = nr = params[4]
        self.S = S = L + nr
        self.nn = nn = (1 << params[0]) - 1
        self.dt = dt = np.uint8 if params[0] <= 8 else np.uint16
        self.ncw = ncw = F * D
        w = dt().itemsize
        rng = np.random.default_rng([seed, D, F, L, n, k])
        self.arena = Arena({(s, p): D for s in range(F) for p in range(S)}, w, cls, odd, seed)
        rows = (rng.integers(0, 1 << (8 * w), (ncw, S)) & nn).astype(dt)
        oc.encode_batch(rows, L)
        self.brows = brows = rows.copy()
        self.eras, self.neras = _corrupt(rng, brows, nr, nn + 1, with_eras, pad=(nn - nr - L) if karn else 0)
        self.bad = self.image(self.arena.host, brows)
        self.orow = orow = brows.copy()
        self.opos = np.zeros((ncw, nr), np.uint32)
        self.ores = oc.decode_batch(orow, L, None, self.eras if with_eras else None,
                                    self.neras if with_eras else None, self.opos)
        self.exp = self.image(self.bad, orow)

    def image(self, base, rows):
        """The arena image `base` with the codeword rows `rows` laid out in the shard buffers."""
        img = base.copy()
        fr = interleave(rows, self.F, self.D)
        for s in range(self.F):
            for p in range(self.S):
                self.arena.put(img, (s, p), fr[s, p])
        return img

    def classes(self):
        """The result classes of the oracle's decode: clean, corrected, failed."""
        return bool((self.ores == 0).any()), bool((self.ores > 0).any()), bool((self.ores == -1).any())

    def require_classes(self):
        """The condition on the inputs of every case of at least 16 codewords."""
        if self.ncw >= 16:
            assert self.classes() == (True, True, True), "inputs without clean, corrected and failed codewords"

    def frames(self):
        """The corrupted symbols as one contiguous strided array [F, S, D]."""
        return interleave(self.brows, self.F, self.D)

    # -- device side -----------------------------------------------------------------------------
    def codec(self, launch_rows=0):
        c, _ = _codecs(self.spec, self.karn)
        if launch_rows:
            c.set_launch_rows(launch_rows)
        return c

    def upload(self, torch):
        """The corrupted arena on the device and the outputs of a call (result pre-filled with 77)."""
        dev = self.arena.upload(torch, self.bad)
        out = {"result": torch.full((self.ncw,), 77, dtype=torch.int32, device="cuda"),
               "positions": torch.zeros((self.ncw, self.nr), dtype=torch.int32, device="cuda"),
               "corr": torch.zeros((self.ncw, self.nr), dtype=torch.uint8 if self.dt == np.uint8 else torch.uint16,
                                   device="cuda")}
        if self.with_eras:
            out["eras"], out["neras"] = _dev(torch, self.eras), _dev(torch, self.neras)
        return dev, out

    def shards(self, torch, dev, s=0):
        return [self.arena.tensor(torch, dev, (s, p)) for p in range(self.S)]

    def table(self, torch, dev, spare=3):
        """The device pointer table [F, S + spare]; the spare entries hold garbage that no call may
        read: odd, non-canonical addresses."""
        rows = [[t.data_ptr() for t in self.shards(torch, dev, s)] + [0x7EADBEEF00000001 + 8 * i for i in range(spare)]
                for s in range(self.F)]
        return torch.tensor(rows, dtype=torch.int64).cuda()

    def outputs(self, torch, dev, out):
        return (download(dev), out["result"].cpu().numpy(), out["positions"].cpu().numpy().view(np.uint32),
                _host(torch, out["corr"]))

    def check(self, torch, dev, out):
        """Assert everything the call left behind against the oracle; returns the outputs."""
        img, res, gpos, gcorr = got = self.outputs(torch, dev, out)
        ores, L = self.ores, self.L
        np.testing.assert_array_equal(res, ores, err_msg="decode results")
        np.testing.assert_array_equal(img, self.exp, err_msg="arena (symbols, guards, or a byte that must not change)")
        for k in np.nonzero(ores > 0)[0]:
            np.testing.assert_array_equal(gpos[k, :ores[k]], self.opos[k, :ores[k]], err_msg=f"positions cw {k}")
        sub = np.nonzero(ores > 0)[0]
        if len(sub):
            sub = sub[np.unique(np.linspace(0, len(sub) - 1, 10).astype(int))]
        for k in sub:                                   # correction patterns of a subset
            d, p = self.brows[k, :L].copy(), self.brows[k, L:].copy()
            cc = np.zeros(self.nr, self.dt)
            r, _ = self.oc.decode(d, p, self.eras[k, :self.neras[k]].tolist(), cc)
            assert r == ores[k]
            np.testing.assert_array_equal(gcorr[k, :r], cc[:r], err_msg=f"corr cw {k}")
        return got

    def untouched(self, torch, dev, out):
        """Nothing was written: the arena as uploaded, the result still pre-filled."""
        torch.cuda.synchronize()
        np.testing.assert_array_equal(download(dev), self.bad)
        assert (out["result"].cpu().numpy() == 77).all()

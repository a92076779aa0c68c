"""What the selection tests (test_select_failed_gpu.py, test_decode_ptrs_select_gpu.py,
test_decode_interleaved_select_gpu.py, test_scrub_select_gpu.py) share.  A `Selection` is a list of
codeword indices over a decode_ptrs_util.Case, with the compact inputs and the expected outputs of
ezrs_decode_ptrs_select / ezrs_decode_interleaved_select worked out from the oracle alone:

  used rows     i < min(count, nsel) with 0 <= sel[i] < ncw: row i decodes codeword k = sel[i] under
                the case's erasures of k; its result, positions and corrections are the oracle's for k
  skipped rows  every other row: nothing of it is read or written; its outputs are the oracle's on an
                all-zero codeword under row i's erasures (the case's erasures of codeword i mod ncw,
                so that skipped rows do carry erasures where the case has them)
  the image     the corrupted image with the oracle-decoded row for every used k and the corrupted
                row for every other k: a corrupted codeword that was not selected stays corrupted"""
import numpy as np

from test_interleaved_gpu import _dev, _host

NONE = -1                                           # ezrs.SEL_NONE: EZRS_SEL_NONE as int64


class Selection:
    def __init__(self, case, sel, count=None):
        self.case, self.count = case, count
        self.sel = sel = np.asarray(sel, np.int64)
        self.nsel = nsel = len(sel)
        lim = nsel if count is None else min(int(count), nsel)
        self.used = used = (np.arange(nsel) < lim) & (sel >= 0) & (sel < case.ncw)   # < 0: above 2^63
        self.ks = ks = sel[used]
        assert len(np.unique(ks)) == len(ks), "the used entries must be distinct"
        nr, L = case.nr, case.L
        we = np.nonzero(case.neras > 0)[0] if case.with_eras and (case.neras > 0).any() else np.arange(case.ncw)
        src = np.where(used, sel, we[np.arange(nsel) % len(we)])    # whose erasures row i carries
        self.eras, self.neras = case.eras[src].copy(), case.neras[src].copy()
        if not case.with_eras:
            self.neras[:] = 0
        self.res = np.zeros(nsel, np.int32)
        self.pos = np.zeros((nsel, nr), np.uint32)
        self.res[used], self.pos[used] = case.ores[ks], case.opos[ks]
        self.zero = {}                              # erasure list -> the oracle on the all-zero word
        for i in np.nonzero(~used)[0]:
            e = tuple(int(x) for x in self.eras[i, :self.neras[i]])
            if e not in self.zero:
                cc = np.zeros(nr, case.dt)
                r, p = case.oc.decode(np.zeros(L, case.dt), np.zeros(nr, case.dt), list(e), cc)
                self.zero[e] = (r, p, cc)
            r, p, _ = self.zero[e]
            self.res[i] = r
            self.pos[i, :max(r, 0)] = p
        rows = case.brows.copy()
        rows[ks] = case.orow[ks]
        self.rows = rows                            # the codeword rows a call must leave behind

    def require_classes(self):
        """Every case selects clean, corrected and failed codewords (checked before the device runs)."""
        r = self.case.ores[self.ks]
        assert (r == 0).any() and (r > 0).any() and (r == -1).any(), "selection without all three classes"

    def upload(self, torch):
        """The compact inputs and outputs of a call on the device (result pre-filled with 77)."""
        c = self.case
        out = {"result": torch.full((self.nsel,), 77, dtype=torch.int32, device="cuda"),
               "positions": torch.zeros((self.nsel, c.nr), dtype=torch.int32, device="cuda"),
               "corr": torch.zeros((self.nsel, c.nr), dtype=torch.uint8 if c.dt == np.uint8 else torch.uint16,
                                   device="cuda")}
        if c.with_eras:
            out["eras"], out["neras"] = _dev(torch, self.eras), _dev(torch, self.neras)
        sel = torch.from_numpy(self.sel).cuda()
        count = None if self.count is None else torch.tensor([self.count], dtype=torch.int64).cuda()
        return sel, count, out

    def check_out(self, torch, out):
        """Assert result, positions and a subset of the corrections against the oracle; returns them."""
        c = self.case
        res = out["result"].cpu().numpy()
        gpos = out["positions"].cpu().numpy().view(np.uint32)
        gcorr = _host(torch, out["corr"])
        np.testing.assert_array_equal(res[self.used], self.res[self.used], err_msg="results of the used rows")
        np.testing.assert_array_equal(res[~self.used], self.res[~self.used], err_msg="results of the skipped rows")
        for i in np.nonzero(self.res > 0)[0]:
            np.testing.assert_array_equal(gpos[i, :self.res[i]], self.pos[i, :self.res[i]], err_msg=f"positions row {i}")
        sub = np.nonzero(self.used & (self.res > 0))[0]
        if len(sub):
            sub = sub[np.unique(np.linspace(0, len(sub) - 1, 10).astype(int))]
        for i in sub:                               # correction patterns of a subset of the used rows
            k = self.sel[i]
            d, p = c.brows[k, :c.L].copy(), c.brows[k, c.L:].copy()
            cc = np.zeros(c.nr, c.dt)
            r, _ = c.oc.decode(d, p, c.eras[k, :c.neras[k]].tolist() if c.with_eras else [], cc)
            assert r == self.res[i]
            np.testing.assert_array_equal(gcorr[i, :r], cc[:r], err_msg=f"corr row {i}")
        for i in np.nonzero(~self.used & (self.res > 0))[0][:10]:   # and of skipped rows with erasures
            e = tuple(int(x) for x in self.eras[i, :self.neras[i]])
            np.testing.assert_array_equal(gcorr[i, :self.res[i]], self.zero[e][2][:self.res[i]], err_msg=f"corr row {i}")
        return res, gpos, gcorr


def classes_first(case, sel):
    """`sel` (as many entries) with one failed, one clean and one corrected codeword in front."""
    lead = [int(np.nonzero(c)[0][0]) for c in (case.ores == -1, case.ores == 0, case.ores > 0)]
    rest = [int(k) for k in sel if int(k) not in lead]
    return np.array(lead + rest[:len(sel) - 3], np.int64)


def mixed_selection(case, seed=0, clean=20, none=7, outside=(0, 5, (1 << 40))):
    """Every codeword the oracle changed or failed plus `clean` clean ones, shuffled, with `none`
    SEL_NONE entries and the out-of-range entries ncw + x for x in `outside` scattered through it."""
    rng = np.random.default_rng([seed, case.ncw])
    hit = (case.ores != 0) | (case.brows != case.orow).any(1)
    ks = np.concatenate([np.nonzero(hit)[0], rng.choice(np.nonzero(~hit)[0], clean, replace=False)])
    sel = np.concatenate([ks, np.full(none, NONE), [case.ncw + x for x in outside]]).astype(np.int64)
    rng.shuffle(sel)
    return sel

"""Mixed-plan batched parity update (ezrs_update_set_create, ezrs_update_ptrs_mixed, ezrs.UpdateSet):
nine stripes in one call, neighbouring stripes never under the same plan, two of them skipped
(EZRS_PLAN_SKIP and the smallest index that names no plan).  The set holds change sets of one, two,
three, four and five positions and the one of every data position, so one launch runs the bodies
that keep 1 .. 4 deltas in registers, the one that reads again, and a full overwrite whose result is
a fresh encode.  Checked bit-exactly against the oracle's encode_batch as test_update_ptrs_batch_gpu.py
checks the one-plan call: everything is carved from ONE arena (update_mixed_util), every table entry
that a stripe's own plan does not use points at a decoy buffer in the arena (valid memory: nothing
can fault), and after the call the WHOLE arena must equal the expected image: parity, changed
shards, untouched new symbols, decoy, guards, skipped stripes."""
import ctypes as C
import errno
import gc

import numpy as np
import pytest

from ptrs_util import download
from recon_mixed_util import codec, ocodec
from update_mixed_util import NEW_PAD, PAD, Stripes, standard_sets

pytestmark = pytest.mark.gpu

SKIP = 0xFFFFFFFF
PLAN_OF = [3, 0, 2, SKIP, 1, 4, 6, 5, 2]            # 6 == nplans: the smallest index out of range
LIVE = [0, 1, 2, 4, 5, 7, 8]
FILL = 77


@pytest.fixture(scope="module")
def torch():
    import torch as T
    if not T.cuda.is_available():
        pytest.skip("no GPU")
    return T


RS251, RS223, CCSDS = ("rs", 255, 251), ("rs", 255, 223), ("ccsds", 255, 223)
RS27, RS1007, RS65503 = ("rs", 31, 27), ("rs", 1023, 1007), ("rs", 65535, 65503)
LEN = {RS251: 10, RS223: 9, CCSDS: 9, RS27: 6, RS1007: 9, RS65503: 9}
# every codec at (1047, A16); the byte form with two row blocks (no plan keeps its deltas) and the
# 32-row block (one delta kept at 16 bytes per lane) at the other five combinations.  1047 bytes at
# align 16: 65 runs (two waves per stripe, the second with one live lane) and a ragged end of 7; 1047
# 16-bit symbols: 130 runs, three waves; 5: the element path only.
CASES = [(spec, 1047, "A16") for spec in (RS251, RS223, CCSDS, RS27, RS1007, RS65503)] + \
        [(spec, n, cls) for spec in (RS223, RS65503)
         for n, cls in ((1047, "A4"), (1047, "A1"), (5, "A16"), (5, "A4"), (5, "A1"))]
IDS = [f"{s[0]}{s[1]}_{s[2]}-d{n}-{cls}" for s, n, cls in CASES]


def _setup(spec, n, cls="A16", plans=None, plan_of=PLAN_OF, **kw):
    import ezrs
    c = codec(spec)
    L = LEN[spec]
    lists = standard_sets(L) if plans is None else plans
    # the misaligned buffer: a parity shard of the stripe that changes three positions
    odd = None if cls == "A16" else ("s", 2, L)
    st = Stripes(spec, L, lists, plan_of, n, cls, odd, **kw)
    assert st.S == L + c.nroots
    ups = [c.update_plan(L, ch) for ch in lists]
    uset = ezrs.UpdateSet(ups)
    assert uset.nplans == len(lists) and uset.nchanged == [len(p) for p in lists]
    assert (uset.length, uset.nroots, uset.device) == (L, c.nroots, c.device)
    return c, ups, uset, st


def _apply(torch, uset, st, plan_of=None):
    dev = st.ar.upload(torch, st.before)
    tab, ntab, n, align = st.tables(torch, dev)
    assert tab.stride(0) == st.S + PAD and ntab.stride(0) == st.maxchg + NEW_PAD
    uset.apply_ptrs_mixed(tab, ntab, st.plan_tensor(torch) if plan_of is None else plan_of, n, align=align)
    np.testing.assert_array_equal(download(dev), st.exp,
                                  err_msg="parity, new data, or a byte that must not be written")
    return dev, tab, ntab


@pytest.mark.parametrize("spec,n,cls", CASES, ids=IDS)
def test_mixed_vs_oracle(torch, spec, n, cls):
    c, ups, uset, st = _setup(spec, n, cls)
    assert st.live == LIVE and [len(st.chg[s]) for s in LIVE] == [4, 1, 3, 2, 5, LEN[spec], 3]
    _apply(torch, uset, st)


def test_wrong_parity_stays_wrong_by_as_much(torch):
    """The old parity is read, not recomputed: another error in every stripe, and for 10-bit symbols
    in uint16_t the error has bits above the symbol, which stay where they are."""
    for spec, n, top in ((RS251, 267, 1 << 8), (RS1007, 75, 1 << 16)):
        oc = ocodec(spec)
        rng = np.random.default_rng(9)
        err = {s: rng.integers(0, top, (n, oc.nroots)).astype(oc.dtype) for s in LIVE}
        assert all(e.any() for e in err.values())
        c, ups, uset, st = _setup(spec, n, err=err)
        _apply(torch, uset, st)


@pytest.mark.parametrize("spec,n,cls", [(RS223, 1047, "A16"), (RS65503, 5, "A4")], ids=["rs255_223", "rs65535_65503"])
def test_one_plan_set_is_the_batch_call(torch, spec, n, cls):
    """A set of one plan with plan_of all zero: the oracle's image, and in a second arena with the
    same input image the bytes of apply_ptrs_batch under that plan."""
    L = LEN[spec]
    c, ups, uset, st = _setup(spec, n, cls, plans=[[L - 1, 0, 3]], plan_of=[0] * 5)
    dev, _, _ = _apply(torch, uset, st)
    dev2 = st.ar.upload(torch, st.before)
    tab, ntab, n_, align = st.tables(torch, dev2)
    ups[0].apply_ptrs_batch(tab, ntab, n_, align=align)
    np.testing.assert_array_equal(download(dev2), download(dev))


def test_chain_update_then_verify(torch):
    """All shards present in one table: apply_ptrs_mixed, then the nlost == 0 plan as a ReconSet over
    the same table with the same stripes skipped says 0 for every live stripe."""
    import ezrs
    c, ups, uset, st = _setup(RS251, 267, everything=True)
    dev, tab, _ = _apply(torch, uset, st)
    rset = ezrs.ReconSet([c.recon_plan(LEN[RS251], [])])
    po = torch.tensor([0 if s in st.live else -1 for s in range(st.ns)], dtype=torch.int32, device="cuda")
    res = torch.full((st.ns * st.n,), FILL, dtype=torch.int32, device="cuda")
    rset.reconstruct_ptrs_mixed(tab, po, st.n, align=16, result=res)
    r = res.cpu().numpy().reshape(st.ns, st.n)
    assert (r[st.live] == 0).all() and (r[st.skipped] == FILL).all()
    np.testing.assert_array_equal(download(dev), st.exp)


def test_plan_of_as_uint32_and_longer_than_the_table(torch):
    c, ups, uset, st = _setup(RS251, 5)
    po = torch.cat([st.plan_tensor(torch), torch.zeros(3, dtype=torch.int32, device="cuda")]).view(torch.uint32)
    _apply(torch, uset, st, plan_of=po)


def test_set_outlives_plans_and_codec(torch):
    c, ups, uset, st = _setup(RS223, 1047)
    del ups, c
    gc.collect()
    torch.cuda.synchronize()
    junk = torch.full((1 << 20,), 0x5A, dtype=torch.uint8, device="cuda")     # reuse what was freed
    _apply(torch, uset, st)
    del junk


def test_all_skipped_and_empty_calls_touch_nothing(torch):
    import ezrs
    c, ups, uset, st = _setup(RS251, 5, plan_of=[SKIP, 6, 7, 1 << 31])
    assert st.live == [] and ezrs.PLAN_SKIP == SKIP
    dev = st.ar.upload(torch, st.before)
    tab, ntab, n, align = st.tables(torch, dev)
    uset.apply_ptrs_mixed(tab, ntab, st.plan_tensor(torch), n, align=align)
    c2, ups2, uset2, st2 = _setup(RS251, 5)
    dev2 = st2.ar.upload(torch, st2.before)
    tab2, ntab2, n2, align2 = st2.tables(torch, dev2)
    uset2.apply_ptrs_mixed(tab2, ntab2, st2.plan_tensor(torch), 0, align=align2)        # shard_len == 0
    po2 = st2.plan_tensor(torch)
    assert ezrs.lib().ezrs_update_ptrs_mixed(uset2._h, po2.data_ptr(), tab2.data_ptr(), tab2.stride(0),
                                             ntab2.data_ptr(), ntab2.stride(0), n2, 0, align2,
                                             ezrs._stream_ptr(None)) == 0                # nstripes == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(download(dev), st.before)
    np.testing.assert_array_equal(download(dev2), st2.before)


def test_argument_checks(torch):
    import ezrs
    L_ = ezrs.lib()
    EINVAL = -errno.EINVAL
    c, ups, uset, st = _setup(RS251, 5)
    dev = st.ar.upload(torch, st.before)
    tab, ntab, n, align = st.tables(torch, dev)
    po = st.plan_tensor(torch)
    sp = ezrs._stream_ptr(None)
    big = C.c_size_t(-1).value
    assert st.maxchg == 10 and max(uset.nchanged) == 10

    def upd(h=uset._h, p=po.data_ptr(), t=tab.data_ptr(), pitch=st.S + PAD, nt=ntab.data_ptr(),
            npitch=st.maxchg + NEW_PAD, n=n, ns=st.ns, al=align):
        return L_.ezrs_update_ptrs_mixed(h, p, t, pitch, nt, npitch, n, ns, al, sp)

    assert upd(h=None) == EINVAL and upd(p=None) == EINVAL and upd(t=None) == EINVAL and upd(nt=None) == EINVAL
    for kw in ({"h": None}, {"p": None}, {"t": None}, {"nt": None}):       # nulls before the empty-call 0
        assert upd(ns=0, **kw) == EINVAL and upd(n=0, **kw) == EINVAL, kw
    assert upd(pitch=st.S - 1) == EINVAL and upd(pitch=st.S - 1, n=0) == EINVAL
    assert upd(npitch=st.maxchg - 1) == EINVAL and upd(npitch=st.maxchg - 1, ns=0) == EINVAL
    for al in (3, 8, 0, 2, 32):
        assert upd(al=al) == EINVAL, al
    assert upd(n=big // 2 + 1, ns=2) == EINVAL and upd(n=2, ns=big) == EINVAL       # nstripes * shard_len
    assert upd(n=big) == EINVAL
    c16, ups16, uset16, st16 = _setup(RS1007, 5)
    dev16 = st16.ar.upload(torch, st16.before)
    tab16, ntab16, _, _ = st16.tables(torch, dev16)
    po16 = st16.plan_tensor(torch)

    def upd16(n, ns, al=2):
        return L_.ezrs_update_ptrs_mixed(uset16._h, po16.data_ptr(), tab16.data_ptr(), st16.S + PAD,
                                         ntab16.data_ptr(), st16.maxchg + NEW_PAD, n, ns, al, sp)

    assert upd16(big // 2 + 1, 1) == EINVAL         # shard_len * datum bytes
    for al in (3, 8, 0, 1):
        assert upd16(5, st16.ns, al) == EINVAL, al
    assert upd(ns=0) == 0 and upd(n=0) == 0         # nothing to do
    torch.cuda.synchronize()
    np.testing.assert_array_equal(download(dev), st.before, err_msg="a refused or empty call wrote")
    np.testing.assert_array_equal(download(dev16), st16.before, err_msg="a refused call wrote")
    assert upd() == 0 and upd16(5, st16.ns) == 0
    np.testing.assert_array_equal(download(dev), st.exp)
    np.testing.assert_array_equal(download(dev16), st16.exp)

    # Python-side validation
    with pytest.raises(ezrs.EzrsError):
        uset.apply_ptrs_mixed(tab, ntab, po[:-1], n)                    # fewer indices than stripes
    with pytest.raises(ezrs.EzrsError):
        uset.apply_ptrs_mixed(tab, ntab, po.cpu(), n)
    with pytest.raises(ezrs.EzrsError):
        uset.apply_ptrs_mixed(tab, ntab, po.to(torch.int64), n)
    with pytest.raises(ezrs.EzrsError):
        uset.apply_ptrs_mixed(tab, ntab, po.to(torch.float32), n)
    with pytest.raises(ezrs.EzrsError):
        uset.apply_ptrs_mixed(tab[:, :st.S - 1], ntab, po, n)
    with pytest.raises(ezrs.EzrsError):
        uset.apply_ptrs_mixed(tab, ntab[:, :st.maxchg - 1], po, n)      # pitch below the largest nchanged
    with pytest.raises(ezrs.EzrsError):
        uset.apply_ptrs_mixed(tab, ntab[:-1], po, n)                    # fewer stripes
    with pytest.raises(ezrs.EzrsError):
        uset.apply_ptrs_mixed(tab, ntab.cpu(), po, n)
    with pytest.raises(ezrs.EzrsError):
        uset.apply_ptrs_mixed(tab.to(torch.int32), ntab, po, n)
    with pytest.raises(ezrs.EzrsError):
        uset.apply_ptrs_mixed(tab, ntab, po, -1)
    with pytest.raises(ezrs.EzrsError):
        uset.apply_ptrs_mixed(tab, ntab, po, n, align=8)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(download(dev), st.exp)


def test_sets_of_plans_that_do_not_match(torch):
    import ezrs
    a, b = codec(RS251), codec(RS223)
    with pytest.raises(ezrs.EzrsError, match="EINVAL"):
        ezrs.UpdateSet([a.update_plan(6, [1]), a.update_plan(7, [1])])     # different len
    with pytest.raises(ezrs.EzrsError, match="EINVAL"):
        ezrs.UpdateSet([a.update_plan(6, [1]), b.update_plan(6, [1])])     # different NROOTS
    with pytest.raises(ezrs.EzrsError, match="EINVAL"):
        ezrs.UpdateSet([a.update_plan(6, [1]), codec(RS1007).update_plan(6, [1])])   # different symbol bits
    with pytest.raises(ezrs.EzrsError):
        ezrs.UpdateSet([a.recon_plan(6, [1])])                             # not an update plan
    assert ezrs.UpdateSet([a.update_plan(6, [1]), a.update_plan(6, [1])]).nchanged == [1, 1]

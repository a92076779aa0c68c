"""Mixed-plan batched reconstruction (ezrs_recon_set_create, ezrs_reconstruct_ptrs_mixed,
ezrs.ReconSet): nine stripes in one call, neighbouring stripes never under the same plan, two of
them skipped (EZRS_PLAN_SKIP and the smallest index that names no plan).  Checked against the oracle
as test_recon_ptrs_batch_gpu.py checks the one-plan call: every shard of every stripe is carved from
ONE arena (recon_mixed_util), the lost buffers hold garbage, the table has three poison pad entries
per stripe and nothing but poison for a skipped stripe.  After the call the WHOLE arena must equal
the expected image: rebuilt bytes, untouched survivors and guards, nothing written for a NULL entry,
skipped stripes as they were."""
import errno
import gc

import numpy as np
import pytest

from ptrs_util import download
from recon_mixed_util import PAD, Stripes, codec, ocodec, standard_plans

pytestmark = pytest.mark.gpu

SKIP = 0xFFFFFFFF
PLAN_OF = [3, 0, 2, SKIP, 1, 4, 6, 5, 2]            # 6 == nplans: the smallest index out of range
SKIPPED = (3, 6)
FILL = 77


@pytest.fixture(scope="module")
def torch():
    import torch as T
    if not T.cuda.is_available():
        pytest.skip("no GPU")
    return T


RS251, RS223, CCSDS = ("rs", 255, 251), ("rs", 255, 223), ("ccsds", 255, 223)
RS27, RS1007, RS65503 = ("rs", 31, 27), ("rs", 1023, 1007), ("rs", 65535, 65503)
LEN = {RS251: 6, RS223: 9, CCSDS: 9, RS27: 6, RS1007: 9, RS65503: 9}
# every codec at (1047, A16); the byte form with two row blocks and the 32-row block at the other
# five combinations.  1047 bytes at align 16: 65 runs (two waves per stripe, the second with one live
# lane) and a ragged end of 7; 1047 16-bit symbols: 130 runs, three waves; 5: the element path only.
CASES = [(spec, 1047, "A16") for spec in (RS251, RS223, CCSDS, RS27, RS1007, RS65503)] + \
        [(spec, n, cls) for spec in (RS223, RS65503)
         for n, cls in ((1047, "A4"), (1047, "A1"), (5, "A16"), (5, "A4"), (5, "A1"))]
IDS = [f"{s[0]}{s[1]}_{s[2]}-d{n}-{cls}" for s, n, cls in CASES]
ODD = (4, 1)                                        # the misaligned buffer: the output of the P1 stripe


def _setup(spec, n, cls, plans=None, plan_of=PLAN_OF, absent=None):
    import ezrs
    c = codec(spec)
    L = LEN[spec]
    lists = standard_plans(L, c.nroots) if plans is None else plans
    if absent is None:                              # the second P2 stripe does not want position 0
        absent = [(8, 0)] if plans is None else []
    st = Stripes(spec, L, lists, plan_of, n, cls, None if cls == "A16" else ODD, absent)
    assert st.S == L + c.nroots
    recons = [c.recon_plan(L, lost) for lost in lists]
    rset = ezrs.ReconSet(recons)
    assert rset.nplans == len(lists) and rset.nlost == [len(p) for p in lists]
    return c, recons, rset, st


def _clean(torch, rset, st, use_result=True, poisoned=()):
    dev = st.ar.upload(torch, st.gone)
    tab, n, align = st.table(torch, dev, poisoned)
    assert tab.stride(0) == st.S + PAD
    res = torch.full((st.ns * n,), FILL, dtype=torch.int32, device="cuda") if use_result else None
    out = rset.reconstruct_ptrs_mixed(tab, st.plan_tensor(torch), n, align=align, result=res)
    assert out is res
    np.testing.assert_array_equal(download(dev), st.exp, err_msg="rebuilt shards, survivors, guards or skipped stripes")
    if use_result:
        np.testing.assert_array_equal(res.cpu().numpy(), st.clean_result(FILL), err_msg="clean results")
    return res


def _corrupted(torch, spec, rset, st):
    """One surviving symbol flipped in every third codeword of every live stripe."""
    NR = ocodec(spec).nroots
    bad, hit = st.corrupt(int(ocodec(spec).nn))
    dev = st.ar.upload(torch, bad)
    tab, n, align = st.table(torch, dev)
    res = torch.full((st.ns * n,), FILL, dtype=torch.int32, device="cuda")
    rset.reconstruct_ptrs_mixed(tab, st.plan_tensor(torch), n, align=align, result=res)
    want = np.full((st.ns, n), FILL, np.int32)
    for s in st.live:
        nl = st.nlost(s)
        want[s] = np.where(hit, -1, nl) if nl < NR else nl          # nlost == NROOTS: nothing to check with
    np.testing.assert_array_equal(res.cpu().numpy(), want.reshape(-1), err_msg="results with wrong survivors")
    after = download(dev)
    img = bad.copy()                                # everything but the rebuilt buffers is as it was,
    for k in st.written:                            # and intact codewords are rebuilt all the same
        a, e = st.ar.get(after, k, st.dt), st.ar.get(st.exp, k, st.dt)
        np.testing.assert_array_equal(a[~hit], e[~hit])
        st.ar.put(img, k, a)
    np.testing.assert_array_equal(after, img, err_msg="a byte outside the rebuilt buffers")


@pytest.mark.parametrize("spec,n,cls", CASES, ids=IDS)
def test_mixed_vs_oracle(torch, spec, n, cls):
    """The clean pass with `result`, the same without it (the verify stripe's table row poisoned: it
    is never read), and the corrupted pass."""
    c, recons, rset, st = _setup(spec, n, cls)
    assert st.live == [0, 1, 2, 4, 5, 7, 8] and (8, 0) not in st.ar.off
    res = _clean(torch, rset, st)
    r = res.cpu().numpy().reshape(st.ns, n)
    assert (r[list(SKIPPED)] == FILL).all() and (r[1] == 0).all() and (r[5] == c.nroots).all()
    _clean(torch, rset, st, use_result=False, poisoned=[1])
    _corrupted(torch, spec, rset, st)


@pytest.mark.parametrize("spec,n,cls", [(RS223, 1047, "A16"), (RS65503, 5, "A4")], ids=["rs255_223", "rs65535_65503"])
def test_one_plan_set_is_the_batch_call(torch, spec, n, cls):
    """A set of one plan with plan_of all zero: the oracle's image through the same harness, and
    the bytes and results of reconstruct_ptrs_batch under that plan."""
    L = LEN[spec]
    lost = [L + 1, 0, 3]
    c, recons, rset, st = _setup(spec, n, cls, plans=[lost], plan_of=[0] * 5)
    res = _clean(torch, rset, st)
    _clean(torch, rset, st, use_result=False)
    _corrupted(torch, spec, rset, st)
    dev = st.ar.upload(torch, st.gone)
    tab, n_, align = st.table(torch, dev)
    res2 = torch.full_like(res, FILL)
    recons[0].reconstruct_ptrs_batch(tab, n_, align=align, result=res2)
    assert torch.equal(res, res2)
    np.testing.assert_array_equal(download(dev), st.exp)


def test_plan_of_as_uint32_and_longer_than_the_table(torch):
    c, recons, rset, st = _setup(RS251, 5, "A16")
    dev = st.ar.upload(torch, st.gone)
    tab, n, align = st.table(torch, dev)
    po = torch.cat([st.plan_tensor(torch), torch.zeros(3, dtype=torch.int32, device="cuda")]).view(torch.uint32)
    res = torch.full((st.ns * n,), FILL, dtype=torch.int32, device="cuda")
    rset.reconstruct_ptrs_mixed(tab, po, n, align=align, result=res)
    np.testing.assert_array_equal(download(dev), st.exp)
    np.testing.assert_array_equal(res.cpu().numpy(), st.clean_result(FILL))


def test_set_outlives_plans_and_codec(torch):
    c, recons, rset, st = _setup(RS223, 1047, "A16")
    del recons, c
    gc.collect()
    torch.cuda.synchronize()
    junk = torch.full((1 << 20,), 0x5A, dtype=torch.uint8, device="cuda")     # reuse what was freed
    _clean(torch, rset, st)
    del junk


def test_all_skipped_and_empty_calls_touch_nothing(torch):
    import ezrs
    c, recons, rset, st = _setup(RS251, 5, "A16", plan_of=[SKIP, 6, 7, 1 << 31], absent=[])
    assert st.live == []
    dev = st.ar.upload(torch, st.gone)
    tab, n, align = st.table(torch, dev)
    res = torch.full((st.ns * n,), FILL, dtype=torch.int32, device="cuda")
    rset.reconstruct_ptrs_mixed(tab, st.plan_tensor(torch), n, align=align, result=res)
    rset.reconstruct_ptrs_mixed(tab, st.plan_tensor(torch), n, align=align)
    rset.reconstruct_ptrs_mixed(tab, st.plan_tensor(torch), 0, align=align, result=res)
    np.testing.assert_array_equal(download(dev), st.gone)
    assert (res == FILL).all()
    assert ezrs.PLAN_SKIP == SKIP


def test_argument_checks(torch):
    import ctypes as C
    import ezrs
    L_ = ezrs.lib()
    EINVAL = -errno.EINVAL
    c, recons, rset, st = _setup(RS251, 5, "A16")
    dev = st.ar.upload(torch, st.gone)
    tab, n, align = st.table(torch, dev)
    po = st.plan_tensor(torch)
    res = torch.full((st.ns * n,), FILL, dtype=torch.int32, device="cuda")
    sp = ezrs._stream_ptr(None)
    big = C.c_size_t(-1).value

    def rec(h=rset._h, p=po.data_ptr(), t=tab.data_ptr(), pitch=st.S + PAD, n=n, ns=st.ns, al=align):
        return L_.ezrs_reconstruct_ptrs_mixed(h, p, t, pitch, n, ns, al, C.c_void_p(res.data_ptr()), sp)

    assert rec(h=None) == EINVAL and rec(p=None) == EINVAL and rec(t=None) == EINVAL
    assert rec(p=None, ns=0) == EINVAL and rec(t=None, n=0) == EINVAL
    assert rec(pitch=st.S - 1) == EINVAL and rec(pitch=st.S - 1, n=0) == EINVAL
    for al in (3, 8, 0, 2, 32):
        assert rec(al=al) == EINVAL, al
    assert rec(n=big // 2 + 1, ns=2) == EINVAL and rec(n=2, ns=big) == EINVAL
    assert rec(ns=0) == 0 and rec(n=0) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(download(dev), st.gone, err_msg="a refused or empty call wrote")
    assert (res == FILL).all()
    assert rec() == 0
    np.testing.assert_array_equal(download(dev), st.exp)

    # Python-side validation
    with pytest.raises(ezrs.EzrsError):
        rset.reconstruct_ptrs_mixed(tab, po[:-1], n)                    # fewer indices than stripes
    with pytest.raises(ezrs.EzrsError):
        rset.reconstruct_ptrs_mixed(tab, po.cpu(), n)
    with pytest.raises(ezrs.EzrsError):
        rset.reconstruct_ptrs_mixed(tab, po.to(torch.int64), n)
    with pytest.raises(ezrs.EzrsError):
        rset.reconstruct_ptrs_mixed(tab, po.to(torch.float32), n)
    with pytest.raises(ezrs.EzrsError):
        rset.reconstruct_ptrs_mixed(tab[:, :st.S - 1], po, n)
    with pytest.raises(ezrs.EzrsError):
        rset.reconstruct_ptrs_mixed(tab, po, n, align=8)
    with pytest.raises(ezrs.EzrsError):
        rset.reconstruct_ptrs_mixed(tab, po, n, result=res[:-1])
    torch.cuda.synchronize()


def test_sets_of_plans_that_do_not_match(torch):
    import ezrs
    a, b = codec(RS251), codec(RS223)
    with pytest.raises(ezrs.EzrsError, match="EINVAL"):
        ezrs.ReconSet([a.recon_plan(6, [1]), a.recon_plan(7, [1])])     # different len
    with pytest.raises(ezrs.EzrsError, match="EINVAL"):
        ezrs.ReconSet([a.recon_plan(6, [1]), b.recon_plan(6, [1])])     # different NROOTS
    with pytest.raises(ezrs.EzrsError, match="EINVAL"):
        ezrs.ReconSet([a.recon_plan(6, [1]), codec(RS1007).recon_plan(6, [1])])   # different symbol bits
    assert ezrs.ReconSet([a.recon_plan(6, [1]), a.recon_plan(6, [1])]).nlost == [1, 1]

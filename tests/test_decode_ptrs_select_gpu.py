"""ezrs_decode_ptrs_select: ezrs_decode_ptrs_batch of only the codewords a device list names.  Cases
are built and decoded by the oracle on the CPU (decode_ptrs_util.Case, decode_select_util.Selection)
and compared bit for bit: the whole arena (a corrupted codeword that was not selected stays
corrupted; guards; every byte that must not change), and per row of the call the result, the
positions and a subset of the correction patterns.  Every table has three garbage spare entries per
stripe, and every selection holds clean, corrected and failed codewords."""
import ctypes as C
import errno
import functools

import numpy as np
import pytest

from decode_ptrs_util import Case
from decode_select_util import NONE, Selection, classes_first, mixed_selection
from ptrs_util import download

pytestmark = pytest.mark.gpu

RS4 = ("rs", 255, 251)


@pytest.fixture(scope="module")
def torch():
    import torch as T
    if not T.cuda.is_available():
        pytest.skip("no GPU")
    return T


@functools.lru_cache(maxsize=None)
def case_of(**kw):
    """One oracle run per geometry, shared by the tests and never modified."""
    return Case(**{"spec": RS4, "L": 10, "seed": 0, **kw})


def run(torch, s, launch_rows=0):
    """One call on a fresh upload; everything asserted against the oracle; returns the outputs."""
    case = s.case
    s.require_classes()
    c = case.codec(launch_rows)
    dev = case.arena.upload(torch, case.bad)
    table = case.table(torch, dev)
    assert table.shape == (case.F, case.S + 3)
    sel, count, out = s.upload(torch)
    res = c.decode_ptrs_select(table, case.L, case.D, sel, count=count, **out)
    assert res is out["result"]
    got = s.check_out(torch, out)
    img = download(dev)
    np.testing.assert_array_equal(img, case.image(case.bad, s.rows),
                                  err_msg="arena (a selected codeword, one that was not, a guard)")
    return (img,) + got


@pytest.mark.parametrize("karn", [False, True], ids=["ezpwd", "karn"])
def test_mixed_selection(torch, karn):
    """Every corrupted codeword and 20 clean ones, shuffled, with 7 SEL_NONE and 3 out-of-range
    entries among them; the skipped rows carry erasures and decode as the all-zero word."""
    case = case_of(D=100, F=70, with_eras=True, karn=karn)
    s = Selection(case, mixed_selection(case))
    assert s.nsel % 256 and s.nsel > 512 and (~s.used).sum() == 10
    assert (s.neras[~s.used] > 0).all()              # the skipped rows carry erasures
    assert set(np.nonzero((case.brows != case.orow).any(1))[0]) <= set(s.ks)
    run(torch, s)


def test_several_passes(torch):
    """About 400 of 103 x 5 codewords staged 256 per pass (set_launch_rows): identical outputs, less
    workspace."""
    case = case_of(D=5, F=103, with_eras=True)
    rng = np.random.default_rng(5)
    s = Selection(case, classes_first(case, rng.permutation(case.ncw)[:401]))
    a = run(torch, s)
    b = run(torch, s, launch_rows=256)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    c = case.codec()
    whole = c.decode_select_workspace_bytes(case.L, s.nsel)
    c.set_launch_rows(256)
    assert 0 < c.decode_select_workspace_bytes(case.L, s.nsel) < whole


@pytest.mark.parametrize("count", [37, 10 ** 6], ids=["count37", "count_above_nsel"])
def test_device_count(torch, count):
    """count[0] = 37 over 300 valid entries: rows from 37 on are skipped and their codewords stay
    corrupted; a count above nsel is clamped to nsel."""
    case = case_of(D=100, F=70)
    rng = np.random.default_rng(37)
    hit = np.nonzero(case.ores != 0)[0]
    sel = np.concatenate([rng.choice(hit, 280, replace=False), rng.choice(np.nonzero(case.ores == 0)[0], 20, replace=False)])
    rng.shuffle(sel)
    sel = classes_first(case, sel)
    s = Selection(case, sel, count=count)
    assert s.used.sum() == min(count, 300) and s.nsel == 300
    if count == 37:
        assert (case.ores[sel[37:]] != 0).any()
    run(torch, s)


def test_odd_addresses(torch):
    case = case_of(D=100, F=70, with_eras=True, cls="A1", odd=(33, 11))
    run(torch, Selection(case, mixed_selection(case, seed=1)))


def test_rs1023_uint16(torch):
    """416 positions per stripe: above EZRS_PTRS_MAX, which does not apply; rows of several chunks."""
    case = case_of(spec=("rs", 1023, 1007), L=400, D=8, F=3)
    rng = np.random.default_rng(3)
    sel = np.concatenate([classes_first(case, rng.permutation(case.ncw)[:17]), [NONE, case.ncw]])
    s = Selection(case, sel)
    assert case.S == 416 and case.dt == np.uint16
    run(torch, s)


def test_run_in_one_stripe(torch):
    """300 consecutive codewords of one stripe of 1000, ascending: what ezrs_select_failed lists for
    a bad sector."""
    case = case_of(D=1000, F=3)
    fail = int(np.nonzero(case.ores == -1)[0][0])    # the run covers the codeword that fails
    f, j = divmod(fail, 1000)
    run(torch, Selection(case, f * 1000 + min(max(j - 150, 0), 700) + np.arange(300)))


def _raw(torch, s, c, table, sel, count, out, pitch=None, nsel=None, has_sel=True, result=True, ws=None,
         ws_bytes=None):
    """ezrs_decode_ptrs_select (ws is None) or ezrs_decode_ptrs_select_ws through ctypes."""
    import ezrs
    Lib = ezrs.lib()
    case = s.case
    p = lambda t: C.c_void_p(t.data_ptr())
    args = [c._h, p(table), table.shape[1] if pitch is None else pitch, case.L, case.D, case.F,
            p(sel) if has_sel else None, s.nsel if nsel is None else nsel, None if count is None else p(count),
            p(out["eras"]) if case.with_eras else None, case.nr, p(out["neras"]) if case.with_eras else None,
            p(out["result"]) if result else None, p(out["positions"]), case.nr, p(out["corr"]), case.nr]
    sp = ezrs._stream_ptr(None)
    if ws is None:
        return Lib.ezrs_decode_ptrs_select(*args, sp)
    return Lib.ezrs_decode_ptrs_select_ws(*args, p(ws), ws_bytes, sp)


def _untouched(torch, case, dev, out):
    torch.cuda.synchronize()
    np.testing.assert_array_equal(download(dev), case.bad)
    assert (out["result"].cpu().numpy() == 77).all()


def test_ws_form(torch):
    """Exactly ezrs_decode_select_workspace_bytes: 0; one byte less: -EINVAL and nothing written."""
    case = case_of(D=100, F=70, with_eras=True)
    s = Selection(case, mixed_selection(case))
    c = case.codec()
    need = c.decode_select_workspace_bytes(case.L, s.nsel)
    assert 0 < need < c.decode_ptrs_workspace_bytes(case.L, case.D, case.F)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    dev = case.arena.upload(torch, case.bad)
    table = case.table(torch, dev)
    sel, count, out = s.upload(torch)
    assert _raw(torch, s, c, table, sel, count, out, ws=ws, ws_bytes=need - 1) == -errno.EINVAL
    _untouched(torch, case, dev, out)
    assert _raw(torch, s, c, table, sel, count, out, ws=ws, ws_bytes=need) == 0
    s.check_out(torch, out)
    np.testing.assert_array_equal(download(dev), case.image(case.bad, s.rows))


def test_host_checks(torch):
    """What the host can check, on a valid table; each leaves the arena untouched."""
    import ezrs
    case = case_of(D=100, F=70)
    s = Selection(case, mixed_selection(case))
    c = case.codec()
    dev = case.arena.upload(torch, case.bad)
    table = case.table(torch, dev)
    sel, count, out = s.upload(torch)
    EINVAL = -errno.EINVAL
    assert _raw(torch, s, c, table, sel, count, out, pitch=case.S - 1) == EINVAL
    assert _raw(torch, s, c, table, sel, count, out, has_sel=False) == EINVAL
    assert _raw(torch, s, c, table, sel, count, out, result=False) == EINVAL
    assert _raw(torch, s, c, table, sel, count, out, nsel=0) == 0
    assert _raw(torch, s, c, table, sel, count, out, nsel=0, has_sel=False, result=False) == 0
    _untouched(torch, case, dev, out)
    with pytest.raises(ezrs.EzrsError):
        c.decode_ptrs_select(table[:, :case.S - 1], case.L, case.D, sel)        # a table too narrow
    with pytest.raises(ezrs.EzrsError):
        c.decode_ptrs_select(table, case.L, case.D, sel.to(torch.int32))
    with pytest.raises(ezrs.EzrsError):
        c.decode_ptrs_select(table, case.L, case.D, sel, result=out["result"][:5])
    _untouched(torch, case, dev, out)

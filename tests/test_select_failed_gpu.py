"""ezrs_select_failed: the device-side list of the codewords whose result is negative, compared bit
for bit with numpy: ascending order, the EZRS_SEL_NONE tail, the count, the clamp to cap, a nonzero
base and the caller-owned workspace.  The kernels work on chunks of 4096 results: the sizes sit on
both sides of one chunk, and at several chunks plus a tail."""
import ctypes as C
import errno

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHUNK = 4096
SIZES = [1, 255, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5]


@pytest.fixture(scope="module")
def torch():
    import torch as T
    if not T.cuda.is_available():
        pytest.skip("no GPU")
    return T


@pytest.fixture(scope="module")
def codec(torch):
    import ezrs
    return ezrs.Codec.rs(255, 251)


def _result(n, seed=0, p_bad=0.3):
    rng = np.random.default_rng([seed, n])
    return rng.choice(np.array([-1, 0, 1, 3], np.int32), n, p=[p_bad, 0.4, (0.6 - p_bad) / 2, (0.6 - p_bad) / 2])


def _expect(res, cap, base=0):
    bad = np.nonzero(res < 0)[0].astype(np.int64) + base
    sel = np.full(cap, -1, np.int64)
    sel[:min(len(bad), cap)] = bad[:cap]
    return sel, len(bad)


@pytest.mark.parametrize("n", SIZES)
def test_list_count_and_tail(torch, codec, n):
    import ezrs
    res = _result(n)
    res[-1] = -1                                     # the last result of the last chunk is listed
    sel, count = codec.select_failed(torch.from_numpy(res).cuda())
    assert sel.dtype == torch.int64 and tuple(sel.shape) == (n,) and tuple(count.shape) == (1,)
    esel, total = _expect(res, n)
    assert total > 0
    assert int(count.cpu()[0]) == total
    np.testing.assert_array_equal(sel.cpu().numpy(), esel)
    assert (esel[total:] == ezrs.SEL_NONE).all()


def test_all_clean_and_all_failed(torch, codec):
    n = 2 * CHUNK + 77
    res = np.abs(_result(n))
    sel, count = codec.select_failed(torch.from_numpy(res).cuda(), cap=100)
    assert int(count.cpu()[0]) == 0 and (sel.cpu().numpy() == -1).all()
    sel, count = codec.select_failed(torch.full((n,), -1, dtype=torch.int32, device="cuda"))
    assert int(count.cpu()[0]) == n
    np.testing.assert_array_equal(sel.cpu().numpy(), np.arange(n))


@pytest.mark.parametrize("cap", [0, 1, 100, 5000])
def test_cap_and_base(torch, codec, cap):
    """cap below the total: the first cap entries, count still the total; cap above it (and above
    n's own chunks): the tail is EZRS_SEL_NONE; sel beyond cap is not written."""
    n, base = 3 * CHUNK + 5, (1 << 40) + 12345
    res = _result(n, seed=1, p_bad=0.05 if cap == 5000 else 0.3)
    esel, total = _expect(res, cap, base)
    assert (total < cap) == (cap == 5000)
    buf = torch.full((cap + 8,), 55, dtype=torch.int64, device="cuda")
    cnt = torch.full((3,), 55, dtype=torch.int64, device="cuda")
    s_in, c_in = buf[:cap], cnt[1:2]
    sel, count = codec.select_failed(torch.from_numpy(res).cuda(), cap=cap, base=base, sel=s_in, count=c_in)
    assert sel is s_in and count is c_in
    np.testing.assert_array_equal(buf.cpu().numpy(), np.concatenate([esel, np.full(8, 55)]))
    np.testing.assert_array_equal(cnt.cpu().numpy(), [55, total, 55])


def test_no_results(torch, codec):
    """n == 0 still writes count[0] = 0 and fills the list."""
    sel, count = codec.select_failed(torch.empty(0, dtype=torch.int32, device="cuda"), cap=10)
    assert int(count.cpu()[0]) == 0 and (sel.cpu().numpy() == -1).all()


def test_ws_form_and_host_checks(torch, codec):
    import ezrs
    L = ezrs.lib()
    n = 3 * CHUNK + 5
    res = _result(n, seed=2)
    dres = torch.from_numpy(res).cuda()
    need = codec.select_workspace_bytes(n)
    assert need == L.ezrs_select_workspace_bytes(n) == 4 * 8
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    sel = torch.full((n,), 55, dtype=torch.int64, device="cuda")
    cnt = torch.full((1,), 55, dtype=torch.int64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    sp = ezrs._stream_ptr(None)
    EINVAL = -errno.EINVAL
    assert L.ezrs_select_failed_ws(codec._h, p(dres), n, 0, p(sel), n, p(cnt), p(ws), need - 1, sp) == EINVAL
    assert L.ezrs_select_failed_ws(codec._h, p(dres), n, 0, p(sel), n, p(cnt), None, need, sp) == EINVAL
    assert L.ezrs_select_failed(codec._h, None, n, 0, p(sel), n, p(cnt), sp) == EINVAL
    assert L.ezrs_select_failed(codec._h, p(dres), n, 0, None, n, p(cnt), sp) == EINVAL
    assert L.ezrs_select_failed(codec._h, p(dres), n, 0, p(sel), n, None, sp) == EINVAL
    assert L.ezrs_select_failed(codec._h, p(dres), n, 2 ** 64 - n, p(sel), n, p(cnt), sp) == EINVAL
    torch.cuda.synchronize()
    assert (sel.cpu().numpy() == 55).all() and int(cnt.cpu()[0]) == 55
    assert L.ezrs_select_failed_ws(codec._h, p(dres), n, 0, p(sel), n, p(cnt), p(ws), need, sp) == 0
    esel, total = _expect(res, n)
    np.testing.assert_array_equal(sel.cpu().numpy(), esel)
    assert int(cnt.cpu()[0]) == total
    assert L.ezrs_select_failed(codec._h, p(dres), n, 2 ** 64 - 1 - n, p(sel), 0, p(cnt), sp) == 0   # no overflow
    with pytest.raises(ezrs.EzrsError):
        codec.select_failed(dres.to(torch.int64))
    with pytest.raises(ezrs.EzrsError):
        codec.select_failed(dres, sel=sel[:10])                                   # shorter than cap

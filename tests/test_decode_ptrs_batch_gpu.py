"""ezrs_decode_ptrs_batch: errors-and-erasures decode of many stripes whose shards are buffers of
their own, named by a pointer table on the device.  Cases are built and decoded by the oracle on the
CPU (decode_ptrs_util.Case) and compared bit for bit: the whole arena, the results, the positions and
a subset of the correction patterns.  The table has three spare entries per stripe that hold
garbage: no call may read them.  Every case holds clean, corrected and failed codewords."""
import ctypes as C
import errno

import numpy as np
import pytest

from decode_ptrs_util import Case

pytestmark = pytest.mark.gpu

RS4 = ("rs", 255, 251)

CASES = [
    # tiles that span many stripes, fast path
    ("d4x70", dict(spec=RS4, L=10, D=4, F=70, seed=0), 16),
    ("d12x70", dict(spec=RS4, L=10, D=12, F=70, with_eras=True, seed=0), 16),
    ("d100x70", dict(spec=RS4, L=10, D=100, F=70, seed=0), 16),
    # element path, stripes straddle tiles
    ("d5x103", dict(spec=RS4, L=10, D=5, F=103, with_eras=True, seed=0), 16),
    # tiles inside one stripe and tiles across two
    ("d1000x3", dict(spec=RS4, L=10, D=1000, F=3, seed=0), 16),
    # 416 positions: above EZRS_PTRS_MAX, which does not apply here
    ("rs1023", dict(spec=("rs", 1023, 1007), L=400, D=8, F=3, seed=0), 16),
]


@pytest.fixture(scope="module")
def torch():
    import torch as T
    if not T.cuda.is_available():
        pytest.skip("no GPU")
    return T


def run(torch, case, align, launch_rows=0):
    case.require_classes()
    c = case.codec(launch_rows)
    dev, out = case.upload(torch)
    table = case.table(torch, dev)
    assert table.shape == (case.F, case.S + 3)
    res = c.decode_ptrs_batch(table, case.L, case.D, align=align, **out)
    assert res is out["result"]
    return case.check(torch, dev, out)


@pytest.mark.parametrize("args,align", [(a, al) for _, a, al in CASES], ids=[i for i, _, _ in CASES])
def test_decode_ptrs_batch_vs_oracle(torch, args, align):
    run(torch, Case(**args), align)


def test_align_selects_the_path(torch):
    """The same stripes under align 16, 4 and 1 (the element path): the same outputs; and with one
    buffer at an odd address, which only align 1 may promise."""
    args = dict(spec=RS4, L=10, D=12, F=70, with_eras=True, seed=0)
    ref = run(torch, Case(**args), 16)
    for align in (4, 1):
        for x, y in zip(ref, run(torch, Case(**args), align)):
            np.testing.assert_array_equal(x, y)
    got = run(torch, Case(cls="A1", odd=(33, 11), **args), 1)
    for x, y in zip(ref[1:], got[1:]):
        np.testing.assert_array_equal(x, y)
    got = run(torch, Case(cls="A4", odd=(33, 2), **args), 4)
    for x, y in zip(ref[1:], got[1:]):
        np.testing.assert_array_equal(x, y)


def test_several_passes(torch):
    """103 x 5 codewords staged 256 per pass (set_launch_rows): identical outputs, less workspace."""
    args = dict(spec=RS4, L=10, D=5, F=103, with_eras=True, seed=0)
    a = run(torch, Case(**args), 1)
    b = run(torch, Case(**args), 1, launch_rows=256)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    c = Case(**args).codec()
    whole = c.decode_ptrs_workspace_bytes(10, 5, 103)
    c.set_launch_rows(256)
    assert 0 < c.decode_ptrs_workspace_bytes(10, 5, 103) < whole


def _raw(torch, case, c, table, out, pitch=None, align=16, F=None, D=None, result=True, ws=None, ws_bytes=None):
    """ezrs_decode_ptrs_batch (ws is None) or ezrs_decode_ptrs_batch_ws through ctypes."""
    import ezrs
    Lib = ezrs.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    args = [c._h, p(table), table.shape[1] if pitch is None else pitch, case.L, case.D if D is None else D,
            case.F if F is None else F, align,
            p(out["eras"]) if case.with_eras else None, case.nr, p(out["neras"]) if case.with_eras else None,
            p(out["result"]) if result else None, p(out["positions"]), case.nr, p(out["corr"]), case.nr]
    sp = ezrs._stream_ptr(None)
    if ws is None:
        return Lib.ezrs_decode_ptrs_batch(*args, sp)
    return Lib.ezrs_decode_ptrs_batch_ws(*args, p(ws), ws_bytes, sp)


def test_ws_form(torch):
    """Exactly ezrs_decode_ptrs_workspace_bytes: 0; one byte less: -EINVAL and nothing written."""
    case = Case(RS4, 10, 12, 70, with_eras=True, seed=0)
    c = case.codec()
    need = c.decode_ptrs_workspace_bytes(case.L, case.D, case.F)
    assert need > c.interleaved_workspace_bytes(case.L, case.D, case.F) > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    dev, out = case.upload(torch)
    table = case.table(torch, dev)
    assert _raw(torch, case, c, table, out, ws=ws, ws_bytes=need - 1) == -errno.EINVAL
    case.untouched(torch, dev, out)
    assert _raw(torch, case, c, table, out, ws=ws, ws_bytes=need) == 0
    case.check(torch, dev, out)


def test_host_checks(torch):
    """What the host can check of a batch call, on a valid table; each leaves the arena untouched."""
    case = Case(RS4, 10, 12, 70, seed=0)
    c = case.codec()
    dev, out = case.upload(torch)
    table = case.table(torch, dev)
    EINVAL = -errno.EINVAL
    assert _raw(torch, case, c, table, out, pitch=case.S - 1) == EINVAL
    assert _raw(torch, case, c, table, out, align=3) == EINVAL
    assert _raw(torch, case, c, table, out, result=False) == EINVAL
    assert _raw(torch, case, c, table, out, F=0) == 0
    assert _raw(torch, case, c, table, out, D=0) == 0
    case.untouched(torch, dev, out)
    import ezrs
    with pytest.raises(ezrs.EzrsError):
        c.decode_ptrs_batch(table[:, :case.S - 1], case.L, case.D)             # a table too narrow
    with pytest.raises(ezrs.EzrsError):
        c.decode_ptrs_batch(table, case.L, case.D, align=3)
    case.untouched(torch, dev, out)

"""ezrs_decode_ptrs: errors-and-erasures decode of one stripe whose shards are buffers of their own,
named by a host array of device pointers.  Every case is built and decoded by the oracle on the CPU
(decode_ptrs_util.Case) and compared bit for bit: the whole arena, the results, the positions and a
subset of the correction patterns.  Every case of at least 16 codewords holds clean, corrected and
failed codewords (a condition on the inputs: the seeds are chosen so that the oracle alone gives
all three)."""
import ctypes as C
import errno

import numpy as np
import pytest

from decode_ptrs_util import Case

pytestmark = pytest.mark.gpu

RS4 = ("rs", 255, 251)

# (id, Case arguments): the smallest shapes at which the kernels can go wrong
CASES = [
    # fast and element path, below, at and across the 256-codeword tile, ragged last tile
    ("d1", dict(spec=RS4, L=10, D=1, seed=0)),
    ("d3", dict(spec=RS4, L=10, D=3, seed=0)),
    ("d4", dict(spec=RS4, L=10, D=4, seed=0)),
    ("d255", dict(spec=RS4, L=10, D=255, seed=0)),
    ("d256", dict(spec=RS4, L=10, D=256, seed=0)),
    ("d260", dict(spec=RS4, L=10, D=260, seed=0)),
    ("d516", dict(spec=RS4, L=10, D=516, seed=0)),
    # under EZRS_PTRS_MAX, rows longer than one 128-byte symbol chunk, erasures
    ("rs255_223", dict(spec=("rs", 255, 223), L=223, D=300, with_eras=True, seed=0)),
    ("ccsds_dual", dict(spec=("ccsds", 255, 223), L=20, D=260, seed=0)),          # bit-sliced family
    ("rs31_19", dict(spec=("rs", 31, 19), L=12, D=100, seed=0)),                  # generic, masked u8
    ("rs65535", dict(spec=("rs", 65535, 65503), L=40, D=37, seed=1)),             # u16 element path
]


@pytest.fixture(scope="module")
def torch():
    import torch as T
    if not T.cuda.is_available():
        pytest.skip("no GPU")
    return T


def run(torch, case, **kw):
    case.require_classes()
    c = case.codec()
    dev, out = case.upload(torch)
    res = c.decode_ptrs(case.shards(torch, dev), case.L, **out, **kw)
    assert res is out["result"]
    return case.check(torch, dev, out)


@pytest.mark.parametrize("args", [a for _, a in CASES], ids=[i for i, _ in CASES])
def test_decode_ptrs_vs_oracle(torch, args):
    run(torch, Case(**args))


def test_alignment_classes(torch):
    """One buffer at 4 mod 16 (a data position) stays on the dword path; one at an odd address (a
    parity position) must take the element path: the same results as with every buffer at 16."""
    ref = run(torch, Case(RS4, 10, 516, seed=0))
    for cls, odd in (("A4", (0, 3)), ("A1", (0, 12))):
        case = Case(RS4, 10, 516, cls=cls, odd=odd, seed=0)
        assert case.arena.off[odd] % 16 == (4 if cls == "A4" else 1)
        got = run(torch, case)
        for x, y in zip(ref[1:], got[1:]):              # results, positions, corrections
            np.testing.assert_array_equal(x, y)


def test_same_as_strided(torch):
    """decode_interleaved on a strided copy of the same symbols: every output equal."""
    case = Case(RS4, 10, 260, with_eras=True, seed=0)
    _, res, pos, corr = run(torch, case)
    c = case.codec()
    fr = torch.from_numpy(case.frames()).cuda()
    _, out = case.upload(torch)
    c.decode_interleaved(fr, **out)
    _, res2, pos2, corr2 = case.outputs(torch, fr, out)
    np.testing.assert_array_equal(res2, res)
    np.testing.assert_array_equal(pos2, pos)
    np.testing.assert_array_equal(corr2, corr)
    from interleave_util import interleave
    np.testing.assert_array_equal(fr.cpu().numpy(), interleave(case.orow, 1, case.D))


def test_karn_semantics(torch):
    """Shortened RS(255,223) under EZRS_SEM_KARN: erasures and positions in the full NN frame."""
    run(torch, Case(("rs", 255, 223), 150, 40, with_eras=True, karn=True, seed=0))


def _raw(torch, case, c, dev, out, shards=None, L=None, D=None, result=True, ws=None, ws_bytes=None):
    """ezrs_decode_ptrs (ws is None) or ezrs_decode_ptrs_ws through ctypes."""
    import ezrs
    Lib = ezrs.lib()
    if shards is None:
        shards = [t.data_ptr() for t in case.shards(torch, dev)]
    arr = (C.c_void_p * len(shards))(*shards)
    p = lambda t: C.c_void_p(t.data_ptr())
    args = [c._h, arr, case.L if L is None else L, case.D if D is None else D,
            p(out["eras"]) if case.with_eras else None, case.nr, p(out["neras"]) if case.with_eras else None,
            p(out["result"]) if result else None, p(out["positions"]), case.nr, p(out["corr"]), case.nr]
    sp = ezrs._stream_ptr(None)
    if ws is None:
        return Lib.ezrs_decode_ptrs(*args, sp)
    return Lib.ezrs_decode_ptrs_ws(*args, p(ws), ws_bytes, sp)


def test_ws_form(torch):
    """Exactly ezrs_decode_ptrs_workspace_bytes: 0; one byte less: -EINVAL and nothing written."""
    case = Case(RS4, 10, 260, with_eras=True, seed=0)
    c = case.codec()
    need = c.decode_ptrs_workspace_bytes(case.L, case.D, 1)
    assert need > c.interleaved_workspace_bytes(case.L, case.D, 1) > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    dev, out = case.upload(torch)
    assert _raw(torch, case, c, dev, out, ws=ws, ws_bytes=need - 1) == -errno.EINVAL
    case.untouched(torch, dev, out)
    assert _raw(torch, case, c, dev, out, ws=ws, ws_bytes=need) == 0
    case.check(torch, dev, out)


def test_host_checks(torch):
    """Every rule the host checks before any launch; each leaves the arena untouched."""
    case = Case(RS4, 10, 260, seed=0)
    c = case.codec()
    dev, out = case.upload(torch)
    EINVAL = -errno.EINVAL
    good = [t.data_ptr() for t in case.shards(torch, dev)]
    assert _raw(torch, case, c, dev, out, shards=good[:5] + [None] + good[6:]) == EINVAL       # a NULL entry
    assert _raw(torch, case, c, dev, out, shards=good[:5] + [good[2]] + good[6:]) == EINVAL    # the same buffer twice
    assert _raw(torch, case, c, dev, out, shards=good[:13] + [good[1] + case.D - 1]) == EINVAL  # one byte shared
    assert _raw(torch, case, c, dev, out, L=0) == EINVAL
    assert _raw(torch, case, c, dev, out, L=c.load + 1) == EINVAL
    assert _raw(torch, case, c, dev, out, result=False) == EINVAL
    assert _raw(torch, case, c, dev, out, D=0) == 0                                            # nothing to do
    case.untouched(torch, dev, out)
    import ezrs
    with pytest.raises(ezrs.EzrsError):
        c.decode_ptrs(case.shards(torch, dev)[:-1], case.L)                                    # a shard short
    assert c.decode_ptrs_workspace_bytes(0, case.D, 1) == 0 == c.decode_ptrs_workspace_bytes(case.L, 0, 1)


def test_ptrs_max(torch):
    """RS(1023,1007) at len 400 names 416 shards, above EZRS_PTRS_MAX: -ENOTSUP, nothing written (the
    batch form decodes the same stripes: test_decode_ptrs_batch_gpu.py)."""
    case = Case(("rs", 1023, 1007), 400, 8, seed=0)
    c = case.codec()
    dev, out = case.upload(torch)
    assert _raw(torch, case, c, dev, out) == -errno.ENOTSUP
    case.untouched(torch, dev, out)

"""ezrs_decode_interleaved_select: ezrs_decode_interleaved of only the codewords a device list
names, on CCSDS depth-I frames and on a striped frame with gaps.  The codewords, their corruption and
the oracle's decode come from decode_ptrs_util.Case (its rows are frame-major, k = f * depth + j);
here they lie in one strided buffer pre-filled with random data, and the whole buffer is compared bit
for bit: the selected codewords as the oracle leaves them, every other codeword still corrupted, and
every element that is no symbol (gaps of sym_stride > depth, the padding of frame_pitch, the ends)
unchanged.  Every selection holds clean, corrected and failed codewords."""
import ctypes as C
import errno
import functools

import numpy as np
import pytest

from decode_ptrs_util import Case
from decode_select_util import Selection, mixed_selection
from interleave_util import frame_view, interleave
from test_interleaved_gpu import _dev, _frames, _host

pytestmark = pytest.mark.gpu

CASES = {
    # CCSDS depth 5 codeblocks, sym_stride == depth, frames back to back
    "ccsds_i5": (dict(spec=("ccsds", 255, 223), L=223, D=5, F=103, with_eras=True), 5, 0, 0),
    # striped frames: gaps of 28 after every symbol row, a padded frame pitch, an odd base
    "striped_gaps": (dict(spec=("rs", 255, 251), L=10, D=100, F=7, with_eras=True), 128, 9, 3),
    # 16-bit symbols, rows longer than a symbol chunk
    "rs1023": (dict(spec=("rs", 1023, 1001), L=200, D=5, F=8, with_eras=True), 6, 1, 0),
}


@pytest.fixture(scope="module")
def torch():
    import torch as T
    if not T.cuda.is_available():
        pytest.skip("no GPU")
    return T


@functools.lru_cache(maxsize=None)
def case_of(name):
    """One oracle run per geometry, shared and never modified."""
    return Case(seed=0, **CASES[name][0])


def layout(case, ss, pad, off, rows, base=None):
    """The flat buffer (a copy of `base`, or random) with the codeword rows `rows` laid out in it."""
    fp = case.S * ss + pad
    if base is None:
        rng = np.random.default_rng([case.D, case.F, ss])
        base = rng.integers(0, 1 << (8 * case.dt().itemsize), off + case.F * fp + 5).astype(case.dt)
    buf = base.copy()
    frame_view(buf, case.F, case.S, case.D, fp, ss, off)[...] = interleave(rows, case.F, case.D)
    return buf, fp


def run(torch, name, sel, count=None, ws=None):
    args, ss, pad, off = CASES[name]
    case = case_of(name)
    s = Selection(case, sel, count)
    s.require_classes()
    bad, fp = layout(case, ss, pad, off, case.brows)
    exp, _ = layout(case, ss, pad, off, s.rows, bad)
    dev = _dev(torch, bad)
    fv = _frames(torch, dev, case.F, case.S, case.D, fp, ss, off)
    dsel, dcount, out = s.upload(torch)
    c = case.codec()
    if ws is None:
        res = c.decode_interleaved_select(fv, dsel, count=dcount, **out)
        assert res is out["result"]
    else:
        import ezrs
        p = lambda t: C.c_void_p(t.data_ptr())
        need = c.decode_select_workspace_bytes(case.L, s.nsel)
        assert need > 0
        wsbuf = torch.empty(need, dtype=torch.uint8, device="cuda")
        a = (c._h, p(fv), fp, ss, case.D, case.L, case.F, p(dsel), s.nsel, None if dcount is None else p(dcount),
             p(out["eras"]), case.nr, p(out["neras"]), p(out["result"]), p(out["positions"]), case.nr, p(out["corr"]),
             case.nr, p(wsbuf))
        sp = ezrs._stream_ptr(None)
        assert ezrs.lib().ezrs_decode_interleaved_select_ws(*a, need - 1, sp) == -errno.EINVAL
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_host(torch, dev), bad)
        assert (out["result"].cpu().numpy() == 77).all()
        assert ezrs.lib().ezrs_decode_interleaved_select_ws(*a, need, sp) == 0
    s.check_out(torch, out)
    np.testing.assert_array_equal(_host(torch, dev), exp,
                                  err_msg="frames (a selected codeword, one that was not, or an element that is no symbol)")
    return s


@pytest.mark.parametrize("name", list(CASES))
def test_mixed_selection(torch, name):
    """Every corrupted codeword and a few clean ones, shuffled, with SEL_NONE and out-of-range
    entries among them."""
    case = case_of(name)
    s = run(torch, name, mixed_selection(case, clean=min(20, int((case.ores == 0).sum()))))
    assert (~s.used).sum() == 10


def test_device_count_and_ws_form(torch):
    """A device count below the list's length, through the caller-owned workspace."""
    case = case_of("striped_gaps")
    sel = mixed_selection(case, seed=2)
    s = run(torch, "striped_gaps", sel, count=len(sel) - 100, ws=True)
    tail = s.sel[len(sel) - 100:]
    tail = tail[(tail >= 0) & (tail < case.ncw)]
    assert (case.ores[tail] != 0).any()             # corrupted codewords past the count: left as they are


def test_host_checks(torch):
    import ezrs
    args, ss, pad, off = CASES["striped_gaps"]
    case = case_of("striped_gaps")
    s = Selection(case, mixed_selection(case))
    bad, fp = layout(case, ss, pad, off, case.brows)
    dev = _dev(torch, bad)
    fv = _frames(torch, dev, case.F, case.S, case.D, fp, ss, off)
    dsel, _, out = s.upload(torch)
    c = case.codec()
    p = lambda t: C.c_void_p(t.data_ptr())
    sp = ezrs._stream_ptr(None)

    def call(fr=p(fv), fp=fp, ss=ss, sel=p(dsel), nsel=s.nsel, res=p(out["result"]), F=case.F):
        return ezrs.lib().ezrs_decode_interleaved_select(c._h, fr, fp, ss, case.D, case.L, F, sel, nsel, None,
                                                         p(out["eras"]), case.nr, p(out["neras"]), res,
                                                         p(out["positions"]), case.nr, p(out["corr"]), case.nr, sp)

    EINVAL = -errno.EINVAL
    assert call(fr=None) == EINVAL
    assert call(ss=case.D - 1) == EINVAL
    assert call(fp=(case.S - 1) * ss + case.D - 1) == EINVAL
    assert call(sel=None) == EINVAL
    assert call(res=None) == EINVAL
    assert call(nsel=0) == 0 and call(nsel=0, sel=None, res=None, fr=None) == 0
    assert call(F=0) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_host(torch, dev), bad)
    assert (out["result"].cpu().numpy() == 77).all()
    with pytest.raises(ezrs.EzrsError):
        c.decode_interleaved_select(fv, dsel.to(torch.int32))
    with pytest.raises(ezrs.EzrsError):
        c.decode_interleaved_select(fv, dsel.cpu())

"""The scrub the selection calls were built for, on one stream with no host synchronisation or read
between its three calls: a verify of every stripe (ezrs_reconstruct_ptrs_batch under an nlost == 0
plan), ezrs_select_failed on the verify's results, ezrs_decode_ptrs_select with the list and the
count still on the device.  What it leaves is what the full decode leaves (decode_ptrs_util.Case.exp),
bit for bit over the whole arena."""
import numpy as np
import pytest

from decode_ptrs_util import Case
from ptrs_util import download

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as T
    if not T.cuda.is_available():
        pytest.skip("no GPU")
    return T


def test_scrub_pipeline(torch):
    case = Case(("rs", 255, 251), L=10, D=100, F=70, seed=0)
    case.require_classes()
    # without erasures a codeword is valid as received exactly when the oracle's result is 0
    failing = np.nonzero(case.ores != 0)[0]
    cap = len(failing) + 50
    c = case.codec()
    verify_plan = c.recon_plan(case.L, [])
    dev = case.arena.upload(torch, case.bad)
    table = case.table(torch, dev)
    verify = torch.full((case.ncw,), 77, dtype=torch.int32, device="cuda")
    result = torch.full((cap,), 77, dtype=torch.int32, device="cuda")
    positions = torch.zeros((cap, case.nr), dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()                         # the uploads, on the default stream
    with torch.cuda.stream(stream):
        verify_plan.reconstruct_ptrs_batch(table, case.D, align=16, result=verify, stream=stream)
        sel, count = c.select_failed(verify, cap=cap, stream=stream)
        c.decode_ptrs_select(table, case.L, case.D, sel, count=count, result=result, positions=positions,
                             stream=stream)
    stream.synchronize()
    v = verify.cpu().numpy()
    np.testing.assert_array_equal(v, np.where(case.ores != 0, -1, 0), err_msg="verify")
    n = int(count.cpu()[0])
    assert n == len(failing)
    sel = sel.cpu().numpy()
    np.testing.assert_array_equal(sel[:n], failing)
    assert (sel[n:] == -1).all() and len(sel) == cap
    np.testing.assert_array_equal(download(dev), case.exp, err_msg="arena after the scrub")
    res = result.cpu().numpy()
    np.testing.assert_array_equal(res[:n], case.ores[failing])
    assert (res[n:] == 0).all()                      # skipped rows: the all-zero word, no erasures
    pos = positions.cpu().numpy().view(np.uint32)
    for i in np.nonzero(res[:n] > 0)[0]:
        np.testing.assert_array_equal(pos[i, :res[i]], case.opos[failing[i], :res[i]], err_msg=f"positions row {i}")

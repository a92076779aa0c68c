"""The interleaved fixture (tests/golden/interleaved_ccsds.npz, generated from the reference codec by
tests/golden/make_interleaved_fixtures.py) against the oracle restatement: de-interleaving the
frames with the tests' own helper and running oracle.Codec per codeword reproduces the reference's
recorded parity, results, corrected frames and positions.  This pins the interleave helper and the
fixture independently of the device."""
import numpy as np
import pytest

import oracle as O
from interleave_util import deinterleave, frame_view, interleave, load_fixture

K, NR = 223, 32
CASES = load_fixture()


def test_fixture_shapes():
    assert sorted(int(c["depth"][0]) for c in CASES) == [4, 5]
    for c in CASES:
        I = int(c["depth"][0])
        F = c["enc"].shape[0]
        assert c["enc"].shape == c["bad"].shape == c["out"].shape == (F, K + NR, I)
        assert c["enc"].dtype == np.uint8 and c["enc"][0].size == 255 * I   # 1275 / 1020 bytes
        assert c["eras"].shape == c["positions"].shape == (F * I, NR)
        res = c["result"]
        assert (res == -1).sum() >= 1 and (res > 0).sum() >= 1 and (c["neras"] > 0).sum() >= 1


def test_helpers_are_inverse_and_match_the_layout():
    rng = np.random.default_rng(1)
    F, S, D, ss, fp, off = 3, 7, 5, 6, 50, 2
    buf = rng.integers(0, 256, off + F * fp).astype(np.uint8)
    v = frame_view(buf, F, S, D, fp, ss, off)
    rows = deinterleave(v)
    for f in range(F):
        for j in range(D):
            for s in range(S):
                assert rows[f * D + j, s] == buf[off + f * fp + s * ss + j]
    np.testing.assert_array_equal(interleave(rows, F, D), v)


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"I{int(c['depth'][0])}")
def test_fixture_vs_oracle(case):
    oc = O.Codec(*O.ccsds_params(K, True))
    I = int(case["depth"][0])
    F = case["enc"].shape[0]
    rows = deinterleave(case["enc"])
    exp = rows.copy()
    rows[:, K:] = 0
    oc.encode_batch(rows, K)
    np.testing.assert_array_equal(rows, exp, err_msg="parity")
    bad = deinterleave(case["bad"])
    pos = np.zeros((F * I, NR), np.uint32)
    res = oc.decode_batch(bad, K, None, case["eras"].copy(), case["neras"].copy(), pos)
    np.testing.assert_array_equal(res, case["result"])
    np.testing.assert_array_equal(interleave(bad, F, I), case["out"])
    for k, r in enumerate(res):
        if r > 0:
            np.testing.assert_array_equal(pos[k, :r], case["positions"][k, :r], err_msg=f"cw {k}")

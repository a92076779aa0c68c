"""The batches of tests/generic_util.py under the oracle alone: every case of the two matrices of
test_generic_gpu.py holds what the GPU tests rely on -- the three result classes, rows past every
block boundary that need work, each special row kind, the reference's partial fix kept on failure
(direct datum) or a failed row left alone and junk bits preserved (masked datum) -- and the oracle
gives the same verdict on a batch whatever its layout.  Each item is a condition of the case and its
seed: a seed that misses one is replaced, the condition stays."""
import numpy as np
import pytest

import generic_util as G

A_IDS = [e[0] for e in G.MATRIX_A]
B_IDS = [e[0] for e in G.MATRIX_B]


def _check_layouts(layouts):
    """The conditions on every layout, and one verdict over all of them."""
    first = layouts[0]
    b = first.packed
    for c in layouts:
        assert c.packed is b
        rows = G.logical_rows(c, c.exp) if not c.split else G.logical_rows(c, None, c.exp_data, c.exp_par)
        G.check_result_mix(c, c.res, rows)
        np.testing.assert_array_equal(c.res, b.res)
        np.testing.assert_array_equal(rows, b.exp)
        for k in np.nonzero(b.res > 0)[0]:
            np.testing.assert_array_equal(c.pos[k, :b.res[k]], b.pos[k, :b.res[k]])
        # padding columns are the sentinel before and after
        if c.split:
            assert (c.exp_data[:, c.L:] == c.fill).all() and (c.exp_par[:, c.nr:] == c.fill).all()
        else:
            assert (c.exp[:, c.S:] == c.fill).all()
        # encode: parity from the oracle, the same in both forms, padding untouched
        np.testing.assert_array_equal(c.enc[:, :c.S], b.clean)
        np.testing.assert_array_equal(c.enc_par[:, :c.nr], b.clean[:, c.L:])
        assert (c.enc[:, c.S:] == c.fill).all() and (c.enc_par[:, c.nr:] == c.fill).all()
        assert (c.enc_data[:, c.L:] == c.fill).all()
        np.testing.assert_array_equal(c.enc_data[:, :c.L], b.clean[:, :c.L])


def _check_corr_rows(b):
    rows = set(b.corr_rows.tolist())
    assert len(rows) <= G.MAX_CORR_ROWS and {0, b.ncw - 1} <= rows
    for edge in range(64, b.ncw, 64):
        assert {edge - 1, edge} <= rows
    # outside the sampled rows the corr array is the sentinel
    rest = np.setdiff1d(np.arange(b.ncw), b.corr_rows)
    assert (b.corr[rest] == b.fill).all()
    if b.ncw >= 22:
        assert any(b.res[k] > 0 and (b.corr[k, :b.res[k]] != b.fill).any() for k in b.corr_rows)


@pytest.mark.parametrize("entry", G.MATRIX_A, ids=A_IDS)
def test_matrix_a_case(entry):
    layouts = [G.case_a(entry, False), G.case_a(entry, True)]
    assert layouts[0].pitch == layouts[0].S + G.A_PITCH_EXTRA
    _check_layouts(layouts)
    _check_corr_rows(layouts[0].packed)


@pytest.mark.parametrize("entry", G.MATRIX_B, ids=B_IDS)
def test_matrix_b_case(entry):
    fallback, fast = G.case_b(entry, False), G.case_b(entry, True)
    geom = entry[5]
    assert fallback.split if geom == "split" else fallback.pitch == geom
    assert not fast.split and fast.pitch == fast.S
    assert not fallback.masked                      # the fast codecs are direct-datum codecs
    _check_layouts([fallback, fast])
    _check_corr_rows(fallback.packed)


def test_matrices_cover_the_block_sizes():
    """Batches on both sides of 64 (u8/32 decode block), of 256 (encode, u16/256 decode) and of 8
    codewords per block (lane kernels), every one but the two full-block cases ending in a partial
    block; masked and direct codecs, both datum widths."""
    ncws = {e[3] for e in G.MATRIX_A}
    assert {1, 64, 65} <= ncws and any(n > 256 for n in ncws) and any(64 < n < 256 for n in ncws)
    assert all(e[3] % 64 for e in G.MATRIX_A if e[3] != 64)
    assert all(e[3] % 256 and e[3] > 128 for e in G.MATRIX_B)
    masked = [G.case_a(e, False).masked for e in G.MATRIX_A]
    assert any(masked) and not all(masked)
    assert {G.case_a(e, False).bits for e in G.MATRIX_A} == {8, 16}

"""The parity-update plan's matrix on the host (ezrs_update_bitmatrix, include/ezrs.h): no GPU.
For each codec and set of changed positions, codewords are encoded by the oracle, the changed
symbols replaced and the codewords encoded again: the difference of the two parities must equal the
bit-column matrix applied in numpy to the difference of the changed symbols, and the matrix must be
the columns `changed` of the rebuild rows of the all-parity reconstruction plan."""
import ctypes as C
import errno

import numpy as np
import pytest

import ezrs
import oracle as O

RS255_223 = O.rs_params(255, 223)
RS255_251 = O.rs_params(255, 251)


def apply_bitmatrix(cols, delta):
    """cols [nroots, nchanged, m], delta [ncw, nchanged] -> [ncw, nroots]: output symbol = XOR over
    the changed positions r and the set bits b of their deltas of cols[row, r, b]."""
    nroots, nchg, m = cols.shape
    out = np.zeros((delta.shape[0], nroots), np.uint16)
    for r in range(nchg):
        x = delta[:, r].astype(np.uint32)
        for b in range(m):
            bit = ((x >> b) & 1).astype(bool)
            out[bit] ^= cols[:, r, b]
    return out


CASES = [
    # (name, codec parameters, len, changed)
    ("rs255_223-first", RS255_223, 223, [0]),
    ("rs255_223-last", RS255_223, 223, [222]),
    ("rs255_223-three", RS255_223, 223, [0, 111, 222]),
    ("rs255_251-l10-one", RS255_251, 10, [3]),
    ("rs255_251-l10-all", RS255_251, 10, list(range(10))),
    ("ccsds255_223-dual", O.ccsds_params(223, True), 223, [5, 100]),
    ("ccsds_conv255_239-l20", O.ccsds_params(239, False), 20, [19]),
    ("rs255_223-l14-unordered", RS255_223, 14, [13, 0]),
    ("rs31_27-l20", O.rs_params(31, 27), 20, [1, 2]),
    ("rs1023_1007-l100", O.rs_params(1023, 1007), 100, [0, 50, 99]),
]
NCW = 32


@pytest.mark.parametrize("name,params,length,changed", CASES, ids=[c[0] for c in CASES])
def test_bitmatrix_vs_oracle(name, params, length, changed):
    mm, _, _, _, nroots, _ = params
    oc = O.Codec(*params)
    S, nchg = length + nroots, len(changed)
    rng = np.random.default_rng(length * 131 + nchg)
    old = rng.integers(0, 1 << mm, (NCW, S)).astype(oc.dtype)
    oc.encode_batch(old, length)
    new = old.copy()
    new[:, changed] = rng.integers(0, 1 << mm, (NCW, nchg)).astype(oc.dtype)
    oc.encode_batch(new, length)

    cols = ezrs.update_bitmatrix(params, length, changed)
    assert cols.shape == (nroots, nchg, mm)
    assert int(cols.max()) < (1 << mm)
    np.testing.assert_array_equal(new[:, length:] ^ old[:, length:],
                                  apply_bitmatrix(cols, old[:, changed] ^ new[:, changed]),
                                  err_msg="parity difference")

    # the columns `changed` of the all-parity plan, whose survivors are exactly the data positions
    full, surv = ezrs.recon_bitmatrix(params, length, list(range(length, S)))
    np.testing.assert_array_equal(surv, np.arange(length))
    np.testing.assert_array_equal(cols, full[:nroots][:, changed, :])

    if nchg == length:                                  # the matrix on the data itself: the parity
        np.testing.assert_array_equal(apply_bitmatrix(cols, new[:, changed]), new[:, length:])


def _raw(params, length, changed, nchanged=None, cols=True, cap=None, null_changed=False):
    mm, poly, fcr, prim, nroots, dual = params
    nchanged = len(changed) if nchanged is None else nchanged
    arr = (C.c_uint32 * max(len(changed), 1))(*changed)
    n = max(nroots * max(len(changed), 1) * mm, 1)
    cbuf = np.zeros(n, np.uint16)
    return ezrs.lib().ezrs_update_bitmatrix(
        mm, poly, fcr, prim, nroots, int(dual), length, None if null_changed else arr, nchanged,
        cbuf.ctypes.data_as(C.c_void_p) if cols else None, n if cap is None else cap)


def test_bitmatrix_errors():
    EINVAL = -errno.EINVAL
    p = RS255_251
    assert _raw(p, 10, [3]) == 0
    assert _raw(p, 10, list(range(10))) == 0
    # invalid codec parameters (the rules of ezrs_create)
    assert _raw((8, 0x11d, 1, 1, 0, False), 10, [3]) == EINVAL       # no parity
    assert _raw((8, 0x11d, 1, 1, 255, False), 10, [3]) == EINVAL     # nroots >= N
    assert _raw((8, 0x101, 1, 1, 4, False), 10, [3]) == EINVAL       # poly not primitive
    assert _raw((17, 0x11d, 1, 1, 4, False), 10, [3]) == EINVAL      # symbol size
    assert _raw((8, 0x11d, 1, 0, 4, False), 10, [3]) == EINVAL       # prim == 0
    assert _raw((5, 0x25, 1, 1, 4, True), 10, [3]) == EINVAL         # dual basis needs m == 8
    # len outside 1..load
    assert _raw(p, 0, [0]) == EINVAL
    assert _raw(p, 1, [0]) == 0
    assert _raw(p, 251, [0]) == 0
    assert _raw(p, 252, [0]) == EINVAL
    # nchanged outside 1..len
    assert _raw(p, 10, [], nchanged=0) == EINVAL
    assert _raw(p, 10, [7], nchanged=1) == 0
    assert _raw(p, 3, [0, 1, 2]) == 0
    assert _raw(p, 3, [0, 1, 2, 3]) == EINVAL                        # nchanged > len (and 3 >= len)
    assert _raw(p, 3, [0, 1, 2, 1]) == EINVAL                        # nchanged > len (and a duplicate)
    # the positions
    assert _raw(p, 10, [10]) == EINVAL                               # a parity position
    assert _raw(p, 10, [9]) == 0
    assert _raw(p, 10, [3, 5, 3]) == EINVAL                          # given twice
    assert _raw(p, 10, [3, 5, 4]) == 0
    # null pointers, capacity
    assert _raw(p, 10, [1], null_changed=True) == EINVAL
    assert _raw(p, 10, [1], cols=False) == EINVAL
    need = 4 * 2 * 8
    assert _raw(p, 10, [1, 2], cap=need - 1) == EINVAL
    assert _raw(p, 10, [1, 2], cap=need) == 0
    with pytest.raises(ezrs.EzrsError):
        ezrs.update_bitmatrix(p, 10, [3, 3])
    with pytest.raises(ezrs.EzrsError):
        ezrs.update_bitmatrix(p, 10, [])

"""The reconstruction plan's matrix on the host (ezrs_recon_bitmatrix, include/ezrs.h): no GPU.
For each codec and loss pattern the bit-column matrix is applied in numpy to the survivors of
oracle-encoded codewords: the rebuild rows must give the oracle's symbols at the lost positions (in
the order of `lost`), the check rows must be zero exactly on the codewords whose survivors are
intact, and the oracle's own errors-and-erasures decode with the same shared erasures must restore
the same words."""
import ctypes as C
import errno

import numpy as np
import pytest

import ezrs
import oracle as O

RS255_223 = O.rs_params(255, 223)
RS255_251 = O.rs_params(255, 251)

CASES = [
    # (name, codec parameters, len, lost)
    ("rs255_223-full-32lost", RS255_223, 223, list(range(0, 64, 2))),
    ("rs255_251-l10", RS255_251, 10, [0, 3, 11, 13]),
    ("ccsds255_223-dual", O.ccsds_params(223, True), 223, [5, 222, 223, 254]),
    ("ccsds_conv255_239-l20", O.ccsds_params(239, False), 20, [35, 0, 7]),
    ("rs255_223-l14", RS255_223, 14, [45, 0, 13, 14]),
    ("rs31_27-l20", O.rs_params(31, 27), 20, [1, 2, 23]),
    ("rs1023_1007-l100", O.rs_params(1023, 1007), 100, [0, 50, 100, 115]),
    ("rs255_251-l10-all-parity", RS255_251, 10, [10, 11, 12, 13]),
    ("rs255_251-l10-none", RS255_251, 10, []),
]
NCW = 32


def apply_bitmatrix(cols, surv_rows):
    """cols [nroots, nsurv, m], surv_rows [ncw, nsurv] -> [ncw, nroots]: output symbol = XOR over the
    survivors c and their set bits b of cols[row, c, b]."""
    nroots, nsurv, m = cols.shape
    out = np.zeros((surv_rows.shape[0], nroots), np.uint16)
    for c in range(nsurv):
        x = surv_rows[:, c].astype(np.uint32)
        for b in range(m):
            bit = ((x >> b) & 1).astype(bool)
            out[bit] ^= cols[:, c, b]
    return out


@pytest.mark.parametrize("name,params,length,lost", CASES, ids=[c[0] for c in CASES])
def test_bitmatrix_vs_oracle(name, params, length, lost):
    mm, _, _, _, nroots, _ = params
    oc = O.Codec(*params)
    S, nlost = length + nroots, len(lost)
    rng = np.random.default_rng(length * 131 + nlost)
    rows = rng.integers(0, 1 << mm, (NCW, S)).astype(oc.dtype)
    oc.encode_batch(rows, length)

    cols, surv = ezrs.recon_bitmatrix(params, length, lost)
    assert cols.shape == (nroots, S - nlost, mm)
    np.testing.assert_array_equal(surv, [p for p in range(S) if p not in set(lost)])
    assert int(cols.max(initial=0)) < (1 << mm)

    out = apply_bitmatrix(cols, rows[:, surv])
    np.testing.assert_array_equal(out[:, :nlost], rows[:, lost], err_msg="rebuild rows")
    assert not out[:, nlost:].any(), "check rows on clean codewords"
    if lost == list(range(length, S)):                  # a pure encode: the oracle's parity
        np.testing.assert_array_equal(out[:, :nroots], rows[:, length:])

    # one survivor symbol altered in every third codeword: the check rows see exactly those
    bad = rows.copy()
    hit = np.arange(NCW) % 3 == 1
    for k in np.nonzero(hit)[0]:
        p = surv[int(rng.integers(0, len(surv)))]
        bad[k, p] ^= rng.integers(1, 1 << mm)
    out = apply_bitmatrix(cols, bad[:, surv])
    if nlost < nroots:
        np.testing.assert_array_equal(out[:, nlost:].any(axis=1), hit, err_msg="check rows")
    else:
        assert out.shape[1] == nlost                    # nothing left to check with

    # the yardstick itself: the oracle's decode with the shared erasures restores the same words
    gone = rows.copy()
    gone[:, lost] = rng.integers(0, 1 << mm, (NCW, nlost)).astype(oc.dtype)
    eras = np.zeros((NCW, nroots), np.uint32)
    eras[:, :nlost] = lost
    res = oc.decode_batch(gone, length, None, eras, np.full(NCW, nlost, np.uint32))
    np.testing.assert_array_equal(gone, rows)
    # the oracle counts an erasure as a correction even when the garbage happened to be right
    np.testing.assert_array_equal(res, np.full(NCW, nlost))


def _raw(params, length, lost, nlost=None, cols=True, cap=None, surv=True):
    mm, poly, fcr, prim, nroots, dual = params
    nlost = len(lost) if nlost is None else nlost
    arr = (C.c_uint32 * max(len(lost), 1))(*lost)
    n = max(nroots * (length + nroots) * mm, 1)
    cbuf = np.zeros(n, np.uint16)
    sbuf = np.zeros(length + nroots + 1, np.uint32)
    return ezrs.lib().ezrs_recon_bitmatrix(
        mm, poly, fcr, prim, nroots, int(dual), length, arr if lost or nlost == 0 else None, nlost,
        cbuf.ctypes.data_as(C.c_void_p) if cols else None, n if cap is None else cap,
        sbuf.ctypes.data_as(C.c_void_p) if surv else None)


def test_bitmatrix_errors():
    EINVAL = -errno.EINVAL
    p = RS255_251
    assert _raw(p, 10, [0, 3, 11, 13]) == 0
    assert _raw(p, 10, []) == 0
    # invalid codec parameters (the rules of ezrs_create)
    assert _raw((8, 0x11d, 1, 1, 0, False), 10, []) == EINVAL        # no parity
    assert _raw((8, 0x11d, 1, 1, 255, False), 10, []) == EINVAL      # nroots >= N
    assert _raw((8, 0x101, 1, 1, 4, False), 10, []) == EINVAL        # poly not primitive
    assert _raw((17, 0x11d, 1, 1, 4, False), 10, []) == EINVAL       # symbol size
    assert _raw((8, 0x11d, 1, 0, 4, False), 10, []) == EINVAL        # prim == 0
    assert _raw((5, 0x25, 1, 1, 4, True), 10, []) == EINVAL          # dual basis needs m == 8
    # len outside 1..load
    assert _raw(p, 0, []) == EINVAL
    assert _raw(p, 252, []) == EINVAL
    assert _raw(p, 251, []) == 0
    # the loss list
    assert _raw(p, 10, [0, 1, 2, 3, 4]) == EINVAL                    # nlost > nroots
    assert _raw(p, 10, [14]) == EINVAL                               # position >= S
    assert _raw(p, 10, [13]) == 0
    assert _raw(p, 10, [3, 5, 3]) == EINVAL                          # duplicate
    # outputs
    assert _raw(p, 10, [1], cols=False) == EINVAL
    assert _raw(p, 10, [1], surv=False) == EINVAL
    need = 4 * 13 * 8
    assert _raw(p, 10, [1], cap=need - 1) == EINVAL
    assert _raw(p, 10, [1], cap=need) == 0
    with pytest.raises(ezrs.EzrsError):
        ezrs.recon_bitmatrix(p, 10, [3, 3])

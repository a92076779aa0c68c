"""The per-codeword RS kernels (ezrs_generic.hip: k_encode_generic / k_decode_generic in their u8/32,
u8/256 and u16/256 instances, k_encode_lanes / k_decode_lanes with LDS and with global tables) and
the fallback decodes of the fast codecs, as batch kernels against the oracle, bit-exact.

Matrix A (generic_util.MATRIX_A): codecs whose own path is the per-codeword kernels, in batches on
both sides of every block size of the file (64 lanes, 256 lanes, 8 codewords per block), ending in a
partial block, with a lone lane and an exactly full block.  Matrix B: fast codecs whose call
geometry (parity in its own buffer, a row pitch above 256) pushes the decode onto the fallbacks; the
same batch also runs as packed rows through the codec's fast path, and the two must agree with each
other and with the oracle on every row kind.  The batches and what they must contain are those of
tests/test_generic_cases_oracle.py."""
import numpy as np
import pytest

import generic_util as G

pytestmark = pytest.mark.gpu

POS_FILL = 0xEEEEEEEE
A_IDS = [e[0] for e in G.MATRIX_A]
B_IDS = [e[0] for e in G.MATRIX_B]


@pytest.fixture(scope="module")
def torch():
    import torch as T
    if not T.cuda.is_available():
        pytest.skip("no GPU")
    return T


def _dev(torch, a):
    """A numpy array on the GPU (uint16 travels as int16, uint32 as int32: same bytes)."""
    a = np.array(a, order="C")                  # a copy: the arrays of a case are read-only
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else
                            a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def _codec(params, path):
    import ezrs
    c = ezrs.Codec(*params)
    assert c.kernel_path == path
    return c


def _check_encode(torch, codec, c):
    """Inline with pitch padding, and split into a parity array nroots + 3 wide from data rows at
    pitch L + 7; padding and the extra parity columns keep their sentinel (they are part of the
    compared arrays)."""
    assert c.pitch > c.S and (c.enc_in[:, c.S:] == c.fill).all()
    d = _dev(torch, c.enc_in)
    codec.encode(d, c.L)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_host(d, c.dtype), c.enc, err_msg="encode, inline")
    d = _dev(torch, c.enc_data)
    p = _dev(torch, np.full(c.enc_par.shape, c.fill, c.dtype))
    codec.encode(d, c.L, p)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_host(p, c.dtype), c.enc_par, err_msg="encode, split: parity")
    np.testing.assert_array_equal(_host(d, c.dtype), c.enc_data, err_msg="encode, split: data")
    assert (c.enc_par[:, c.nr:] == c.fill).all() and c.enc_par.shape[1] == c.nr + 3


def _decode(torch, codec, c):
    """Decode the case's layout on the GPU with erasures, positions and corr (each output nroots + 2
    wide, prefilled); returns (rows or (data, parity), results, positions, corr) on the host."""
    wide = c.nr + 2
    eras, neras = _dev(torch, c.eras), _dev(torch, c.neras)
    pos = _dev(torch, np.full((c.ncw, wide), POS_FILL, np.uint32))
    corr = _dev(torch, np.full((c.ncw, wide), c.fill, c.dtype))
    if c.split:
        d, p = _dev(torch, c.data), _dev(torch, c.par)
        r = codec.decode(d, c.L, parity=p, eras=eras, neras=neras, positions=pos, corr=corr)
    else:
        d, p = _dev(torch, c.cw), None
        r = codec.decode(d, c.L, eras=eras, neras=neras, positions=pos, corr=corr)
    torch.cuda.synchronize()
    got = (_host(d, c.dtype), _host(p, c.dtype)) if c.split else _host(d, c.dtype)
    return got, _host(r, np.int32), _host(pos, np.uint32), _host(corr, c.dtype)


def _check_decode(c, got, res, pos, corr, what):
    """Results, the whole arrays (padding included), positions[:r], corr[:r] on the sampled rows and
    the untouched extra columns against the oracle; then the result mix on what the GPU gave."""
    np.testing.assert_array_equal(res, c.res, err_msg=f"{what}: results")
    if c.split:
        np.testing.assert_array_equal(got[0], c.exp_data, err_msg=f"{what}: data")
        np.testing.assert_array_equal(got[1], c.exp_par, err_msg=f"{what}: parity")
        rows = G.logical_rows(c, None, got[0], got[1])
    else:
        np.testing.assert_array_equal(got, c.exp, err_msg=f"{what}: rows")
        rows = G.logical_rows(c, got)
    for k in np.nonzero(c.res > 0)[0]:
        np.testing.assert_array_equal(pos[k, :c.res[k]], c.pos[k, :c.res[k]],
                                      err_msg=f"{what}: positions of row {k}")
    for k in c.corr_rows:
        if c.res[k] > 0:
            np.testing.assert_array_equal(corr[k, :c.res[k]], c.corr[k, :c.res[k]],
                                          err_msg=f"{what}: corr of row {k}")
    assert (pos[:, c.nr:] == POS_FILL).all(), f"{what}: positions beyond nroots written"
    assert (corr[:, c.nr:] == c.fill).all(), f"{what}: corr beyond nroots written"
    G.check_result_mix(c, res, rows)
    return rows


# ---- matrix A -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", G.MATRIX_A, ids=A_IDS)
def test_generic_encode(torch, entry):
    _check_encode(torch, _codec(entry[1], "generic"), G.case_a(entry, False))


@pytest.mark.parametrize("entry", G.MATRIX_A, ids=A_IDS)
def test_generic_decode_inline(torch, entry):
    c = G.case_a(entry, False)
    assert c.pitch == c.S + G.A_PITCH_EXTRA
    _check_decode(c, *_decode(torch, _codec(entry[1], "generic"), c), "inline")


@pytest.mark.parametrize("entry", G.MATRIX_A, ids=A_IDS)
def test_generic_decode_split(torch, entry):
    c = G.case_a(entry, True)
    assert c.data.shape[1] == c.L + 5 and c.par.shape[1] == c.nr + 3
    _check_decode(c, *_decode(torch, _codec(entry[1], "generic"), c), "split")


# ---- matrix B -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", G.MATRIX_B, ids=B_IDS)
def test_fallback_encode(torch, entry):
    _, params, L, ncw, seed, _, path = entry
    _check_encode(torch, _codec(params, path), G.make_case(params, L, ncw, seed, G.A_PITCH_EXTRA, False))


@pytest.mark.parametrize("entry", G.MATRIX_B, ids=B_IDS)
def test_fallback_decode_matches_fast_path(torch, entry):
    codec = _codec(entry[1], entry[6])
    slow, fast = G.case_b(entry, False), G.case_b(entry, True)
    assert slow.split or slow.pitch == 300
    assert fast.pitch == fast.S and not fast.split
    got_s, res_s, pos_s, corr_s = _decode(torch, codec, slow)
    rows_s = _check_decode(slow, got_s, res_s, pos_s, corr_s, "fallback")
    got_f, res_f, pos_f, corr_f = _decode(torch, codec, fast)
    rows_f = _check_decode(fast, got_f, res_f, pos_f, corr_f, "fast path")
    np.testing.assert_array_equal(res_s, res_f)
    np.testing.assert_array_equal(rows_s, rows_f)
    for k in np.nonzero(res_s > 0)[0]:
        np.testing.assert_array_equal(pos_s[k, :res_s[k]], pos_f[k, :res_s[k]], err_msg=f"positions of row {k}")
        np.testing.assert_array_equal(corr_s[k, :res_s[k]], corr_f[k, :res_s[k]], err_msg=f"corr of row {k}")

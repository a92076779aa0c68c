"""In-place parity update of interleaved frames (ezrs_update_create / ezrs_update_interleaved).
Every geometry: a flat buffer of random data with the codewords encoded by the oracle, and a second
flat buffer that holds the new contents of the changed symbols with its own pitch, stride, padding
and base offset, random everywhere.  After the call the WHOLE frames buffer must equal the first
buffer with the changed symbols replaced and the parity encoded again by the oracle (gaps, padding
and the base offset untouched), and the newsyms buffer must be byte-identical to before.  All
comparisons are bit-exact."""
import ctypes as C
import errno
import gc

import numpy as np
import pytest

import oracle as O
from interleave_util import deinterleave, frame_view, interleave

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as T
    if not T.cuda.is_available():
        pytest.skip("no GPU")
    return T


def _dev(torch, a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).view(torch.uint16).cuda()
    return torch.from_numpy(a).cuda()


def _host(torch, t):
    if t.dtype == torch.uint16:
        return t.cpu().view(torch.int16).numpy().view(np.uint16)
    return t.cpu().numpy()


def _params(spec):
    kind, n, k = spec
    return O.rs_params(n, k) if kind == "rs" else O.ccsds_params(k, kind == "ccsds")


def _codec(spec, karn=False):
    import ezrs
    kind, n, k = spec
    c = ezrs.Codec.rs(n, k) if kind == "rs" else ezrs.Codec.ccsds(k, dual=kind == "ccsds")
    if karn:
        c.semantics = "karn"
    return c


def _view(torch, dev, geo):
    F, S, D, fp, ss, off = geo
    return torch.as_strided(dev, (F, S, D), (fp, ss, 1), off)


def _expect(oc, buf, geo, L, changed, nv):
    """`buf` with the symbols at `changed` replaced by nv [F, nchanged, D] as given and the parity
    encoded again by the oracle from the values masked to the symbol; a parity symbol's bits above
    the symbol stay."""
    F, _, D = geo[:3]
    dt = oc.dtype
    exp = buf.copy()
    ev = frame_view(exp, *geo)
    rows = deinterleave(ev & dt(oc.nn))
    rows[:, changed] = deinterleave(nv & dt(oc.nn))
    oc.encode_batch(rows, L)
    full = (1 << (8 * dt().itemsize)) - 1
    ev[:, L:, :] = (ev[:, L:, :] & dt(full - oc.nn)) | interleave(rows, F, D)[:, L:, :]
    ev[:, changed, :] = nv
    return exp


def _make(spec, D, ss, L, F, pad, off, changed, newlay=None, high_bits=False):
    """(frames buffer, its geometry, newsyms buffer, its geometry, expectation, oracle codec).
    newlay: (stride, frame pad, base offset) of newsyms; None: the stride of the frames, no pad, no
    offset (aligned wherever the frames' rows are)."""
    oc = O.Codec(*_params(spec))
    nr, dt = oc.nroots, oc.dtype
    S, nchg = L + nr, len(changed)
    fp = S * ss + pad
    rng = np.random.default_rng(D * 1009 + ss * 31 + L + F + 7 * off + nchg)
    full = 1 << (8 * dt().itemsize)
    buf = rng.integers(0, full, off + F * fp + 5).astype(dt)
    geo = (F, S, D, fp, ss, off)
    fv = frame_view(buf, *geo)
    fv[...] &= dt(oc.nn)
    rows = deinterleave(fv)
    oc.encode_batch(rows, L)
    fv[...] = interleave(rows, F, D)
    if high_bits:                                   # old data and old parity carry bits above the symbol
        fv[...] |= rng.integers(0, full, (F, S, D)).astype(dt) & dt(full - 1 - oc.nn)
    nss, npad, noff = newlay or (ss, 0, 0)
    nfp = nchg * nss + npad
    nbuf = rng.integers(0, full, noff + F * nfp + 5).astype(dt)     # random everywhere, bits above the symbol too
    ngeo = (F, nchg, D, nfp, nss, noff)
    exp = _expect(oc, buf, geo, L, changed, frame_view(nbuf, *ngeo))
    return buf, geo, nbuf, ngeo, exp, oc


def _run(torch, spec, D, ss, L, F, pad, off, changed, newlay=None, karn=False, high_bits=False):
    """Update one geometry and assert both buffers; returns the updated host buffer."""
    c = _codec(spec, karn)
    buf, geo, nbuf, ngeo, exp, _ = _make(spec, D, ss, L, F, pad, off, changed, newlay, high_bits)
    plan = c.update_plan(L, changed)
    assert plan.nchanged == len(changed) and plan.changed == list(changed)
    dev, ndev = _dev(torch, buf), _dev(torch, nbuf)
    plan.apply(_view(torch, dev, geo), _view(torch, ndev, ngeo))
    got = _host(torch, dev)
    np.testing.assert_array_equal(got, exp, err_msg="parity, new data, or an element that must not be written")
    np.testing.assert_array_equal(_host(torch, ndev), nbuf, err_msg="newsyms was written")
    return got


RS251, RS252, RS223, RS1007 = ("rs", 255, 251), ("rs", 255, 252), ("rs", 255, 223), ("rs", 1023, 1007)
CASES = [
    # (codec, depth, sym_stride, len, nframes, frame pad, base offset, changed, newsyms layout)
    (RS251, 777, 800, 10, 2, 13, 0, [3], (800, 0, 0)),        # element path (odd frame pitch)
    (RS251, 777, 800, 10, 2, 13, 0, [3], (800, 0, 1)),
    (RS251, 777, 800, 10, 2, 13, 0, [3], (800, 0, 3)),
    # frames aligned to 16 bytes: the path is chosen by the alignment of newsyms alone
    (RS251, 777, 800, 10, 2, 16, 0, [3], (784, 0, 0)),        # 16-byte path + ragged end
    (RS251, 777, 800, 10, 2, 16, 0, [3], (784, 0, 4)),        # dword path + ragged end
    (RS251, 777, 800, 10, 2, 16, 0, [3], (784, 0, 1)),        # element path
    (RS251, 777, 800, 10, 2, 16, 0, [3], (780, 0, 0)),        # dword path by the stride of newsyms
    (RS251, 777, 800, 10, 2, 16, 0, [3], (784, 4, 0)),        # dword path by the pitch of newsyms
    (RS251, 777, 800, 10, 2, 13, 1, [0, 9], (784, 0, 0)),     # misaligned frames, aligned newsyms
    (RS251, 1040, 1056, 10, 3, 32, 16, [0, 3, 5, 7, 9], (1056, 16, 0)),   # 16-byte path, a group of four + a fifth
    (RS252, 1, 1, 6, 1, 0, 0, [2], None),                     # 3 rows in a block of 4; lanes outnumber codewords
    (RS252, 3, 3, 6, 1, 0, 0, [2], None),
    (RS252, 5, 5, 6, 1, 0, 0, [2], None),
    (RS252, 17, 17, 6, 1, 0, 0, [2], None),
    (RS223, 300, 304, 223, 1, 0, 0, [0], None),               # 32 rows: two row blocks, old and new read per block
    (RS223, 300, 304, 223, 1, 0, 0, [5, 222], None),          # ... two positions, one by one in each block
    (RS223, 48, 48, 223, 1, 0, 0, list(range(0, 223, 37)), None),   # seven, two blocks: two apply8x2 pairs + three
    (("rs", 255, 215), 40, 48, 30, 2, 0, 0, [1, 29], None),   # 40 rows: a padded last block
    (("ccsds", 255, 223), 260, 260, 223, 1, 0, 0, [5, 100], None),  # dual basis
    (RS1007, 130, 136, 100, 2, 3, 1, [0, 50, 99], None),      # uint16_t element path
    (RS1007, 75, 80, 100, 2, 0, 0, [0, 50, 99], None),        # uint16_t 16-byte path + ragged end
    (RS1007, 70, 70, 100, 1, 0, 0, [0, 50, 99], None),        # uint16_t dword path
    (("rs", 65535, 65503), 24, 24, 40, 1, 0, 0, [7], None),   # RB = 32, m = 16, the fix constant
    # every count of deltas kept in registers, and the forms that read the old parity late
    (RS251, 1040, 1056, 10, 3, 32, 16, [9, 0, 4, 2], (1056, 16, 0)),      # four kept, 16-byte path
    (("rs", 255, 243), 100, 112, 20, 1, 0, 0, [4, 11], None), # 12 rows in one block of 16, two kept
    (RS1007, 72, 72, 100, 1, 0, 0, [3, 98], None),            # uint16_t 16-byte path, two kept
    (("rs", 65535, 65503), 24, 24, 40, 1, 0, 0, [7, 8, 30], None),        # RB = 32: a group of two + one
]


def _id(c):
    lay = "" if c[8] is None else "-n" + "_".join(map(str, c[8]))
    return f"{c[0][0]}{c[0][1]}_{c[0][2]}-d{c[1]}-s{c[2]}-l{c[3]}-f{c[4]}-p{c[5]}-o{c[6]}-c{len(c[7])}x{c[7][0]}{lay}"


@pytest.mark.parametrize("spec,D,ss,L,F,pad,off,changed,newlay", CASES, ids=[_id(c) for c in CASES])
def test_update_vs_oracle(torch, spec, D, ss, L, F, pad, off, changed, newlay):
    _run(torch, spec, D, ss, L, F, pad, off, changed, newlay)


def test_masked_symbols(torch):
    """RS(31,27) in uint8_t with random bits above bit 4 in the old data, the new data and the old
    parity: parity low bits as from the oracle on the masked values, parity high bits unchanged,
    data stored as given (_expect)."""
    _run(torch, ("rs", 31, 27), 100, 100, 20, 2, 7, 0, [1, 2], high_bits=True)


SMALL = (RS251, 1040, 1056, 10, 3, 32, 16)


def test_old_parity_is_not_recomputed(torch):
    """A parity that was wrong by e before the call is wrong by the same e afterwards."""
    changed = [0, 3, 5]
    buf, geo, nbuf, ngeo, exp, _ = _make(*SMALL, changed)
    L = SMALL[3]
    pat = np.zeros_like(buf)
    pv = frame_view(pat, *geo)
    pv[0, L + 1, 7] = 0x5A
    pv[1, L + 3, 1039] = 0x01
    pv[2, L, ::3] = 0xC3
    plan = _codec(SMALL[0]).update_plan(L, changed)
    dev, ndev = _dev(torch, buf ^ pat), _dev(torch, nbuf)
    plan.apply(_view(torch, dev, geo), _view(torch, ndev, ngeo))
    np.testing.assert_array_equal(_host(torch, dev) ^ exp, pat)


def test_identity(torch):
    """newsyms equal to the current data: a byte-identical buffer."""
    changed = [9, 2]
    buf, geo, _, _, _, _ = _make(*SMALL, changed)
    plan = _codec(SMALL[0]).update_plan(SMALL[3], changed)
    dev = _dev(torch, buf)
    fv = _view(torch, dev, geo)
    plan.apply(fv, fv[:, changed, :].contiguous())
    np.testing.assert_array_equal(_host(torch, dev), buf)


def test_chain_verify_and_plans_outlive_codec(torch):
    """Two plans back to back on a non-default stream after their codec is gone; the result verifies
    (an nlost == 0 reconstruction plan returns 0 everywhere) and equals the oracle's."""
    spec, D, ss, L, F, pad, off = SMALL
    a, b = [0, 3], [5]
    c = _codec(spec)
    pa, pb = c.update_plan(L, a), c.update_plan(L, b)
    del c
    gc.collect()
    buf, geo, nbuf_a, ngeo_a, exp_a, oc = _make(spec, D, ss, L, F, pad, off, a)
    rng = np.random.default_rng(5)
    nb = rng.integers(0, 256, (F, 1, D)).astype(np.uint8)
    exp = _expect(oc, exp_a, geo, L, b, nb)
    dev, nda, ndb = _dev(torch, buf), _dev(torch, nbuf_a), _dev(torch, nb)
    fv = _view(torch, dev, geo)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        pa.apply(fv, _view(torch, nda, ngeo_a), stream=st)
        pb.apply(fv, ndb, stream=st)
    st.synchronize()
    np.testing.assert_array_equal(_host(torch, dev), exp)
    res = torch.full((F * D,), 77, dtype=torch.int32, device="cuda")
    _codec(spec).recon_plan(L, []).reconstruct(fv, result=res)
    assert (res.cpu().numpy() == 0).all()
    np.testing.assert_array_equal(_host(torch, dev), exp)


def test_agrees_with_encode_interleaved(torch):
    """encode_interleaved on a copy of the updated data writes the parity the update left."""
    changed = [1, 8]
    got = _run(torch, *SMALL, changed, (1056, 16, 0))
    _, geo, _, _, _, _ = _make(*SMALL, changed, (1056, 16, 0))
    L = SMALL[3]
    again = got.copy()
    frame_view(again, *geo)[:, L:, :] = 0
    dev = _dev(torch, again)
    _codec(SMALL[0]).encode_interleaved(_view(torch, dev, geo))
    np.testing.assert_array_equal(_host(torch, dev), got)


def test_karn_semantics_same_frame(torch):
    """Positions are relative to the first data symbol under both semantics: identical output."""
    a = _run(torch, RS223, 64, 64, 14, 2, 0, 0, [13, 0])
    b = _run(torch, RS223, 64, 64, 14, 2, 0, 0, [13, 0], karn=True)
    np.testing.assert_array_equal(a, b)


def test_argument_checks(torch):
    import ezrs
    L_ = ezrs.lib()
    EINVAL, ENOTSUP = -errno.EINVAL, -errno.ENOTSUP
    c = ezrs.Codec.rs(255, 251)
    sp = ezrs._stream_ptr(None)
    L, nr, D, F = 10, 4, 8, 3
    S = L + nr

    def create(changed, length=L, codec=c, out=True, null=False, n=None):
        h = C.c_void_p()
        arr = (C.c_uint32 * max(len(changed), 1))(*changed)
        rc = L_.ezrs_update_create(C.byref(h) if out else None, codec._h if codec else None, length,
                                   None if null else arr, len(changed) if n is None else n)
        if rc == 0:
            assert L_.ezrs_update_destroy(h) == 0
        else:
            assert not h.value
        return rc

    assert create([0, 3]) == 0
    assert create([0], codec=None) == EINVAL and create([0], out=False) == EINVAL
    assert create([0], null=True) == EINVAL
    assert create([0], length=0) == EINVAL and create([0], length=1) == 0
    assert create([0], length=252) == EINVAL and create([0], length=251) == 0
    assert create([0], n=0) == EINVAL and create([0], n=1) == 0
    assert create([0, 1, 2], length=3) == 0
    assert create([0, 1, 2, 1], length=3) == EINVAL             # nchanged > len
    assert create([L]) == EINVAL and create([L - 1]) == 0       # position >= len
    assert create([3, 5, 3]) == EINVAL and create([3, 5, 4]) == 0   # given twice
    assert L_.ezrs_update_destroy(None) == 0
    # the device table of a GF(2^16) plan with 32 parity symbols: per changed position 16 bits x 32
    # rows of dwords and its position, then the 32 parity positions and the 32 row constants
    wide = ezrs.Codec.rs(65535, 65503)
    nmax = ((64 << 20) // 4 - 64) // (16 * 32 + 1)
    assert 4 * (nmax * (16 * 32 + 1) + 64) <= 64 << 20 < 4 * ((nmax + 1) * (16 * 32 + 1) + 64)
    assert create(list(range(nmax + 1)), length=nmax + 1, codec=wide) == ENOTSUP
    assert create(list(range(nmax)), length=nmax + 1, codec=wide) == 0

    nchg = 2
    plan = c.update_plan(L, [0, 3])
    buf = torch.zeros(F * S * D, dtype=torch.uint8, device="cuda")
    new = torch.full((F * nchg * D,), 9, dtype=torch.uint8, device="cuda")
    fr, nw = C.c_void_p(buf.data_ptr()), C.c_void_p(new.data_ptr())

    def upd(h=plan._h, fr=fr, fp=S * D, ss=D, D=D, F=F, nw=nw, nfp=nchg * D, nss=D):
        return L_.ezrs_update_interleaved(h, fr, fp, ss, D, F, nw, nfp, nss, sp)

    before, nbefore = buf.clone(), new.clone()
    assert upd(F=0) == 0 and upd(F=0, D=0, fr=None, nw=None) == 0   # nothing to do, nothing touched
    torch.cuda.synchronize()
    assert torch.equal(buf, before) and torch.equal(new, nbefore)
    assert upd() == 0
    assert upd(h=None) == EINVAL
    assert upd(fr=None) == EINVAL
    assert upd(nw=None) == EINVAL
    assert upd(D=0) == EINVAL
    assert upd(ss=D - 1) == EINVAL and upd(ss=D) == 0
    assert upd(nss=D - 1) == EINVAL and upd(nss=D) == 0
    assert upd(fp=(S - 1) * D + D - 1) == EINVAL and upd(fp=(S - 1) * D + D) == 0
    assert upd(nfp=(nchg - 1) * D + D - 1) == EINVAL and upd(nfp=(nchg - 1) * D + D) == 0
    assert upd(fp=0, nfp=0, F=1) == 0                           # one frame: the pitches are not used
    big = (2 ** (8 * C.sizeof(C.c_size_t)) - 1) // 2 + 1        # depth * 2 frames overflows size_t
    assert upd(D=big, ss=big, nss=big, fp=2 ** 62, nfp=2 ** 62, F=2) == EINVAL
    torch.cuda.synchronize()

    fv, nv = buf.view(F, S, D), new.view(F, nchg, D)
    plan.apply(fv, nv)
    with pytest.raises(ezrs.EzrsError):
        plan.apply(fv.cpu(), nv)
    with pytest.raises(ezrs.EzrsError):
        plan.apply(fv, nv.cpu())
    with pytest.raises(ezrs.EzrsError):
        plan.apply(buf.view(F * S, D), nv)                      # rank
    with pytest.raises(ezrs.EzrsError):
        plan.apply(buf.view(-1)[:F * (S - 1) * D].view(F, S - 1, D), nv)    # another length
    with pytest.raises(ezrs.EzrsError):
        plan.apply(fv, new.view(-1)[:F * D].view(F, 1, D))      # one row of newsyms for two positions
    with pytest.raises(ezrs.EzrsError):
        plan.apply(fv, new.view(-1)[:F * nchg * (D - 1)].view(F, nchg, D - 1))  # another depth
    with pytest.raises(ezrs.EzrsError):
        plan.apply(fv, new.view(-1)[:(F - 1) * nchg * D].view(F - 1, nchg, D))  # another frame count
    with pytest.raises(ezrs.EzrsError):
        plan.apply(fv, torch.zeros((F, nchg, D), dtype=torch.int16, device="cuda"))
    with pytest.raises(ezrs.EzrsError):
        c.update_plan(L, [1, 1])
    torch.cuda.synchronize()

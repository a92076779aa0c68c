"""Interleaved frames (ezrs_encode_interleaved / ezrs_decode_interleaved): CCSDS depth-I codeblocks
and striped shards.  Symbol s of codeword j of frame f is element f*frame_pitch + s*sym_stride + j.
Every case is checked bit-exactly against the oracle run on the numpy-de-interleaved rows: the
whole buffer (symbols and every non-symbol element, pre-filled with random data), the results, the
positions and, for a subset of codewords, the correction patterns."""
import ctypes as C
import errno

import numpy as np
import pytest

import oracle as O
from interleave_util import deinterleave, frame_view, interleave, load_fixture

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
    if a.dtype == np.uint32:
        return torch.from_numpy(a.view(np.int32)).cuda()
    return torch.from_numpy(a).cuda()


def _host(torch, t):
    if t.dtype == torch.uint16:
        return t.cpu().view(torch.int16).numpy().view(np.uint16)
    return t.cpu().numpy()


def _codecs(spec, karn=False):
    import ezrs
    kind, n, k = spec
    if kind == "rs":
        c, p = ezrs.Codec.rs(n, k), O.rs_params(n, k)
    else:
        c, p = ezrs.Codec.ccsds(k, dual=kind == "ccsds"), O.ccsds_params(k, kind == "ccsds")
    if karn:
        c.semantics = "karn"
    return c, O.Codec(*p, karn=karn)


def _frames(torch, dev, F, S, D, fp, ss, off):
    return torch.as_strided(dev, (F, S, D), (fp, ss, 1), off)


def _corrupt(rng, rows, nr, maxval, with_eras, pad=0):
    """0..nr/2 symbol errors per codeword and one overwhelmed codeword (test_shards_vs_oracle's
    pattern); with_eras: every fourth codeword also carries 1..4 erasures (2e + f <= nr), one of
    them on an uncorrupted symbol, some repeated.  pad: Karn semantics, positions in the NN frame."""
    ncw, S = rows.shape
    eras = np.zeros((ncw, nr), np.uint32)
    neras = np.zeros(ncw, np.uint32)
    nerr = rng.integers(0, nr // 2 + 1, ncw)
    over = int(rng.integers(0, ncw))
    for k in range(ncw):
        e, f = int(nerr[k]), 0
        if k == over:
            e = nr // 2 + 3
        elif with_eras and k % 4 == 1:
            f = int(rng.integers(1, min(4, nr) + 1))
            e = min(e, (nr - f) // 2)
        e = min(e, S - f)
        locs = rng.choice(S, e + f, replace=False)
        vals = rng.integers(1, maxval, e + f).astype(rows.dtype)
        if f > 1:
            vals[e] = 0
        rows[k, locs] ^= vals
        ep = locs[e:].astype(np.uint32) + pad
        if f > 2 and k % 8 == 1:
            ep[1] = ep[0]
        eras[k, :f] = ep
        neras[k] = f
    return eras, neras


def _run(torch, spec, D, ss, L, F, pad, off=0, with_eras=False, karn=False, launch_rows=0, ws=False):
    """Encode and decode one geometry on the device and assert everything against the oracle;
    returns the device outputs (for comparisons between runs)."""
    import ezrs
    c, oc = _codecs(spec, karn)
    if launch_rows:
        c.set_launch_rows(launch_rows)
    nr, dt = c.nroots, c.dtype
    S = L + nr
    maxval = c.nn + 1
    fp = S * ss + pad
    ncw = F * D
    rng = np.random.default_rng(D * 1009 + ss * 31 + L + F)
    buf = rng.integers(0, 1 << (8 * dt().itemsize), off + F * fp + 5).astype(dt)
    frame_view(buf, F, S, D, fp, ss, off)[...] &= c.nn          # symbols inside the field
    L_ = ezrs.lib()
    sp = ezrs._stream_ptr(None)
    wsbuf = None
    if ws:
        need = c.interleaved_workspace_bytes(L, D, F)
        assert need > 0
        wsbuf = torch.empty(need, dtype=torch.uint8, device="cuda")

    # encode: only the parity symbols change
    dev = _dev(torch, buf)
    fv = _frames(torch, dev, F, S, D, fp, ss, off)
    if ws:
        args = (c._h, C.c_void_p(fv.data_ptr()), fp, ss, D, L, F, C.c_void_p(wsbuf.data_ptr()))
        assert L_.ezrs_encode_interleaved_ws(*args, need - 1, sp) == -errno.EINVAL
        assert L_.ezrs_encode_interleaved_ws(*args, need, sp) == 0
    else:
        c.encode_interleaved(fv)
    exp = buf.copy()
    ev = frame_view(exp, F, S, D, fp, ss, off)
    rows = deinterleave(ev)
    oc.encode_batch(rows, L)
    ev[...] = interleave(rows, F, D)
    enc = _host(torch, dev)
    np.testing.assert_array_equal(enc, exp, err_msg="encode (parity, or an element that is not parity)")
    assert np.array_equal(deinterleave(frame_view(buf, F, S, D, fp, ss, off))[:, :L], rows[:, :L])

    # decode
    brows = rows.copy()
    eras, neras = _corrupt(rng, brows, nr, maxval, with_eras, pad=c.load - L if karn else 0)
    bad = exp.copy()
    frame_view(bad, F, S, D, fp, ss, off)[...] = interleave(brows, F, D)
    dev = _dev(torch, bad)
    fv = _frames(torch, dev, F, S, D, fp, ss, off)
    pos = torch.zeros((ncw, nr), dtype=torch.int32, device="cuda")
    corr = torch.zeros((ncw, nr), dtype=c.torch_dtype, device="cuda")
    de, dn = (_dev(torch, eras), _dev(torch, neras)) if with_eras else (None, None)
    if ws:
        res = torch.empty(ncw, dtype=torch.int32, device="cuda")
        args = (c._h, C.c_void_p(fv.data_ptr()), fp, ss, D, L, F,
                C.c_void_p(de.data_ptr()) if with_eras else None, nr,
                C.c_void_p(dn.data_ptr()) if with_eras else None, C.c_void_p(res.data_ptr()),
                C.c_void_p(pos.data_ptr()), nr, C.c_void_p(corr.data_ptr()), nr,
                C.c_void_p(wsbuf.data_ptr()))
        assert L_.ezrs_decode_interleaved_ws(*args, need - 1, sp) == -errno.EINVAL
        assert L_.ezrs_decode_interleaved_ws(*args, need, sp) == 0
    else:
        res = c.decode_interleaved(fv, eras=de, neras=dn, positions=pos, corr=corr)
    orow = brows.copy()
    opos = np.zeros((ncw, nr), np.uint32)
    ores = oc.decode_batch(orow, L, None, eras if with_eras else None, neras if with_eras else None, opos)
    expd = bad.copy()
    frame_view(expd, F, S, D, fp, ss, off)[...] = interleave(orow, F, D)
    res = res.cpu().numpy()
    dec = _host(torch, dev)
    gpos = pos.cpu().numpy().view(np.uint32)
    gcorr = _host(torch, corr)
    np.testing.assert_array_equal(res, ores, err_msg="decode results")
    assert (ores > 0).any()
    np.testing.assert_array_equal(dec, expd, err_msg="decode (symbols, or an element that is no symbol)")
    for k in np.nonzero(ores > 0)[0]:
        np.testing.assert_array_equal(gpos[k, :ores[k]], opos[k, :ores[k]], err_msg=f"positions cw {k}")
    # correction patterns of a subset: the first and last corrected codewords and eight in between
    sub = np.nonzero(ores > 0)[0]
    sub = sub[np.unique(np.linspace(0, len(sub) - 1, 10).astype(int))]
    for k in sub:
        d, p = brows[k, :L].copy(), brows[k, L:].copy()
        cc = np.zeros(nr, dt)
        r, _ = oc.decode(d, p, eras[k, :neras[k]].tolist(), cc)
        assert r == ores[k]
        np.testing.assert_array_equal(gcorr[k, :r], cc[:r], err_msg=f"corr cw {k}")
    return enc, res, dec, gpos


CASES = [
    # (codec, depth, sym_stride, len, nframes, pad, base offset, erasures)
    (("rs", 255, 223), 1, 1, 223, 300, 0, 0, False),          # degenerate = row form
    (("rs", 255, 223), 5, 5, 223, 103, 3, 1, True),           # 515 cw: > 2 tiles, frames straddle tiles
    (("rs", 255, 223), 8, 8, 100, 70, 0, 0, False),           # fast path, shortened
    (("rs", 255, 223), 4, 4, 223, 129, 4, 0, True),           # fast path, last tile partial
    (("ccsds", 255, 223), 5, 5, 223, 60, 0, 0, True),         # dual basis: bit-sliced family
    (("ccsds_conv", 255, 239), 2, 2, 239, 200, 1, 0, False),
    (("rs", 255, 251), 777, 800, 251, 1, 0, 0, False),        # striped shards, gaps of 23
    (("rs", 255, 239), 1027, 1027, 239, 2, 5, 3, False),      # depth > tile, odd, odd base
    (("rs", 31, 19), 3, 3, 12, 500, 0, 0, False),             # generic u8 (masked), shortened
    (("rs", 1023, 1001), 5, 6, 1001, 40, 0, 0, True),         # u16
    (("rs", 65535, 65503), 3, 3, 400, 20, 2, 0, False),       # u16, rows longer than a symbol chunk
]


@pytest.mark.parametrize("spec,D,ss,L,F,pad,off,we", CASES,
                         ids=[f"{c[0][0]}{c[0][1]}_{c[0][2]}-d{c[1]}-s{c[2]}-l{c[3]}-f{c[4]}" for c in CASES])
def test_interleaved_vs_oracle(torch, spec, D, ss, L, F, pad, off, we):
    _run(torch, spec, D, ss, L, F, pad, off, with_eras=we)


def test_fast_path_needs_alignment(torch):
    """Depth 8 frames at an odd base and depth 4 with an odd frame pitch: the dword path must not
    be taken (same results through the general path)."""
    _run(torch, ("rs", 255, 223), 8, 8, 50, 40, 0, off=1)
    _run(torch, ("rs", 255, 223), 4, 4, 60, 70, 3)
    _run(torch, ("rs", 255, 223), 260, 264, 20, 3, 8)         # fast path, depth > tile, gaps


def test_chunk_boundaries(torch):
    """The 515-codeword case staged 256 codewords per pass (set_launch_rows): identical outputs."""
    a = _run(torch, ("rs", 255, 223), 5, 5, 223, 103, 3, 1, with_eras=True)
    b = _run(torch, ("rs", 255, 223), 5, 5, 223, 103, 3, 1, with_eras=True, launch_rows=256)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    import ezrs
    c = ezrs.Codec.rs(255, 223)
    whole = c.interleaved_workspace_bytes(223, 5, 103)
    c.set_launch_rows(256)
    assert 0 < c.interleaved_workspace_bytes(223, 5, 103) < whole


def test_ws_form(torch):
    """Caller-owned workspace of exactly ezrs_interleaved_workspace_bytes; one byte less: -EINVAL."""
    _run(torch, ("rs", 255, 223), 4, 4, 223, 129, 4, with_eras=True, ws=True)
    _run(torch, ("ccsds", 255, 223), 5, 5, 223, 60, 0, ws=True)


def test_karn_semantics(torch):
    """Shortened RS(255,223) under EZRS_SEM_KARN: erasures and positions in the full NN frame."""
    _run(torch, ("rs", 255, 223), 5, 5, 150, 60, 2, with_eras=True, karn=True)


def test_lost_shard(torch):
    """A stripe of 10 data + 16 parity shards (RS(255,239) shortened), byte j of every shard forming
    codeword j; shard 3 is lost (zeroed): the same erasure in every codeword."""
    import ezrs
    c, oc = _codecs(("rs", 255, 239))
    K, nr, slen, pitch = 10, 16, 1000, 1024
    rng = np.random.default_rng(3)
    host = rng.integers(0, 256, (K + nr, pitch)).astype(np.uint8)
    shards = torch.from_numpy(host.copy()).cuda()
    frames = shards[None][:, :, :slen]
    c.encode_interleaved(frames)
    rows = deinterleave(host[None, :, :slen])
    oc.encode_batch(rows, K)
    exp = host.copy()
    exp[:, :slen] = interleave(rows, 1, slen)[0]
    np.testing.assert_array_equal(shards.cpu().numpy(), exp)
    shards[3, :slen] = 0
    eras = torch.full((slen, 1), 3, dtype=torch.int32, device="cuda")
    neras = torch.ones(slen, dtype=torch.int32, device="cuda")
    pos = torch.zeros((slen, nr), dtype=torch.int32, device="cuda")
    res = c.decode_interleaved(frames, eras=eras, neras=neras, positions=pos)
    lost = exp.copy()
    lost[3, :slen] = 0
    orow = deinterleave(lost[None, :, :slen])
    opos = np.zeros((slen, nr), np.uint32)
    ores = oc.decode_batch(orow, K, None, np.full((slen, 1), 3, np.uint32), np.ones(slen, np.uint32), opos)
    res = res.cpu().numpy()
    np.testing.assert_array_equal(res, ores)
    # a codeword whose lost byte was zero anyway is valid as received: 0; every other one: 1
    assert ((res == 1) == (exp[3, :slen] != 0)).all() and (res[res != 1] == 0).all()
    assert (pos[:, 0].cpu().numpy()[res == 1] == 3).all()
    np.testing.assert_array_equal(shards.cpu().numpy(), exp)


def test_fixture_on_device(torch):
    """The reference-pinned RS_CCSDS(255,223) I = 5 / I = 4 frames (tests/golden)."""
    import ezrs
    c = ezrs.Codec.ccsds(223, dual=True)
    for case in load_fixture():
        I = int(case["depth"][0])
        F = case["enc"].shape[0]
        blank = case["enc"].copy()
        blank[:, 223:, :] = 0
        buf = torch.from_numpy(blank.reshape(-1)).cuda()
        c.encode_interleaved(buf.view(F, 255, I))
        np.testing.assert_array_equal(buf.cpu().numpy().reshape(F, 255, I), case["enc"])
        buf = torch.from_numpy(case["bad"].reshape(-1).copy()).cuda()
        pos = torch.zeros((F * I, 32), dtype=torch.int32, device="cuda")
        res = c.decode_interleaved(buf.view(F, 255, I), eras=_dev(torch, case["eras"]),
                                   neras=_dev(torch, case["neras"]), positions=pos).cpu().numpy()
        np.testing.assert_array_equal(res, case["result"])
        np.testing.assert_array_equal(buf.cpu().numpy().reshape(F, 255, I), case["out"])
        gp = pos.cpu().numpy().view(np.uint32)
        for k, r in enumerate(res):
            if r > 0:
                np.testing.assert_array_equal(gp[k, :r], case["positions"][k, :r])


def test_argument_checks(torch):
    """Every -EINVAL rule of the interleaved calls, and nframes == 0."""
    import ezrs
    L_ = ezrs.lib()
    EINVAL = -errno.EINVAL
    c = ezrs.Codec.rs(255, 223)
    h, sp = c._h, ezrs._stream_ptr(None)
    D, L, F, nr = 4, 223, 3, 32
    S = L + nr
    buf = torch.zeros(F * S * D, dtype=torch.uint8, device="cuda")
    res = torch.full((F * D,), 77, dtype=torch.int32, device="cuda")
    aux = torch.zeros((F * D, nr), dtype=torch.int32, device="cuda")
    fr, rs, ax = (C.c_void_p(t.data_ptr()) for t in (buf, res, aux))
    fp = S * D

    def enc(h=h, fr=fr, fp=fp, ss=D, D=D, L=L, F=F):
        return L_.ezrs_encode_interleaved(h, fr, fp, ss, D, L, F, sp)

    def dec(h=h, fr=fr, fp=fp, ss=D, D=D, L=L, F=F, eras=None, es=0, neras=None, rs=rs, pos=None,
            ps=0, corr=None, cs=0):
        return L_.ezrs_decode_interleaved(h, fr, fp, ss, D, L, F, eras, es, neras, rs, pos, ps, corr,
                                          cs, sp)

    assert enc() == 0 and dec() == 0
    for f in (enc, dec):
        assert f(h=None) == EINVAL
        assert f(fr=None) == EINVAL
        assert f(D=0) == EINVAL
        assert f(ss=D - 1) == EINVAL
        assert f(L=0) == EINVAL and f(L=224) == EINVAL
        assert f(fp=(S - 1) * D + D - 1) == EINVAL
        assert f(fp=(S - 1) * D + D) == 0
        assert f(fp=0, F=1) == 0                            # one frame: the pitch is not used
        assert f(F=0) == 0 and f(F=0, D=0, fr=None) == 0    # nothing to do
    assert dec(rs=None) == EINVAL
    assert dec(neras=ax) == EINVAL                          # counts without positions
    assert dec(eras=ax, es=0, neras=ax) == EINVAL
    assert dec(eras=ax, es=nr, neras=ax) == 0
    assert dec(pos=ax, ps=nr - 1) == EINVAL and dec(pos=ax, ps=nr) == 0
    small = torch.zeros((F * D, nr), dtype=torch.uint8, device="cuda")
    cp = C.c_void_p(small.data_ptr())
    assert dec(corr=cp, cs=nr - 1) == EINVAL and dec(corr=cp, cs=nr) == 0
    assert dec(F=1, D=1, pos=ax, ps=0, corr=cp, cs=0, eras=ax, es=0, neras=ax) == 0   # one codeword
    # the _ws forms: null or short workspace
    need = c.interleaved_workspace_bytes(L, D, F)
    assert need == L_.ezrs_interleaved_workspace_bytes(h, L, D, F) > 0
    assert L_.ezrs_interleaved_workspace_bytes(None, L, D, F) == 0
    assert L_.ezrs_encode_interleaved_ws(h, fr, fp, D, D, L, F, None, need, sp) == EINVAL
    assert L_.ezrs_encode_interleaved_ws(h, fr, fp, D, D, L, F, None, 0, sp) == EINVAL
    assert L_.ezrs_encode_interleaved_ws(h, fr, fp, D, D, L, 0, None, 0, sp) == 0
    assert L_.ezrs_decode_interleaved_ws(h, fr, fp, D, D, L, 0, None, 0, None, None, None, 0, None, 0,
                                         None, 0, sp) == 0
    torch.cuda.synchronize()
    # the Python mirror validates the tensor
    with pytest.raises(ezrs.EzrsError):
        c.encode_interleaved(buf.view(F * S, D))                       # not 3-D
    with pytest.raises(ezrs.EzrsError):
        c.encode_interleaved(buf.view(F, S, D).cpu())                  # not on the device
    with pytest.raises(ezrs.EzrsError):
        c.encode_interleaved(buf.view(F, S, D).to(torch.int32))        # element size
    with pytest.raises(ezrs.EzrsError):
        c.encode_interleaved(buf.view(F, D, S).transpose(1, 2))        # last dimension strided
    with pytest.raises(ezrs.EzrsError):
        c.encode_interleaved(buf.view(-1)[:F * nr * D].view(F, nr, D))  # no data symbol

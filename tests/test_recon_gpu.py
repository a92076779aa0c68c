"""Shared-erasure reconstruction of interleaved frames (ezrs_recon_create /
ezrs_reconstruct_interleaved).  Every geometry: a flat buffer of random data, the codewords encoded
by the oracle, the lost symbols overwritten with garbage; after reconstruct the WHOLE buffer must
equal the oracle-encoded one (gaps, padding and the base offset untouched).  Then one survivor
symbol is flipped in every third codeword: result must be -1 exactly there and nlost elsewhere."""
import ctypes as C
import errno

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


def _codecs(spec, karn=False):
    import ezrs
    kind, n, k = spec
    c = ezrs.Codec.rs(n, k) if kind == "rs" else ezrs.Codec.ccsds(k, dual=kind == "ccsds")
    if karn:
        c.semantics = "karn"
    return c, O.Codec(*_params(spec))


def _frames(torch, dev, F, S, D, fp, ss, off):
    return torch.as_strided(dev, (F, S, D), (fp, ss, 1), off)


def _make(spec, D, ss, L, F, pad, off, lost, high_bits=False):
    """(encoded flat buffer, the same with garbage in the lost symbols, geometry)."""
    oc = O.Codec(*_params(spec))
    nr, dt = oc.nroots, oc.dtype
    S = L + nr
    fp = S * ss + pad
    rng = np.random.default_rng(D * 1009 + ss * 31 + L + F + 7 * off + len(lost))
    full = 1 << (8 * dt().itemsize)
    buf = rng.integers(0, full, off + F * fp + 5).astype(dt)
    fv = frame_view(buf, F, S, D, fp, ss, off)
    fv[...] &= oc.nn
    rows = deinterleave(fv)
    oc.encode_batch(rows, L)
    fv[...] = interleave(rows, F, D)
    if high_bits:                                   # survivors carry bits above the symbol
        hi = rng.integers(0, full, (F, S, D)).astype(dt) & dt(full - 1 - oc.nn)
        hi[:, lost, :] = 0                          # rebuilt symbols come back without them
        fv[...] |= hi
    exp = buf.copy()
    frame_view(buf, F, S, D, fp, ss, off)[:, lost, :] = rng.integers(0, full, (F, len(lost), D)).astype(dt)
    return exp, buf, (F, S, D, fp, ss, off), rng, oc


def _run(torch, spec, D, ss, L, F, pad, off, lost, karn=False, high_bits=False, use_result=True):
    """Reconstruct one geometry and assert buffer and results; returns the rebuilt host buffer."""
    c, _ = _codecs(spec, karn)
    exp, gone, geo, rng, oc = _make(spec, D, ss, L, F, pad, off, lost, high_bits)
    Fn, S, _, fp, _, _ = geo
    nlost, ncw = len(lost), F * D
    plan = c.recon_plan(L, lost)
    assert plan.nlost == nlost and plan.lost == list(lost)
    assert plan.survivors == [p for p in range(S) if p not in set(lost)]

    dev = _dev(torch, gone)
    res = torch.full((ncw,), 77, dtype=torch.int32, device="cuda") if use_result else None
    plan.reconstruct(_frames(torch, dev, *geo), result=res)
    got = _host(torch, dev)
    np.testing.assert_array_equal(got, exp, err_msg="rebuilt symbols, or an element that is not lost")
    if use_result:
        np.testing.assert_array_equal(res.cpu().numpy(), np.full(ncw, nlost), err_msg="clean results")

    # one survivor symbol flipped in every third codeword
    if use_result:
        bad = gone.copy()
        bv = frame_view(bad, *geo[:3], geo[3], geo[4], geo[5])
        hit = np.arange(ncw) % 3 == 1
        surv = np.array(plan.survivors)
        for k in np.nonzero(hit)[0]:
            f, j = divmod(int(k), D)
            bv[f, surv[int(rng.integers(0, len(surv)))], j] ^= int(rng.integers(1, oc.nn + 1))
        before = bad.copy()
        dev = _dev(torch, bad)
        res.fill_(77)
        plan.reconstruct(_frames(torch, dev, *geo), result=res)
        r = res.cpu().numpy()
        if nlost < c.nroots:
            np.testing.assert_array_equal(r, np.where(hit, -1, nlost), err_msg="results with wrong survivors")
        else:
            np.testing.assert_array_equal(r, np.full(ncw, nlost))      # nothing left to check with
        after = _host(torch, dev)
        keep = np.ones(after.shape, bool)
        frame_view(keep, *geo[:3], geo[3], geo[4], geo[5])[:, lost, :] = False
        np.testing.assert_array_equal(after[keep], before[keep], err_msg="an element that is not lost")
        # the codewords with intact survivors are rebuilt all the same
        av, ev = frame_view(after, *geo[:3], geo[3], geo[4], geo[5]), frame_view(exp, *geo[:3], geo[3], geo[4], geo[5])
        ok = ~hit.reshape(F, D)
        for f in range(F):
            np.testing.assert_array_equal(av[f][:, ok[f]], ev[f][:, ok[f]])
    return got


RS251 = ("rs", 255, 251)
CASES = [
    # (codec, depth, sym_stride, len, nframes, frame pad, base offset, lost)
    (RS251, 777, 800, 10, 2, 13, 0, [0, 3, 11, 13]),          # element/dword path, ragged depth
    (RS251, 777, 800, 10, 2, 13, 1, [0, 3, 11, 13]),          # misaligned bases
    (RS251, 777, 800, 10, 2, 13, 3, [0, 3, 11, 13]),
    (RS251, 1024, 1024, 10, 1, 0, 0, [12, 1]),                # 16-byte path, check rows
    (("rs", 255, 252), 1, 1, 6, 1, 0, 0, [2]),                # lanes outnumber codewords
    (("rs", 255, 252), 3, 3, 6, 1, 0, 0, [2]),
    (("rs", 255, 252), 5, 5, 6, 1, 0, 0, [2]),
    (("rs", 255, 252), 17, 17, 6, 1, 0, 0, [2]),
    (("rs", 255, 223), 300, 304, 223, 1, 0, 0, list(range(0, 64, 2))),   # 32 rows x 223 survivors
    (("ccsds", 255, 223), 260, 260, 223, 1, 0, 0, [5, 222, 223, 254]),   # dual basis
    (("rs", 1023, 1007), 130, 136, 100, 2, 3, 1, [0, 50, 100, 115]),     # uint16_t
    (("rs", 1023, 1007), 75, 80, 100, 2, 0, 0, [0, 50, 100, 115]),       # uint16_t, 16-byte path + ragged end
    (("rs", 1023, 1007), 70, 70, 100, 1, 0, 0, [0, 50, 100, 115]),       # uint16_t, dword path
    (("rs", 255, 215), 40, 48, 30, 2, 0, 0, list(range(1, 70, 7))),      # 40 rows: two row blocks, check rows in both
    (RS251, 500, 512, 10, 2, 0, 0, []),                       # verify only
]


@pytest.mark.parametrize("spec,D,ss,L,F,pad,off,lost", CASES,
                         ids=[f"{c[0][0]}{c[0][1]}_{c[0][2]}-d{c[1]}-s{c[2]}-l{c[3]}-f{c[4]}-o{c[6]}-n{len(c[7])}"
                              for c in CASES])
def test_reconstruct_vs_oracle(torch, spec, D, ss, L, F, pad, off, lost):
    _run(torch, spec, D, ss, L, F, pad, off, lost)


def test_pure_encode_matches_encode_interleaved(torch):
    """All four parity shards lost, 16-byte path, several frames: the oracle's parity, and what
    encode_interleaved writes on the same data."""
    spec, D, ss, L, F, pad, off, lost = RS251, 1040, 1056, 10, 3, 32, 16, [13, 12, 11, 10]
    got = _run(torch, spec, D, ss, L, F, pad, off, lost)
    c, _ = _codecs(spec)
    _, gone, geo, _, _ = _make(spec, D, ss, L, F, pad, off, lost)
    dev = _dev(torch, gone)
    c.encode_interleaved(_frames(torch, dev, *geo))
    np.testing.assert_array_equal(_host(torch, dev), got)


def test_masked_symbols(torch):
    """RS(31,27) in uint8_t, survivors with random bits above bit 4: survivors untouched, rebuilt
    symbols equal the oracle's 5-bit values."""
    _run(torch, ("rs", 31, 27), 100, 100, 20, 2, 7, 0, [1, 2, 23], high_bits=True)


def test_verify_leaves_buffer_alone(torch):
    """nlost == 0: byte-identical buffer, result 0 or -1 (asserted inside _run)."""
    _run(torch, RS251, 500, 512, 10, 1, 0, 0, [])


def test_without_result(torch):
    """result=None on a 16-byte-path shape: the data is rebuilt and nothing else written."""
    _run(torch, RS251, 1024, 1024, 10, 1, 0, 0, [12, 1], use_result=False)
    _run(torch, RS251, 777, 800, 10, 2, 13, 1, [0, 3, 11, 13], use_result=False)


def test_karn_semantics_same_frame(torch):
    """Positions are relative to the first data symbol under both semantics: identical output."""
    a = _run(torch, ("rs", 255, 223), 64, 64, 14, 2, 0, 0, [45, 0, 13, 14])
    b = _run(torch, ("rs", 255, 223), 64, 64, 14, 2, 0, 0, [45, 0, 13, 14], karn=True)
    np.testing.assert_array_equal(a, b)


def test_equivalent_to_decode_interleaved(torch):
    """The staged decode given the same erasures in every codeword: a byte-identical buffer."""
    spec, D, ss, L, F, pad, off, lost = CASES[0]
    got = _run(torch, spec, D, ss, L, F, pad, off, lost)
    c, _ = _codecs(spec)
    _, gone, geo, _, _ = _make(spec, D, ss, L, F, pad, off, lost)
    dev = _dev(torch, gone)
    ncw = F * D
    eras = torch.from_numpy(np.tile(np.array(lost, np.int32), (ncw, 1))).cuda()
    neras = torch.full((ncw,), len(lost), dtype=torch.int32, device="cuda")
    res = c.decode_interleaved(_frames(torch, dev, *geo), eras=eras, neras=neras)
    assert (res.cpu().numpy() >= 0).all()
    np.testing.assert_array_equal(_host(torch, dev), got)


def test_plan_outlives_codec_and_streams(torch):
    """The plan keeps nothing of the codec; a non-default stream; two plans back to back."""
    import gc
    spec, D, ss, L, F, pad, off = RS251, 1024, 1040, 10, 2, 16, 0
    lost_a, lost_b = [0, 3, 11, 13], [5, 12]
    c, _ = _codecs(spec)
    pa, pb = c.recon_plan(L, lost_a), c.recon_plan(L, lost_b)
    del c
    gc.collect()
    exp, gone, geo, rng, _ = _make(spec, D, ss, L, F, pad, off, lost_a)
    dev = _dev(torch, gone)
    fv = _frames(torch, dev, *geo)
    res = torch.empty(F * D, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        pa.reconstruct(fv, result=res, stream=st)
        fv[:, lost_b, :] = 0xA5                                  # lose others, rebuild those
        pb.reconstruct(fv, result=res, stream=st)
    st.synchronize()
    np.testing.assert_array_equal(_host(torch, dev), exp)
    assert (res.cpu().numpy() == len(lost_b)).all()


def test_argument_checks(torch):
    import ezrs
    L_ = ezrs.lib()
    EINVAL, ENOTSUP = -errno.EINVAL, -errno.ENOTSUP
    c = ezrs.Codec.rs(255, 251)
    sp = ezrs._stream_ptr(None)
    L, nr, D, F = 10, 4, 8, 3
    S = L + nr

    def create(lost, length=L, codec=c, out=True):
        h = C.c_void_p()
        arr = (C.c_uint32 * max(len(lost), 1))(*lost)
        rc = L_.ezrs_recon_create(C.byref(h) if out else None, codec._h if codec else None, length, arr,
                                  len(lost))
        if rc == 0:
            assert L_.ezrs_recon_destroy(h) == 0
        else:
            assert not h.value
        return rc

    assert create([0, 3]) == 0 and create([]) == 0
    assert create([3, 5, 3]) == EINVAL                          # duplicate
    assert create([S]) == EINVAL and create([S - 1]) == 0       # position >= S
    assert create([0, 1, 2, 3, 4]) == EINVAL                    # nlost > NROOTS
    assert create([0], length=0) == EINVAL and create([0], length=252) == EINVAL
    assert create([0], codec=None) == EINVAL and create([0], out=False) == EINVAL
    assert L_.ezrs_recon_destroy(None) == 0
    wide = ezrs.Codec.rs(65535, 65503)
    assert create([1, 2], length=65503, codec=wide) == ENOTSUP  # device table above 64 MiB
    assert create([1, 2], length=1000, codec=wide) == 0

    plan = c.recon_plan(L, [0, 3])
    buf = torch.zeros(F * S * D, dtype=torch.uint8, device="cuda")
    res = torch.full((F * D,), 77, dtype=torch.int32, device="cuda")
    fr, rs = C.c_void_p(buf.data_ptr()), C.c_void_p(res.data_ptr())

    def rec(h=plan._h, fr=fr, fp=S * D, ss=D, D=D, F=F, rs=rs):
        return L_.ezrs_reconstruct_interleaved(h, fr, fp, ss, D, F, rs, sp)

    assert rec() == 0 and rec(rs=None) == 0
    assert rec(h=None) == EINVAL
    assert rec(fr=None) == EINVAL
    assert rec(D=0) == EINVAL
    assert rec(ss=D - 1) == EINVAL
    assert rec(fp=(S - 1) * D + D - 1) == EINVAL and rec(fp=(S - 1) * D + D) == 0
    assert rec(fp=0, F=1) == 0                                  # one frame: the pitch is not used
    res.fill_(77)
    before = buf.clone()
    assert rec(F=0) == 0 and rec(F=0, D=0, fr=None) == 0        # nothing to do, nothing touched
    torch.cuda.synchronize()
    assert (res == 77).all() and torch.equal(buf, before)
    with pytest.raises(ezrs.EzrsError):
        plan.reconstruct(buf.view(F, S, D).cpu())
    with pytest.raises(ezrs.EzrsError):
        plan.reconstruct(buf.view(F * S, D))
    with pytest.raises(ezrs.EzrsError):
        plan.reconstruct(buf.view(-1)[:F * (S - 1) * D].view(F, S - 1, D))   # another length
    with pytest.raises(ezrs.EzrsError):
        c.recon_plan(L, [1, 1])

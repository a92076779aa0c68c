"""Batched pointer-table reconstruction (ezrs_reconstruct_ptrs_batch, Recon.reconstruct_ptrs_batch,
ezrs.ptr_table): several stripes per call, every shard of every stripe a buffer of its own, carved
from ONE arena (ptrs_util) with keys (stripe, position), so addresses are monotonic neither in the
position nor in the stripe.  The codewords are encoded by the oracle; the buffers of the lost shards
hold garbage; the table has three pad entries per stripe that hold a poison address.  After the call
the WHOLE arena must equal the oracle's (rebuilt bytes, untouched survivors, intact guards, nothing
written for a NULL entry) and result is nlost everywhere.  Then one survivor symbol is flipped in
every third codeword of every stripe: result is -1 exactly there."""
import ctypes as C
import errno

import numpy as np
import pytest

import oracle as O
from ptrs_util import Arena, download

pytestmark = pytest.mark.gpu

POISON = 0x0DEAD0000BAD0001                        # odd, not even a canonical address: never dereferenced
PAD = 3


@pytest.fixture(scope="module")
def torch():
    import torch as T
    if not T.cuda.is_available():
        pytest.skip("no GPU")
    return T


def _params(spec):
    kind, n, k = spec
    return O.rs_params(n, k) if kind == "rs" else O.ccsds_params(k, kind == "ccsds")


def _codec(spec):
    import ezrs
    kind, n, k = spec
    return ezrs.Codec.rs(n, k) if kind == "rs" else ezrs.Codec.ccsds(k, dual=kind == "ccsds")


_ROWS, _NN = {}, {}


def _nn(spec):
    if spec not in _NN:
        _NN[spec] = int(O.Codec(*_params(spec)).nn)
    return _NN[spec]


def _rows(spec, L, n, ns):
    """ns stripes of n oracle-encoded codewords of length L, [ns, n, L + nroots]; computed once,
    never modified."""
    key = (spec, L, n, ns)
    if key not in _ROWS:
        oc = O.Codec(*_params(spec))
        rng = np.random.default_rng(L * 7919 + n * 31 + ns)
        rows = (rng.integers(0, 1 << 16, (ns * n, L + oc.nroots)) & oc.nn).astype(oc.dtype)
        oc.encode_batch(rows, L)
        rows = rows.reshape(ns, n, -1)
        rows.setflags(write=False)
        _ROWS[key] = rows
    return _ROWS[key]


def _want(lost, ns, wanted):
    """Per stripe, the lost positions that get a buffer (default: all of them)."""
    return [list(lost) if wanted is None else list(wanted[s]) for s in range(ns)]


def _stripes(spec, L, lost, n, ns, cls="A16", odd=None, wanted=None, seed=1):
    """The arena of ns stripes.  Returns (arena, expected host image, input host image with garbage
    in the lost buffers)."""
    rows = _rows(spec, L, n, ns)
    S, dt = rows.shape[2], rows.dtype
    want = _want(lost, ns, wanted)
    have = [(s, p) for s in range(ns) for p in range(S) if p not in set(lost) or p in want[s]]
    ar = Arena({k: n for k in have}, dt.itemsize, cls, odd, seed)
    rng = np.random.default_rng(seed + 100)
    exp = ar.host.copy()
    for s, p in have:
        ar.put(exp, (s, p), rows[s, :, p])
    gone = exp.copy()
    for s in range(ns):
        for p in want[s]:
            ar.put(gone, (s, p), rng.integers(0, 1 << (8 * dt.itemsize), n).astype(dt))
    return ar, exp, gone


def _tensors(torch, ar, dev, S, ns):
    return [[ar.tensor(torch, dev, (s, p)) if (s, p) in ar.off else None for p in range(S)] for s in range(ns)]


def _table(torch, ar, dev, S, ns, lost):
    """(table with PAD poison entries per stripe, shard_len, align) through ezrs.ptr_table."""
    import ezrs
    tab, n, align = ezrs.ptr_table(_tensors(torch, ar, dev, S, ns), optional=lost)
    assert tab.shape == (ns, S) and tab.dtype == torch.int64 and tab.is_cuda
    pad = torch.tensor([POISON], dtype=torch.int64).to(tab.device).expand(ns, PAD)
    return torch.cat([tab, pad], dim=1).contiguous(), n, align


_ALIGN = {"A16": lambda w: 16, "A4": lambda w: 4, "A1": lambda w: w}


def _run(torch, spec, L, lost, n, ns, cls="A16", odd=None, wanted=None, use_result=True):
    c = _codec(spec)
    plan = c.recon_plan(L, lost)
    S, nlost = L + c.nroots, len(lost)
    ar, exp, gone = _stripes(spec, L, lost, n, ns, cls, odd, wanted)
    want = _want(lost, ns, wanted)
    dev = ar.upload(torch, gone)
    tab, n_, align = _table(torch, ar, dev, S, ns, lost)
    assert n_ == n and align == _ALIGN[cls](ar.w) and tab.stride(0) == S + PAD
    res = torch.full((ns * n,), 77, dtype=torch.int32, device="cuda") if use_result else None
    plan.reconstruct_ptrs_batch(tab, n, align=align, result=res)
    got = download(dev)
    np.testing.assert_array_equal(got, exp, err_msg="rebuilt shards, survivors or guards")
    if not use_result:
        return got, None
    np.testing.assert_array_equal(res.cpu().numpy(), np.full(ns * n, nlost), err_msg="clean results")

    # one survivor symbol flipped in every third codeword of every stripe
    rng = np.random.default_rng(n + nlost)
    hit = np.arange(n) % 3 == 1
    bad = gone.copy()
    surv = plan.survivors
    nn = _nn(spec)
    dtp = np.uint8 if ar.w == 1 else np.uint16
    for s in range(ns):
        for k in np.nonzero(hit)[0]:
            p = surv[int(rng.integers(0, len(surv)))]
            v = ar.get(bad, (s, p), dtp)
            v[k] ^= int(rng.integers(1, nn + 1))
            ar.put(bad, (s, p), v)
    dev = ar.upload(torch, bad)
    tab, _, _ = _table(torch, ar, dev, S, ns, lost)
    res.fill_(77)
    plan.reconstruct_ptrs_batch(tab, n, align=align, result=res)
    r = res.cpu().numpy()
    if nlost < c.nroots:
        np.testing.assert_array_equal(r, np.tile(np.where(hit, -1, nlost), ns),
                                      err_msg="results with wrong survivors")
    else:
        np.testing.assert_array_equal(r, np.full(ns * n, nlost))    # nothing left to check with
    after = download(dev)
    want_img = bad.copy()                           # everything but the rebuilt buffers is as it was,
    for s in range(ns):                             # and intact codewords are rebuilt all the same
        for p in want[s]:
            a, e = ar.get(after, (s, p), dtp), ar.get(exp, (s, p), dtp)
            np.testing.assert_array_equal(a[~hit], e[~hit])
            ar.put(want_img, (s, p), a)
    np.testing.assert_array_equal(after, want_img, err_msg="a byte outside the rebuilt buffers")
    return got, r


RS251, LOST4 = ("rs", 255, 251), [0, 3, 11, 13]
RS223, RS1007 = ("rs", 255, 223), ("rs", 1023, 1007)
CASES = [
    # (codec, len, lost, shard_len, stripes, class, misaligned buffer)
    (RS251, 10, LOST4, 1077, 3, "A16", None),       # 16*64 + 16*3 + 5: a full wave, a 3-lane wave, a tail of 5
    (RS251, 10, LOST4, 267, 3, "A4", (1, 5)),       # 4*64 + 4*2 + 3, one buffer at 4 mod 16
    (RS251, 10, LOST4, 71, 5, "A1", (3, 6)),        # one buffer at an odd address: element by element
    (RS251, 10, LOST4, 71, 5, "A1", (2, 3)),        # ... an output
    (RS251, 10, LOST4, 1, 67, "A16", None),         # tail only: several workgroups of one-lane stripes
    (RS223, 223, list(range(0, 64, 2)), 1045, 2, "A16", None),      # 32 lost: two row blocks
    (RS223, 223, [5, 100, 222, 240], 1045, 2, "A16", None),         # 4 lost with result: 32 rows
    (("ccsds", 255, 223), 223, [5, 222, 223, 254], 85, 2, "A16", None),     # dual basis
    (RS1007, 100, [0, 50, 101], 523, 3, "A16", None),               # uint16_t: 8*64 + 8 + 3
    (RS1007, 100, [0, 50, 101], 523, 3, "A1", (1, 7)),              # align 2, a buffer at 2 mod 4
]


@pytest.mark.parametrize("spec,L,lost,n,ns,cls,odd", CASES,
                         ids=[f"{c[0][0]}{c[0][1]}_{c[0][2]}-l{c[1]}-n{len(c[2])}-d{c[3]}-s{c[4]}-{c[5]}-"
                              f"{'' if c[6] is None else 'o%d.%d' % c[6]}" for c in CASES])
def test_reconstruct_ptrs_batch_vs_oracle(torch, spec, L, lost, n, ns, cls, odd):
    _run(torch, spec, L, lost, n, ns, cls, odd)


def test_null_entries_per_stripe(torch):
    """Three stripes under one 4-lost plan: stripe 0 wants only lost[0], stripe 1 nothing, stripe 2
    everything.  Only those shards are written (whole-arena comparison inside _run) and `result` is
    what it is with every buffer given, in the clean and in the flipped run."""
    spec, L, lost, n = RS223, 14, [45, 0, 13, 14], 130
    _, full = _run(torch, spec, L, lost, n, 3)
    _, part = _run(torch, spec, L, lost, n, 3, wanted=[[lost[0]], [], lost])
    np.testing.assert_array_equal(part, full)
    assert (part == -1).any() and (part == 4).any()
    _run(torch, RS251, 10, LOST4, 267, 3, "A4", (2, 5), wanted=[[LOST4[0]], [], LOST4])


def test_without_result(torch):
    _run(torch, RS251, 10, LOST4, 1077, 3, use_result=False)
    _run(torch, RS251, 10, LOST4, 71, 5, "A1", (3, 6), use_result=False)


def test_verify_writes_nothing(torch):
    """nlost == 0: the arena is byte-identical, result 0 / -1 (asserted inside _run)."""
    _run(torch, RS251, 10, [], 267, 3)


def test_all_parity_is_encode(torch):
    """lost = the parity positions: the oracle's encode (rows come from O.Codec.encode_batch)."""
    _run(torch, RS251, 10, [10, 11, 12, 13], 267, 3)
    _run(torch, RS251, 10, [13, 12, 11, 10], 71, 2, "A4", (1, 12))


def test_above_the_one_stripe_limit(torch):
    """RS(1023,1007) len 400 has 416 positions: more pointers than one ezrs_reconstruct_ptrs call
    carries (-ENOTSUP), none too many for a table on the device."""
    import ezrs
    spec, L, lost, n = RS1007, 400, [0, 200, 401], 25
    c = _codec(spec)
    S = L + c.nroots
    assert S == 416 > 320
    plan = c.recon_plan(L, lost)
    buf = torch.zeros(S * n, dtype=torch.uint16, device="cuda")
    arr = (C.c_void_p * S)(*[buf.data_ptr() + 2 * n * p for p in range(S)])
    assert ezrs.lib().ezrs_reconstruct_ptrs(plan._h, arr, n, None, ezrs._stream_ptr(None)) == -errno.ENOTSUP
    _run(torch, spec, L, lost, n, 2)


def test_agrees_with_one_stripe_calls(torch):
    """The same input image through the batch call and through a loop of one-stripe calls: the same
    bytes everywhere and the same results."""
    spec, L, n, ns = RS251, 10, 267, 3
    lost = [0, 3, 11]                               # one syndrome left to check with
    c = _codec(spec)
    plan = c.recon_plan(L, lost)
    S = L + c.nroots
    ar, exp, gone = _stripes(spec, L, lost, n, ns, "A4", (1, 5))
    for s in range(ns):                             # a survivor symbol wrong in some codewords
        v = ar.get(gone, (s, 5), np.uint8)
        v[s::5] ^= 0x21
        ar.put(gone, (s, 5), v)
    dev1, dev2 = ar.upload(torch, gone), ar.upload(torch, gone)
    r1 = torch.full((ns * n,), 77, dtype=torch.int32, device="cuda")
    r2 = r1.clone()
    tab, _, align = _table(torch, ar, dev1, S, ns, lost)
    plan.reconstruct_ptrs_batch(tab, n, align=align, result=r1)
    for s, shards in enumerate(_tensors(torch, ar, dev2, S, ns)):
        plan.reconstruct_ptrs(shards, result=r2[s * n:(s + 1) * n])
    torch.cuda.synchronize()
    assert torch.equal(r1, r2) and (r1 == -1).any() and (r1 == 3).any()
    np.testing.assert_array_equal(download(dev1), download(dev2))


def test_argument_checks(torch):
    import ezrs
    L_ = ezrs.lib()
    EINVAL = -errno.EINVAL
    sp = ezrs._stream_ptr(None)
    big = C.c_size_t(-1).value

    def checks(spec, L, lost, n, ns, bad_aligns):
        c = _codec(spec)
        S = L + c.nroots
        plan = c.recon_plan(L, lost)
        ar, exp, gone = _stripes(spec, L, lost, n, ns)
        dev = ar.upload(torch, gone)
        tab, _, align = _table(torch, ar, dev, S, ns, lost)
        res = torch.full((ns * n,), 77, dtype=torch.int32, device="cuda")

        def rec(h=plan._h, t=tab.data_ptr(), pitch=S + PAD, n=n, ns=ns, al=align):
            return L_.ezrs_reconstruct_ptrs_batch(h, t, pitch, n, ns, al, C.c_void_p(res.data_ptr()), sp)

        assert rec(h=None) == EINVAL and rec(t=None) == EINVAL
        assert rec(pitch=S - 1) == EINVAL
        for al in bad_aligns:
            assert rec(al=al) == EINVAL, al
        if ar.w == 2:
            assert rec(n=big // 2 + 1, ns=1) == EINVAL           # shard_len * datum bytes
        assert rec(n=big // 2 + 1, ns=2) == EINVAL               # nstripes * shard_len
        assert rec(n=big) == EINVAL and rec(n=2, ns=big) == EINVAL
        assert rec(t=None, ns=0) == EINVAL and rec(pitch=S - 1, n=0) == EINVAL
        assert rec(ns=0) == 0 and rec(n=0) == 0                  # nothing to do
        torch.cuda.synchronize()
        np.testing.assert_array_equal(download(dev), gone, err_msg="a refused or empty call wrote")
        assert (res == 77).all()
        assert rec() == 0                                        # and the good call
        np.testing.assert_array_equal(download(dev), exp)
        return plan, tab, n, res, dev

    plan, tab, n, res, dev = checks(RS251, 10, LOST4, 71, 3, (3, 8, 0, 2, 32))
    checks(RS1007, 100, [0, 50, 101], 24, 2, (3, 8, 0, 1))

    # Python-side validation
    plan.reconstruct_ptrs_batch(tab, n, align=16, result=res)
    with pytest.raises(ezrs.EzrsError):
        plan.reconstruct_ptrs_batch(tab[:, :13], n)                     # fewer entries than positions
    with pytest.raises(ezrs.EzrsError):
        plan.reconstruct_ptrs_batch(tab.cpu(), n)
    with pytest.raises(ezrs.EzrsError):
        plan.reconstruct_ptrs_batch(tab.to(torch.int32), n)
    with pytest.raises(ezrs.EzrsError):
        plan.reconstruct_ptrs_batch(tab.t().contiguous().t(), n)        # last dimension not contiguous
    with pytest.raises(ezrs.EzrsError):
        plan.reconstruct_ptrs_batch(tab[0], n)
    with pytest.raises(ezrs.EzrsError):
        plan.reconstruct_ptrs_batch(tab, n, align=8)
    with pytest.raises(ezrs.EzrsError):
        plan.reconstruct_ptrs_batch(tab, n, result=res[:-1])
    with pytest.raises(ezrs.EzrsError):
        plan.reconstruct_ptrs_batch(tab, n, result=res.to(torch.int16))
    torch.cuda.synchronize()


def test_ptr_table(torch):
    import ezrs
    spec, L, lost, n, ns = RS251, 10, LOST4, 71, 2
    S = 14
    for cls, odd, want in (("A16", None, 16), ("A4", (1, 5), 4), ("A1", (0, 6), 1)):
        ar, exp, gone = _stripes(spec, L, lost, n, ns, cls, odd, wanted=[[0], lost])
        dev = ar.upload(torch, gone)
        ts = _tensors(torch, ar, dev, S, ns)
        tab, n_, align = ezrs.ptr_table(ts, optional=lost)
        assert (n_, align) == (n, want)
        host = tab.cpu().numpy()
        for s in range(ns):
            for p in range(S):
                assert host[s, p] == (0 if ts[s][p] is None else ts[s][p].data_ptr())
        assert host[0, 3] == 0 and host[1, 3] != 0
    with pytest.raises(ezrs.EzrsError):
        ezrs.ptr_table(ts, optional=[0, 3, 11])                         # stripe 0 has None at 13 too
    with pytest.raises(ezrs.EzrsError):
        ezrs.ptr_table([[None if p == 5 else t for p, t in enumerate(ts[1])]], optional=lost)
    with pytest.raises(ezrs.EzrsError):
        ezrs.ptr_table([ts[1], [t[:-1] if p == 2 else t for p, t in enumerate(ts[1])]])
    with pytest.raises(ezrs.EzrsError):
        ezrs.ptr_table([ts[1], ts[1][:-1]])
    with pytest.raises(ezrs.EzrsError):
        ezrs.ptr_table([[t.cpu() if p == 2 else t for p, t in enumerate(ts[1])]])
    with pytest.raises(ezrs.EzrsError):
        ezrs.ptr_table([[dev[:2 * n:2] if p == 2 else t for p, t in enumerate(ts[1])]])
    with pytest.raises(ezrs.EzrsError):
        ezrs.ptr_table([[dev[:2 * n].view(torch.int16) if p == 2 else t for p, t in enumerate(ts[1])]])

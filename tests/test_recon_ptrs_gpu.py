"""Pointer-array reconstruction (ezrs_reconstruct_ptrs, Recon.reconstruct_ptrs): every shard of one
stripe is a buffer of its own, carved from an arena (ptrs_util).  The codewords are encoded by the
oracle; the buffers of the lost shards hold garbage; after the call the WHOLE arena must equal the
oracle's (rebuilt bytes, untouched survivors, intact guards, nothing written for a NULL entry).
Then one survivor symbol is flipped in every third codeword: result is -1 exactly there."""
import ctypes as C
import errno

import numpy as np
import pytest

import oracle as O
from ptrs_util import Arena, download

pytestmark = pytest.mark.gpu


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


def _rows(spec, L, n):
    """n oracle-encoded codewords of length L, [n, L + nroots]; computed once, never modified."""
    key = (spec, L, n)
    if key not in _ROWS:
        oc = O.Codec(*_params(spec))
        rng = np.random.default_rng(L * 7919 + n)
        rows = (rng.integers(0, 1 << 16, (n, L + oc.nroots)) & oc.nn).astype(oc.dtype)
        oc.encode_batch(rows, L)
        rows.setflags(write=False)
        _ROWS[key] = rows
    return _ROWS[key]


def _stripe(torch, spec, L, lost, n, cls="A16", odd=None, wanted=None, high_bits=False, seed=1):
    """The arena of one stripe.  wanted: the lost positions that get a buffer (default: all).
    Returns (arena, expected host image, input host image with garbage in the lost buffers)."""
    rows = _rows(spec, L, n)
    S = rows.shape[1]
    dt = rows.dtype
    wanted = list(lost) if wanted is None else wanted
    have = [p for p in range(S) if p not in set(lost) or p in wanted]
    ar = Arena({p: n for p in have}, dt.itemsize, cls, odd, seed)
    rng = np.random.default_rng(seed + 100)
    exp = ar.host.copy()
    for p in have:
        v = rows[:, p].copy()
        if high_bits and p not in lost:             # survivors carry bits above the symbol
            v |= rng.integers(0, 256, n).astype(dt) & dt.type(0xE0)
        ar.put(exp, p, v)
    gone = exp.copy()
    for p in wanted:
        ar.put(gone, p, rng.integers(0, 1 << (8 * dt.itemsize), n).astype(dt))
    return ar, exp, gone


def _shards(torch, ar, dev, S):
    return [ar.tensor(torch, dev, p) if p in ar.off else None for p in range(S)]


def _run(torch, spec, L, lost, n, cls="A16", odd=None, wanted=None, high_bits=False, use_result=True):
    c = _codec(spec)
    plan = c.recon_plan(L, lost)
    S, nlost = L + c.nroots, len(lost)
    ar, exp, gone = _stripe(torch, spec, L, lost, n, cls, odd, wanted, high_bits)
    wanted = list(lost) if wanted is None else wanted
    dev = ar.upload(torch, gone)
    res = torch.full((n,), 77, dtype=torch.int32, device="cuda") if use_result else None
    plan.reconstruct_ptrs(_shards(torch, ar, dev, S), result=res)
    got = download(dev)
    np.testing.assert_array_equal(got, exp, err_msg="rebuilt shards, survivors or guards")
    if not use_result:
        return got, None
    clean = res.cpu().numpy()
    np.testing.assert_array_equal(clean, np.full(n, nlost), err_msg="clean results")

    # one survivor symbol flipped in every third codeword
    rng = np.random.default_rng(n + nlost)
    hit = np.arange(n) % 3 == 1
    bad = gone.copy()
    surv = plan.survivors
    nn = _nn(spec)
    dtp = np.uint8 if ar.w == 1 else np.uint16
    for k in np.nonzero(hit)[0]:
        p = surv[int(rng.integers(0, len(surv)))]
        v = ar.get(bad, p, dtp)
        v[k] ^= int(rng.integers(1, nn + 1))
        ar.put(bad, p, v)
    dev = ar.upload(torch, bad)
    res.fill_(77)
    plan.reconstruct_ptrs(_shards(torch, ar, dev, S), result=res)
    r = res.cpu().numpy()
    if nlost < c.nroots:
        np.testing.assert_array_equal(r, np.where(hit, -1, nlost), err_msg="results with wrong survivors")
    else:
        np.testing.assert_array_equal(r, np.full(n, nlost))     # nothing left to check with
    after = download(dev)
    want = bad.copy()                               # everything but the rebuilt buffers is as it was,
    for p in wanted:                                # and intact codewords are rebuilt all the same
        a, e = ar.get(after, p, dtp), ar.get(exp, p, dtp)
        np.testing.assert_array_equal(a[~hit], e[~hit])
        ar.put(want, p, a)
    np.testing.assert_array_equal(after, want, err_msg="a byte outside the rebuilt buffers")
    return got, r


RS251, LOST4 = ("rs", 255, 251), [0, 3, 11, 13]
CASES = [
    # (codec, len, lost, shard_len, class, misaligned position)
    (RS251, 10, LOST4, 777, "A16", None),                       # 16-byte body + 9 ragged, 10 survivors
    (RS251, 10, LOST4, 777, "A4", 5),
    (RS251, 10, LOST4, 777, "A1", 5),                           # a survivor misaligned
    (RS251, 10, LOST4, 777, "A1", 3),                           # only an output misaligned
    (("rs", 255, 252), 6, [2], 1, "A16", None),                 # lanes outnumber codewords
    (("rs", 255, 252), 6, [2], 3, "A16", None),
    (("rs", 255, 252), 6, [2], 5, "A16", None),
    (("rs", 255, 252), 6, [2], 17, "A16", None),
    (("rs", 255, 223), 223, list(range(0, 64, 2)), 300, "A16", None),   # 255 pointers, two row blocks
    (("ccsds", 255, 223), 223, [5, 222, 223, 254], 260, "A16", None),   # dual basis
    (("rs", 1023, 1007), 100, [0, 50, 101], 75, "A16", None),   # uint16_t forms
    (("rs", 1023, 1007), 100, [0, 50, 101], 70, "A4", 7),
    (("rs", 1023, 1007), 100, [0, 50, 101], 70, "A1", 7),
    (("rs", 65535, 65503), 40, [7], 24, "A16", None),           # RB = 32 and the `fix` constant
]


@pytest.mark.parametrize("spec,L,lost,n,cls,odd", CASES,
                         ids=[f"{c[0][0]}{c[0][1]}_{c[0][2]}-l{c[1]}-n{len(c[2])}-d{c[3]}-{c[4]}-o{c[5]}"
                              for c in CASES])
def test_reconstruct_ptrs_vs_oracle(torch, spec, L, lost, n, cls, odd):
    _run(torch, spec, L, lost, n, cls, odd)


def test_masked_symbols(torch):
    """RS(31,27) in uint8_t: survivors carry bits above bit 4 and stay as they are; the rebuilt
    shards equal the oracle's 5-bit values."""
    _run(torch, ("rs", 31, 27), 20, [1, 2, 23], 100, high_bits=True)


def test_without_result(torch):
    _run(torch, RS251, 10, LOST4, 777, use_result=False)
    _run(torch, RS251, 10, LOST4, 777, "A1", 5, use_result=False)


def test_degraded_read(torch):
    """Only lost[1] has a buffer, the other three entries are NULL: only that shard is written
    (whole-arena comparison inside _run) and `result` is what it is with every buffer given, in
    the clean and in the flipped run."""
    _, full = _run(torch, RS251, 10, LOST4, 777)
    _, part = _run(torch, RS251, 10, LOST4, 777, wanted=[LOST4[1]])
    np.testing.assert_array_equal(part, full)
    # RS(255,251) has no syndrome left to check four lost shards with; a code that has
    spec, L, lost = ("rs", 255, 223), 14, [45, 0, 13, 14]
    _, full = _run(torch, spec, L, lost, 260)
    _, part = _run(torch, spec, L, lost, 260, wanted=[lost[1]])
    np.testing.assert_array_equal(part, full)
    assert (part == -1).any() and (part == 4).any()


def test_all_parity_is_encode(torch):
    """lost = the parity positions: the oracle's encode (rows come from O.Codec.encode_batch)."""
    _run(torch, RS251, 10, [10, 11, 12, 13], 777)
    _run(torch, RS251, 10, [13, 12, 11, 10], 64, "A4", 12)


def test_verify_writes_nothing(torch):
    """nlost == 0: the arena is byte-identical, result 0 / -1 (asserted inside _run)."""
    _run(torch, RS251, 10, [], 500)


def test_agrees_with_strided(torch):
    """One stripe laid out both ways: the same bytes and the same result."""
    spec, L, n = RS251, 10, 777
    c = _codec(spec)
    lost = [0, 3, 11]                               # one syndrome left to check with
    plan = c.recon_plan(L, lost)
    S = L + c.nroots
    ar, exp, gone = _stripe(torch, spec, L, lost, n)
    # a survivor symbol wrong in some codewords, so that result has both values
    v = ar.get(gone, 5, np.uint8)
    v[::5] ^= 0x21
    ar.put(gone, 5, v)
    dev = ar.upload(torch, gone)
    shards = _shards(torch, ar, dev, S)
    frames = torch.stack(shards).unsqueeze(0).contiguous()     # [1, S, n]
    r1 = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    r2 = r1.clone()
    plan.reconstruct(frames, result=r1)
    plan.reconstruct_ptrs(shards, result=r2)
    torch.cuda.synchronize()
    assert torch.equal(r1, r2) and (r1 == -1).any() and (r1 == 3).any()
    assert torch.equal(torch.stack(shards), frames[0])


def test_pointer_array_is_read_during_the_call(torch):
    """The host array is zeroed right after the call returns, before any synchronisation."""
    import ezrs
    spec, L, n = RS251, 10, 1 << 16
    c = _codec(spec)
    plan = c.recon_plan(L, LOST4)
    S = L + c.nroots
    ar, exp, gone = _stripe(torch, spec, L, LOST4, n)
    dev = ar.upload(torch, gone)
    shards = _shards(torch, ar, dev, S)
    arr = (C.c_void_p * S)(*[t.data_ptr() for t in shards])
    torch.cuda.synchronize()
    rc = ezrs.lib().ezrs_reconstruct_ptrs(plan._h, arr, n, None, ezrs._stream_ptr(None))
    C.memset(arr, 0, C.sizeof(arr))
    assert rc == 0
    np.testing.assert_array_equal(download(dev), exp)


def test_argument_checks(torch):
    import ezrs
    L_ = ezrs.lib()
    EINVAL, ENOTSUP = -errno.EINVAL, -errno.ENOTSUP
    sp = ezrs._stream_ptr(None)
    c = _codec(RS251)
    L, n = 10, 64
    S = L + c.nroots
    plan = c.recon_plan(L, [0, 3])
    buf = torch.zeros(S * 2 * n, dtype=torch.uint8, device="cuda")
    res = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    base = buf.data_ptr()
    ptr = [base + 2 * n * p for p in range(S)]

    def rec(ptrs=ptr, h=plan._h, n=n, arr=True, rs=res):
        a = (C.c_void_p * S)(*ptrs) if arr else None
        return L_.ezrs_reconstruct_ptrs(h, a, n, C.c_void_p(rs.data_ptr()) if rs is not None else None, sp)

    def but(p, v):
        q = list(ptr)
        q[p] = v
        return q

    assert rec() == 0 and rec(rs=None) == 0
    assert rec(h=None) == EINVAL and rec(arr=False) == EINVAL
    assert rec(but(5, None)) == EINVAL                          # a NULL survivor
    assert rec(but(3, None)) == 0 and rec(but(0, None)) == 0    # an unwanted shard
    assert rec(but(3, ptr[5])) == EINVAL                        # an output on a survivor
    assert rec(but(3, ptr[5] + n - 1)) == EINVAL                # ... overlapping its last element
    assert rec(but(3, ptr[5] + n)) == 0                         # ... right behind it
    assert rec(but(3, ptr[0] + n - 1)) == EINVAL                # two outputs overlapping by one element
    assert rec(but(3, ptr[0] - n + 1)) == EINVAL
    assert rec(but(3, ptr[0] + n)) == 0
    torch.cuda.synchronize()
    res.fill_(77)
    buf.fill_(0x5A)
    before = buf.clone()
    assert rec(n=0) == 0 and rec(but(5, None), n=0) == 0        # nothing to do, nothing touched
    torch.cuda.synchronize()
    assert (res == 77).all() and torch.equal(buf, before)

    # Python-side validation
    sh = [buf[2 * n * p:2 * n * p + n] for p in range(S)]
    plan.reconstruct_ptrs(sh)
    with pytest.raises(ezrs.EzrsError):
        plan.reconstruct_ptrs(sh[:-1])
    with pytest.raises(ezrs.EzrsError):
        plan.reconstruct_ptrs([None if p == 5 else t for p, t in enumerate(sh)])   # a survivor
    with pytest.raises(ezrs.EzrsError):
        plan.reconstruct_ptrs([t.cpu() if p == 2 else t for p, t in enumerate(sh)])
    with pytest.raises(ezrs.EzrsError):
        plan.reconstruct_ptrs([t[:-1] if p == 2 else t for p, t in enumerate(sh)])
    with pytest.raises(ezrs.EzrsError):
        plan.reconstruct_ptrs([buf[:2 * n:2] if p == 2 else t for p, t in enumerate(sh)])
    with pytest.raises(ezrs.EzrsError):
        plan.reconstruct_ptrs([t.view(torch.int16) if p == 2 else t for p, t in enumerate(sh)])
    plan.reconstruct_ptrs([None if p == 3 else t for p, t in enumerate(sh)])
    torch.cuda.synchronize()


def test_pointer_limit(torch):
    """EZRS_PTRS_MAX = 320 pointers: RS(65535,65503) shortened to len + NROOTS = 320 runs (and is
    right, against the oracle), 321 is -ENOTSUP."""
    import ezrs
    spec = ("rs", 65535, 65503)
    _run(torch, spec, 288, [7], 8)
    c = _codec(spec)
    plan = c.recon_plan(289, [7])
    n, S = 8, 321
    buf = torch.zeros(S * 2 * n, dtype=torch.uint16, device="cuda")
    before = buf.clone()
    arr = (C.c_void_p * S)(*[buf.data_ptr() + 4 * n * p for p in range(S)])
    rc = ezrs.lib().ezrs_reconstruct_ptrs(plan._h, arr, n, None, ezrs._stream_ptr(None))
    assert rc == -errno.ENOTSUP
    with pytest.raises(ezrs.EzrsError):
        plan.reconstruct_ptrs([buf[2 * n * p:2 * n * p + n] for p in range(S)])
    torch.cuda.synchronize()
    assert torch.equal(buf, before)

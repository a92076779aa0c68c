"""Pointer-array parity update (ezrs_update_ptrs, Update.apply_ptrs): only what the call needs is on
the device.  The arena (ptrs_util) holds the changed shards, the parity shards and the new symbols
of one stripe and nothing else; every other entry of `shards` is None.  The old stripe is encoded
by the oracle; after the call the WHOLE arena must equal the one with the changed shards replaced
and the parity encoded again by the oracle (newsyms and guards untouched).  Bit-exact."""
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


_OC, _OLD = {}, {}


def _oracle(spec):
    if spec not in _OC:
        _OC[spec] = O.Codec(*_params(spec))
    return _OC[spec]


def _old(spec, L, n):
    """n oracle-encoded codewords of length L, [n, L + nroots]; computed once, never modified."""
    key = (spec, L, n)
    if key not in _OLD:
        oc = _oracle(spec)
        rng = np.random.default_rng(L * 104729 + n)
        rows = (rng.integers(0, 1 << 16, (n, L + oc.nroots)) & oc.nn).astype(oc.dtype)
        oc.encode_batch(rows, L)
        rows.setflags(write=False)
        _OLD[key] = rows
    return _OLD[key]


def _stripe(spec, L, changed, n, cls="A16", odd=None, everything=False, err=None, seed=2):
    """The arena of one update: keys ("s", p) for the shards it holds (the changed and the parity
    positions; all positions with everything=True) and ("n", r) for the new symbols of changed[r].
    err: XOR-ed into the old parity [n, nroots], which then must stay wrong by as much.
    Returns (arena, input host image, expected host image)."""
    oc = _oracle(spec)
    old = _old(spec, L, n)
    S, dt = old.shape[1], old.dtype
    full = 1 << (8 * dt.itemsize)
    held = range(S) if everything else sorted(set(changed) | set(range(L, S)))
    sizes = {("s", p): n for p in held}
    sizes.update({("n", r): n for r in range(len(changed))})
    ar = Arena(sizes, dt.itemsize, cls, odd, seed)
    rng = np.random.default_rng(seed + 1000 + n)
    new = rng.integers(0, full, (n, len(changed))).astype(dt)   # bits above the symbol too
    rows = old.copy()
    rows[:, changed] = new & dt.type(oc.nn)
    oc.encode_batch(rows, L)
    e = np.zeros((n, S - L), dt) if err is None else err
    before, exp = ar.host.copy(), ar.host.copy()
    for p in held:
        ar.put(before, ("s", p), old[:, p] ^ (e[:, p - L] if p >= L else 0))
        ar.put(exp, ("s", p), rows[:, p] ^ (e[:, p - L] if p >= L else 0))
    for r, p in enumerate(changed):
        ar.put(before, ("n", r), new[:, r])
        ar.put(exp, ("n", r), new[:, r])
        ar.put(exp, ("s", p), new[:, r])            # the data is stored as given
    return ar, before, exp


def _args(torch, ar, dev, S, nchg):
    shards = [ar.tensor(torch, dev, ("s", p)) if ("s", p) in ar.off else None for p in range(S)]
    return shards, [ar.tensor(torch, dev, ("n", r)) for r in range(nchg)]


def _run(torch, spec, L, changed, n, cls="A16", odd=None, err=None):
    c = _codec(spec)
    plan = c.update_plan(L, changed)
    S = L + c.nroots
    ar, before, exp = _stripe(spec, L, changed, n, cls, odd, err=err)
    dev = ar.upload(torch, before)
    shards, news = _args(torch, ar, dev, S, len(changed))
    assert sum(t is not None for t in shards) == len(changed) + c.nroots    # nothing else exists
    plan.apply_ptrs(shards, news)
    np.testing.assert_array_equal(download(dev), exp,
                                  err_msg="parity, new data, or a byte that must not be written")


RS251, RS252, RS223, RS1007 = ("rs", 255, 251), ("rs", 255, 252), ("rs", 255, 223), ("rs", 1023, 1007)
CASES = [
    # (codec, len, changed, shard_len, class, misaligned buffer)
    (RS251, 10, [3], 777, "A16", None),
    (RS251, 10, [3], 777, "A4", ("s", 3)),
    (RS251, 10, [3], 777, "A1", ("n", 0)),                      # only the newsyms buffer misaligned
    (RS251, 10, [3], 777, "A1", ("s", 12)),                     # a parity buffer misaligned
    (RS251, 10, [0, 3, 5, 7, 9], 1040, "A16", None),            # a group of four plus a fifth
    (RS251, 10, [9, 0, 4, 2], 1040, "A16", None),               # four kept in registers
    (RS252, 6, [2], 1, "A16", None),                            # lanes outnumber codewords
    (RS252, 6, [2], 3, "A16", None),
    (RS252, 6, [2], 5, "A16", None),
    (RS252, 6, [2], 17, "A16", None),
    (RS223, 223, [5, 222], 300, "A16", None),                   # two row blocks
    (("rs", 255, 215), 30, [1, 29], 40, "A16", None),           # a padded last block
    (("ccsds", 255, 223), 223, [5, 100], 260, "A16", None),     # dual basis
    (RS1007, 100, [0, 50, 99], 75, "A16", None),                # uint16_t forms
    (RS1007, 100, [0, 50, 99], 70, "A4", ("s", 50)),
    (RS1007, 100, [0, 50, 99], 70, "A1", ("n", 2)),
    (("rs", 65535, 65503), 40, [7, 8, 30], 24, "A16", None),    # RB = 32 and m = 16
]


@pytest.mark.parametrize("spec,L,changed,n,cls,odd", CASES,
                         ids=[f"{c[0][0]}{c[0][1]}_{c[0][2]}-l{c[1]}-c{len(c[2])}-d{c[3]}-{c[4]}-"
                              f"{'' if c[5] is None else c[5][0] + str(c[5][1])}" for c in CASES])
def test_update_ptrs_vs_oracle(torch, spec, L, changed, n, cls, odd):
    _run(torch, spec, L, changed, n, cls, odd)


def test_wrong_parity_stays_wrong_by_as_much(torch):
    """The old parity is read, not recomputed."""
    n = 777
    e = np.random.default_rng(9).integers(0, 256, (n, 4)).astype(np.uint8)
    _run(torch, RS251, 10, [3], n, err=e)
    _run(torch, RS251, 10, [0, 3, 5, 7, 9], n, "A1", ("s", 11), err=e)


def test_chain_update_then_verify(torch):
    """All shards present: apply_ptrs, then an nlost == 0 reconstruct_ptrs says 0 everywhere."""
    spec, L, changed, n = RS251, 10, [9, 0, 4, 2], 1040
    c = _codec(spec)
    S = L + c.nroots
    ar, before, exp = _stripe(spec, L, changed, n, everything=True)
    dev = ar.upload(torch, before)
    shards, news = _args(torch, ar, dev, S, len(changed))
    c.update_plan(L, changed).apply_ptrs(shards, news)
    res = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    c.recon_plan(L, []).reconstruct_ptrs(shards, result=res)
    assert (res == 0).all()
    np.testing.assert_array_equal(download(dev), exp)


def test_agrees_with_strided(torch):
    """One stripe laid out both ways: Update.apply and Update.apply_ptrs write the same bytes."""
    spec, L, changed, n = RS1007, 100, [0, 50, 99], 75
    c = _codec(spec)
    S = L + c.nroots
    plan = c.update_plan(L, changed)
    ar, before, exp = _stripe(spec, L, changed, n, everything=True)
    dev = ar.upload(torch, before)
    shards, news = _args(torch, ar, dev, S, len(changed))
    def stacked(ts):                                # [1, len(ts), n], a copy
        return torch.stack([t.view(torch.int16) for t in ts]).unsqueeze(0).contiguous()

    frames = stacked(shards)
    plan.apply(frames.view(torch.uint16), stacked(news).view(torch.uint16))
    plan.apply_ptrs(shards, news)
    torch.cuda.synchronize()
    assert torch.equal(stacked(shards), frames)
    np.testing.assert_array_equal(download(dev), exp)


def test_argument_checks(torch):
    import ezrs
    L_ = ezrs.lib()
    EINVAL = -errno.EINVAL
    sp = ezrs._stream_ptr(None)
    c = _codec(RS251)
    L, n, changed = 10, 64, [3, 7]
    S = L + c.nroots
    plan = c.update_plan(L, changed)
    buf = torch.zeros((S + 2) * 2 * n, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr()
    ptr = [base + 2 * n * p if p in changed or p >= L else None for p in range(S)]
    new = [base + 2 * n * (S + r) for r in range(2)]

    def upd(ptrs=ptr, news=new, h=plan._h, n=n, arr=True, narr=True):
        a = (C.c_void_p * S)(*ptrs) if arr else None
        b = (C.c_void_p * 2)(*news) if narr else None
        return L_.ezrs_update_ptrs(h, a, b, n, sp)

    def but(p, v, src=ptr):
        q = list(src)
        q[p] = v
        return q

    assert upd() == 0
    assert upd(h=None) == EINVAL and upd(arr=False) == EINVAL and upd(narr=False) == EINVAL
    assert upd(but(3, None)) == EINVAL                          # NULL at a changed position
    assert upd(but(L + 1, None)) == EINVAL                      # NULL at a parity position
    assert upd(news=but(1, None, new)) == EINVAL                # NULL in newsyms
    assert upd(news=but(0, ptr[3], new)) == EINVAL              # newsyms[r] on shards[changed[r]]
    assert upd(news=but(0, ptr[3] + n - 1, new)) == EINVAL      # ... overlapping by one element
    assert upd(news=but(0, ptr[3] + n, new)) == 0
    assert upd(but(L, ptr[7] + n - 1)) == EINVAL                # a parity buffer on a changed one
    assert upd(but(L, ptr[7] + n)) == 0
    assert upd(news=[new[0], new[0]]) == 0                      # two read buffers may coincide
    torch.cuda.synchronize()
    buf.fill_(0x5A)
    before = buf.clone()
    assert upd(n=0) == 0 and upd(but(3, None), n=0) == 0        # nothing to do, nothing touched
    torch.cuda.synchronize()
    assert torch.equal(buf, before)

    # Python-side validation
    sh = [None if q is None else buf[2 * n * p:2 * n * p + n] for p, q in enumerate(ptr)]
    nw = [buf[2 * n * (S + r):2 * n * (S + r) + n] for r in range(2)]
    buf.zero_()
    plan.apply_ptrs(sh, nw)
    plan.apply_ptrs([buf[:3] if t is None else t for t in sh], nw)      # unused entries are ignored
    with pytest.raises(ezrs.EzrsError):
        plan.apply_ptrs(sh[:-1], nw)
    with pytest.raises(ezrs.EzrsError):
        plan.apply_ptrs(but(3, None, sh), nw)
    with pytest.raises(ezrs.EzrsError):
        plan.apply_ptrs(but(L + 2, None, sh), nw)
    with pytest.raises(ezrs.EzrsError):
        plan.apply_ptrs(sh, [nw[0], None])
    with pytest.raises(ezrs.EzrsError):
        plan.apply_ptrs(sh, nw[:1])
    with pytest.raises(ezrs.EzrsError):
        plan.apply_ptrs(sh, [nw[0], nw[1][:-1]])
    with pytest.raises(ezrs.EzrsError):
        plan.apply_ptrs(sh, [nw[0], nw[1].cpu()])
    with pytest.raises(ezrs.EzrsError):
        plan.apply_ptrs(sh, [nw[0], sh[3]])                     # the library's overlap check
    torch.cuda.synchronize()


def test_pointer_limit(torch):
    """2*nchanged + NROOTS pointers: 144 changed positions of RS(65535,65503) make 320 and run,
    145 make 322 and are -ENOTSUP."""
    import ezrs
    spec = ("rs", 65535, 65503)
    _run(torch, spec, 150, list(range(144)), 8)
    c = _codec(spec)
    L, n, nchg = 150, 8, 145
    plan = c.update_plan(L, list(range(nchg)))
    S = L + c.nroots
    buf = torch.zeros((S + nchg) * n, dtype=torch.uint16, device="cuda")
    sh = [buf[n * p:n * p + n] for p in range(S)]
    nw = [buf[n * (S + r):n * (S + r) + n] for r in range(nchg)]
    a = (C.c_void_p * S)(*[t.data_ptr() for t in sh])
    b = (C.c_void_p * nchg)(*[t.data_ptr() for t in nw])
    assert ezrs.lib().ezrs_update_ptrs(plan._h, a, b, n, ezrs._stream_ptr(None)) == -errno.ENOTSUP
    with pytest.raises(ezrs.EzrsError):
        plan.apply_ptrs(sh, nw)

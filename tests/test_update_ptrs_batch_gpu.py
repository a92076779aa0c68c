"""Batched pointer-table parity update (ezrs_update_ptrs_batch, Update.apply_ptrs_batch): several
stripes per call, and only what the call needs is on the device.  ONE arena (ptrs_util) holds the
changed shards, the parity shards and the new symbols of every stripe, keys ("s", stripe, position)
and ("n", stripe, r); the table entry of every other position is a poison address, or 0 in alternate
stripes, and both tables have pad entries that hold the poison address.  The old stripes are encoded
by the oracle; after the call the WHOLE arena must equal the one with the changed shards replaced
and the parity encoded again by the oracle (new symbols and guards untouched).  Bit-exact."""
import ctypes as C
import errno

import numpy as np
import pytest

import oracle as O
from ptrs_util import Arena, download

pytestmark = pytest.mark.gpu

POISON = 0x0DEAD0000BAD0001                        # odd, not even a canonical address: never dereferenced
NEW_PAD = 2


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


def _old(spec, L, n, ns):
    """ns stripes of n oracle-encoded codewords of length L, [ns * n, L + nroots]; computed once,
    never modified."""
    key = (spec, L, n, ns)
    if key not in _OLD:
        oc = _oracle(spec)
        rng = np.random.default_rng(L * 104729 + n * 31 + ns)
        rows = (rng.integers(0, 1 << 16, (ns * n, L + oc.nroots)) & oc.nn).astype(oc.dtype)
        oc.encode_batch(rows, L)
        rows.setflags(write=False)
        _OLD[key] = rows
    return _OLD[key]


def _stripes(spec, L, changed, n, ns, cls="A16", odd=None, everything=False, err=None, seed=2):
    """The arena of one batched update: ("s", st, p) for the shards it holds (the changed and the
    parity positions; all positions with everything=True) and ("n", st, r) for the new symbols of
    changed[r].  err: XOR-ed into the old parity [ns * n, nroots], which then must stay wrong by as
    much.  Returns (arena, input host image, expected host image)."""
    oc = _oracle(spec)
    old = _old(spec, L, n, ns)
    S, dt = old.shape[1], old.dtype
    full = 1 << (8 * dt.itemsize)
    held = range(S) if everything else sorted(set(changed) | set(range(L, S)))
    sizes = {("s", st, p): n for st in range(ns) for p in held}
    sizes.update({("n", st, r): n for st in range(ns) for r in range(len(changed))})
    ar = Arena(sizes, dt.itemsize, cls, odd, seed)
    rng = np.random.default_rng(seed + 1000 + n)
    new = rng.integers(0, full, (ns * n, len(changed))).astype(dt)      # bits above the symbol too
    rows = old.copy()
    rows[:, changed] = new & dt.type(oc.nn)
    oc.encode_batch(rows, L)
    e = np.zeros((ns * n, S - L), dt) if err is None else err
    before, exp = ar.host.copy(), ar.host.copy()
    for st in range(ns):
        sl = slice(st * n, (st + 1) * n)
        for p in held:
            x = e[sl, p - L] if p >= L else 0
            ar.put(before, ("s", st, p), old[sl, p] ^ x)
            ar.put(exp, ("s", st, p), rows[sl, p] ^ x)
        for r, p in enumerate(changed):
            ar.put(before, ("n", st, r), new[sl, r])
            ar.put(exp, ("n", st, r), new[sl, r])
            ar.put(exp, ("s", st, p), new[sl, r])   # the data is stored as given
    return ar, before, exp


def _tensors(torch, ar, dev, S, ns, nchg):
    shards = [[ar.tensor(torch, dev, ("s", st, p)) if ("s", st, p) in ar.off else None for p in range(S)]
              for st in range(ns)]
    return shards, [[ar.tensor(torch, dev, ("n", st, r)) for r in range(nchg)] for st in range(ns)]


def _tables(torch, ar, dev, S, ns, changed, L):
    """(table, new_table, shard_len, align) through ezrs.ptr_table.  The entries of `table` that the
    update does not use: the poison address in even stripes, 0 in odd ones; new_table is padded with
    NEW_PAD poison entries per stripe."""
    import ezrs
    shards, news = _tensors(torch, ar, dev, S, ns, len(changed))
    used = set(changed) | set(range(L, S))
    unused = [p for p in range(S) if ("s", 0, p) not in ar.off]
    assert not (set(unused) & used)
    tab, n, a1 = ezrs.ptr_table(shards, optional=unused)
    ntab, n2, a2 = ezrs.ptr_table(news)
    assert n == n2 and tab.shape == (ns, S) and ntab.shape == (ns, len(changed))
    if unused:
        tab[0::2, unused] = torch.tensor(POISON, dtype=torch.int64).to(tab.device)
    pad = torch.tensor([POISON], dtype=torch.int64).to(ntab.device).expand(ns, NEW_PAD)
    return tab, torch.cat([ntab, pad], dim=1).contiguous(), n, min(a1, a2)


_ALIGN = {"A16": lambda w: 16, "A4": lambda w: 4, "A1": lambda w: w}


def _run(torch, spec, L, changed, n, ns, cls="A16", odd=None, err=None):
    c = _codec(spec)
    plan = c.update_plan(L, changed)
    S = L + c.nroots
    ar, before, exp = _stripes(spec, L, changed, n, ns, cls, odd, err=err)
    dev = ar.upload(torch, before)
    tab, ntab, n_, align = _tables(torch, ar, dev, S, ns, changed, L)
    assert n_ == n and align == _ALIGN[cls](ar.w) and ntab.stride(0) == len(changed) + NEW_PAD
    plan.apply_ptrs_batch(tab, ntab, n, align=align)
    np.testing.assert_array_equal(download(dev), exp,
                                  err_msg="parity, new data, or a byte that must not be written")


RS251, RS223, RS1007 = ("rs", 255, 251), ("rs", 255, 223), ("rs", 1023, 1007)
FOUR, FIVE = [9, 0, 4, 2], [5, 100, 101, 222, 7]
CASES = [
    # (codec, len, changed, shard_len, stripes, class, misaligned buffer)
    (RS251, 10, [3], 1077, 3, "A16", None),         # 16*64 + 16*3 + 5: a full wave, a 3-lane wave, a tail of 5
    (RS251, 10, [3], 267, 3, "A4", ("s", 1, 3)),    # 4*64 + 4*2 + 3, one buffer at 4 mod 16
    (RS251, 10, [3], 71, 5, "A1", ("n", 2, 0)),     # only a new-symbols buffer at an odd address
    (RS251, 10, [3], 71, 5, "A1", ("s", 3, 12)),    # a parity buffer at an odd address
    (RS251, 10, [3], 1, 67, "A16", None),           # tail only: several workgroups of one-lane stripes
    (RS251, 10, FOUR, 1077, 3, "A16", None),        # four kept in registers
    (RS251, 10, FOUR, 267, 3, "A4", ("s", 0, 11)),
    (RS251, 10, FOUR, 71, 5, "A1", ("n", 4, 2)),
    (RS251, 10, FOUR, 1, 67, "A16", None),
    (RS223, 223, [100], 1045, 2, "A16", None),      # one block kept in registers
    (RS223, 223, FIVE, 1045, 2, "A16", None),       # the NC == 0 path over two row blocks
    (RS1007, 100, [0, 99], 523, 3, "A16", None),    # uint16_t: 8*64 + 8 + 3
    (RS1007, 100, [0, 99], 523, 3, "A1", ("s", 1, 99)),             # align 2, a buffer at 2 mod 4
]


@pytest.mark.parametrize("spec,L,changed,n,ns,cls,odd", CASES,
                         ids=[f"{c[0][0]}{c[0][1]}_{c[0][2]}-l{c[1]}-c{len(c[2])}-d{c[3]}-s{c[4]}-{c[5]}-"
                              f"{'' if c[6] is None else c[6][0] + '%d.%d' % c[6][1:]}" for c in CASES])
def test_update_ptrs_batch_vs_oracle(torch, spec, L, changed, n, ns, cls, odd):
    _run(torch, spec, L, changed, n, ns, cls, odd)


def test_wrong_parity_stays_wrong_by_as_much(torch):
    """The old parity is read, not recomputed: another error in every stripe, and for 10-bit symbols
    in uint16_t the error has bits above the symbol, which stay where they are."""
    n, ns = 267, 3
    e = np.random.default_rng(9).integers(0, 256, (ns * n, 4)).astype(np.uint8)
    _run(torch, RS251, 10, [3], n, ns, err=e)
    _run(torch, RS251, 10, [0, 3, 5, 7, 9], n, ns, "A1", ("s", 2, 11), err=e)
    e = np.random.default_rng(10).integers(0, 1 << 16, (ns * 75, 16)).astype(np.uint16)
    _run(torch, RS1007, 100, [0, 99], 75, ns, err=e)


def test_chain_update_then_verify(torch):
    """All shards present in one table: apply_ptrs_batch, then an nlost == 0 reconstruct_ptrs_batch
    on the same table says 0 everywhere."""
    spec, L, changed, n, ns = RS251, 10, FOUR, 267, 3
    c = _codec(spec)
    S = L + c.nroots
    ar, before, exp = _stripes(spec, L, changed, n, ns, everything=True)
    dev = ar.upload(torch, before)
    tab, ntab, _, align = _tables(torch, ar, dev, S, ns, changed, L)
    c.update_plan(L, changed).apply_ptrs_batch(tab, ntab, n, align=align)
    res = torch.full((ns * n,), 77, dtype=torch.int32, device="cuda")
    c.recon_plan(L, []).reconstruct_ptrs_batch(tab, n, align=align, result=res)
    assert (res == 0).all()
    np.testing.assert_array_equal(download(dev), exp)


def test_agrees_with_one_stripe_calls(torch):
    """The same input image through the batch call and through a loop of one-stripe calls."""
    spec, L, changed, n, ns = RS1007, 100, [0, 50, 99], 75, 3
    c = _codec(spec)
    S = L + c.nroots
    plan = c.update_plan(L, changed)
    ar, before, exp = _stripes(spec, L, changed, n, ns, "A4", ("s", 1, 50))
    dev1, dev2 = ar.upload(torch, before), ar.upload(torch, before)
    tab, ntab, _, align = _tables(torch, ar, dev1, S, ns, changed, L)
    plan.apply_ptrs_batch(tab, ntab, n, align=align)
    shards, news = _tensors(torch, ar, dev2, S, ns, len(changed))
    for st in range(ns):
        plan.apply_ptrs(shards[st], news[st])
    torch.cuda.synchronize()
    np.testing.assert_array_equal(download(dev1), download(dev2))
    np.testing.assert_array_equal(download(dev1), exp)


def test_argument_checks(torch):
    import ezrs
    L_ = ezrs.lib()
    EINVAL = -errno.EINVAL
    sp = ezrs._stream_ptr(None)
    big = C.c_size_t(-1).value

    def checks(spec, L, changed, n, ns, bad_aligns):
        c = _codec(spec)
        S, nchg = L + c.nroots, len(changed)
        plan = c.update_plan(L, changed)
        ar, before, exp = _stripes(spec, L, changed, n, ns)
        dev = ar.upload(torch, before)
        tab, ntab, _, align = _tables(torch, ar, dev, S, ns, changed, L)

        def upd(h=plan._h, t=tab.data_ptr(), pitch=S, nt=ntab.data_ptr(), npitch=nchg + NEW_PAD, n=n, ns=ns,
                al=align):
            return L_.ezrs_update_ptrs_batch(h, t, pitch, nt, npitch, n, ns, al, sp)

        assert upd(h=None) == EINVAL and upd(t=None) == EINVAL and upd(nt=None) == EINVAL
        assert upd(pitch=S - 1) == EINVAL and upd(npitch=nchg - 1) == EINVAL
        for al in bad_aligns:
            assert upd(al=al) == EINVAL, al
        if ar.w == 2:
            assert upd(n=big // 2 + 1, ns=1) == EINVAL           # shard_len * datum bytes
        assert upd(n=big // 2 + 1, ns=2) == EINVAL               # nstripes * shard_len
        assert upd(n=big) == EINVAL and upd(n=2, ns=big) == EINVAL
        assert upd(nt=None, ns=0) == EINVAL and upd(npitch=nchg - 1, n=0) == EINVAL
        assert upd(ns=0) == 0 and upd(n=0) == 0                  # nothing to do
        torch.cuda.synchronize()
        np.testing.assert_array_equal(download(dev), before, err_msg="a refused or empty call wrote")
        assert upd() == 0
        np.testing.assert_array_equal(download(dev), exp)
        return plan, tab, ntab, n, dev

    plan, tab, ntab, n, dev = checks(RS251, 10, [3, 7], 71, 3, (3, 8, 0, 2, 32))
    checks(RS1007, 100, [0, 99], 24, 2, (3, 8, 0, 1))

    # Python-side validation
    plan.apply_ptrs_batch(tab, ntab, n, align=16)
    with pytest.raises(ezrs.EzrsError):
        plan.apply_ptrs_batch(tab[:, :13], ntab, n)
    with pytest.raises(ezrs.EzrsError):
        plan.apply_ptrs_batch(tab, ntab[:, :1], n)
    with pytest.raises(ezrs.EzrsError):
        plan.apply_ptrs_batch(tab, ntab[:-1], n)                        # fewer stripes
    with pytest.raises(ezrs.EzrsError):
        plan.apply_ptrs_batch(tab, ntab.cpu(), n)
    with pytest.raises(ezrs.EzrsError):
        plan.apply_ptrs_batch(tab.to(torch.int32), ntab, n)
    with pytest.raises(ezrs.EzrsError):
        plan.apply_ptrs_batch(tab, ntab, n, align=8)
    torch.cuda.synchronize()

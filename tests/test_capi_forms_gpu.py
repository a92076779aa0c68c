"""GPU tests of the C ABI's entry-point families (include/ezrs.h, include/ezbch.h):

* every encode form and every decode form of one codec computes what the oracle computes, on rows
  whose pitch is wider than the row (an element-versus-byte stride slip cannot pass);
* every -EINVAL rule of the plain, shard, host and BCH forms, one below each bound and at it, the
  single-codeword exemptions and the zero-count returns;
* ezrs_decode_host keeps ezrs_decode's row-pitch rule for rows that carry their parity."""
import ctypes as C
import errno

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

EINVAL = -errno.EINVAL


@pytest.fixture(scope="module")
def torch():
    import torch as T
    if not T.cuda.is_available():
        pytest.skip("no GPU")
    return T


def _p(a, off=0):
    """Pointer to a torch tensor or a numpy array (None stays NULL), `off` bytes in."""
    if a is None:
        return None
    return C.c_void_p((a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data) + off)


def _dev(torch, a):
    """A numpy array on the GPU (uint16 travels as int16: same bytes)."""
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else
                            a.view(np.int32) if a.dtype == np.uint32 else a.copy()).cuda()


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


# ---- 1. every form agrees with the oracle ---------------------------------------------------------
CASES = {
    "rs255_223_full": (lambda E: E.Codec.rs(255, 223), lambda: O.Codec(*O.rs_params(255, 223)), 223),
    "rs255_223_len100": (lambda E: E.Codec.rs(255, 223), lambda: O.Codec(*O.rs_params(255, 223)), 100),
    "rs1023_991_u16_len50": (lambda E: E.Codec(10, 0x409, 1, 1, 32, 0),
                             lambda: O.Codec(10, 0x409, 1, 1, 32), 50),
}
NCW = 5


def _oracle_decode(oc, rows, length, eras, neras, fill):
    """rows [n, length + nroots] (packed) -> corrected rows, results, positions, corr: the batch
    oracle, and its single-codeword form for the correction values (the batch form has none)."""
    nr = oc.nroots
    exp = rows.copy()
    pos = np.full((len(rows), nr), 0xEEEEEEEE, np.uint32)
    res = oc.decode_batch(exp, length, None, eras, neras, pos)
    corr = np.full((len(rows), nr), fill, rows.dtype)
    for k in range(len(rows)):
        d, p = rows[k, :length].copy(), rows[k, length:].copy()
        r, ps = oc.decode(d, p, eras[k, :neras[k]].tolist(), corr[k])
        assert r == res[k] and list(ps) == list(pos[k, :max(r, 0)])
        assert np.array_equal(np.concatenate([d, p]), exp[k])
    return exp, res, pos, corr


def _check_decode(got_rows, exp_rows, res, pos, corr, ref, what):
    exp, eres, epos, ecorr = ref
    np.testing.assert_array_equal(got_rows, exp_rows, err_msg=what)
    np.testing.assert_array_equal(res, eres, err_msg=what)
    for k, r in enumerate(eres):
        if r > 0:
            np.testing.assert_array_equal(pos[k, :r], epos[k, :r], err_msg=f"{what} positions {k}")
            np.testing.assert_array_equal(corr[k, :r], ecorr[k, :r], err_msg=f"{what} corr {k}")


@pytest.mark.parametrize("case", list(CASES))
def test_every_form_agrees(torch, case):
    import ezrs
    L_ = ezrs.lib()
    mk, mko, L = CASES[case]
    c, oc = mk(ezrs), mko()
    h, sp = c._h, ezrs._stream_ptr(None)
    dt, w, nr = c.dtype, c.info.datum_bytes, c.nroots
    fill = 0xA5 if w == 1 else 0x2A5
    S, P = L + nr, L + nr + 3                         # row, and its pitch (padding keeps `fill`)
    rng = np.random.default_rng(0xF0 + L)
    rows = np.full((NCW, P), fill, dt)
    rows[:, :L] = rng.integers(0, c.nn + 1, (NCW, L))
    enc = rows.copy()
    oc.encode_batch(enc, L)                           # parity into columns L..L+nr of each row
    assert (enc[:, S:] == fill).all() and (enc[:, L:S] != rows[:, L:S]).any()
    nb = c.workspace_bytes(NCW)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device="cuda")

    # -- encode, rows ---------------------------------------------------------------------------
    def dev_form(f):
        d = _dev(torch, rows)
        assert f(d) == 0
        return _host(d, dt)

    def host_form(f):
        d = rows.copy()
        assert f(d) == 0
        return d

    forms = {
        "ezrs_encode": dev_form(lambda d: L_.ezrs_encode(h, _p(d), P, L, _p(d, L * w), P, NCW, sp)),
        "ezrs_encode_ws": dev_form(lambda d: L_.ezrs_encode_ws(h, _p(d), P, L, _p(d, L * w), P, NCW,
                                                               _p(ws), nb, sp)),
        "ezrs_encode_rows": dev_form(lambda d: L_.ezrs_encode_rows(h, _p(d), P, L, NCW, sp)),
        "ezrs_encode_rows_ws": dev_form(lambda d: L_.ezrs_encode_rows_ws(h, _p(d), P, L, NCW, _p(ws), nb, sp)),
        "ezrs_encode_host": host_form(lambda d: L_.ezrs_encode_host(h, _p(d), P, L, _p(d, L * w), P, NCW, 0)),
        "ezrs_encode_rows_host": host_form(lambda d: L_.ezrs_encode_rows_host(h, _p(d), P, L, NCW, 0)),
    }
    for name, got in forms.items():
        np.testing.assert_array_equal(got, enc, err_msg=name)

    # -- encode, one interleaved frame of depth NCW (symbol s of codeword j at s * SS + j) --------
    SS = NCW + 3
    fr = np.full((S, SS), fill, dt)
    fr[:L, :NCW] = rows[:, :L].T
    fr_enc = fr.copy()
    fr_enc[:, :NCW] = enc[:, :S].T
    ilb = L_.ezrs_interleaved_workspace_bytes(h, L, NCW, 1)
    ilws = torch.empty(ilb, dtype=torch.uint8, device="cuda")
    for name, f in {
        "ezrs_encode_interleaved": lambda d: L_.ezrs_encode_interleaved(h, _p(d), S * SS, SS, NCW, L, 1, sp),
        "ezrs_encode_interleaved_ws": lambda d: L_.ezrs_encode_interleaved_ws(h, _p(d), S * SS, SS, NCW, L, 1,
                                                                              _p(ilws), ilb, sp),
    }.items():
        d = _dev(torch, fr)
        assert f(d) == 0, name
        np.testing.assert_array_equal(_host(d, dt), fr_enc, err_msg=name)

    # -- the corrupted batch: 2 errors in row 1, 3 in row 3 (one of them an erasure) ------------------
    bad = enc.copy()
    bad[1, [3, L + 5]] ^= np.array([1, 2], dt)
    bad[3, [0, L - 1, S - 1]] ^= np.array([3, 1, 2], dt)
    eras = np.zeros((NCW, nr), np.uint32)
    neras = np.zeros(NCW, np.uint32)
    eras[3, 0], neras[3] = L - 1, 1
    ref = _oracle_decode(oc, np.ascontiguousarray(bad[:, :S]), L, eras, neras, fill)
    assert list(ref[1]) == [0, 2, 0, 3, 0]
    np.testing.assert_array_equal(ref[0], enc[:, :S])

    def outs(n):
        return (np.full(n, 77, np.int32), np.full((n, nr), 0xEEEEEEEE, np.uint32), np.full((n, nr), fill, dt))

    def dev_decode(f, src, n=NCW):
        d, de, dn = _dev(torch, src), _dev(torch, eras), _dev(torch, neras)
        r, q, co = (_dev(torch, a) for a in outs(n))
        assert f(d, de, dn, r, q, co) == 0
        return _host(d, dt), _host(r, np.int32), _host(q, np.uint32), _host(co, dt)

    dforms = {
        "ezrs_decode(parity NULL)": lambda d, e, n, r, q, co: L_.ezrs_decode(
            h, _p(d), P, L, None, 0, _p(e), nr, _p(n), _p(r), _p(q), nr, _p(co), nr, NCW, sp),
        "ezrs_decode(parity)": lambda d, e, n, r, q, co: L_.ezrs_decode(
            h, _p(d), P, L, _p(d, L * w), P, _p(e), nr, _p(n), _p(r), _p(q), nr, _p(co), nr, NCW, sp),
        "ezrs_decode_ws": lambda d, e, n, r, q, co: L_.ezrs_decode_ws(
            h, _p(d), P, L, None, 0, _p(e), nr, _p(n), _p(r), _p(q), nr, _p(co), nr, NCW, _p(ws), nb, sp),
    }
    for name, f in dforms.items():
        got, r, q, co = dev_decode(f, bad)
        _check_decode(got, enc, r, q, co, ref, name)
    got = bad.copy()
    r, q, co = outs(NCW)
    assert L_.ezrs_decode_host(h, _p(got), P, L, None, 0, _p(eras), nr, _p(neras), _p(r), _p(q), nr,
                               _p(co), nr, NCW, 0) == 0
    _check_decode(got, enc, r, q, co, ref, "ezrs_decode_host")
    fr_bad = fr_enc.copy()
    fr_bad[:, :NCW] = bad[:, :S].T
    for name, f in {
        "ezrs_decode_interleaved": lambda d, e, n, r, q, co: L_.ezrs_decode_interleaved(
            h, _p(d), S * SS, SS, NCW, L, 1, _p(e), nr, _p(n), _p(r), _p(q), nr, _p(co), nr, sp),
        "ezrs_decode_interleaved_ws": lambda d, e, n, r, q, co: L_.ezrs_decode_interleaved_ws(
            h, _p(d), S * SS, SS, NCW, L, 1, _p(e), nr, _p(n), _p(r), _p(q), nr, _p(co), nr, _p(ilws), ilb,
            sp),
    }.items():
        got, r, q, co = dev_decode(f, fr_bad)
        _check_decode(got, fr_enc, r, q, co, ref, name)

    # -- two shards of 2 L + 7 data symbols in chunks of L: rows of L, L and 7 symbols ----------------
    slen, T = 2 * L + 7, 7
    R = L_.ezrs_shard_codewords(h, slen, L)
    elen = L_.ezrs_shard_encoded_len(h, slen, L)
    assert (R, elen) == (3, slen + 3 * nr)
    SP = elen + 3
    cws = [(i, j * S, L if j < 2 else T) for i in range(2) for j in range(3)]   # shard, offset, length
    sh = np.full((2, SP), fill, dt)
    for i, o, n in cws:
        sh[i, o:o + n] = rng.integers(0, c.nn + 1, n)
    sh_enc = sh.copy()
    for i, o, n in cws:
        rc, par = oc.encode(sh[i, o:o + n])
        assert rc >= 0
        sh_enc[i, o + n:o + n + nr] = par
    d = _dev(torch, sh)
    assert L_.ezrs_encode_shards(h, _p(d), SP, slen, L, 2, sp) == 0
    np.testing.assert_array_equal(_host(d, dt), sh_enc, err_msg="ezrs_encode_shards")
    sh_bad = sh_enc.copy()
    i, o, n = cws[1]
    sh_bad[i, [o + 3, o + n + 5]] ^= np.array([1, 2], dt)
    i, o, n = cws[5]
    sh_bad[i, [o, o + n - 1, o + n + nr - 1]] ^= np.array([3, 1, 2], dt)
    seras = np.zeros((6, nr), np.uint32)
    sneras = np.zeros(6, np.uint32)
    seras[5, 0], sneras[5] = T - 1, 1
    eres, epos, ecorr = outs(6)
    for k, (i, o, n) in enumerate(cws):
        dd, pp = sh_bad[i, o:o + n].copy(), sh_bad[i, o + n:o + n + nr].copy()
        eres[k], ps = oc.decode(dd, pp, seras[k, :sneras[k]].tolist(), ecorr[k])
        epos[k, :len(ps)] = ps
        assert np.array_equal(dd, sh_enc[i, o:o + n]) and np.array_equal(pp, sh_enc[i, o + n:o + n + nr])
    assert list(eres) == [0, 2, 0, 0, 0, 3]
    d, de, dn = _dev(torch, sh_bad), _dev(torch, seras), _dev(torch, sneras)
    r, q, co = (_dev(torch, a) for a in outs(6))
    assert L_.ezrs_decode_shards(h, _p(d), SP, slen, L, 2, _p(de), nr, _p(dn), _p(r), _p(q), nr, _p(co), nr,
                                 sp) == 0
    _check_decode(_host(d, dt), sh_enc, _host(r, np.int32), _host(q, np.uint32), _host(co, dt),
                  (None, eres, epos, ecorr), "ezrs_decode_shards")


# ---- 2. the argument rules ------------------------------------------------------------------------
def _rules(f, nulls, bounds, one, zero):
    """f(**overrides) calls one entry point.  nulls: arguments that must not be NULL; bounds:
    {stride argument: its bound, or (bound, further overrides the rule needs)}; one: overrides
    that make the batch one codeword with zero strides (legal); zero: a zero count with every
    pointer NULL (legal: nothing is looked at after the codec)."""
    assert f() == 0
    assert f(h=None) == EINVAL
    for k in nulls:
        assert f(**{k: None}) == EINVAL, k
    for k, b in bounds.items():
        b, kw = b if isinstance(b, tuple) else (b, {})
        assert f(**{**kw, k: b - 1}) == EINVAL, k
        assert f(**{**kw, k: b}) == 0, k
    assert f(**one) == 0
    assert f(**zero) == 0


def _rs_rule_tables(L_, h, L, nr, N, dp, pp, rs, ax, cp, tail, decode_rows_rule=True):
    """The closures and rule tables of the split / rows encode and the decode of one flavour
    (device forms with their stream, _ws forms with their workspace, host forms with chunk 0):
    `tail` maps (name of the form) -> the trailing arguments."""
    S = L + nr

    def enc(name):
        def f(h=h, d=dp, ds=S, L=L, p=pp, ps=nr, n=N):
            return getattr(L_, name)(h, d, ds, L, p, ps, n, *tail(name))
        return f

    def encr(name):
        def f(h=h, d=dp, ds=S, L=L, n=N):
            return getattr(L_, name)(h, d, ds, L, n, *tail(name))
        return f

    def dec(name):
        def f(h=h, d=dp, ds=S, L=L, p=None, ps=0, eras=None, es=0, neras=None, rs=rs, pos=None, qs=0,
              corr=None, cs=0, n=N):
            return getattr(L_, name)(h, d, ds, L, p, ps, eras, es, neras, rs, pos, qs, corr, cs, n,
                                     *tail(name))
        return f

    enc_t = dict(nulls=["d", "p"], bounds={"ds": L, "ps": nr},
                 one=dict(n=1, ds=0, ps=0), zero=dict(n=0, d=None, p=None, ds=0, L=0, ps=0))
    encr_t = dict(nulls=["d"], bounds={"ds": S}, one=dict(n=1, ds=0), zero=dict(n=0, d=None, ds=0, L=0))
    dec_t = dict(nulls=["d", "rs"],
                 bounds={"ps": (nr, dict(p=pp, ds=L)), "qs": (nr, dict(pos=ax)), "cs": (nr, dict(corr=cp)),
                         "es": (1, dict(eras=ax, neras=ax))},
                 one=dict(n=1, ds=0, eras=ax, es=0, neras=ax, pos=ax, qs=0, corr=cp, cs=0),
                 zero=dict(n=0, d=None, rs=None, ds=0, L=0))
    if decode_rows_rule:
        dec_t["bounds"]["ds"] = S                        # parity == NULL: rows carry their parity
    return enc, encr, dec, enc_t, encr_t, dec_t


def _rs_common(f, L, load):
    assert f(L=0) == EINVAL and f(L=load + 1) == EINVAL


def test_argument_rules_plain(torch):
    """ezrs_encode / _rows / ezrs_decode and their _ws forms on RS(255,223), three rows."""
    import ezrs
    L_ = ezrs.lib()
    c = ezrs.Codec.rs(255, 223)
    h, sp = c._h, ezrs._stream_ptr(None)
    N, L, nr = 3, 223, 32
    rows = torch.zeros((N, L + nr), dtype=torch.uint8, device="cuda")      # all-zero rows are codewords
    par = torch.zeros((N, nr), dtype=torch.uint8, device="cuda")
    res = torch.full((N,), 77, dtype=torch.int32, device="cuda")
    aux = torch.zeros((N, nr), dtype=torch.int32, device="cuda")
    cor = torch.zeros((N, nr), dtype=torch.uint8, device="cuda")
    need = c.workspace_bytes(N)
    assert need == L_.ezrs_workspace_bytes(h, N) > 0 and L_.ezrs_workspace_bytes(None, N) == 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    wsarg = {"ws": _p(ws), "wb": need}
    tail = lambda name: (wsarg["ws"], wsarg["wb"], sp) if name.endswith("_ws") else (sp,)
    enc, encr, dec, enc_t, encr_t, dec_t = _rs_rule_tables(L_, h, L, nr, N, _p(rows), _p(par), _p(res),
                                                           _p(aux), _p(cor), tail)
    for name, mk, t in (("ezrs_encode", enc, enc_t), ("ezrs_encode_ws", enc, enc_t),
                        ("ezrs_encode_rows", encr, encr_t), ("ezrs_encode_rows_ws", encr, encr_t),
                        ("ezrs_decode", dec, dec_t), ("ezrs_decode_ws", dec, dec_t)):
        f = mk(name)
        _rules(f, **t)
        _rs_common(f, L, c.load)
        if name.endswith("_ws"):                      # null or short workspace
            wsarg.update(ws=None)
            assert f() == EINVAL, name
            wsarg.update(ws=_p(ws), wb=need - 1)
            assert f() == EINVAL, name
            wsarg.update(wb=need)
            assert f() == 0, name
    for name in ("ezrs_decode", "ezrs_decode_ws"):
        f = dec(name)
        assert f(neras=_p(aux)) == EINVAL               # counts without positions
        assert f(es=5) == 0                             # eras == NULL: its stride is not looked at
        assert f(p=_p(par), ps=0, ds=0, n=1) == 0       # one codeword, separate parity
        assert f(p=_p(par), ps=nr, ds=L - 1) == EINVAL and f(p=_p(par), ps=nr, ds=L) == 0
    assert L_.ezrs_encode(h, None, 0, 0, None, 0, 0, sp) == 0
    torch.cuda.synchronize()
    assert (res.cpu().numpy() == 0).all()


def test_argument_rules_shards(torch):
    """ezrs_encode_shards / ezrs_decode_shards: geometry first, then nshards == 0."""
    import ezrs
    L_ = ezrs.lib()
    c = ezrs.Codec.rs(255, 223)
    h, sp = c._h, ezrs._stream_ptr(None)
    nr, chunk, slen, NS = 32, 100, 207, 2
    elen = L_.ezrs_shard_encoded_len(h, slen, chunk)
    assert elen == slen + 3 * nr and L_.ezrs_shard_codewords(h, slen, chunk) == 3
    sh = torch.zeros((NS, elen + 5), dtype=torch.uint8, device="cuda")
    res = torch.full((NS * 3,), 77, dtype=torch.int32, device="cuda")
    aux = torch.zeros((NS * 3, nr), dtype=torch.int32, device="cuda")
    cor = torch.zeros((NS * 3, nr), dtype=torch.uint8, device="cuda")
    ax, cp = _p(aux), _p(cor)

    def enc(h=h, sh=_p(sh), sp_=elen + 5, slen=slen, chunk=chunk, n=NS):
        return L_.ezrs_encode_shards(h, sh, sp_, slen, chunk, n, sp)

    def dec(h=h, sh=_p(sh), sp_=elen + 5, slen=slen, chunk=chunk, n=NS, eras=None, es=0, neras=None,
            rs=_p(res), pos=None, qs=0, corr=None, cs=0):
        return L_.ezrs_decode_shards(h, sh, sp_, slen, chunk, n, eras, es, neras, rs, pos, qs, corr, cs, sp)

    for f in (enc, dec):
        assert f() == 0
        assert f(h=None) == EINVAL and f(sh=None) == EINVAL
        assert f(chunk=0) == EINVAL and f(chunk=c.load + 1) == EINVAL and f(slen=0) == EINVAL
        assert f(sp_=elen - 1) == EINVAL and f(sp_=elen) == 0
        assert f(n=0) == 0                              # nothing to do, with a valid geometry
        assert f(n=0, sh=None) == EINVAL and f(n=0, chunk=0) == EINVAL    # the geometry comes first
    assert dec(rs=None) == EINVAL and dec(rs=None, n=0) == EINVAL
    assert dec(neras=ax) == EINVAL
    assert dec(eras=ax, es=0, neras=ax) == EINVAL and dec(eras=ax, es=1, neras=ax) == 0
    assert dec(es=5) == 0
    assert dec(pos=ax, qs=nr - 1) == EINVAL and dec(pos=ax, qs=nr) == 0
    assert dec(corr=cp, cs=nr - 1) == EINVAL and dec(corr=cp, cs=nr) == 0
    # one shard of one codeword: the stride rules do not apply
    assert dec(n=1, slen=chunk, eras=ax, es=0, neras=ax, pos=ax, qs=0, corr=cp, cs=0) == 0
    torch.cuda.synchronize()
    assert (res.cpu().numpy() == 0).all()


ENCODE_HOST_NO_PARITY = (b"ezrs_encode_host: parity is required (rows that carry their own parity: "
                         b"ezrs_encode_rows_host)")


def test_argument_rules_host(torch):
    """The host-memory forms keep the device forms' rules (the row-pitch rule of ezrs_decode_host
    with parity == NULL: test_decode_host_row_pitch_rule)."""
    import ezrs
    L_ = ezrs.lib()
    c = ezrs.Codec.rs(255, 223)
    h = c._h
    N, L, nr = 3, 223, 32
    rows = np.zeros((N, L + nr), np.uint8)
    par = np.zeros((N, nr), np.uint8)
    res = np.full(N, 77, np.int32)
    aux = np.zeros((N, nr), np.uint32)
    cor = np.zeros((N, nr), np.uint8)
    enc, encr, dec, enc_t, encr_t, dec_t = _rs_rule_tables(L_, h, L, nr, N, _p(rows), _p(par), _p(res),
                                                           _p(aux), _p(cor), lambda name: (0,),
                                                           decode_rows_rule=False)
    for name, mk, t in (("ezrs_encode_host", enc, enc_t), ("ezrs_encode_rows_host", encr, encr_t),
                        ("ezrs_decode_host", dec, dec_t)):
        f = mk(name)
        _rules(f, **t)
        _rs_common(f, L, c.load)
    f = dec("ezrs_decode_host")
    assert f(ds=L + nr) == 0                            # parity == NULL, rows at their bound
    assert f(neras=_p(aux)) == EINVAL
    assert f(es=5) == 0
    assert f(p=_p(par), ps=0, ds=0, n=1) == 0
    assert f(p=_p(par), ps=nr, ds=L - 1) == EINVAL and f(p=_p(par), ps=nr, ds=L) == 0
    assert (res == 0).all() and not rows.any() and not par.any()
    f = enc("ezrs_encode_host")
    assert f() == 0
    assert f(p=None) == EINVAL
    assert L_.ezrs_last_error() == ENCODE_HOST_NO_PARITY


def test_argument_rules_bch(torch):
    """ezbch_* on BCH(255,239,2), three rows of 20 data bytes."""
    import ezrs
    L_ = ezrs.lib()
    b = ezrs.BCH.nkt(255, 239, 2)
    h, sp = b._h, ezrs._stream_ptr(None)
    N, L, eb, t = 3, 20, b.ecc_bytes, b.t
    assert (eb, t) == (2, 2)
    S = L + eb

    def tables(dp, ep, rp, lp, yp, tail):
        """(closure, rule table) per form of one flavour; tail: the trailing arguments."""
        def enc(name):
            def f(h=h, d=dp, ds=S, L=L, e=ep, es=eb, n=N):
                return getattr(L_, name)(h, d, ds, L, e, es, n, *tail(name))
            return f

        def encr(name):
            def f(h=h, d=dp, ds=S, L=L, n=N):
                return getattr(L_, name)(h, d, ds, L, n, *tail(name))
            return f

        def dec(name):
            def f(h=h, d=dp, ds=S, L=L, e=None, es=0, rs=rp, loc=None, ls=0, n=N):
                return getattr(L_, name)(h, d, ds, L, e, es, rs, loc, ls, n, *tail(name))
            return f

        def dec1(name, src, bound):                     # the ECC-difference and syndrome forms
            def f(h=h, s=src, ss=bound, L=L, rs=rp, loc=None, ls=0, n=N):
                return getattr(L_, name)(h, s, ss, L, rs, loc, ls, n, *tail(name))
            return f

        return {
            "encode": (enc, dict(nulls=["d", "e"], bounds={"ds": L, "es": eb}, one=dict(n=1, ds=0, es=0),
                                 zero=dict(n=0, d=None, e=None, ds=0, es=0))),
            "encode_rows": (encr, dict(nulls=["d"], bounds={"ds": S}, one=dict(n=1, ds=0),
                                       zero=dict(n=0, d=None, ds=0))),
            "decode": (dec, dict(nulls=["d", "rs"],
                                 bounds={"ds": S, "es": (eb, dict(e=ep, ds=L)), "ls": (t, dict(loc=lp))},
                                 one=dict(n=1, ds=0, loc=lp, ls=0), zero=dict(n=0, d=None, rs=None, ds=0))),
            "decode_ecc": (lambda name: dec1(name, ep, eb),
                           dict(nulls=["s", "rs"], bounds={"ss": eb, "ls": (t, dict(loc=lp))},
                                one=dict(n=1, ss=0, loc=lp, ls=0), zero=dict(n=0, s=None, rs=None, ss=0))),
            "decode_syn": (lambda name: dec1(name, yp, 2 * t),
                           dict(nulls=["s", "rs"], bounds={"ss": 2 * t, "ls": (t, dict(loc=lp))},
                                one=dict(n=1, ss=0, loc=lp, ls=0), zero=dict(n=0, s=None, rs=None, ss=0))),
        }

    rows = torch.zeros((N, S), dtype=torch.uint8, device="cuda")           # all-zero rows are codewords
    ecc = torch.zeros((N, eb), dtype=torch.uint8, device="cuda")
    res = torch.full((N,), 77, dtype=torch.int32, device="cuda")
    loc = torch.zeros((N, t), dtype=torch.int32, device="cuda")
    syn = torch.zeros((N, 2 * t), dtype=torch.int32, device="cuda")
    T = tables(_p(rows), _p(ecc), _p(res), _p(loc), _p(syn), lambda name: (sp,))
    for form in ("encode", "encode_rows", "decode", "decode_ecc", "decode_syn"):
        mk, t_ = T[form]
        _rules(mk("ezbch_" + form), **t_)
    torch.cuda.synchronize()
    assert (res.cpu().numpy() == 0).all()
    hrows, hecc = np.zeros((N, S), np.uint8), np.zeros((N, eb), np.uint8)
    hres, hloc = np.full(N, 77, np.int32), np.zeros((N, t), np.uint32)
    hsyn = np.zeros((N, 2 * t), np.uint32)
    T = tables(_p(hrows), _p(hecc), _p(hres), _p(hloc), _p(hsyn),
               lambda name: () if name == "ezbch_decode_syn_host" else (0,))
    for form in ("encode", "encode_rows", "decode", "decode_syn"):
        mk, t_ = T[form]
        _rules(mk(f"ezbch_{form}_host"), **t_)
    assert (hres == 0).all() and not hrows.any() and not hecc.any()


# ---- 3. ezrs_decode_host and the row pitch ----------------------------------------------------------
def test_decode_host_row_pitch_rule(torch):
    """parity == NULL says that every row carries its parity, so rows of more than one codeword
    are at least len + NROOTS apart: ezrs_decode refuses a smaller pitch with -EINVAL, and the host
    form, which has the same contract with host pointers, refuses it too and touches nothing."""
    import ezrs
    L_ = ezrs.lib()
    c = ezrs.Codec.rs(255, 223)
    h, sp = c._h, ezrs._stream_ptr(None)
    N, L, nr, FILL = 3, 223, 32, 0xC3
    res = np.full(N, 77, np.int32)
    dres = torch.full((N,), 77, dtype=torch.int32, device="cuda")
    dbuf = torch.zeros(N * (L + nr), dtype=torch.uint8, device="cuda")
    assert L_.ezrs_decode(h, _p(dbuf), L + 1, L, None, 0, None, 0, None, _p(dres), None, 0, None, 0, N,
                          sp) == EINVAL
    # the caller's array: exactly N * (L + 1) bytes inside a larger buffer
    guard = 4096
    buf = np.full(guard + N * (L + 1) + guard, FILL, np.uint8)
    arr = buf[guard:guard + N * (L + 1)]
    arr[:] = np.random.default_rng(3).integers(0, 256, arr.size)
    before = buf.copy()
    assert L_.ezrs_decode_host(h, _p(arr), L + 1, L, None, 0, None, 0, None, _p(res), None, 0, None, 0, N,
                               0) == EINVAL
    np.testing.assert_array_equal(buf, before)
    assert (res == 77).all()
    ok = np.zeros((N, L + nr), np.uint8)
    assert L_.ezrs_decode_host(h, _p(ok), L + nr, L, None, 0, None, 0, None, _p(res), None, 0, None, 0, N,
                               0) == 0
    assert (res == 0).all() and not ok.any()
    torch.cuda.synchronize()

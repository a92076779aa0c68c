"""One case generator for the tests of the per-codeword RS kernels (ezrs_generic.hip) and of the
fallback decodes: tests/test_generic_cases_oracle.py (CPU: the oracle alone shows that every batch
holds what the GPU tests rely on) and tests/test_generic_gpu.py (the kernels against the oracle).

A batch follows the input shape of test_wide_vs_oracle -- loads from 0 to 1.5x the capacity, a
random prefix of the corrupted positions flagged as erasures, every fifth row lightly loaded -- and
adds, by row index modulo 11, one row kind each of the erasure lists and error patterns that the
reference treats specially (KINDS), and on masked codecs (symbol narrower than the datum) junk in
the bits above the symbol.  Everything here is plain numpy; the arrays of a case are shared between
tests and are read-only."""
import functools
import types

import numpy as np

import oracle as O

# row kinds, by i % 11 (every other residue: RANDOM)
RANDOM, CLEAN_ERASURE, REPEATED_ERASURE, ERASURE_OUT_OF_RANGE, TOO_MANY_ERASURES, FIRST_LAST, \
    PARITY_ONLY = range(7)
KIND_OF_RESIDUE = {1: CLEAN_ERASURE, 2: REPEATED_ERASURE, 3: ERASURE_OUT_OF_RANGE,
                   4: TOO_MANY_ERASURES, 6: FIRST_LAST, 7: PARITY_ONLY}
KINDS = {CLEAN_ERASURE: "an erasure on a clean symbol",
         REPEATED_ERASURE: "a repeated erasure position",
         ERASURE_OUT_OF_RANGE: "an erasure equal to L + nroots",
         TOO_MANY_ERASURES: "neras = nroots + 1",
         FIRST_LAST: "erasures only on the first and last symbol",
         PARITY_ONLY: "errors only in the parity"}
PARITY_JUNK_EVERY = 13          # masked codecs: rows i % 13 == 12 carry junk in one parity element
MAX_CORR_ROWS = 24              # rows that also go through the single-codeword oracle (corr)
ENC_SPLIT_DATA_EXTRA, ENC_SPLIT_PARITY_EXTRA = 7, 3     # split encode: data pitch L + 7, parity nroots + 3
DEC_SPLIT_DATA_EXTRA, DEC_SPLIT_PARITY_EXTRA = 5, 3     # split decode: data pitch L + 5, parity nroots + 3
ORACLE_THREADS = 8


def fill_of(dtype):
    """The sentinel of padding columns and of untouched output entries (test_capi_forms_gpu's)."""
    return 0xA5 if np.dtype(dtype).itemsize == 1 else 0x2A5


def _frozen(ns):
    for v in vars(ns).values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return ns


def _corr_rows(ncw, kind):
    """At most MAX_CORR_ROWS rows spread over the batch: the first and the last row, one row on each
    side of every 64-row boundary, then the first row of each fixed kind, then evenly spaced rows."""
    rows = [0, ncw - 1]
    for b in range(64, ncw, 64):
        rows += [b - 1, b]
    for kd in (PARITY_ONLY, CLEAN_ERASURE, REPEATED_ERASURE, FIRST_LAST, ERASURE_OUT_OF_RANGE,
               TOO_MANY_ERASURES):
        hit = np.nonzero(kind == kd)[0]
        if len(hit):
            rows.append(int(hit[0]))
    rows += [int(x) for x in np.linspace(0, ncw - 1, MAX_CORR_ROWS)]
    out = []
    for r in rows:
        if r not in out and len(out) < MAX_CORR_ROWS:
            out.append(r)
    return np.array(sorted(out))


@functools.lru_cache(maxsize=None)
def _batch(params, L, ncw, seed):
    """The batch as packed rows [ncw, L + nroots], with the oracle's verdict on it."""
    mm, poly, fcr, prim, nr, dual = params
    oc = O.Codec(*params)
    nn, dt = oc.nn, oc.dtype
    bits = 8 * np.dtype(dt).itemsize
    masked = mm != bits
    S = L + nr
    fill = fill_of(dt)
    rng = np.random.default_rng(seed)

    def junk(size=None):            # nonzero bits above the symbol
        return (rng.integers(1, 1 << (bits - mm), size) << mm).astype(dt)

    clean = rng.integers(0, nn + 1, (ncw, S)).astype(dt)
    if masked:                      # every data element; encode must mask it and leave it in place
        clean[:, :L] |= junk((ncw, L))
    clean[:, L:] = fill
    enc_in = clean.copy()
    assert oc.encode_batch(clean, L) == 0

    cw = clean.copy()
    eras = np.zeros((ncw, nr + 1), np.uint32)
    neras = np.zeros(ncw, np.uint32)
    kind = np.array([KIND_OF_RESIDUE.get(i % 11, RANDOM) for i in range(ncw)])
    nerr = np.zeros(ncw, np.int64)
    pjunk = np.zeros(ncw, bool)
    for i in range(ncw):
        kd = kind[i]
        m = int(rng.integers(0, 3 * nr // 2 + 1)) if i % 5 else int(rng.integers(0, 3))
        m = min(m, S)
        if kd == CLEAN_ERASURE:
            m = min(m, S - 1)
        elif kd == REPEATED_ERASURE:
            m = max(m, 1)
        elif kd == FIRST_LAST:
            m = 2
        elif kd == PARITY_ONLY:
            m = int(rng.integers(1, max(nr // 2, 1) + 1))
        if kd == FIRST_LAST:
            locs = np.array([0, S - 1])
        elif kd == PARITY_ONLY:
            locs = L + rng.choice(nr, m, replace=False)
        else:
            locs = rng.choice(S, m, replace=False)
        cw[i, locs] ^= rng.integers(1, nn + 1, m).astype(dt)
        nerr[i] = m
        ne = min(int(rng.integers(0, m + 1)), nr)
        eras[i, :ne] = locs[:ne]
        if kd == CLEAN_ERASURE:
            ne = min(ne, nr - 1)
            eras[i, ne] = rng.choice(np.setdiff1d(np.arange(S), locs))
            ne += 1
        elif kd == REPEATED_ERASURE:
            ne = min(max(ne, 1), nr - 1)
            eras[i, :ne] = locs[:ne]
            eras[i, ne] = eras[i, rng.integers(0, ne)]
            ne += 1
        elif kd == ERASURE_OUT_OF_RANGE:
            ne = min(ne, nr - 1)
            at = int(rng.integers(0, ne + 1))
            eras[i, ne] = eras[i, at]
            eras[i, at] = S
            ne += 1
        elif kd == TOO_MANY_ERASURES:
            ne = nr + 1
            eras[i, :ne] = rng.choice(S, ne, replace=False)
        elif kd == FIRST_LAST:
            ne = 2
            eras[i, :2] = locs
        elif kd == PARITY_ONLY:
            ne = 0
        eras[i, ne:] = 0
        neras[i] = ne
        if masked and i % PARITY_JUNK_EVERY == PARITY_JUNK_EVERY - 1:
            cw[i, L + int(rng.integers(0, nr))] |= junk()
            pjunk[i] = True

    exp = cw.copy()
    pos = np.zeros((ncw, nr), np.uint32)
    res = oc.decode_batch(exp, L, None, eras, neras, pos, nthreads=ORACLE_THREADS)
    # correction values: the single-codeword oracle (the batch form has none) on a few rows
    corr_rows = _corr_rows(ncw, kind)
    corr = np.full((ncw, nr), fill, dt)
    for k in corr_rows:
        d, p = cw[k, :L].copy(), cw[k, L:].copy()
        r, ps = oc.decode(d, p, eras[k, :neras[k]].tolist(), corr[k])
        assert r == res[k] and list(ps) == list(pos[k, :max(r, 0)])
        assert np.array_equal(np.concatenate([d, p]), exp[k])
    return _frozen(types.SimpleNamespace(
        params=params, L=L, ncw=ncw, seed=seed, nr=nr, S=S, nn=nn, mm=mm, dtype=dt, bits=bits,
        masked=masked, fill=fill, clean=clean, enc_in=enc_in, cw=cw, eras=eras, neras=neras,
        kind=kind, nerr=nerr, pjunk=pjunk, exp=exp, res=res, pos=pos, corr_rows=corr_rows, corr=corr))


def _spread(rows, pitch, fill):
    out = np.full((rows.shape[0], pitch), fill, rows.dtype)
    out[:, :rows.shape[1]] = rows
    return out


@functools.lru_cache(maxsize=None)
def make_case(params, L, ncw, seed, pitch_extra=0, split=False):
    """The batch of (params, L, ncw, seed) -- the same rows whatever the layout -- laid out as rows
    that carry their parity at pitch L + nroots + pitch_extra, or (split) as data rows at pitch
    L + 5 and parity rows at pitch nroots + 3, with the oracle's decode of that layout.

    Fields (b = the packed batch, all of whose fields are here too):
      enc_in, enc         encode input (parity columns hold the sentinel) and the oracle's output
      enc_data, enc_par   the split encode: data at pitch L + 7, the oracle's parity nroots + 3 wide
      cw / data, par      the corrupted rows, inline / split
      exp / exp_data, exp_par, res, pos   oracle.decode_batch of that layout
      eras, neras         [ncw, nroots + 1], [ncw]
      corr_rows, corr     rows decoded by the single-codeword oracle too, and their corr
      kind, nerr, pjunk   per row: its kind, its corrupted symbols, junk in a parity element"""
    b = _batch(params, L, ncw, seed)
    oc = O.Codec(*params)
    nr, fill = b.nr, b.fill
    c = types.SimpleNamespace(**vars(b))
    c.packed = b
    c.split = split
    c.pitch = L + nr + pitch_extra
    c.enc_in = _spread(b.enc_in, c.pitch, fill)
    c.enc = c.enc_in.copy()
    assert oc.encode_batch(c.enc, L) == 0
    c.enc_data = _spread(b.enc_in[:, :L], L + ENC_SPLIT_DATA_EXTRA, fill)
    c.enc_par = np.full((ncw, nr + ENC_SPLIT_PARITY_EXTRA), fill, b.dtype)
    assert oc.encode_batch(c.enc_data, L, c.enc_par) == 0
    c.pos = np.zeros((ncw, nr), np.uint32)
    if split:
        c.data = _spread(b.cw[:, :L], L + DEC_SPLIT_DATA_EXTRA, fill)
        c.par = _spread(b.cw[:, L:], nr + DEC_SPLIT_PARITY_EXTRA, fill)
        c.exp_data, c.exp_par = c.data.copy(), c.par.copy()
        c.res = oc.decode_batch(c.exp_data, L, c.exp_par, b.eras, b.neras, c.pos,
                                nthreads=ORACLE_THREADS)
        c.cw = c.exp = None
    else:
        c.cw = _spread(b.cw, c.pitch, fill)
        c.exp = c.cw.copy()
        c.res = oc.decode_batch(c.exp, L, None, b.eras, b.neras, c.pos, nthreads=ORACLE_THREADS)
    return _frozen(c)


def logical_rows(c, rows=None, data=None, par=None):
    """The [ncw, L + nroots] symbols of a laid-out batch (inline rows, or split data and parity)."""
    if rows is not None:
        return rows[:, :c.S]
    return np.concatenate([data[:, :c.L], par[:, :c.nr]], axis=1)


def check_result_mix(c, res, rows_after):
    """What a decoded batch must show for the comparison with the oracle to have teeth; `res` and
    `rows_after` ([ncw, L + nroots], see logical_rows) are the oracle's or the GPU's.  Raises
    AssertionError naming the condition.  Batches of fewer than 22 rows (a lone lane) hold neither
    every row kind nor the three result classes and are exempt from those two conditions."""
    b = c.packed
    before = b.cw
    assert res.shape == (c.ncw,) and rows_after.shape == before.shape
    failed = res == -1
    changed = (rows_after != before).any(axis=1)
    if c.ncw >= 22:
        assert (res == 0).any() and (res > 0).any() and failed.any(), "three result classes"
        for kd, name in KINDS.items():
            assert (b.kind == kd).any(), name
        assert (b.neras[b.kind == TOO_MANY_ERASURES] == c.nr + 1).all()
        assert (res[(b.kind == ERASURE_OUT_OF_RANGE) | (b.kind == TOO_MANY_ERASURES)] == -1).all()
    if b.masked:
        assert not (changed & failed).any(), "masked: a failed row is left alone"
        himask = ~np.array(b.nn, b.dtype)
        assert np.array_equal(rows_after[:, :c.L] & himask, before[:, :c.L] & himask), "data junk bits"
        assert (before[:, :c.L] & himask).all(), "every data element carries junk"
        assert (res[b.pjunk] == -1).all(), "parity junk gives -1"
        if c.ncw >= PARITY_JUNK_EVERY:
            assert b.pjunk.any()
    elif c.L == b.nn - c.nr:
        # a full-length codeword has no pad, and the locator's roots are distinct, so neither of the
        # two failures that follow a correction (a root in the pad, a zero denominator:
        # rs_base:1625-1648) can happen: every -1 comes before the first fix
        assert not (changed & failed).any(), "direct, full length: no fix before a failure"
    elif c.ncw >= 22:
        assert (changed & failed).any(), "direct: a partial fix kept on failure"
    if c.ncw > 64:
        assert (res[64:] != 0).any(), "a nonzero result beyond row 64"
    if c.ncw > 256:
        assert (res[256:] != 0).any(), "a nonzero result beyond row 256"
    light = (b.kind == RANDOM) & (b.neras == 0) & ~b.pjunk & (b.nerr <= c.nr // 2)
    assert np.array_equal(res[light], b.nerr[light]), "rows within capacity: result = error count"
    assert np.array_equal(rows_after[light], b.clean[light]), "rows within capacity: restored"


# ---- the matrices -----------------------------------------------------------------------------------
def _rs(n, k):
    return O.rs_params(n, k)


# The seed of a case is the first one (from 1) with which the batch meets check_result_mix under the
# oracle.  A direct-datum codec at full length cannot show a partial fix (see check_result_mix), so
# each such case has a shortened companion (_lenNN) that does.
#
# Matrix A: codecs whose own path is the per-codeword kernels.  (id, params, L, ncw, seed)
MATRIX_A = [
    ("rs3_1", _rs(3, 1), 1, 65, 1),                                # u8/32, smallest field, NROOTS 2
    ("rs7_5", _rs(7, 5), 3, 300, 1),                               # u8/32 masked
    ("rs15_11", _rs(15, 11), 11, 300, 1),                          # u8/32 masked
    ("rs31_19_len12", _rs(31, 19), 12, 129, 1),                    # u8/32 masked, shortened
    ("rs31_19_full", _rs(31, 19), 19, 129, 1),                     # ... and full
    ("rs31_19_lone", _rs(31, 19), 12, 1, 1),                       # a lone lane
    ("rs31_19_block", _rs(31, 19), 12, 64, 1),                     # an exactly full decode block
    ("rs127_63", _rs(127, 63), 50, 257, 1),                        # u8/256 masked, NROOTS 64
    ("rs255_245", _rs(255, 245), 200, 300, 1),                     # u8/32, outside the plane-sliced list
    ("rs255_245_lone", _rs(255, 245), 200, 1, 1),
    ("rs255_245_block", _rs(255, 245), 200, 64, 1),
    ("rs255_224_nroots31", _rs(255, 224), 224, 65, 1),             # u8/32, top of wmask
    ("rs255_224_nroots31_len100", _rs(255, 224), 100, 65, 1),      # ... shortened: partial fixes
    ("rs255_222_nroots33", _rs(255, 222), 222, 257, 1),            # u8/256, first above the template boundary
    ("rs255_222_nroots33_len100", _rs(255, 222), 100, 257, 2),     # ... shortened: partial fixes
    ("fcr0", (8, 0x11d, 0, 1, 8, False), 100, 300, 1),             # fcr = 0
    ("dual_0x187_nroots16", (8, 0x187, 120, 11, 16, True), 100, 300, 1),   # dual basis, per-codeword kernel
    ("rs511_479", _rs(511, 479), 479, 70, 1),                      # lanes, LDS tables, masked
    ("rs4095_4063", _rs(4095, 4063), 1000, 70, 1),                 # lanes, nn = 4095 (last LDS size), masked
    ("rs8191_8159", _rs(8191, 8159), 700, 70, 1),                  # lanes, global tables, masked
    ("rs32767_32727_nroots40", _rs(32767, 32727), 300, 70, 1),     # u16/256 masked, global tables
    ("rs1023_959_nroots64", _rs(1023, 959), 959, 100, 1),          # u16/256, LDS tables
    ("rs65535_65471_nroots64", _rs(65535, 65471), 300, 70, 2),     # u16/256, global tables
    ("rs65535_65279_nroots256", _rs(65535, 65279), 300, 40, 1),    # u16/256 at the engine's NROOTS limit
]
A_PITCH_EXTRA = 3

# Matrix B: fast codecs pushed onto the fallbacks by the geometry of the call.
# (id, params, L, ncw, seed, geometry, kernel_path); geometry: "split", or the pitch of inline rows
MATRIX_B = [
    ("rs255_223_full_split", _rs(255, 223), 223, 600, 1, "split", "planeslice"),
    ("rs255_223_len100_split", _rs(255, 223), 100, 600, 1, "split", "planeslice"),
    ("rs255_223_len191_pitch300", _rs(255, 223), 191, 600, 2, 300, "planeslice"),
    ("rs255_247_len200_pitch300", _rs(255, 247), 200, 600, 1, 300, "planeslice"),
    ("ccsds223_dual_split", O.ccsds_params(223, True), 223, 600, 1, "split", "bitslice"),
    ("ccsds223_dual_pitch300", O.ccsds_params(223, True), 223, 600, 1, 300, "bitslice"),
    ("ccsds223_dual_len100_split", O.ccsds_params(223, True), 100, 600, 1, "split", "bitslice"),
    ("ccsds239_conv_split", O.ccsds_params(239, False), 239, 600, 1, "split", "planeslice"),
    ("ccsds239_conv_len100_split", O.ccsds_params(239, False), 100, 600, 1, "split", "planeslice"),
    ("rs255_128_nroots127_split", _rs(255, 128), 128, 600, 1, "split", "generic"),
    ("rs255_128_nroots127_len60_split", _rs(255, 128), 60, 600, 1, "split", "generic"),
    ("rs65535_65503_len700_split", _rs(65535, 65503), 700, 130, 1, "split", "wide"),
]


def case_a(entry, split):
    _, params, L, ncw, seed = entry
    return make_case(params, L, ncw, seed, A_PITCH_EXTRA, split)


def case_b(entry, fast):
    """The fallback geometry of a matrix B entry, or (fast) the same batch as packed inline rows."""
    _, params, L, ncw, seed, geom, _ = entry
    if fast:
        return make_case(params, L, ncw, seed, 0, False)
    if geom == "split":
        return make_case(params, L, ncw, seed, 0, True)
    return make_case(params, L, ncw, seed, geom - (L + params[4]), False)

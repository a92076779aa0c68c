"""Geometry sweep of the plane-sliced BCH tile path (ezbch_ps_tile.hpp: k_bch_ps, k_bch_ps_decode)
against the oracle, for both plane-sliced codecs: row lengths from one byte to the frame, row pitches
packed, with a gap, 16-aligned, at the path's limit (128) and one past it (129, the fallback
kernels), bases at byte offsets 0, 1 and 15 of a larger random-filled buffer, batches of one short
row up to two tiles and a row, separate ECC arrays at pitches up to 4096 and one past it.  Every
comparison is of the whole buffer: the bytes before the base, the gaps between a row's end and the
pitch, and the tail must come back as they went in."""
import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

# (m, t), ecc_bytes, frame bytes, row lengths
PS = {(10, 4): (5, 128, (1, 2, 11, 16, 59, 121, 122)),
      (8, 2): (2, 32, (1, 2, 13, 14, 29))}
CASES = [(m, t, L) for (m, t), (_, _, Ls) in PS.items() for L in Ls]
IDS = [f"m{m}t{t}-L{L}" for m, t, L in CASES]
OFFSETS = (0, 1, 15)
NCW = (1, 3, 255, 256, 257, 513)            # a tile is 256 rows
TAIL = 37


@pytest.fixture(scope="module")
def torch():
    import torch as T
    if not T.cuda.is_available():
        pytest.skip("no GPU")
    return T


@pytest.fixture(scope="module")
def codecs(torch):
    import ezrs
    return {mt: (O.BCH(*mt), ezrs.BCH(*mt)) for mt in PS}


def pitches(L, eb):
    """(kind, pitch): packed, one byte of gap, the next multiple of 16, the plane-sliced path's
    widest, and the first pitch of the fallback kernels."""
    return [("packed", L + eb), ("gap1", L + eb + 1), ("al16", (L + eb + 15) // 16 * 16),
            ("128", 128), ("129", 129)]


def test_sweep_reaches_every_span_end():
    """The span of a launch ends at (ncw - 1) pitch + L (encode) or + L + ecc_bytes (decode) bytes
    from its base; the sweep below must put that end at residues 0 (no 16-byte piece crosses it), 1
    and 15 mod 16, and unaligned ends both past 64 bytes and below (a re-read window that starts
    before the base), for both codecs and both kernels."""
    for (m, t), (eb, frame, Ls) in PS.items():
        for extra in (0, eb):
            spans = {(n - 1) * p + L + extra for L in Ls for _, p in pitches(L, eb) if p <= 128
                     for n in NCW}
            assert {0, 1, 15} <= {s % 16 for s in spans}, (m, t, extra)
            assert any(s < 64 and s % 16 for s in spans) and any(s >= 64 and s % 16 for s in spans)
        assert max(Ls) + eb <= frame and frame <= 128


def layout(rng, off, ncw, pitch):
    """A random-filled flat buffer with room for ncw rows of `pitch` bytes at byte offset off and a
    tail, and its [ncw, pitch] view (numpy: contiguous, so the oracle's batch calls take it)."""
    buf = rng.integers(0, 256, off + ncw * pitch + TAIL, dtype=np.uint8)
    return buf, lambda b: b[off:off + ncw * pitch].reshape(ncw, pitch)


def dev_rows(torch, buf, off, ncw, width, pitch):
    flat = torch.from_numpy(buf).cuda()
    return flat, flat.as_strided((ncw, width), (pitch, 1), off)


@pytest.mark.parametrize("m,t,L", CASES, ids=IDS)
def test_encode_inline(torch, codecs, m, t, L):
    """Rows with the ECC inline at every (pitch kind, base offset, ncw): the whole buffer equals
    the input with only the oracle's ECC columns replaced."""
    oc, c = codecs[m, t]
    eb = PS[m, t][0]
    rng = np.random.default_rng(1000 * m + L)
    for kind, pitch in pitches(L, eb):
        for off in OFFSETS:
            for ncw in NCW:
                buf, rows = layout(rng, off, ncw, pitch)
                exp = buf.copy()
                oc.encode_batch(rows(exp), L)
                flat, view = dev_rows(torch, buf, off, ncw, L + eb, pitch)
                c.encode(view, L)
                np.testing.assert_array_equal(flat.cpu().numpy(), exp,
                                              err_msg=f"pitch {kind}={pitch} off={off} ncw={ncw}")


@pytest.mark.parametrize("m,t,L", CASES, ids=IDS)
def test_encode_separate_ecc(torch, codecs, m, t, L):
    """The ECC into its own array, pre-filled with random bytes, at every (ECC pitch, ECC base
    offset, ncw), the data pitch and base offset cycling through theirs: only the ecc_bytes of each
    row change, and the data buffer not at all.  ECC pitch 4097 is the first of the fallback."""
    oc, c = codecs[m, t]
    eb = PS[m, t][0]
    rng = np.random.default_rng(2000 * m + L)
    dpitches = [L, L + 1, (L + 15) // 16 * 16, 128, 129]
    i = 0
    for epitch in (eb, eb + 1, 8, 4096, 4097):
        for eoff in (0, 3):
            for ncw in NCW:
                pitch, off = dpitches[i % 5], OFFSETS[(i // 5) % 3]
                i += 1
                buf, rows = layout(rng, off, ncw, pitch)
                ebuf, erows = layout(rng, eoff, ncw, epitch)
                exp = ebuf.copy()
                oc.encode_batch(rows(buf), L, erows(exp))
                flat, view = dev_rows(torch, buf, off, ncw, L, pitch)
                eflat, eview = dev_rows(torch, ebuf, eoff, ncw, eb, epitch)
                c.encode(view, L, ecc=eview)
                what = f"epitch={epitch} eoff={eoff} ncw={ncw} pitch={pitch} off={off}"
                np.testing.assert_array_equal(eflat.cpu().numpy(), exp, err_msg="ecc: " + what)
                np.testing.assert_array_equal(flat.cpu().numpy(), buf, err_msg="data: " + what)


def corrupt(rows, L, eb, t, rng, turn):
    """Flip bits of the codewords in rows[:, :L + eb]: row 0, the batch's last row (in its final 16
    bytes and in its ECC), rows 255 and 256 and a random quarter of the others get 1 .. t + 1 flips
    (every count comes up as `turn` advances), the first of them in the row's first byte and the
    second in its last ECC byte."""
    ncw, nbits = len(rows), 8 * (L + eb)                    # ecc_bits = 8 ecc_bytes for both codecs
    counts = np.zeros(ncw, np.int64)
    sel = rng.random(ncw) < 0.25
    counts[sel] = rng.integers(1, t + 2, int(sel.sum()))
    for j, k in enumerate(dict.fromkeys(k for k in (0, ncw - 1, 255, 256) if k < ncw)):
        counts[k] = 1 + (turn + j) % (t + 1)
    for k in np.nonzero(counts)[0]:
        lo = max(0, nbits - 128) if k == ncw - 1 else 0
        pos = [int(rng.integers(lo, lo + 8)), int(rng.integers(nbits - 8, nbits))]
        if k == ncw - 1:
            pos.append(int(rng.integers(8 * L, nbits)))     # the last row's ECC
        pos = list(dict.fromkeys(pos))[:counts[k]]
        rest = [p for p in (lo + rng.permutation(nbits - lo)).tolist() if p not in pos]
        for p in pos + rest[:counts[k] - len(pos)]:
            rows[k, p >> 3] ^= 0x80 >> (p & 7)
    return counts


@pytest.mark.parametrize("m,t,L", CASES, ids=IDS)
def test_decode_inline(torch, codecs, m, t, L):
    """Decode of rows with the ECC inline (packed rows: the fused kernel; other pitches: the lane
    kernel) with 0 .. t and t + 1 flips per row: results, locations and the whole buffer equal the
    oracle applied to the row slices; gaps, head and tail untouched."""
    oc, c = codecs[m, t]
    eb = PS[m, t][0]
    rng = np.random.default_rng(3000 * m + L)
    turn = 0
    for kind, pitch in pitches(L, eb):
        for off in OFFSETS:
            for ncw in NCW:
                buf, rows = layout(rng, off, ncw, pitch)
                oc.encode_batch(rows(buf), L)
                counts = corrupt(rows(buf), L, eb, t, rng, turn)
                turn += 1
                exp = buf.copy()
                eloc = np.zeros((ncw, t), np.uint32)
                eres = oc.decode_batch(rows(exp), L, errloc=eloc)
                assert (eres[counts <= t] == counts[counts <= t]).all()
                flat, view = dev_rows(torch, buf, off, ncw, L + eb, pitch)
                loc = torch.zeros((ncw, t), dtype=torch.int32, device="cuda")
                res = c.decode(view, L, errloc=loc).cpu().numpy()
                what = f"pitch {kind}={pitch} off={off} ncw={ncw}"
                np.testing.assert_array_equal(res, eres, err_msg="result: " + what)
                np.testing.assert_array_equal(flat.cpu().numpy(), exp, err_msg="buffer: " + what)
                got = loc.cpu().numpy().view(np.uint32)
                for k in np.nonzero(eres > 0)[0]:
                    np.testing.assert_array_equal(got[k, :eres[k]], eloc[k, :eres[k]],
                                                  err_msg=f"locations of row {k}: " + what)


# ---- the lane kernels' staged-image write-back (k_bch_decode<T, NW> with lds_fix) ----------------
# codecs without a plane-sliced path: (m, t) -> T, NW, where the field tables are, how locate is built
LANE = {(12, 5): "T=5 NW=1, tables in LDS, locate inline",
        (13, 8): "T=8 NW=2, tables in global memory, locate out of line"}
LANE_LS = (1, 11, 59)
LANE_NCW = (2, 63, 64, 65, 255, 256, 257, 513)      # a wave is 64 rows, a block 256
LANE_CASES = [(m, t, L) for (m, t) in LANE for L in LANE_LS]


@pytest.fixture(scope="module")
def lane_codecs(torch):
    import ezrs
    return {mt: (O.BCH(*mt), ezrs.BCH(*mt)) for mt in LANE}


def lane_flips(rows, L, oc, rng):
    """Row k gets k mod (t + 2) flips, 0 .. t + 1; the first and the last row of every 64-row wave
    get t.  All in the codeword's 8 L + ecc_bits bits, the first in the row's first byte and the
    second in its last ECC byte that holds code bits, so both ends of a row's span are corrected."""
    ncw, t, nbits = len(rows), oc.t, 8 * L + oc.ecc_bits
    counts = np.arange(ncw) % (t + 2)
    counts[0::64] = t
    counts[63::64] = t
    counts[ncw - 1] = t
    for k in np.nonzero(counts)[0]:
        pos = [int(rng.integers(0, 8)), int(rng.integers(nbits - 8, nbits))]
        rest = [p for p in rng.permutation(nbits).tolist() if p not in pos]
        for p in (pos + rest)[:counts[k]]:
            rows[k, p >> 3] ^= 0x80 >> (p & 7)
    return counts


@pytest.mark.parametrize("m,t,L", LANE_CASES, ids=[f"m{m}t{t}-L{L}" for m, t, L in LANE_CASES])
def test_lane_decode_packed_rows_at_odd_offset(torch, lane_codecs, m, t, L):
    """Packed rows with inline ECC through the lane kernels, which correct in the block's staged
    LDS image and write back the 16-byte pieces that hold flips: bases at byte offsets 0, 1 and 15,
    batches around the wave (64 rows) and block (256 rows) sizes, 0 .. t + 1 flips per row.  Result,
    error locations and the whole flat buffer (the bytes before the base and the tail included)
    equal the oracle's.
    The rows are staged, so that write-back runs, while rows_offset + 256 pitch + 8 <= 65536 bytes
    of LDS, rows_offset = 2048 NW + the field tables when m <= 12 (((3 n + 1) 2 rounded up to 16):
    BCH(12,5), pitch 59 + 8:  2048 + 24576 + 256 * 67 + 8 = 43784;
    BCH(13,8), pitch 59 + 13: 4096 + 256 * 72 + 8 = 22536."""
    oc, c = lane_codecs[m, t]
    eb = oc.ecc_bytes
    nw = (oc.ecc_bits + 63) // 64
    tabs = ((3 * oc.n + 1) * 2 + 15) // 16 * 16 if m <= 12 else 0
    assert 2048 * nw + tabs + 256 * (max(LANE_LS) + eb) + 8 <= 65536
    rng = np.random.default_rng(4000 * m + L)
    pitch = L + eb
    for off in OFFSETS:
        for ncw in LANE_NCW:
            buf, rows = layout(rng, off, ncw, pitch)
            oc.encode_batch(rows(buf), L)
            counts = lane_flips(rows(buf), L, oc, rng)
            exp = buf.copy()
            eloc = np.zeros((ncw, t), np.uint32)
            eres = oc.decode_batch(rows(exp), L, errloc=eloc)
            assert (eres[counts <= t] == counts[counts <= t]).all()
            flat, view = dev_rows(torch, buf, off, ncw, pitch, pitch)
            loc = torch.zeros((ncw, t), dtype=torch.int32, device="cuda")
            res = c.decode(view, L, errloc=loc).cpu().numpy()
            what = f"off={off} ncw={ncw}"
            np.testing.assert_array_equal(res, eres, err_msg="result: " + what)
            np.testing.assert_array_equal(flat.cpu().numpy(), exp, err_msg="buffer: " + what)
            got = loc.cpu().numpy().view(np.uint32)
            for k in np.nonzero(eres > 0)[0]:
                np.testing.assert_array_equal(got[k, :eres[k]], eloc[k, :eres[k]],
                                              err_msg=f"locations of row {k}: " + what)

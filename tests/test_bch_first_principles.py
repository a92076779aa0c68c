"""The BCH restatement (oracle/ezbch_oracle.c) against first principles (bch_first_principles.py),
for every codec of test_bch_gpu.CODECS at L = max_len, max_len // 3 and 1: the generator is the lcm
of the minimal polynomials of alpha .. alpha^2t, the ECC is the remainder of d(x) x^E, the
syndromes are r(alpha^j), at most t flips decode to the one codeword they came from with the flips
reported in ascending order, and beyond t a decode either fails (-74, row untouched) or lands on a
codeword at the distance it reports.  No decoder on the reference side."""
import numpy as np
import pytest

import bch_first_principles as FP
import oracle as O
from test_bch_gpu import CODECS

EBADMSG = 74
IDS = [f"m{m}t{t}" for m, t in CODECS]


@pytest.fixture(scope="module")
def codes():
    cache = {}

    def get(m, t):
        if (m, t) not in cache:
            cache[m, t] = (FP.Code(m, t), O.BCH(m, t))
        return cache[m, t]
    return get


def lengths(fp):
    return sorted({fp.max_len, max(1, fp.max_len // 3), 1})


def codeword(fp, rng, L):
    data = rng.integers(0, 256, L, dtype=np.uint8)
    return np.concatenate([data, np.frombuffer(fp.ecc_of(data), np.uint8)])


def test_helper_knows_the_textbook_codes():
    """The helper itself against published generators: BCH(15,7,2) x^8+x^7+x^6+x^4+1,
    BCH(15,5,3) x^10+x^8+x^5+x^4+x^2+x+1, BCH(31,21,2) octal 3551 (Lin & Costello, table 6.1)."""
    assert FP.genpoly(4, 0x13, 1) == 0b10011
    assert FP.genpoly(4, 0x13, 2) == 0b111010001
    assert FP.genpoly(4, 0x13, 3) == 0b10100110111
    assert FP.genpoly(5, 0x25, 2) == 0o3551
    assert FP.remainder(0b1101 << 3, 0b1011) == 0b001      # x^6 + x^5 + x^3 mod x^3 + x + 1
    assert [FP.reported(p) for p in (0, 7, 8, 13)] == [7, 0, 15, 10]


@pytest.mark.parametrize("m,t", CODECS, ids=IDS)
def test_generator_is_the_lcm_of_minimal_polynomials(codes, m, t):
    fp, oc = codes(m, t)
    assert oc.poly == fp.poly
    g = oc.genpoly()                                        # coefficient of x^j at index j
    assert sum(int(c) << j for j, c in enumerate(g)) == fp.g
    assert fp.g.bit_length() - 1 == oc.ecc_bits == fp.ecc_bits
    assert (oc.n, oc.ecc_bytes, oc.max_len) == (fp.n, fp.ecc_bytes, fp.max_len)


@pytest.mark.parametrize("m,t", CODECS, ids=IDS)
def test_encode_is_the_remainder(codes, m, t):
    fp, oc = codes(m, t)
    rng = np.random.default_rng(77 * m + t)
    for L in lengths(fp):
        rows = [rng.integers(0, 256, L, dtype=np.uint8) for _ in range(2)]
        rows += [np.zeros(L, np.uint8), np.full(L, 255, np.uint8)]
        rows.append(np.zeros(L, np.uint8))
        rows[-1][-1] = 1                                    # d(x) = 1: the ECC is x^E mod g
        for data in rows:
            ecc = fp.ecc_of(data)
            assert oc.encode(data).tobytes() == ecc, f"L={L}"
            assert fp.is_codeword(data.tobytes() + ecc)
            assert int.from_bytes(ecc, "big") & ((1 << fp.pad) - 1) == 0


@pytest.mark.parametrize("m,t", CODECS, ids=IDS)
def test_syndromes_are_evaluations_at_alpha_powers(codes, m, t):
    fp, oc = codes(m, t)
    rng = np.random.default_rng(91 * m + t)
    for i, L in enumerate(lengths(fp)):
        nbits = fp.nbits(L)
        cw = codeword(fp, rng, L)
        assert fp.is_codeword(cw)
        for ne in (1, min(t + 2, nbits)):
            flips = rng.choice(nbits, ne, replace=False)
            bad = cw.copy()
            FP.flip(bad, flips)
            want = fp.syndromes(flips, nbits)
            assert oc.syndromes(bad[:L], bad[L:]).tolist() == want, f"L={L} ne={ne}"
            if i == 0 and ne > 1:
                # once per codec, the whole received word term by term (the shortest length: the
                # linearity shortcut above is what keeps the long ones cheap)
                assert fp.syndromes_of_word(fp.word(bad)) == want
        assert oc.syndromes(cw[:L], cw[L:]).tolist() == [0] * (2 * t)


def forced(nbits, L, ne, rng):
    """ne distinct flip positions, the edges first: bit 0, the last data bit, the first ECC bit and
    the last bit of the word."""
    edge = [0, 8 * L - 1, 8 * L, nbits - 1]
    pos = list(dict.fromkeys(edge))[:ne]
    rest = [p for p in rng.permutation(nbits).tolist() if p not in pos]
    return pos + rest[:ne - len(pos)]


@pytest.mark.parametrize("m,t", CODECS, ids=IDS)
def test_up_to_t_flips_decode_exactly(codes, m, t):
    fp, oc = codes(m, t)
    rng = np.random.default_rng(13 * m + t)
    for L in lengths(fp):
        nbits = fp.nbits(L)
        for ne, edges in ((0, False), (1, False), (1, True), ((t + 1) // 2, True), (t, False), (t, True)):
            cw = codeword(fp, rng, L)
            flips = forced(nbits, L, ne, rng) if edges else rng.choice(nbits, ne, replace=False).tolist()
            if edges and ne == 1:
                flips = [nbits - 1]
            bad = cw.copy()
            FP.flip(bad, flips)
            data, ecc = bad[:L].copy(), bad[L:].copy()
            r, loc = oc.correct(data, ecc)
            assert r == ne, f"L={L} ne={ne}"
            assert np.array_equal(np.concatenate([data, ecc]), cw)
            assert loc.tolist() == sorted(FP.reported(p) for p in flips)


@pytest.mark.parametrize("m,t", CODECS, ids=IDS)
def test_beyond_t_fails_clean_or_lands_on_a_codeword(codes, m, t):
    fp, oc = codes(m, t)
    rng = np.random.default_rng(17 * m + t)
    for L in lengths(fp):
        nbits = fp.nbits(L)
        for ne in sorted({min(t + 1, nbits), min(t + 2, nbits), min(2 * t + 1, nbits)}):
            for _ in range(8):
                bad = codeword(fp, rng, L)
                FP.flip(bad, rng.choice(nbits, ne, replace=False))
                data, ecc = bad[:L].copy(), bad[L:].copy()
                r, loc = oc.correct(data, ecc)
                out = np.concatenate([data, ecc])
                if r < 0:
                    assert r == -EBADMSG
                    assert np.array_equal(out, bad), "a failed decode changed the row"
                else:
                    assert r <= t and len(set(loc.tolist())) == r
                    assert fp.is_codeword(out), f"L={L} ne={ne}: result {r} but not a codeword"
                    assert FP.distance(out, bad) == r

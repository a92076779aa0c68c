"""Binary BCH from first principles, for the tests: Python ints as GF(2) polynomials (bit k = the
coefficient of x^k), small lists as GF(2^m) tables, and no decoder.

A primitive binary BCH code of length n = 2^m - 1 correcting t errors is determined by its field
polynomial: the generator is the lcm of the minimal polynomials of alpha .. alpha^2t, the systematic
ECC of a message is the unique remainder of d(x) x^E by it, and a word within t flips of a codeword
has exactly that codeword as its decode.  Everything here follows from those three statements and
the byte conventions of the codec's interface:

* a row is data || ECC, read MSB first; bit p of the row (p = 0 the MSB of the first data byte) is
  the coefficient of x^(nbits - 1 - p), nbits = 8 len + ecc_bits;
* the ECC is left-justified in ecc_bytes = ceil(m t / 8) big-endian bytes, the 8 ecc_bytes -
  ecc_bits low bits zero;
* an error at bit p is reported as (p & ~7) | (7 - (p & 7)): byte index and LSB-first bit in it.
"""

# init_bch's default field polynomials, m = 5 .. 15
DEFAULT_POLY = {5: 0x25, 6: 0x43, 7: 0x83, 8: 0x11D, 9: 0x211, 10: 0x409, 11: 0x805, 12: 0x1053,
                13: 0x201B, 14: 0x402B, 15: 0x8003}


def field(m, poly):
    """(exp, log) of GF(2^m) = GF(2)[x] / poly by repeated multiplication by x: exp[i] = x^i for
    0 <= i < 2n (doubled, so exp[log a + log b] needs no reduction), log[exp[i]] = i, log[0] = -1."""
    n = (1 << m) - 1
    assert poly >> m == 1, "poly must have degree m"
    exp, log = [0] * (2 * n), [-1] * (n + 1)
    x = 1
    for i in range(n):
        assert log[x] == -1, f"x has order {i} < 2^{m} - 1: {poly:#x} is not primitive"
        exp[i] = exp[i + n] = x
        log[x] = i
        x <<= 1
        if x >> m:
            x ^= poly
    assert x == 1, "x^(2^m - 1) != 1"
    return exp, log


def clmul(a, b):
    """Carry-less product of two GF(2) polynomials."""
    r = 0
    while b:
        low = b & -b
        r ^= a * low                    # a << (index of b's lowest set bit)
        b ^= low
    return r


def remainder(value, g):
    """value mod g over GF(2)."""
    dg = g.bit_length()
    while value.bit_length() >= dg:
        value ^= g << (value.bit_length() - dg)
    return value


def cosets(n, t):
    """The distinct cyclotomic cosets {c, 2c, 4c, ..} mod n of 1 .. 2t, in order of first appearance."""
    out, seen = [], set()
    for c in range(1, 2 * t + 1):
        c %= n
        if c in seen:
            continue
        cs, j = [], c
        while j not in cs:
            cs.append(j)
            j = 2 * j % n
        seen.update(cs)
        out.append(cs)
    return out


def minpoly(exp, log, coset):
    """prod (x - alpha^c) over the coset: a polynomial over GF(2^m) whose coefficients must all land
    in GF(2)."""
    mp = [1]                                                # coefficient of x^k at index k
    for c in coset:
        root, nx = exp[c], [0] * (len(mp) + 1)
        for k, a in enumerate(mp):
            nx[k + 1] ^= a                                  # a x^k * x
            if a:
                nx[k] ^= exp[log[a] + log[root]]            # a x^k * root  (minus = plus)
        mp = nx
    assert all(a in (0, 1) for a in mp), "minimal polynomial with a coefficient outside GF(2)"
    return sum(a << k for k, a in enumerate(mp))


def genpoly(m, poly, t):
    """lcm of the minimal polynomials of alpha^1 .. alpha^2t: the product of the distinct ones."""
    exp, log = field(m, poly)
    g = 1
    for cs in cosets((1 << m) - 1, t):
        g = clmul(g, minpoly(exp, log, cs))
    return g


def reported(p):
    """The location the codec reports for an error at MSB-first bit p of data || ECC."""
    return (p & ~7) | (7 - (p & 7))


class Code:
    """BCH(2^m - 1, ., t) over the default (or a given) field polynomial."""

    def __init__(self, m, t, poly=None):
        self.m, self.t, self.n = m, t, (1 << m) - 1
        self.poly = DEFAULT_POLY[m] if poly is None else poly
        self.exp, self.log = field(m, self.poly)
        self.g = genpoly(m, self.poly, t)
        self.ecc_bits = self.g.bit_length() - 1
        # the interface's ECC field is sized for m t bits (init_bch), even where cosets shared
        # between alpha .. alpha^2t make deg g smaller: ecc_bits = deg g <= m t
        assert self.ecc_bits <= m * t
        self.ecc_bytes = (m * t + 7) // 8
        self.pad = 8 * self.ecc_bytes - self.ecc_bits
        self.max_len = (self.n - self.ecc_bits) // 8

    def nbits(self, length):
        return 8 * length + self.ecc_bits

    def ecc_of(self, data):
        """ECC bytes of the data bytes: (data << ecc_bits) mod g, left-justified, big-endian."""
        r = remainder(int.from_bytes(bytes(data), "big") << self.ecc_bits, self.g)
        return (r << self.pad).to_bytes(self.ecc_bytes, "big")

    def word(self, row):
        """The polynomial of a row of len + ecc_bytes bytes (its unused low ECC bits dropped)."""
        return int.from_bytes(bytes(row), "big") >> self.pad

    def is_codeword(self, row):
        return remainder(self.word(row), self.g) == 0

    def syndromes(self, bit_positions, nbits):
        """S_1 .. S_2t of an error pattern: S_j = sum alpha^(j (nbits - 1 - p)) over the flipped
        MSB-first bits p.  Syndromes are linear and a codeword's are zero, so these are also the
        syndromes of any codeword with those bits flipped."""
        out = []
        for j in range(1, 2 * self.t + 1):
            s = 0
            for p in bit_positions:
                s ^= self.exp[j * (nbits - 1 - int(p)) % self.n]
            out.append(s)
        return out

    def syndromes_of_word(self, value):
        """S_1 .. S_2t of a whole received word r(x), evaluated term by term: S_j = r(alpha^j)."""
        degs = [d for d in range(value.bit_length()) if value >> d & 1]
        return [self._sum(j, degs) for j in range(1, 2 * self.t + 1)]

    def _sum(self, j, degs):
        s = 0
        for d in degs:
            s ^= self.exp[j * d % self.n]
        return s


def flip(row, positions):
    """Flip MSB-first bits of a bytearray / uint8 row in place."""
    for p in positions:
        row[int(p) >> 3] ^= 0x80 >> (int(p) & 7)


def distance(a, b):
    """Hamming distance of two equal-length byte rows."""
    return bin(int.from_bytes(bytes(a), "big") ^ int.from_bytes(bytes(b), "big")).count("1")

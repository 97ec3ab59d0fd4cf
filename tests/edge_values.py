"""Field elements that uniformly random draws never produce, for the tests of every reduction (beside structured.py, which varies WHICH
coefficients are zero; this module varies their values).

The radix-2^29 Montgomery code (csrc/fp29.hpp) and the int8 matrix-core reductions (the fold of the high half, the one-word Barrett
quotient, r >= p ? r - p : r) are right only if a handful of carry, borrow and quotient-estimate cases are: a carry through an all-ones
32-bit word, a borrow through all-zero 29-bit digits, a result of exactly 0 or p - 1, a remainder at or above 2^256 before the last
correction.  On uniform residues each has probability about 2^-32 per word.  The pool below holds the values that sit on those edges;
targeted_rows() builds polynomials whose VALUES at chosen points are pool members, so that the outputs of an encode, the inputs of a
decode's 1/den scaling and the values a validation compares are edge values too.  Plain Python ints only: no oracle, no GPU."""
import random


def packed_bits(n_limbs):
    return 64 * n_limbs


def edge_pool(p, n_limbs):
    """sorted distinct residues below p on the edges of the packed words (32 bits), the digits (29 bits) and the int8 split"""
    bits = packed_bits(n_limbs)
    nb = bits // 8
    v = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2]
    e = (1 << bits) - p                      # the smallest residue whose + p leaves the packed width
    v += [e - 1, e, e + 1]
    for j in range(1, bits // 32 + 1):       # word boundaries: a carry into, and a borrow out of, an all-ones / all-zero word
        v += [(1 << (32 * j)) - 1, 1 << (32 * j), (1 << (32 * j)) + 1]
    for j in range(1, 10):                   # digit boundaries (2^(29 j) beyond the modulus comes back as a residue)
        v += [(1 << (29 * j)) - 1, 1 << (29 * j)]
    for byte in ("80", "7f", "ff", "01", "fe"):       # the sign boundary of the int8 split and of the - 128 bias
        v.append(int(byte * nb, 16))
    v += [int("ff00" * (nb // 2), 16), int("00ff" * (nb // 2), 16)]
    return sorted({x % p for x in v})


def montgomery_radix(n_limbs):
    return 1 << (261 if n_limbs == 4 else 87)


def montgomery_preimages(p, n_limbs):
    """v R^-1 mod p for every pool value v: a kernel that brings these into Montgomery form holds the pool's digit patterns inside"""
    rinv = pow(montgomery_radix(n_limbs), -1, p)
    return [v * rinv % p for v in edge_pool(p, n_limbs)]


def operands(p, n_limbs):
    """the pool and its pre-images, distinct, in a fixed order: the operand list of the element-wise tests"""
    return sorted(set(edge_pool(p, n_limbs)) | set(montgomery_preimages(p, n_limbs)))


def reduced_pool(p, n_limbs):
    """{0, 1, p - 1, 2^bits - p, one value whose low digits are all ones, one pre-image}: small enough for all 5-tuples"""
    ones = ((1 << (29 * (8 if n_limbs == 4 else 2))) - 1) % p
    return sorted({0, 1, p - 1, ((1 << packed_bits(n_limbs)) - p) % p, ones, montgomery_preimages(p, n_limbs)[-1]})


def n_limbs_of(p):
    return 1 if p < 1 << 64 else 4


def evaluate_rows(p, x, rows):
    """[row][point]: Horner in Python ints"""
    out = []
    for row in rows:
        vals = []
        for xv in x:
            acc = 0
            for co in reversed(row):
                acc = (acc * xv + co) % p
            vals.append(acc)
        out.append(vals)
    return out


def _newton_to_monomial(p, xs, ys, inv):
    """coefficients (low first) of the polynomial of degree < len(xs) through (xs, ys); inv[i][j] = 1 / (xs[i] - xs[j]), j < i"""
    d = len(xs)
    dd = list(ys)
    for lvl in range(1, d):                  # divided differences in place
        for i in range(d - 1, lvl - 1, -1):
            dd[i] = (dd[i] - dd[i - 1]) * inv[i][i - lvl] % p
    co = [0] * d
    for i in range(d - 1, -1, -1):           # co = co * (X - xs[i]) + dd[i]
        nxt = [0] * d
        for l in range(d - 1):
            nxt[l + 1] = co[l]
        for l in range(d):
            nxt[l] = (nxt[l] - xs[i] * co[l]) % p
        nxt[0] = (nxt[0] + dd[i]) % p
        co = nxt
    return co


def interpolate(p, xs, ys):
    """coefficients (low first) of the polynomial of degree < len(xs) with the values ys at the points xs"""
    inv = [[pow(xs[i] - xs[j], -1, p) for j in range(i)] for i in range(len(xs))]
    return _newton_to_monomial(p, [v % p for v in xs], ys, inv)


def fits_32_balanced_digits(v):
    """True when v is 32 base-256 digits in -128 .. 127: what one entry of a full-size int8 matrix image holds"""
    carry = 0
    for b in range(32):
        t = ((v >> (8 * b)) & 0xff) + carry
        carry = 1 if t > 127 else 0
    return not carry and v >> 256 == 0


def targeted_rows(p, x, where, d, count, seed=0):
    """`count` coefficient rows of degree < d whose values at the d points x[j], j in `where`, are pool values: row k has
    pool[(k + 7 i + seed) % len(pool)] at the i-th of them, so len(pool) consecutive rows put every value at every position once"""
    assert len(where) == d and len(set(where)) == d
    pool = edge_pool(p, n_limbs_of(p))
    xs = [x[j] % p for j in where]
    inv = [[pow(xs[i] - xs[j], -1, p) for j in range(i)] for i in range(d)]
    return [_newton_to_monomial(p, xs, [pool[(k + 7 * i + seed) % len(pool)] for i in range(d)], inv) for k in range(count)]


def targets(p, d, count, seed=0):
    """the values targeted_rows puts at its points: [row][i]"""
    pool = edge_pool(p, n_limbs_of(p))
    return [[pool[(k + 7 * i + seed) % len(pool)] for i in range(d)] for k in range(count)]


def edge_rows(p, d, count, seed=0):
    """`count` rows of d coefficients, every one a pool value: the first len(pool) rows walk the pool as targeted_rows does (every value
    at every position once); the row after them is p - 1 throughout (the largest sum), and the rest draw from the pool and, one entry in
    four, from its Montgomery pre-images"""
    nl = n_limbs_of(p)
    pool, pre = edge_pool(p, nl), montgomery_preimages(p, nl)
    rnd = random.Random(seed)
    rows = []
    for k in range(count):
        if k < len(pool):
            rows.append([pool[(k + 7 * i + seed) % len(pool)] for i in range(d)])
        elif k == len(pool):
            rows.append([p - 1] * d)
        else:
            rows.append([rnd.choice(pre) if rnd.random() < 0.25 else rnd.choice(pool) for _ in range(d)])
    return rows

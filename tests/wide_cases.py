"""Matrices, inputs and the integer behind one output for the tests of the full-size matrix-core mat-vec (k_mm8w and its balanced
launch k_mm8w_flat, csrc/hb_mfma_wide.hip) through hb_matrix_from_host + hb_matvec, at any modulus in [2^254, 2^256).

The kernel's reduction ends in a one-word Barrett quotient that may come out one short; for p > 2^255 the remainder can then reach
2^256.  Random and plainly edge-valued inputs never get there (0 of 14 000 outputs of a 22 x 22 matrix); inputs SOLVED so that outputs
are pool values of edge_values.py do, hundreds of times a launch (tests/test_wide_cases_host.py counts them with fold_model.py).
Plain Python ints only: no oracle, no GPU."""
import functools
import random

import edge_values as ev

ALL_7F = int("7f" * 32, 16)         # 32 digits of 127: the largest value of 32 balanced base-256 digits
FIXED_ROWS = 4                      # zeros, ones, the largest fitting residue, the fitting residue of the largest digit sum


def digit_sum(v):
    """sum of |digit| over the 32 balanced base-256 digits of v (as mm8w_from_host splits an entry)"""
    total, carry = 0, 0
    for b in range(32):
        t = ((v >> (8 * b)) & 0xff) + carry
        carry = 1 if t > 127 else 0
        total += 256 - t if carry else t
    assert not carry and v >> 256 == 0
    return total


def largest_fitting(p):
    """the largest residue below p that is 32 balanced digits: 0x7f..7f, or p - 1 when p is not above that (then every residue fits)"""
    v = min(p - 1, ALL_7F)
    assert ev.fits_32_balanced_digits(v)
    return v


def heaviest_fitting(p):
    """the fitting residue below p with the largest sum of |digits|: every digit below the top one -128 -- the largest |digit| and the
    smallest value a top digit allows -- under the largest top digit that keeps the value below p: 0x7e7f..7f80 (127 + 31 * 128 = 4095)
    where p is above it.  The tight case of the image's column bound `bias`."""
    low = 128 * ((256 ** 31 - 1) // 255)
    top = min(127, (p - 1 + low) >> 248)
    v = (top << 248) - low
    assert 0 <= v < p and ev.fits_32_balanced_digits(v) and digit_sum(v) == top + 31 * 128
    assert top == 127 or ((top + 1) << 248) - low >= p
    return v


def _random_fitting(p, rnd):
    while True:
        v = sum(rnd.randrange(-128, 128) << (8 * b) for b in range(32))
        if 0 <= v < p:
            return v


def fitting_matrix(p, n_out, d, seed):
    """n_out x d, every entry below p and 32 balanced base-256 digits (what an entry of the int8 image holds: a matrix with one entry
    that is not goes to the integer kernel).  Rows 0 .. 3: zeros; ones; largest_fitting(p) throughout; heaviest_fitting(p) throughout.
    The rest: one entry in two a random fitting residue, the other a fitting member of edge_values.operands(p, 4)."""
    assert n_out > FIXED_ROWS
    rnd = random.Random(seed)
    ops = [v for v in ev.operands(p, 4) if ev.fits_32_balanced_digits(v)]
    assert len(ops) >= 20
    m = [[0] * d, [1] * d, [largest_fitting(p)] * d, [heaviest_fitting(p)] * d]
    for _ in range(n_out - FIXED_ROWS):
        m.append([_random_fitting(p, rnd) if rnd.random() < 0.5 else rnd.choice(ops) for _ in range(d)])
    return m


def _inverse(p, a):
    """inverse of a square matrix mod p by Gauss-Jordan elimination, or None when it is singular"""
    k = len(a)
    w = [list(r) + [int(i == j) for j in range(k)] for i, r in enumerate(a)]
    for c in range(k):
        piv = next((r for r in range(c, k) if w[r][c]), None)
        if piv is None:
            return None
        w[c], w[piv] = w[piv], w[c]
        inv = pow(w[c][c], -1, p)
        w[c] = [v * inv % p for v in w[c]]
        for r in range(k):
            f = w[r][c]
            if r != c and f:
                wc = w[c]
                w[r] = [(v - f * u) % p for v, u in zip(w[r], wc)]
    return [r[k:] for r in w]


def _spread(items, k):
    """k of the items, evenly spread, the first and the last among them"""
    if k == 1:
        return [items[-1]]
    return [items[(j * (len(items) - 1)) // (k - 1)] for j in range(k)]


def targeted_system(p, m, seed=0):
    """-> (rows, cols, inverse): k = min(d, n_out - 3) rows spread over the whole matrix -- so over every row tile, whatever its height
    -- with the last row among them, k columns, and the inverse of that k x k sub-matrix.  Of the rows 0 .. 3 only the heaviest can be
    among them: the zero row has no inverse and the three constant rows are multiples of one another."""
    n_out, d = len(m), len(m[0])
    usable = list(range(FIXED_ROWS - 1, n_out))
    k = min(d, len(usable))
    rnd = random.Random(seed)
    for attempt in range(20):
        rows = _spread(usable, k) if attempt == 0 else sorted(rnd.sample(usable[:-1], k - 1) + [n_out - 1])
        cols = _spread(list(range(d)), k) if attempt == 0 or k == d else sorted(rnd.sample(range(d), k))
        inv = _inverse(p, [[m[r][c] for c in cols] for r in rows])
        if inv is not None:
            assert len(set(rows)) == k and len(set(cols)) == k and rows[-1] == n_out - 1
            return rows, cols, inv
    raise AssertionError("no invertible sub-matrix found")


def image_bias(m):
    """the column bound of the int8 image: 128 * (the largest sum of |digits| over a row) + 1  (mm8w_from_host)"""
    return 128 * max(sum(digit_sum(v) for v in row) for row in m) + 1


def biased_sum(p, m, x, i, bias=None):
    """-> (S, CR): the integer the kernel's 63 int32 columns hold for row i of M x -- every input byte enters as a signed byte, its
    value less 128, and every column carries `bias` so that none is negative:
        S = sum_l M[i][l] x_l - 0x80..80 rowsum_i + bias sum_{c < 63} 2^(8c)
    -- and the per-row constant CR = -(S - sum_l M[i][l] x_l) mod p that takes both back out (before the shift of the fold, which
    fold_model.reduce_model adds itself).  This RESTATES the image's bias rule inside the tests, as _full_size_image of
    test_gpu_edge_values.py restates its digit rule: if the image changes, this has to follow, whatever the kernels compute."""
    row = m[i]
    bias = image_bias(m) if bias is None else bias
    dot = sum(a * b for a, b in zip(row, x))
    s = dot - int("80" * 32, 16) * sum(row) + bias * sum(1 << (8 * c) for c in range(63))
    assert s >= 0
    return s, (dot - s) % p


class Case:
    """One (modulus, shape, chunk count): the matrix, the chunks' inputs and what the targeted ones aim at."""

    def __init__(self, p, n_out, d, count, period=None):
        self.p, self.n_out, self.d, self.count = p, n_out, d, count
        self.m = fitting_matrix(p, n_out, d, seed=1000 * n_out + d)
        self.bias = image_bias(self.m)
        self.rows, self.cols, inv = targeted_system(p, self.m, seed=n_out + d)
        pool = ev.edge_pool(p, 4)
        ln = len(pool)
        self.period = period = min(count, period or count)
        k = len(self.rows)
        free = [c for c in range(d) if c not in set(self.cols)]
        n_blocks = -(-period // ln)
        plain = ev.edge_rows(p, d, ((n_blocks + 1) // 2) * ln, seed=n_out)           # block (a): ln rows walk the pool, then p - 1 .., then draws
        fill = ev.edge_rows(p, max(len(free), 1), (n_blocks // 2 + 1) * ln, seed=d)  # the inputs block (b) does not solve for
        tg = ev.targets(p, k, ln, seed=n_out + d)
        base, self.targeted = [], {}
        for c in range(period):
            blk, kk = divmod(c, ln)
            if blk % 2 == 0:
                base.append(plain[(blk // 2) * ln + kk])
                continue
            # block (b): outputs tg[kk] at the chosen rows, rotated by one row a block so that the blocks differ
            rot = blk // 2
            want = [tg[kk][(i + rot) % k] for i in range(k)]
            x = [0] * d
            for j, col in enumerate(free):
                x[col] = fill[(blk // 2) * ln + kk][j]
            rhs = [(want[i] - sum(self.m[r][col] * x[col] for col in free)) % p for i, r in enumerate(self.rows)]
            for j, col in enumerate(self.cols):
                x[col] = sum(a * b for a, b in zip(inv[j], rhs)) % p
            base.append(x)
            self.targeted[c] = list(zip(self.rows, want))
        self.base = base

    def x(self, c):
        """the d inputs of chunk c (a chunk count above the period repeats the period's chunks: every chunk stays edge-valued and
        the Python-int reference stays small)"""
        return self.base[c % self.period]

    def targets_of(self, c):
        """[(row, value)] of a targeted chunk, [] for a plain one"""
        return self.targeted.get(c % self.period, [])

    @functools.cached_property
    def base_outputs(self):
        p = self.p
        return [[sum(a * b for a, b in zip(row, x)) % p for row in self.m] for x in self.base]

    def outputs(self, c):
        """the n_out outputs of chunk c in Python ints (computed once for the whole case and left unchanged)"""
        return self.base_outputs[c % self.period]


@functools.lru_cache(maxsize=None)
def case(p, n_out, d, count, period=None):
    return Case(p, n_out, d, count, period)

"""Shared by tests/test_pairing_host.py, tests/test_g1_host.py and tests/test_gpu_fq_tower.py: the operands at which the 14-digit Fq of
BLS12-381 and the tower above it are driven, and what Python ints say the results are.  The same case runs through hb_selftest_pairing
(the bodies of csrc/hb_fq12_elem.hpp built by the host compiler) and through hb_debug_pair_op (the same bodies built for the device):
a case is (a words, b words or None, expected words), the runner is the caller's.  Every comparison is exact.

fq_edge_pool() is the counterpart of edge_values.edge_pool for 14 digits of 29 bits and 12 words of 32: the values at which a carry, a
borrow or the conditional subtraction of the Montgomery product goes wrong, and their Montgomery pre-images v 2^-406, so that the DIGITS
the kernel multiplies are those patterns too (a residue is converted on load: the digits inside are v 2^406 mod Q)."""
import functools
import random

import numpy as np

import g1_support as s
import pairing_support as ps

from honeybadgermpc_amd.bls12_381 import Q
from honeybadgermpc_amd.bls12_381_pairing import Fq2, Fq6, Fq12

OPS = dict(FQ2_MUL=0, FQ2_SQR=1, FQ2_MUL_NR=2, FQ2_INV=3, FQ6_MUL=4, FQ6_MUL_BY_01=5, FQ6_MUL_BY_1=6, FQ6_MUL_NR=7, FQ6_INV=8, FQ12_MUL=9, FQ12_SQR=10,
           FQ12_MUL_BY_014=11, FQ12_CONJ=12, FQ12_FROBENIUS=13, FQ12_INV=14, FQ12_FINAL_EXP=15, FQ12_CYCLO_SQR=16)
FQ_OPS = dict(FQ_MUL=17, FQ_MUL_LAZY=18, FQ_INV=19)              # include/hbmpc_hip_debug.h
TWO = ("FQ2_MUL", "FQ6_MUL", "FQ6_MUL_BY_01", "FQ6_MUL_BY_1", "FQ12_MUL", "FQ12_MUL_BY_014")
MODELLED = [n for n in OPS if n not in ("FQ12_FINAL_EXP", "FQ12_CYCLO_SQR")]

MONT = 1 << (29 * 14)                                            # the Montgomery radix of fq_params: 2^406
ONES13 = (1 << 377) - 1                                          # thirteen 29-bit digits of all ones, the top digit 0
ONES_TOP = (0xC << 377) | ONES13                                 # ... and the largest top digit below Q's


def pre_image(v):
    """the residue whose Montgomery digits are v's"""
    return v * pow(MONT, -1, Q) % Q


@functools.lru_cache(maxsize=None)
def fq_edge_pool():
    """sorted distinct residues below Q (a tuple)"""
    vals = [0, 1, 2, Q - 1, Q - 2, (Q - 1) // 2, (Q + 1) // 2, ONES13, ONES_TOP]
    for j in range(1, 14):                                       # a digit boundary: a carry into, a borrow out of digit j
        vals += [(1 << (29 * j)) - 1, 1 << (29 * j), (1 << (29 * j)) + 1]
    for j in range(1, 12):                                       # a word boundary of the twelve-word memory form
        vals += [(1 << (32 * j)) - 1, 1 << (32 * j)]
    wrap = ((1 << 384) - Q) % Q                                  # what the twelve words hold beyond a multiple of Q
    vals += [wrap - 1, wrap, wrap + 1]
    assert all(0 <= v < Q for v in vals)
    return tuple(sorted(set(vals) | {pre_image(v) for v in vals}))


@functools.lru_cache(maxsize=None)
def lazy_pool():
    """the reduced pool of FQ_MUL_LAZY: with the pre-image of Q - 1 the factors are 8 (Q - 1), the stated bound of fq_mul"""
    return (0, 1, Q - 1, ONES13, ONES_TOP, pre_image(Q - 1))


# ---------------------------------------------------------------- Fq operations: coordinate 0, the other eleven copied through
@functools.lru_cache(maxsize=None)
def _pool_words():
    return s.words(fq_edge_pool(), 6)


def fq_operands(idx):
    """(len(idx), 72) uint64: coordinate 0 of item i is pool[idx[i]], coordinate k is pool[(idx[i] + 7 k) % len(pool)]"""
    w, idx = _pool_words(), np.asarray(idx, dtype=np.int64)
    return np.ascontiguousarray(np.concatenate([w[(idx + 7 * k) % len(w)] for k in range(12)], axis=1))


def _with_coordinate_0(a_words, values):
    out = a_words.copy()
    out[:, :6] = s.words(values, 6)
    return out


@functools.lru_cache(maxsize=None)
def fq_mul_case():
    """every ordered pair of the pool -> (a, b, want)"""
    pool = fq_edge_pool()
    n = len(pool)
    ia, ib = np.repeat(np.arange(n), n), np.tile(np.arange(n), n)
    a, b = fq_operands(ia), fq_operands(ib)
    return a, b, _with_coordinate_0(a, [pool[i] * pool[j] % Q for i, j in zip(ia.tolist(), ib.tolist())])


@functools.lru_cache(maxsize=None)
def fq_mul_lazy_case(sa, sb):
    """ka = 2^sa, kb = 2^sb over every ordered pair of the reduced pool -> (arg, a, b, want); the other coordinates are the full pool's"""
    pool, red = fq_edge_pool(), lazy_pool()
    at = [pool.index(v) for v in red]
    pairs = [(i, j) for i in at for j in at]
    a, b = fq_operands([i for i, _ in pairs]), fq_operands([j for _, j in pairs])
    return 16 * sa + sb, a, b, _with_coordinate_0(a, [(pool[i] << sa) * (pool[j] << sb) % Q for i, j in pairs])


@functools.lru_cache(maxsize=None)
def fq_inv_case():
    """-> (a, want): x inv(x) = 1 and 0 -> 0 are asserted here, on the expected values"""
    pool = fq_edge_pool()
    inv = [pow(v, Q - 2, Q) for v in pool]
    assert all((v * w % Q == 1) if v else (w == 0) for v, w in zip(pool, inv))
    a = fq_operands(np.arange(len(pool)))
    return a, _with_coordinate_0(a, inv)


# ---------------------------------------------------------------- tower operands
def rand12(rnd):
    return Fq12.from_coords([rnd.randrange(Q) for _ in range(12)])


def edge_operands():
    """Fq12 operands: random ones, then 0, 1 and Q - 1 in every coordinate in turn (the others random), then all-equal edge values"""
    rnd = random.Random(5)
    out = [rand12(rnd) for _ in range(4)]
    for k in range(12):
        for v in (0, 1, Q - 1):
            co = [rnd.randrange(Q) for _ in range(12)]
            co[k] = v
            out.append(Fq12.from_coords(co))
    out += [Fq12.from_coords([v] * 12) for v in (0, 1, Q - 1)] + [Fq12.one()]
    return out


@functools.lru_cache(maxsize=None)
def tower_operands():
    """edge_operands(), then len(pool) elements whose coordinate k is pool[(m + 7 k) % len(pool)] (every pool value at every coordinate
    once), then sparse elements: the all-(Q - 1) one, c1 = 0, c0 = 0, and two of the three Fq2 coordinates of c0 (and of c1) zero -- the
    zero branches of the inversions and the shapes a line or a Frobenius image has --, then elements whose halves cancel.  A tuple of
    Fq12."""
    pool = fq_edge_pool()
    n = len(pool)
    out = edge_operands()
    out += [Fq12.from_coords([pool[(m + 7 * k) % n] for k in range(12)]) for m in range(n)]
    rnd = random.Random(29)
    r6 = lambda: Fq6(*(Fq2(rnd.randrange(Q), rnd.randrange(Q)) for _ in range(3)))
    top = Fq6(*(Fq2(Q - 1, Q - 1) for _ in range(3)))
    out += [Fq12(top, top), Fq12(r6()), Fq12(top), Fq12(Fq6.zero(), r6()), Fq12(Fq6.zero(), top), Fq12(Fq6(Fq2(0, Q - 1))), Fq12(Fq6(Fq2(Q - 1, 0)), Fq6.zero())]
    z = Fq2.zero()
    for at in range(3):
        for x in (Fq2(rnd.randrange(Q), rnd.randrange(Q)), Fq2(Q - 1, Q - 1), Fq2(0, 1)):
            lone = Fq6(*(x if k == at else z for k in range(3)))
            out += [Fq12(lone, r6()), Fq12(r6(), lone), Fq12(lone, lone)]
    # halves that cancel: the Karatsuba operand sums a0 + a1 are then EXACTLY Q (2 Q, 4 Q one level down), a product with such a factor
    # is a multiple of Q, and REDC returns Q itself for it: only the conditional subtraction makes that 0
    neg = lambda co: [(Q - v) % Q for v in co]
    for v in (1, Q - 1, (Q - 1) // 2, ONES13, pre_image(1)):
        out.append(Fq12.from_coords([v, Q - v] * 6))                         # c0 + c1 = Q in every Fq2
    for _ in range(2):
        h = [rnd.randrange(Q) for _ in range(6)]
        out.append(Fq12.from_coords(h + neg(h)))                             # c1 = -c0 in Fq12
        x, y = h[:2], h[2:4]
        out.append(Fq12.from_coords(x + neg(x) + y + y + neg(y) + x))        # c1 = -c0, then c2 = -c1, inside the Fq6 halves
        out.append(Fq12.from_coords(x + y + neg(x) + neg(x) + neg(y) + x))   # c2 = -c0; and the halves cancel as well
    return tuple(out)


def model_op(name, a, b, arg):
    f2 = lambda x: Fq12(Fq6(x, a.c0.c1, a.c0.c2), a.c1)
    f6 = lambda x: Fq12(x, a.c1)
    return {
        "FQ2_MUL": lambda: f2(a.c0.c0 * b.c0.c0),
        "FQ2_SQR": lambda: f2(a.c0.c0.square()),
        "FQ2_MUL_NR": lambda: f2(a.c0.c0.mul_by_nonresidue()),
        "FQ2_INV": lambda: f2(a.c0.c0.inverse()),
        "FQ6_MUL": lambda: f6(a.c0 * b.c0),
        "FQ6_MUL_BY_01": lambda: f6(a.c0.mul_by_01(b.c0.c0, b.c0.c1)),
        "FQ6_MUL_BY_1": lambda: f6(a.c0.mul_by_1(b.c0.c0)),
        "FQ6_MUL_NR": lambda: f6(a.c0.mul_by_nonresidue()),
        "FQ6_INV": lambda: f6(a.c0.inverse()),
        "FQ12_MUL": lambda: a * b,
        "FQ12_SQR": lambda: a.square(),
        "FQ12_MUL_BY_014": lambda: a.mul_by_014(b.c0.c0, b.c0.c1, b.c0.c2),
        "FQ12_CONJ": lambda: a.conjugate(),
        "FQ12_FROBENIUS": lambda: a.frobenius_map(arg),
        "FQ12_INV": lambda: a.inverse(),
    }[name]()


@functools.lru_cache(maxsize=None)
def _tower_words():
    a = tower_operands()
    return ps.gt_words(list(a)), ps.gt_words(list(a[1:] + a[:1]))


@functools.lru_cache(maxsize=None)
def tower_case(name, arg=0):
    """a = tower_operands(), b = a rotated by one -> (a words, b words or None, the model's words)"""
    a = tower_operands()
    b = a[1:] + a[:1]
    aw, bw = _tower_words()
    return aw, (bw if name in TWO else None), ps.gt_words([model_op(name, x, y, arg) for x, y in zip(a, b)])


def easy_part(f):
    """f^((Q^6 - 1)(Q^2 + 1)) by the model: into the cyclotomic subgroup"""
    r = f.conjugate() * f.inverse()
    return r.frobenius_map(2) * r


@functools.lru_cache(maxsize=None)
def cyclotomic_operands():
    """-> (raw, cyc): non-zero operands with edge coordinates (of edge_operands and of the pool's walk), and their images under the
    easy part with 1 appended: elements of the cyclotomic subgroup, where Granger and Scott's squaring is a squaring"""
    walk = tower_operands()[len(edge_operands()):]
    raw = [x for x in edge_operands()[:12] + [walk[0], walk[len(walk) // 3]] if not (x.c0.is_zero() and x.c1.is_zero())]
    return raw, [easy_part(x) for x in raw] + [Fq12.one()]


@functools.lru_cache(maxsize=None)
def final_exp_operands():
    """eight operands: four random, four with edge coordinates; the model (slow) is asked about MODEL_FINAL_EXP of them"""
    e = edge_operands()
    walk = tower_operands()[len(e):]
    return e[:4] + [e[4], e[9], walk[3], Fq12.from_coords([Q - 1] * 12)]


MODEL_FINAL_EXP = (1, 6)


# ---------------------------------------------------------------- the bare square root
@functools.lru_cache(maxsize=None)
def sqrt_case():
    """the squares of the pool and the pool itself -> (values, expected flags by Euler's criterion, expected roots: a^((Q + 1) / 4), or
    0 for a non-residue)"""
    pool = fq_edge_pool()
    vals = [v * v % Q for v in pool] + list(pool)
    flags = [1 if pow(a, (Q - 1) // 2, Q) in (0, 1) else 0 for a in vals]
    roots = [pow(a, (Q + 1) // 4, Q) if f else 0 for a, f in zip(vals, flags)]
    assert all(r * r % Q == a for a, f, r in zip(vals, flags, roots) if f) and flags[:len(pool)] == [1] * len(pool) and 0 in flags
    return vals, flags, roots

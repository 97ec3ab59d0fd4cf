"""Shared by tests/test_fixedpoint_sqrt_host.py and tests/test_gpu_fixedpoint_sqrt.py: the count table, the hb_selftest_fxsqrt runner, the
whole chain through the host bodies on degree-0 shares, and the operands the accuracy and end-to-end tests use."""
from fractions import Fraction
from math import isqrt

import bitdec_cases as bc
import division_cases as dc

NORM_MASK, FIRST, TRUNC_STEP = range(3)
GH, R, OUT = range(3)
SQRT, RSQRT, BOTH = 1, 2, 3
SHAPES = [(8, 4), (16, 8), (32, 16), (64, 32), (64, 40)]

# (k, f, kappa, theta, what) | width | planes | triples | opens, worked out by hand from the formulas, res = 2 for BOTH, else 1:
#   truncations = 1 [g0] + 3 (theta - 1) + (1 + res) [the last iteration] + res [the result] = 3 theta - 1 + 2 res
#   planes  = (k + kappa) + truncations (width + kappa)
#   triples = bit_triples(k-1) + preor_triples(k-1) + 1 [scale] + 1 [G0] + 3 (theta - 1) + (1 + res) + res
#   opens   = bit_opens(k-1) + preor_levels(k-1) + 1 + 2 + 4 theta + 2
# with bit_triples(7) = 15, (15) = 51, (63) = 363, preor_triples(7) = 9, (15) = 28, (63) = 186, bit_opens(7) = 5, (15) = 6, (63) = 8 (the division's
# table), and the widths of the derivation: g0 h0 just above 2^(2 (k - 1) + 12) is the widest product, 2 k + 12 bits with the sign, but
# for the inverse root at f = 62, where h T' < 2^63 sqrt(2) 2^(3 + 92.5) takes 161.
TABLE = [
    ((64, 32, 32, 4, SQRT), 140, 96 + 13 * 172, 363 + 186 + 14, 35),
    ((64, 32, 32, 4, RSQRT), 140, 96 + 13 * 172, 363 + 186 + 14, 35),
    ((64, 32, 32, 4, BOTH), 140, 96 + 15 * 172, 363 + 186 + 16, 35),
    ((64, 32, 32, 3, SQRT), 140, 96 + 10 * 172, 363 + 186 + 11, 31),
    ((64, 62, 32, 4, SQRT), 140, 96 + 13 * 172, 363 + 186 + 14, 35),
    ((64, 62, 32, 4, RSQRT), 161, 96 + 13 * 193, 363 + 186 + 14, 35),
    ((8, 4, 8, 1, SQRT), 28, 16 + 4 * 36, 15 + 9 + 5, 17),
    ((8, 4, 8, 2, BOTH), 28, 16 + 9 * 36, 15 + 9 + 10, 21),
    ((16, 8, 8, 2, SQRT), 44, 24 + 7 * 52, 51 + 28 + 8, 23),
    ((16, 8, 8, 2, BOTH), 44, 24 + 9 * 52, 51 + 28 + 10, 23),
]
DEFAULT_THETA = {(8, 4): 1, (16, 8): 2, (32, 16): 3, (64, 32): 4, (64, 40): 4, (64, 62): 4}


# ---- operands -------------------------------------------------------------------------------------------------------------------
def operands(rnd, k, f, extra=2):
    """the issue's list: the fixed values, every bit length 1 .. k - 1 at both ends and `extra` random values (so both parities of
    e + 1 - f), all below 2^(k-1)"""
    top = 1 << (k - 1)
    xs = [0, 1, 2, 3, 1 << f, (1 << f) + 1, (1 << f) - 1, (1 << (k - 2)) - 1, 1 << (k - 2), top - 1]
    for nb in range(1, k):
        xs += [1 << (nb - 1), (1 << nb) - 1] + [rnd.randrange(1 << (nb - 1), 1 << nb) for _ in range(extra)]
    assert all(0 <= x < top for x in xs) and {x.bit_length() for x in xs} == set(range(k))
    return xs


def in_rsqrt_contract(x, k, f):
    """2^(3f/2) / sqrt(x) < 2^(k-2)"""
    return x > 0 and 1 << (3 * f) < x << (2 * (k - 2))


def exact_rsqrt(x, f):
    """2^(3f/2) / sqrt(x) to 2^-64"""
    return Fraction(isqrt((1 << (3 * f + 128)) // x), 1 << 64)


def r1_sets(rnd, limits):
    """all-zero, all-ones and one random r1 for every truncation"""
    return [[0] * len(limits), [(1 << m) - 1 for m in limits], [rnd.randrange(1 << m) for m in limits]]


def e2e_inputs(rnd, k, f, count):
    """`count` operands inside the inverse root's contract too (0 aside, which gives 0 either way): the ends, 2^f and its neighbours, and
    random values of random lengths"""
    xs = [x for x in (0, (1 << (k - 1)) - 1, 1 << (k - 2), (1 << (k - 2)) - 1, 1 << f, (1 << f) + 1, (1 << f) - 1, 3, 2, 1) if x == 0 or in_rsqrt_contract(x, k, f)]
    while len(xs) < count:
        nb = rnd.randrange(1, k)
        x = rnd.randrange(1 << (nb - 1), 1 << nb)
        if in_rsqrt_contract(x, k, f):
            xs.append(x)
    return xs[:count]


# ---- the bodies on the host ---------------------------------------------------------------------------------------------------
def run_sqrt(p, nl, what, operands, params, outs, count):
    """hb_selftest_fxsqrt over lists of ints: params as the header lists them -> (rc, [out lists])"""
    return bc._run("hb_selftest_fxsqrt", 4, p, nl, what, operands, params, outs, count)


ok = dc.ok


def weight_rows(fs, p, k, f, what):
    """D_i = W_i - W_{i-1} mod p from sqrt_weights, flat, set after set"""
    sets = fs.sqrt_weights(k, f, what)
    sets = sets if what == BOTH else (sets,)
    return [(w - (ws[i - 1] if i else 0)) % p for ws in sets for i, w in enumerate(ws)]


def chain_on_host(fs, fd, bd, p, nl, xvals, k, f, kappa, theta, what, rnd, all_ones=()):
    """the whole chain through hb_selftest_fxsqrt and hb_selftest_div (the bit decomposition through hb_selftest_bd) for ONE holder of
    degree-0 shares: what a step opens is what its mask wrote.  all_ones: truncations (in step order) dealt an all-ones r1 in element 0.
    -> (results [result][element], the r1 of every truncation [truncation][element])"""
    count = len(xvals)
    lay = fs.sqrt_layout(k, f, kappa, theta, what)
    theta, width = lay["theta"], lay["width"]
    nbits, n, beta, res = width + kappa, k - 1, 1 << (k - 1), 2 if what == BOTH else 1
    shifts = fs.sqrt_shifts(k, theta, what)
    x = [v % p for v in xvals]
    used, r1s = [0], []

    def triples(rows):
        used[0] += rows
        ta, tb = ([rnd.randrange(p) for _ in range(rows * count)] for _ in range(2))
        return ta, tb, [a * b % p for a, b in zip(ta, tb)]

    def planes(m):
        rows = [[rnd.getrandbits(1) for _ in range(count)] for _ in range(nbits)]
        if len(r1s) in all_ones:
            for i in range(m):
                rows[i][0] = 1
        r1s.append([sum(rows[i][e] << i for i in range(m)) for e in range(count)])
        return bc.flat(rows)

    def truncate(opened, t, products):
        """fixedpoint_division's products to truncation masks -> (the masks, opened; product + r1; m)"""
        m = shifts[len(r1s)]
        assert shifts[len(r1s):len(r1s) + products] == [m] * products
        both = [v for _ in range(products) for v in planes(m)]
        masked, s = ok(dc.run_div(p, nl, dc.PRODUCT_STEP, [opened, t[0], t[1], t[2], None, None, None, None, both], [dc.TRUNC, products, width, m, kappa],
                                  [products, products], count))
        return masked, s, m

    inv = lambda m: [pow(2, -m, p)]
    bd_planes = bc.flat([[rnd.getrandbits(1) for _ in range(count)] for _ in range(k + kappa)])
    c, _ = bc.run_fxp_mask(p, nl, x, bd_planes, k, n, kappa, count)
    y = bc.bodies_chain(bd, p, nl, c, bd_planes[:n * count], n, count, rnd)
    used[0] += bd.bit_triples(n)
    for level in range(fd.preor_levels(n)):
        ta, tb, tab = triples(fd.preor_level_triples(n, level))
        masked, = ok(dc.run_div(p, nl, dc.OR_MASK, [y, ta, tb], [n, level, 1], [2 * fd.preor_level_triples(n, level)], count))
        y, = ok(dc.run_div(p, nl, dc.OR_COMBINE, [masked, ta, tb, tab], [n, level, 1], [y], count))
    t = triples(1)
    masked, kept = ok(run_sqrt(p, nl, NORM_MASK, [x, y, weight_rows(fs, p, k, f, what), t[0], t[1]], [n, res], [2, 1 + res], count))
    tw = kept[count:]
    t2 = triples(1)
    masked, h = ok(run_sqrt(p, nl, FIRST, [masked, t[0], t[1], t[2], [fs.a_prime(k)], [fs.Y0_SLOPE], t2[0], t2[1]], [], [2, 1], count))
    opened, s, m = truncate(masked, t2, 1)
    gh, rows = h, 1
    for i in range(theta):
        t = triples(1)
        masked, gh = ok(run_sqrt(p, nl, TRUNC_STEP, [opened, s, inv(m), None, gh if rows == 1 else None, t[0], t[1]], [GH, rows, BOTH, m], [2, 2], count))
        opened, s, m = truncate(masked, t, 1)
        which = BOTH if i < theta - 1 else what
        rows = 2 if which == BOTH else 1
        t = triples(rows)
        masked, = ok(run_sqrt(p, nl, TRUNC_STEP, [opened, s, inv(m), [3 * beta], gh, t[0], t[1]], [R, 1, which, m], [2 * rows], count))
        opened, s, m = truncate(masked, t, rows)
    t = triples(res)
    masked, = ok(run_sqrt(p, nl, TRUNC_STEP, [opened, s, inv(m), None, tw, t[0], t[1]], [OUT, res, what, m], [2 * res], count))
    opened, s, m = truncate(masked, t, res)
    outs = [ok(dc.run_div(p, nl, dc.TRUNC_STEP, [opened[q * count:(q + 1) * count], s[q * count:(q + 1) * count], inv(m)], [dc.T_RESULT, 1, 0, m], [1], count))[0]
            for q in range(res)]
    assert used[0] == lay["n_triples"] and len(r1s) == len(shifts)
    return outs, r1s


# ---- GPU side ---------------------------------------------------------------------------------------------------------------------
def selftest_on_tensors(ctx, what, operands, params, out_rows, count):
    """hb_selftest_fxsqrt over the limbs of device tensors (None: absent; a list of ints: constants in host memory), no Python ints in
    between -> [(rows, count, limbs) int64 tensors on the host], one an entry of out_rows (0: absent)"""
    import ctypes

    import numpy as np

    from honeybadgermpc_amd._capi import ints_to_limbs, load_library, np_ptr

    p, nl = ctx.modulus, ctx.n_limbs
    keep = [None if o is None else (ints_to_limbs(list(o), p, 8 * nl) if isinstance(o, list) else np.ascontiguousarray(o.cpu().numpy())) for o in operands]
    ptrs = (ctypes.c_void_p * 8)(*([None if a is None else a.ctypes.data for a in keep] + [None] * (8 - len(keep))))
    outs = [np.zeros((max(r * count, 1), nl), dtype=np.int64) if r else None for r in out_rows]
    optrs = (ctypes.c_void_p * 2)(*([None if o is None else o.ctypes.data for o in outs] + [None] * (2 - len(outs))))
    prm = (ctypes.c_int64 * 4)(*(list(params) + [0] * (4 - len(params))))
    rc = load_library().hb_selftest_fxsqrt(np_ptr(ints_to_limbs([p], p + 1, 8 * nl)), nl, what, ptrs, prm, optrs, count)
    assert rc == 0, rc
    return [None if o is None else ctx.torch.from_numpy(o[:r * count]).view(r, count, nl) for o, r in zip(outs, out_rows)]


def truncation_planes(lay, kappa):
    """-> [first plane of every truncation in step order] from a sqrt_layout"""
    nb = lay["width"] + kappa
    starts = []
    for name, (start, stop) in sorted(lay["planes"].items(), key=lambda kv: kv[1]):
        if name != "bit_decompose":
            starts += list(range(start, stop, nb))
    return starts

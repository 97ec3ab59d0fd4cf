"""Shared by tests/test_fixedpoint_division_host.py and tests/test_gpu_fixedpoint_division.py: the count table, the prefix OR on Python
ints from the wiring model alone, the hb_selftest_div runner, the whole division chained through the host bodies on degree-0 shares,
and the operands the accuracy and end-to-end tests use."""
import ctypes

import numpy as np

import bitdec_cases as bc

OR_MASK, OR_COMBINE, NORM_MASK, PRODUCT_STEP, TRUNC_STEP, PAIR_MASK = range(6)
SIGN, NORM, FIRST, TRUNC = range(4)
T_RESULT, T_RECIP, T_GOLD = range(3)

PREOR_TRIPLES = {1: 0, 2: 1, 3: 2, 5: 5, 8: 12, 9: 13, 11: 17, 33: 81, 63: 186, 256: 1024}          # the issue's list
OR_PLANES = (1, 2, 3, 5, 8, 9, 33)

# (k, f, kappa, theta, signed) | width | planes | triples | opens, worked out by hand from the issue's formulas:
#   planes  = [k + kappa signed] + (k + kappa) + (2 theta + 1) (width + kappa)
#   triples = [(2 k - 3) + 1 signed] + bit_triples(k-1) + preor_triples(k-1) + (2 signed | 1) + 1 + 2 + 2 (theta - 1) + 1
#   opens   = [(1 + carry_levels(k-1)) + 1 signed] + bit_opens(k-1) + preor_levels(k-1) + 1 + 2 + 2 + 2 (theta - 1) + 2
# with bit_triples(7) = 9 + 6, bit_triples(15) = 37 + 14, bit_triples(63) = 363 (bitdec_cases.TABLE's rule: one product a g-only node,
# two a full one, and one a bit above bit 0), preor_triples(7) = 3 * 3, (15) = 4 * 7, (63) = 186, and the widths of the derivation: 2 k
# for k = 2 f.
TABLE = [
    ((64, 32, 32, 5, True), 128, 1952, 689, 37),               # the issue's figures at the paper's theta
    ((64, 32, 32, 5, False), 128, 1856, 562, 29),
    ((64, 32, 32, 7, True), 128, 2592, 693, 41),               # the default theta: two iterations more
    ((64, 32, 32, 7, False), 128, 2496, 566, 33),
    ((8, 4, 8, 3, True), 16, 200, 48, 24),
    ((8, 4, 8, 3, False), 16, 184, 33, 19),
    ((16, 8, 8, 5, True), 32, 488, 123, 31),
    ((16, 8, 8, 5, False), 32, 464, 92, 25),
]


# ---- Python ints ------------------------------------------------------------------------------------------------------------
def prefix_or_on_ints(fd, bits, from_top=True):
    """the network of preor_nodes on 0 / 1 ints -> the planes; no level may read a plane it writes"""
    n = len(bits)
    y = list(bits)
    at = (lambda r: n - 1 - r) if from_top else (lambda r: r)
    for level in range(fd.preor_levels(n)):
        nodes = fd.preor_nodes(n, level)
        written = {j for j, _ in nodes}
        assert all(0 <= q < j <= n - 1 and q not in written for j, q in nodes), (n, level)
        assert len(written) == len(nodes)
        for j, q in nodes:
            y[at(j)] = y[at(j)] + y[at(q)] - y[at(j)] * y[at(q)]
    return y


def admissible_a(b, k, f):
    """the largest |a| with |a 2^f / b| < 2^(k-2) that is a signed k-bit value"""
    a = min(((abs(b) << (k - 2)) - 1) >> f, (1 << (k - 1)) - 1)
    assert (a << f) < abs(b) << (k - 2)
    return a


def r1_limits(fd, k, f, theta):
    """m of the 2 theta + 1 truncations in step order"""
    return [2 * (k - 1 - f), f] + [2 * f] * (2 * theta - 1)


def targeted_pairs(rnd, k, f, extra=200):
    """(a, b): |b| in [2^(k-2), 2^(k-1)) with the largest admissible |a|, |b| = 1, both signs, a = 0, every magnitude of b"""
    top = 1 << (k - 1)
    pairs = []
    for b in (top - 1, top // 2, top // 2 + 1, 1, 2, 3, (1 << (2 * f - 1)) % top or 1, ((1 << (2 * f - 1)) + 1) % top or 1):
        for sb in (1, -1):
            a = admissible_a(b, k, f)
            pairs += [(a, sb * b), (-a, sb * b), (0, sb * b), (a // 2, sb * b), (1, sb * b)]
    for _ in range(extra):
        nb = rnd.randrange(1, k)
        b = rnd.randrange(1 << (nb - 1), 1 << nb) * rnd.choice((1, -1))
        a = admissible_a(b, k, f)
        pairs.append((rnd.choice((a, -a, rnd.randrange(-a, a + 1))), b))
    return pairs


# ---- the bodies on the host ---------------------------------------------------------------------------------------------------
def run_div(p, nl, what, operands, params, outs, count):
    """hb_selftest_div over lists of ints.  operands: up to 9 lists (None: absent); outs: a row count (zero-filled), a list of ints
    (an array the body updates in place) or None -> (rc, [out lists])"""
    from honeybadgermpc_amd._capi import ints_to_limbs, limbs_to_ints, load_library, np_ptr

    lib = load_library()
    nb = 8 * nl
    arrays = [None if o is None else ints_to_limbs(list(o) or [0], p, nb) for o in operands]
    ptrs = (ctypes.c_void_p * 9)(*([None if x is None else x.ctypes.data for x in arrays] + [None] * (9 - len(arrays))))
    bufs, sizes = [], []
    for o in outs:
        if o is None:
            bufs.append(None), sizes.append(0)
        elif isinstance(o, int):
            bufs.append(np.zeros((max(o * count, 1), nl), dtype=np.uint64)), sizes.append(o * count)
        else:
            bufs.append(np.array(ints_to_limbs(list(o) or [0], p, nb))), sizes.append(len(o))
    optrs = (ctypes.c_void_p * 2)(*([None if b is None else b.ctypes.data for b in bufs] + [None] * (2 - len(bufs))))
    prm = (ctypes.c_int64 * 5)(*(list(params) + [0] * (5 - len(params))))
    rc = lib.hb_selftest_div(np_ptr(ints_to_limbs([p], p + 1, nb)), nl, what, ptrs, prm, optrs, count)
    return rc, [None if b is None else limbs_to_ints(b[:s], nb) for b, s in zip(bufs, sizes)]


def ok(result):
    rc, outs = result
    assert rc == 0
    return outs


def chain_on_host(fd, bd, p, nl, avals, bvals, k, f, kappa, theta, signed, rnd, all_ones=()):
    """steps 1 to 6 through hb_selftest_div (the bit decomposition through hb_selftest_bd, the sign bit in the clear) for ONE holder
    of degree-0 shares: what a step opens is what its mask wrote.  all_ones: truncations (0 .. 2 theta) dealt an all-ones r1 in
    element 0.  -> (result, (c, v'), the r1 of every truncation [truncation][element])"""
    count = len(avals)
    lay = fd.div_layout(k, f, kappa, theta, signed)
    width, nbits = lay["width"], lay["width"] + kappa
    alpha, shift = 1 << (2 * f), 2 * (k - 1 - f)
    a, b = [v % p for v in avals], [v % p for v in bvals]
    used = [0]

    def triples(rows):
        used[0] += rows
        ta, tb = ([rnd.randrange(p) for _ in range(rows * count)] for _ in range(2))
        return ta, tb, [x * y % p for x, y in zip(ta, tb)]

    r1s = []

    def planes(m):
        """one truncation's bit planes, flat, with the r1 they deal recorded"""
        rows = [[rnd.getrandbits(1) for _ in range(count)] for _ in range(nbits)]
        if len(r1s) in all_ones:
            for i in range(m):
                rows[i][0] = 1
        r1s.append([sum(rows[i][e] << i for i in range(m)) for e in range(count)])
        return bc.flat(rows)

    u, x = None, b
    if signed:
        u = [1 if v < 0 else 0 for v in bvals]
        ta, tb, tab = triples(1)
        masked, = ok(run_div(p, nl, PAIR_MASK, [u, b, ta, tb], [], [2], count))
        x, = ok(run_div(p, nl, PRODUCT_STEP, [masked, ta, tb, tab, b], [SIGN, 1], [1], count))
        assert x == [abs(v) % p for v in bvals]
    n = k - 1
    bd_planes = bc.flat([[rnd.getrandbits(1) for _ in range(count)] for _ in range(k + kappa)])
    c, _ = bc.run_fxp_mask(p, nl, x, bd_planes, k, n, kappa, count)
    y = bc.bodies_chain(bd, p, nl, c, bd_planes[:n * count], n, count, rnd)
    used[0] += bd.bit_triples(n)
    for level in range(fd.preor_levels(n)):
        ta, tb, tab = triples(fd.preor_level_triples(n, level))
        masked, = ok(run_div(p, nl, OR_MASK, [y, ta, tb], [n, level, 1], [2 * fd.preor_level_triples(n, level)], count))
        y, = ok(run_div(p, nl, OR_COMBINE, [masked, ta, tb, tab], [n, level, 1], [y], count))
    products = 2 if signed else 1
    ta, tb, tab = triples(products)
    masked, v = ok(run_div(p, nl, NORM_MASK, [x, y, u, ta, tb], [n], [2 * products, 1], count))
    cv, = ok(run_div(p, nl, PRODUCT_STEP, [masked, ta, tb, tab, v], [NORM, products], [2], count))
    na, nb, nab = triples(1)
    opened, = ok(run_div(p, nl, PRODUCT_STEP, [masked, ta, tb, tab, v, [fd.alpha_prime(k)], na, nb], [NORM, products], [2], count))
    masked, s = ok(run_div(p, nl, PRODUCT_STEP, [opened, na, nb, nab, None, None, None, None, planes(shift)], [TRUNC, 1, width, shift, kappa], [1, 1], count))
    ta, tb, tab = triples(2)
    inv = lambda m: [pow(2, -m, p)]
    opened, = ok(run_div(p, nl, TRUNC_STEP, [masked, s, inv(shift), None, None, b, a, ta, tb], [T_RECIP, 1, 2, shift], [4], count))
    masked, kept = ok(run_div(p, nl, PRODUCT_STEP, [opened, ta, tb, tab, None, [alpha], None, None, planes(f)], [FIRST, 2, width, f, kappa], [1, 2], count))
    s, xin, m, rows = kept[:count], kept[count:], f, 1
    for _ in range(theta - 1):
        ta, tb, tab = triples(2)
        opened, = ok(run_div(p, nl, TRUNC_STEP, [masked, s, inv(m), [alpha], xin, None, None, ta, tb], [T_GOLD, rows, 2, m], [4], count))
        both = planes(2 * f) + planes(2 * f)
        masked, s = ok(run_div(p, nl, PRODUCT_STEP, [opened, ta, tb, tab, None, None, None, None, both], [TRUNC, 2, width, 2 * f, kappa], [2, 2], count))
        xin, m, rows = None, 2 * f, 2
    ta, tb, tab = triples(1)
    opened, = ok(run_div(p, nl, TRUNC_STEP, [masked, s, inv(m), [alpha], xin, None, None, ta, tb], [T_GOLD, rows, 1, m], [2], count))
    masked, s = ok(run_div(p, nl, PRODUCT_STEP, [opened, ta, tb, tab, None, None, None, None, planes(2 * f)], [TRUNC, 1, width, 2 * f, kappa], [1, 1], count))
    out, = ok(run_div(p, nl, TRUNC_STEP, [masked, s, inv(2 * f)], [T_RESULT, 1, 0, 2 * f], [1], count))
    assert used[0] == lay["n_triples"] - (fd.carry_triples(k - 1) if signed else 0) and len(r1s) == 2 * theta + 1
    return out, (cv[:count], cv[count:]), r1s


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def e2e_inputs(rnd, k, f, count, signed):
    """(a, b) of `count` elements: b of both signs and +-1, |b| = 2^(k-1) - 1 with the largest admissible a, a = 0 (unsigned: b > 0)"""
    top = 1 << (k - 1)
    big = top - 1
    pairs = [(admissible_a(big, k, f), big), (-admissible_a(big, k, f), -big), (admissible_a(1, k, f), 1), (admissible_a(1, k, f), -1), (0, 5 % top or 1), (0, -big),
             (-1, 3), (admissible_a(top // 2, k, f), -(top // 2))]
    while len(pairs) < count:
        nb = rnd.randrange(1, k)
        b = rnd.randrange(1 << (nb - 1), 1 << nb) * rnd.choice((1, -1))
        a = admissible_a(b, k, f)
        pairs.append((rnd.randrange(-a, a + 1), b))
    if not signed:
        pairs = [(a, abs(b)) for a, b in pairs]
    return [a for a, _ in pairs[:count]], [b for _, b in pairs[:count]]

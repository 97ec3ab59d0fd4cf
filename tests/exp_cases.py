"""Shared by tests/test_fixedpoint_exp_host.py and tests/test_gpu_fixedpoint_exp.py: the count table, exact enclosures of 2^X and e^X from
integers alone, the operands the accuracy tests use, the hb_selftest_fxexp runner, the whole chain through the host rows on degree-0
shares, and the steps composed from what the package had."""
from math import isqrt

import bitdec_cases as bc
import demux_cases as xc

FINISH_LOOKUP_MASK, PRODUCTS_TRUNC, TREE_STEP = range(3)
SHAPES = [(8, 4), (16, 8), (64, 32), (64, 40)]
MERGES = [(1, 1), (2, 1), (2, 2), (4, 3), (4, 4)]               # 4, 8 and 16 entries on either side of the lazy group of 7; 128 and 256 entries

# (k, f, kappa, g) | fraction groups | tree | planes | triples | opens | demux rows by level [(group, opened, products)], worked out by hand:
#   s = k + 2, W = 2 s + 2, mi = bit_length(k - 3); the integer group has mi + 1 bits and comes last
#   planes  = (k + 1 + kappa) + G (W + kappa): one truncation a product of the tree (G - 1 of them) and the result
#   triples = bit_triples(k) + G;  opens = bit_opens(k) + max demux_levels(w) + 2 (ceil(log2 G) + 1)
# with bit_triples(8) = 19, (16) = 57, (64) = 373 and bit_opens(8) = 5, (16) = 6, (64) = 8, and the demultiplexer's table: m = 2: opened [4],
# products [4]; m = 3: [4, 6], [4, 8]; m = 4: [8, 8], [8, 16]; m = 5: [8, 8, 18], [8, 16, 32]; m = 7: [12, 14, 24], [12, 24, 128]; m = 8: [16, 16, 32], [16, 32, 256]
TABLE = [
    ((8, 4, 8, 2), [(0, 2), (2, 2)], [1], 17 + 2 * 30, 19 + 2, 5 + 2 + 4,
     [[(0, 4, 4), (1, 4, 4), (2, 8, 8)], [(2, 8, 16)]]),
    ((16, 8, 8, 3), [(0, 3), (3, 3), (6, 2)], [1, 1], 25 + 3 * 46, 57 + 3, 6 + 3 + 6,
     [[(0, 4, 4), (1, 4, 4), (2, 4, 4), (3, 8, 8)], [(0, 6, 8), (1, 6, 8), (3, 8, 16)], [(3, 18, 32)]]),
    ((64, 32, 32, 8), [(0, 8), (8, 8), (16, 8), (24, 8)], [2, 1], 97 + 4 * 166, 373 + 4, 8 + 3 + 6,
     [[(j, 16, 16) for j in range(4)] + [(4, 12, 12)], [(j, 16, 32) for j in range(4)] + [(4, 14, 24)], [(j, 32, 256) for j in range(4)] + [(4, 24, 128)]]),
    ((64, 32, 32, 4), [(4 * j, 4) for j in range(8)], [4, 2, 1], 97 + 8 * 166, 373 + 8, 8 + 3 + 8,
     [[(j, 8, 8) for j in range(8)] + [(8, 12, 12)], [(j, 8, 16) for j in range(8)] + [(8, 14, 24)], [(8, 24, 128)]]),
]
# exp: W + kappa more planes for the exponent's truncation, k + 1 bits decomposed (bit_triples(9) = 25, (17) = 65, (65) = 385; bit_opens as above)
EXP_TABLE = [((8, 4, 8, 2), 18 + 3 * 30, 25 + 2, 1 + 5 + 2 + 4), ((16, 8, 8, 3), 26 + 4 * 46, 65 + 3, 1 + 6 + 3 + 6), ((64, 32, 32, 8), 98 + 5 * 166, 385 + 4, 1 + 8 + 3 + 6)]

EXTRA = 64                                                        # an enclosure is of value 2^(f + EXTRA)
_P = 384


# ---- exact values: integer enclosures ---------------------------------------------------------------------------------------------
def _roots(n):
    """[(lo, hi)] enclosing 2^(2^-i) 2^_P for i = 0 .. n, by repeated isqrt"""
    out = [(2 << _P, 2 << _P)]
    for _ in range(n):
        lo, hi = out[-1]
        out.append((isqrt(lo << _P), isqrt(hi << _P) + 1))
    return out


_ROOTS = _roots(80)


def exp2_enclosure(x, f):
    """-> (lo, hi) ints with lo <= 2^(x / 2^f) 2^(f + EXTRA) <= hi for the signed int x"""
    e, frac = x >> f, x & ((1 << f) - 1)
    lo = hi = 1 << _P
    for b in range(f):
        if (frac >> (f - 1 - b)) & 1:
            lo, hi = (lo * _ROOTS[b + 1][0]) >> _P, -((-hi * _ROOTS[b + 1][1]) >> _P)
    shift = e + f + EXTRA - _P
    if shift >= 0:
        return lo << shift, hi << shift
    return lo >> -shift, -((-hi) >> -shift)


def _exp_unit(num, f):
    """-> (lo, hi) enclosing e^(num / 2^f) 2^_P for 0 <= num <= 2^f: the series with every term floored (lo) or ceiled (hi) and the
    remainder, below twice the first term left out, added to hi"""
    lo = hi = tl = th = 1 << _P
    for i in range(1, 120):
        tl, th = (tl * num >> f) // i, -((-th * num >> f) // i) + 1
        lo, hi = lo + tl, hi + th
    return lo, hi + 2 * th + 2


_E = _exp_unit(1, 0)


def exp_enclosure(x, f):
    """-> (lo, hi) ints with lo <= e^(x / 2^f) 2^(f + EXTRA) <= hi for the signed int x: e^n e^r, n = floor(X), from the rational series"""
    n, num = x >> f, x & ((1 << f) - 1)
    if n < -300:
        return 0, 1
    if n > 300:                                                           # far outside every contract: e^300 > 2^432
        return 1 << 432, 1 << 10000
    lo, hi = _exp_unit(num, f)
    for _ in range(abs(n)):
        if n > 0:
            lo, hi = (lo * _E[0]) >> _P, -((-hi * _E[1]) >> _P)
        else:
            lo, hi = (lo << _P) // _E[1], -((-hi << _P) // _E[0])
    shift = _P - f - EXTRA
    return lo >> shift, -((-hi) >> shift)


def error_ulps(result, enclosure):
    """the largest |result - exact| over the enclosure, in units of 2^-EXTRA ulps (an int)"""
    lo, hi = enclosure
    return max(abs((result << EXTRA) - lo), abs((result << EXTRA) - hi))


def in_exp2_contract(x, k, f):
    """2^X 2^f < 2^(k-2)"""
    return -(1 << (k - 1)) <= x < ((k - 2 - f) << f)


def in_exp_contract(x, k, f):
    """e^X 2^f (1 + 2^(1-f)) < 2^(k-2): the exponent's rounding may not carry the result over"""
    hi = exp_enclosure(x, f)[1]
    return -(1 << (k - 1)) <= x < 1 << (k - 1) and hi + (hi >> (f - 1)) + 1 < 1 << (k - 2 + EXTRA)


def largest_in_contract(k, f, natural):
    test = in_exp_contract if natural else in_exp2_contract
    lo, hi = 0, 1 << (k - 1)
    while lo + 1 < hi:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if test(mid, k, f) else (lo, mid)
    return lo


def operands(fe, rnd, k, f, g, natural, extra):
    """the issue's list: 0, +-1, the largest in-contract x, -f 2^f (result 1) and -f 2^f - 1 (result 0), -2^(k-1), an all-ones and an all-zero
    fraction, each group alone all ones, and `extra` seeded values, half of them spread over the in-contract exponents"""
    top = largest_in_contract(k, f, natural)
    ones = (1 << f) - 1
    test = in_exp_contract if natural else in_exp2_contract
    xs = [0, 1, -1, top, top - 1, -(f << f), -(f << f) - 1, -(f << f) + 1, -(1 << (k - 1)), -(1 << (k - 1)) + 1, ones, -ones - 1]
    xs += [((1 << w) - 1) << o for o, w in fe.exp2_groups(k, f, g)] + [-(3 << f) | (((1 << w) - 1) << o) for o, w in fe.exp2_groups(k, f, g)]
    xs += [x for x in (1 << f, (1 << f) | ones, (3 << f) | ones, -(2 << f), top - ones) if test(x, k, f)]
    for i in range(extra):
        xs.append(rnd.randrange(-(f + 2) << f, top + 1) if i & 1 else rnd.randrange(-(1 << (k - 1)), top + 1))
    assert all(test(x, k, f) for x in xs) and not test(top + 1, k, f)
    return xs


def r1_extremes(limits):
    return [[0] * len(limits), [(1 << m) - 1 for m in limits]]


# ---- the rows on the host ---------------------------------------------------------------------------------------------------------
def run_exp(p, nl, what, operands_, params, outs, count):
    """hb_selftest_fxexp over lists of ints: params as the header lists them -> (rc, [out lists])"""
    return bc._run("hb_selftest_fxexp", 3 + 6 * 8, p, nl, what, operands_, params, outs, count)


def ok(result):
    rc, outs = result
    assert rc == 0, rc
    return outs


def lookup_on_ints(p, wl, wh, opened, ta, tab, table, count):
    """F = sum_y T_y (d_lo e_hi + d_lo Q_hi + e_hi P_lo + PQ_y) on Python ints; the arrays [row][element]"""
    out = []
    for e in range(count):
        acc = 0
        for hi in range(1 << wh):
            for lo in range(1 << wl):
                y = (hi << wl) | lo
                acc += table[y] * bc.beaver(opened[lo][e], opened[(1 << wl) + hi][e], ta[lo][e], ta[(1 << wl) + hi][e], tab[y][e], p)
        out.append(acc % p)
    return out


def chain_on_host(fe, bd, dx, p, nl, xvals, k, f, kappa, g, natural, rnd, all_ones=()):
    """the whole chain through hb_selftest_fxexp, hb_selftest_demux, hb_selftest_div and hb_selftest_fxp (the bit decomposition through
    hb_selftest_bd) for ONE holder of degree-0 shares: what a step opens is what its mask wrote.  all_ones: truncations (in step
    order) dealt an all-ones r1 in element 0.  -> (results [element], the r1 of every truncation [truncation][element])"""
    import division_cases as dc

    count = len(xvals)
    lay = fe.exp_layout(k, f, kappa, g) if natural else fe.exp2_layout(k, f, kappa, g)
    n, width, s = lay["bits"], lay["width"], k + fe.GUARD_BITS
    nbits, fractions, mi = width + kappa, lay["groups"], (k - 3).bit_length()
    G = len(fractions)
    widths = [w for _, w in fractions] + [mi + 1]
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

    x = [v % p for v in xvals]
    if natural:
        L, fl = fe.exponent_factor(k)
        prod = [v * L % p for v in x]
        tp = planes(fl)
        masked, r1 = bc.run_fxp_mask(p, nl, prod, tp, width, fl, kappa, count)
        x, = ok(bc.run_fxp(p, nl, 1, [prod, masked, r1, [pow(2, -fl, p)]], [width, fl, kappa], [1], count))
    xp = [(v + (f << f)) % p for v in x]
    bd_planes = bc.flat([[rnd.getrandbits(1) for _ in range(count)] for _ in range(n + 1 + kappa)])
    c, _ = bc.run_fxp_mask(p, nl, xp, bd_planes, n + 1, n, kappa, count)
    y = bc.bodies_chain(bd, p, nl, c, bd_planes[:n * count], n, count, rnd)
    used[0] += bd.bit_triples(n)
    row = lambda r: y[r * count:(r + 1) * count]
    group_bits = [bc.flat([row(o + i) for i in range(w)]) for o, w in fractions] + [bc.flat([row(f + i) for i in range(mi)] + [row(n - 1)])]
    tables = fe.exp2_tables(k, f, g)
    flat_tables, table_off = [], []
    for t in tables:
        table_off.append(len(flat_tables))
        flat_tables += t
    tree = lay["tree"]
    first = triples(tree[0] if tree else 1)
    pairs0 = len(first[0]) // count
    masked0, kept = [0] * (2 * pairs0 * count), [0] * ((G + 1) * count)
    stores = [[0] * (dx.demux_group_rows(w) * count) if w >= 2 else None for w in widths]
    pending = [(1, 0, fractions[j][0], 0, table_off[j], j) for j, w in enumerate(widths) if w == 1]
    for level, lv in enumerate(lay["demux_rows"]):
        ta, tab, masks, spans, oo, po = [], [], [], [], 0, 0
        for j, orows, prows in lv:
            a, ab = xc.level_triples(dx, widths[j], level, count, p, rnd)
            ta += bc.flat(a)
            tab += bc.flat(ab)
            mk, = ok(xc.run_demux(p, nl, xc.MASK, [group_bits[j], stores[j], bc.flat(a)], [widths[j], level], [orows], count))
            masks += mk
            spans.append((j, oo, orows, po, prows))
            oo, po = oo + orows, po + prows
        last = list(pending)
        pending = []
        for j, o, orows, q, prows in spans:
            if level == dx.demux_levels(widths[j]) - 1:
                _, wl, wh = dx.demux_plan(widths[j])[level].merges[0]
                last.append((wl, wh, o, q, table_off[j], j))
            else:
                stores[j], = ok(xc.run_demux(p, nl, xc.FINISH, [masks[o * count:(o + orows) * count], ta[o * count:(o + orows) * count], tab[q * count:(q + prows) * count]],
                                             [widths[j], level], [stores[j]], count))
        for at in range(0, len(last), 8):
            chunk = last[at:at + 8]
            masked0, kept = ok(run_exp(p, nl, FINISH_LOOKUP_MASK, [y, masks, ta, tab, flat_tables, first[0], first[1]],
                                       [len(chunk), pairs0, G + 1] + [v for grp in chunk for v in grp], [masked0, kept], count))
    inv = [pow(2, -s, p)]
    trip = first
    carry = kept[(G - 1) * count:G * count] if G > 1 and G & 1 else None
    for i, products in enumerate(tree):
        both = [v for _ in range(products) for v in planes(s)]
        masked, sv = ok(run_exp(p, nl, PRODUCTS_TRUNC, [masked0, trip[0], trip[1], trip[2], both], [products, width, s, kappa], [products, products], count))
        last_level = i == len(tree) - 1
        trip = triples(1 if last_level else tree[i + 1])
        cin = kept[G * count:] if last_level else carry
        values = products + (cin is not None)
        masked0, odd = ok(run_exp(p, nl, TREE_STEP, [masked, sv, inv, cin, trip[0], trip[1]], [products, s], [2 * (values // 2), 1 if values & 1 else None], count))
        carry = None if last_level else odd
    masked, sv = ok(run_exp(p, nl, PRODUCTS_TRUNC, [masked0, trip[0], trip[1], trip[2], planes(s)], [1, width, s, kappa], [1, 1], count))
    out, = ok(dc.run_div(p, nl, dc.TRUNC_STEP, [masked, sv, inv], [dc.T_RESULT, 1, 0, s], [1], count))
    assert used[0] == lay["n_triples"] and len(r1s) == (1 if natural else 0) + len(fe.exp2_shifts(k, f, g))
    return out, r1s


# ---- GPU side ---------------------------------------------------------------------------------------------------------------------
def selftest_on_tensors(ctx, what, operands_, params, out_rows, count, outs_in=None):
    """hb_selftest_fxexp over the limbs of device tensors (None: absent; a list of ints: constants in host memory) -> [(rows, count,
    limbs) int64 tensors on the host], one an entry of out_rows (0: absent); outs_in: what the outputs hold before the call"""
    import ctypes

    import numpy as np

    from honeybadgermpc_amd._capi import ints_to_limbs, load_library, np_ptr

    p, nl = ctx.modulus, ctx.n_limbs
    keep = [None if o is None else (ints_to_limbs(list(o), p, 8 * nl) if isinstance(o, list) else np.ascontiguousarray(o.cpu().numpy())) for o in operands_]
    ptrs = (ctypes.c_void_p * 8)(*([None if a is None else a.ctypes.data for a in keep] + [None] * (8 - len(keep))))
    outs = [np.zeros((max(r * count, 1), nl), dtype=np.int64) if r else None for r in out_rows]
    for o, init in zip(outs, outs_in or []):
        if o is not None and init is not None and count:
            o[:] = init.cpu().numpy().reshape(o.shape)
    optrs = (ctypes.c_void_p * 2)(*([None if o is None else o.ctypes.data for o in outs] + [None] * (2 - len(outs))))
    prm = (ctypes.c_int64 * 51)(*(list(params) + [0] * (51 - len(params))))
    rc = load_library().hb_selftest_fxexp(np_ptr(ints_to_limbs([p], p + 1, 8 * nl)), nl, what, ptrs, prm, optrs, count)
    assert rc == 0, rc
    return [None if o is None else ctx.torch.from_numpy(o[:r * count]).view(r, count, nl) for o, r in zip(outs, out_rows)]


def truncation_planes(lay, kappa):
    """-> [first plane of every truncation in step order] from an exp2_layout or exp_layout"""
    nb = lay["width"] + kappa
    starts = []
    for name, (start, stop) in sorted(lay["planes"].items(), key=lambda kv: kv[1]):
        if name != "bit_decompose":
            starts += list(range(start, stop, nb))
    return starts


def deal_demux_triples(ctx, fe, dx, rnd, p, n, t, lay, widths, count):
    """-> [party] lists of (ta, tab) a level, as exp2_demux_rows lists them, dealt at degree t, each with a canary row after its last"""
    levels = []
    for level, lv in enumerate(lay["demux_rows"]):
        ta, tab = [], []
        for j, orows, prows in lv:
            a, ab = xc.level_triples(dx, widths[j], level, count, p, rnd)
            assert (len(a), len(ab)) == (orows, prows)
            ta += a
            tab += ab
        for v in (ta, tab):
            v.append([rnd.randrange(p) for _ in range(count)])
        levels.append((bc.deal_planes(ctx, rnd, p, n, t, ta), bc.deal_planes(ctx, rnd, p, n, t, tab)))
    return [[(ta[i], tab[i]) for ta, tab in levels] for i in range(n)]

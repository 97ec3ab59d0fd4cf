"""Shared by tests/test_fixedpoint_trig_host.py and tests/test_gpu_fixedpoint_trig.py: the count table, exact enclosures of sine and cosine
from integers alone -- by half-angle roots and angle addition for turns, by a series of their own for radians, neither the code that
builds the tables --, the operands the accuracy tests use, the steps of csrc/hb_fxtrig.hip on Python ints, the hb_selftest_fxtrig
runner and the whole chain through the host rows on degree-0 shares."""
from math import isqrt

import bitdec_cases as bc
import demux_cases as xc

FINISH_LOOKUP_MASK, CPRODUCTS_TRUNC, TREE_STEP = range(3)
BOTH, COS, SIN = range(3)
MERGES = [(1, 1), (2, 1), (2, 2), (4, 3), (4, 4)]
SPLITS = (1, 2, 4, 8, 16)
WANTS = [("sin", "cos"), ("cos",), ("sin",), ("cos", "sin")]

# (k, f, kappa, g, radians, want) | groups | tree | planes | triples beyond bit_triples(ft) | opens beyond bit_opens(ft) | demux rows by level,
# worked out by hand:
#   turns: ft = f, kv = k; radians: ft = f + 3, fl = k + 3, m = k, 2^(k+1) / 3 < L < 2^(k+1): W_turn = 2 k + 1, and |y| < 2^k: kv = k + 1
#   s = ft + 7, W = 2 s + 2; planes = [W_turn + kappa] + (kv + kappa) + (W + kappa) (2 per inner product + (2 or 1) for the last)
#   triples = 3 per inner product + 3 for the last (2 where the cosine alone is wanted);  opens = [1] + max demux_levels(w) + 2 ceil(log2 G)
# with the demultiplexer's table: m = 2: opened [4], products [4]; m = 3: [4, 6], [4, 8]; m = 4: [8, 8], [8, 16]; m = 8: [16, 16, 32], [16, 32, 256]
TABLE = [
    ((8, 4, 8, 4, False, ("sin", "cos")), [(0, 4)], [], 16, 0, 2, [[(0, 8, 8)], [(0, 8, 16)]]),
    ((8, 4, 8, 2, False, ("sin", "cos")), [(0, 2), (2, 2)], [1], 16 + 2 * 32, 3, 1 + 2, [[(0, 4, 4), (1, 4, 4)]]),
    ((16, 8, 8, 3, False, ("cos",)), [(0, 3), (3, 3), (6, 2)], [1, 1], 24 + 3 * 40, 3 + 2, 2 + 4,
     [[(0, 4, 4), (1, 4, 4), (2, 4, 4)], [(0, 6, 8), (1, 6, 8)]]),
    ((16, 8, 8, 4, True, ("sin", "cos")), [(0, 4), (4, 4), (8, 3)], [1, 1], 41 + 25 + 4 * 46, 6, 1 + 2 + 4,
     [[(0, 8, 8), (1, 8, 8), (2, 4, 4)], [(0, 8, 16), (1, 8, 16), (2, 6, 8)]]),
    ((64, 32, 32, 8, False, ("sin", "cos")), [(0, 8), (8, 8), (16, 8), (24, 8)], [2, 1], 96 + 6 * 112, 9, 3 + 4,
     [[(j, 16, 16) for j in range(4)], [(j, 16, 32) for j in range(4)], [(j, 32, 256) for j in range(4)]]),
    ((64, 32, 32, 4, False, ("sin",)), [(4 * j, 4) for j in range(8)], [4, 2, 1], 96 + 13 * 112, 18 + 3, 2 + 6,
     [[(j, 8, 8) for j in range(8)], [(j, 8, 16) for j in range(8)]]),
]

EXTRA = 64                                                        # an enclosure is of value 2^(f + EXTRA)
_P = 384
_ONE = 1 << _P


# ---- exact values: integer enclosures ---------------------------------------------------------------------------------------------
def _mul(a, b):
    """the product of two intervals of values 2^_P"""
    prods = [x * y for x in a for y in b]
    return min(prods) >> _P, -((-max(prods)) >> _P)


def _half_angles(n):
    """[((cos lo, cos hi), (sin lo, sin hi))] of 2 pi / 2^i for i = 0 .. n, times 2^_P: cos(t / 2) = sqrt((1 + cos t) / 2) and sin(t / 2) =
    sqrt((1 - cos t) / 2) from the quarter turn down"""
    out = [((_ONE, _ONE), (0, 0)), ((-_ONE, -_ONE), (0, 0)), ((0, 0), (_ONE, _ONE))]
    for _ in range(n - 2):
        (clo, chi), _ = out[-1]
        out.append(((isqrt((_ONE + clo) << (_P - 1)), isqrt((_ONE + chi) << (_P - 1)) + 1), (isqrt((_ONE - chi) << (_P - 1)), isqrt((_ONE - clo) << (_P - 1)) + 1)))
    return out


_HALVES = _half_angles(80)


def cis_enclosure(num, bits):
    """-> ((cos lo, cos hi), (sin lo, sin hi)) enclosing cos and sin of 2 pi num / 2^bits, times 2^_P: angle addition over the set bits"""
    c, s = (_ONE, _ONE), (0, 0)
    for b in range(bits):
        if (num >> (bits - 1 - b)) & 1:
            hc, hs = _HALVES[b + 1]
            cc, ss, cs, sc = _mul(c, hc), _mul(s, hs), _mul(c, hs), _mul(s, hc)
            c, s = (cc[0] - ss[1], cc[1] - ss[0]), (cs[0] + sc[0], cs[1] + sc[1])
    return c, s


def turns_enclosure(x, f):
    """-> {"cos": (lo, hi), "sin": (lo, hi)} ints enclosing cos / sin (2 pi x / 2^f) 2^(f + EXTRA) for the signed int x"""
    c, s = cis_enclosure(x % (1 << f), f)
    shift = _P - f - EXTRA
    return {"cos": (c[0] >> shift, -((-c[1]) >> shift)), "sin": (s[0] >> shift, -((-s[1]) >> shift))}


def _atan_inv(x):
    total, power, n = 0, _ONE // x, 0
    while power:
        total += -(power // (2 * n + 1)) if n & 1 else power // (2 * n + 1)
        power //= x * x
        n += 1
    return total


_PI = 4 * (_atan_inv(2) + _atan_inv(3))                          # Euler's pi / 4 = atan(1/2) + atan(1/3); within 2^12 units of 2^-_P


def radians_enclosure(x, f):
    """-> {"cos", "sin"} as turns_enclosure for the angle x / 2^f RADIANS: t = X - 2 pi n in [-pi, pi] within 2^-300, the Taylor series
    at t (terms beyond |t| fall; 200 of them leave nothing), and sine and cosine move by no more than the angle does"""
    n = (x << _P) // (2 * _PI << f)
    t = ((x << _P) >> f) - 2 * _PI * n
    if t > _PI:
        t -= 2 * _PI
    t2 = t * t >> _P
    sin = term = t
    cos = cterm = _ONE
    for i in range(1, 200):
        if not term and not cterm:
            break
        cterm = (cterm * t2 >> _P) // ((2 * i - 1) * (2 * i))
        term = (term * t2 >> _P) // ((2 * i) * (2 * i + 1))
        cos += cterm if i % 2 == 0 else -cterm
        sin += term if i % 2 == 0 else -term
    slack, shift = 1 << (_P - 300), _P - f - EXTRA
    return {"cos": ((cos - slack) >> shift, -((-cos - slack) >> shift)), "sin": ((sin - slack) >> shift, -((-sin - slack) >> shift))}


def error_ulps(result, enclosure):
    """the largest |result - exact| over the enclosure, in units of 2^-EXTRA ulps (an int)"""
    lo, hi = enclosure
    return max(abs((result << EXTRA) - lo), abs((result << EXTRA) - hi))


def centered(v, p):
    return v - p if v > p // 2 else v


def operands(rnd, k, f, extra):
    """the issue's list: 0, +-quarter, half and whole turns, +-1 ulp around each, +-2^(k-1), and `extra` seeded values.  (With k - f < 2 the
    turns that do not fit are left out.)"""
    top = 1 << (k - 1)
    xs = []
    for turn in (0, 1 << f >> 2, -(1 << f >> 2), 1 << f >> 1, -(1 << f >> 1), 1 << f, -(1 << f), 3 << f >> 2):
        xs += [turn - 1, turn, turn + 1]
    xs += [top - 1, -top, -top + 1, (1 << f) - 1 if f < k - 1 else 0]
    xs = [x for x in xs if -top <= x < top]
    return xs + [rnd.randrange(-top, top) for _ in range(extra)]


def r1_extremes(limits):
    return [[0] * len(limits), [(1 << m) - 1 for m in limits]]


# ---- the steps on Python ints -----------------------------------------------------------------------------------------------------
def triples_of(mode):
    return 2 if mode == COS else 3


def comps_of(mode):
    return 2 if mode == BOTH else 1


def operand_values(re, im, mode, side, p):
    """what operand `side` of a product in `mode` hands to each of the product's triples"""
    return [re, im] if mode == COS else [re, im, (re + im) % p]


def components(prods, mode, p):
    """the kept components from the products of a complex product's triples"""
    if mode == BOTH:
        return [(prods[0] - prods[1]) % p, (prods[2] - prods[0] - prods[1]) % p]
    return [(prods[2] - prods[0] - prods[1]) % p if mode == SIN else (prods[0] - prods[1]) % p]


def lookup_on_ints(p, wl, wh, opened, ta, tab, table, count):
    """F = sum_y T_y (d_lo e_hi + d_lo Q_hi + e_hi P_lo + PQ_y) on Python ints; the arrays [row][element]; T signed or a residue"""
    out = []
    for e in range(count):
        acc = 0
        for hi in range(1 << wh):
            for lo in range(1 << wl):
                y = (hi << wl) | lo
                acc += table[y] * bc.beaver(opened[lo][e], opened[(1 << wl) + hi][e], ta[lo][e], ta[(1 << wl) + hi][e], tab[y][e], p)
        out.append(acc % p)
    return out


# ---- the rows on the host ---------------------------------------------------------------------------------------------------------
def run_trig(p, nl, what, operands_, params, outs, count):
    """hb_selftest_fxtrig over lists of ints: params as the header lists them -> (rc, [out lists])"""
    return bc._run("hb_selftest_fxtrig", 5 + 6 * 8, p, nl, what, operands_, params, outs, count)


def ok(result):
    rc, outs = result
    assert rc == 0, rc
    return outs


def chain_on_host(ft, bd, dx, p, nl, xvals, k, f, kappa, g, radians, want, rnd, split=1, all_ones=()):
    """the whole chain through hb_selftest_fxtrig, hb_selftest_demux and hb_selftest_fxp (the bit decomposition through hb_selftest_bd) for
    ONE holder of degree-0 shares: what a step opens is what its mask wrote.  all_ones: truncations (in step order) dealt an all-ones r1
    in element 0.  -> (results {name: [element]}, the r1 of every truncation [truncation][element])"""
    count = len(xvals)
    lay = ft.trig_layout(k, f, kappa, g, radians, want)
    width, fbits, groups, tree, modes, shifts = lay["width"], lay["ft"], lay["groups"], lay["tree"], lay["modes"], lay["shifts"]
    G, widths = len(groups), [w for _, w in groups]
    used, r1s = [0], []

    def triples(rows):
        used[0] += rows
        ta, tb = ([rnd.randrange(p) for _ in range(rows * count)] for _ in range(2))
        return ta, tb, [a * b % p for a, b in zip(ta, tb)]

    def planes(nbits, m):
        rows = [[rnd.getrandbits(1) for _ in range(count)] for _ in range(nbits)]
        if len(r1s) in all_ones:
            for i in range(m):
                rows[i][0] = 1
        r1s.append([sum(rows[i][e] << i for i in range(m)) for e in range(count)])
        return bc.flat(rows)

    v = [x % p for x in xvals]
    if radians:
        L, _, m = ft.turn_factor(k)
        prod = [x * L % p for x in v]
        tw = lay["turn_width"]
        masked, r1 = bc.run_fxp_mask(p, nl, prod, planes(tw + kappa, m), tw, m, kappa, count)
        v, = ok(bc.run_fxp(p, nl, 1, [prod, masked, r1, [pow(2, -m, p)]], [tw, m, kappa], [1], count))
    kv = lay["kv"]
    bd_planes = bc.flat([[rnd.getrandbits(1) for _ in range(count)] for _ in range(kv + kappa)])
    c, _ = bc.run_fxp_mask(p, nl, v, bd_planes, kv, fbits, kappa, count)
    y = bc.bodies_chain(bd, p, nl, c, bd_planes[:fbits * count], fbits, count, rnd)
    used[0] += bd.bit_triples(fbits)
    row = lambda r: y[r * count:(r + 1) * count]
    group_bits = [bc.flat([row(o + i) for i in range(w)]) for o, w in groups]
    flat_tables, table_off = [], []
    for ctab, stab in ft.trig_tables(k, f, g, radians):
        table_off.append(len(flat_tables))
        flat_tables += [t % p for t in ctab + stab]
    mode0 = modes[0] if tree else BOTH
    first = triples(tree[0] * triples_of(mode0)) if tree else ([0], [0], [0])
    pairs0 = tree[0] if tree else 0
    masked0, kept = [0] * (2 * triples_of(mode0) * pairs0 * count), [0] * (2 * G * count)
    stores = [[0] * (dx.demux_group_rows(w) * count) if w >= 2 else None for w in widths]
    pending = [(1, 0, groups[j][0], 0, table_off[j], j) for j, w in enumerate(widths) if w == 1]

    def lookups(last, masks, ta, tab):
        nonlocal masked0, kept
        for at in range(0, len(last), 8):
            chunk = last[at:at + 8]
            masked0, kept = ok(run_trig(p, nl, FINISH_LOOKUP_MASK, [y, masks or None, ta or None, tab or None, flat_tables, first[0], first[1]],
                                        [len(chunk), pairs0, G, mode0, split] + [x for grp in chunk for x in grp], [masked0 or None, kept], count))
            masked0 = masked0 or []

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
        lookups(last, masks, ta, tab)
    if pending:
        lookups(pending, [], [], [])
    names = tuple(want)
    if not tree:
        res = {"cos": kept[:count], "sin": kept[count:2 * count]}
        assert used[0] == lay["n_triples"]
        return {n: res[n] for n in names}, r1s
    trip = first
    carry = kept[(2 * G - 2) * count:] if G & 1 else None
    for i, products in enumerate(tree):
        mode, m = modes[i], shifts[i]
        comps = comps_of(mode) * products
        both = [x for _ in range(comps) for x in planes(width + kappa, m)]
        masked, sv = ok(run_trig(p, nl, CPRODUCTS_TRUNC, [masked0, trip[0], trip[1], trip[2], both], [products, mode, width, m, kappa], [comps, comps], count))
        inv = [pow(2, -m, p)]
        if i == len(tree) - 1:
            _, res = ok(run_trig(p, nl, TREE_STEP, [masked, sv, inv, None, None, None], [comps, 1, m, 0], [None, comps], count))
            out = {"cos": res[:count], "sin": res[count:]} if mode == BOTH else {"cos" if mode == COS else "sin": res}
            assert used[0] == lay["n_triples"] and len(r1s) == len(ft.trig_shifts(k, f, g, radians, want))
            return {n: out[n] for n in names}, r1s
        nmode = modes[i + 1]
        trip = triples(tree[i + 1] * triples_of(nmode))
        values = products + (carry is not None)
        masked0, carry = ok(run_trig(p, nl, TREE_STEP, [masked, sv, inv, carry, trip[0], trip[1]], [comps, 0, m, nmode],
                                     [2 * triples_of(nmode) * (values // 2), 2 if values & 1 else None], count))


# ---- GPU side ---------------------------------------------------------------------------------------------------------------------
def selftest_on_tensors(ctx, what, operands_, params, out_rows, count, outs_in=None):
    """hb_selftest_fxtrig over the limbs of device tensors (None: absent; a list of ints: constants in host memory) -> [(rows, count,
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
    prm = (ctypes.c_int64 * 53)(*(list(params) + [0] * (53 - len(params))))
    rc = load_library().hb_selftest_fxtrig(np_ptr(ints_to_limbs([p], p + 1, 8 * nl)), nl, what, ptrs, prm, optrs, count)
    assert rc == 0, rc
    return [None if o is None else ctx.torch.from_numpy(o[:r * count]).view(r, count, nl) for o, r in zip(outs, out_rows)]


def truncation_planes(lay, kappa):
    """-> [(first plane, planes)] of every truncation in step order from a trig_layout"""
    out = []
    for name, (start, stop) in sorted(lay["planes"].items(), key=lambda kv: kv[1]):
        if name == "turns":
            out.append((start, stop - start))
        elif name != "bit_decompose":
            nb = lay["width"] + kappa
            out += [(s, nb) for s in range(start, stop, nb)]
    return out

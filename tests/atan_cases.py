"""Shared by tests/test_fixedpoint_atan_host.py and tests/test_gpu_fixedpoint_atan.py: the hb_selftest_fxatan runner, the steps on Python
ints, the shape of the ladder restated, the operands of the end-to-end tests, and an INTEGER enclosure of atan2(y, x) 2^f built from
nothing of the module's (its own Taylor sums, its own Machin pi): no float decides a verdict."""
import ctypes
from fractions import Fraction

import bitdec_cases as bc
import division_cases as dc

SIGN_MASK, ABS, SELECT_MASK, SELECT, FIRST, LEVEL, POLY_MASK, ASSEMBLE, FINISH = range(9)
DEGREES = (3, 5, 7, 13, 23)
SHAPES = [(16, 8), (64, 32), (64, 61)]                                  # (k, f) of the structured comparisons: k = 2 f twice, f = k - 3


# ---- the shape of the ladder, restated ------------------------------------------------------------------------------------------
def levels(d):
    """bit_length((d - 1) / 2): the levels after level 0"""
    return ((d - 1) // 2).bit_length()


def level_odd(level, d):
    """the j of the odd powers t^(2j+1) level `level` >= 1 forms"""
    return [j for j in range(1 << (level - 1), 1 << level) if 2 * j + 1 <= d]


def level_square(level, d):
    return 1 <= level < levels(d)


def level_products(level, d):
    return 1 if level == 0 else len(level_odd(level, d)) + int(level_square(level, d))


def total_products(d):
    return sum(level_products(l, d) for l in range(levels(d) + 1))


# ---- the enclosure --------------------------------------------------------------------------------------------------------------
_SLACK = 1 << 20


def _atan_units(num, den, w):
    """atan(num / den) in units of 2^-w for 0 <= num / den <= 1/2, within _SLACK units: the alternating Taylor sum in integers, every
    operation floored (each step is off by a few units, and there are fewer than w steps)"""
    z = (num << w) // den
    z2 = z * z >> w
    total, term, n = 0, z, 0
    while term:
        total += -(term // (2 * n + 1)) if n & 1 else term // (2 * n + 1)
        term = term * z2 >> w
        n += 1
    return total


_CACHE = {}


def _pi_units(w):
    """(lo, hi) around pi 2^w: Machin, 16 atan(1/5) - 4 atan(1/239)"""
    if w not in _CACHE:
        mid = 16 * _atan_units(1, 5, w) - 4 * _atan_units(1, 239, w)
        _CACHE[w] = (mid - 20 * _SLACK, mid + 20 * _SLACK)
    return _CACHE[w]


def _atan_unit_interval(num, den, w):
    """(lo, hi) around atan(num / den) 2^w for 0 <= num <= den, den > 0: atan Q = atan(1/2) + atan((2 Q - 1) / (2 + Q)), the second argument
    in [-1/2, 1/3]"""
    a, b = 2 * num - den, 2 * den + num
    mid = _atan_units(1, 2, w) + (_atan_units(a, b, w) if a >= 0 else -_atan_units(-a, b, w))
    return mid - 2 * _SLACK, mid + 2 * _SLACK


def atan2_enclosure(y, x, f, turns=False):
    """-> (lo, hi) Fractions around atan2(y, x) 2^f (turns: over 2 pi), in ulps of 2^-f, f + 64 guard bits; (0, 0) -> (0, 0); y = 0, x < 0
    -> +pi, as math.atan2"""
    if x == 0 and y == 0:
        return Fraction(0), Fraction(0)
    w = 2 * f + 128
    ax, ay = abs(x), abs(y)
    c = ax < ay
    lo, hi = _atan_unit_interval(min(ax, ay), max(ax, ay), w)
    plo, phi = _pi_units(w)
    if turns:                                                               # the octant's angle over 2 pi; the rest is exact
        lo, hi, quarter = Fraction(max(lo, 0), 2 * phi), Fraction(hi, 2 * plo), (Fraction(1, 4), Fraction(1, 4))
        half = (Fraction(1, 2), Fraction(1, 2))
    else:
        lo, hi = Fraction(max(lo, 0), 1 << w), Fraction(hi, 1 << w)
        quarter, half = (Fraction(plo, 2 << w), Fraction(phi, 2 << w)), (Fraction(plo, 1 << w), Fraction(phi, 1 << w))
    if c:                                                                   # past the diagonal: pi / 2 - a
        lo, hi = quarter[0] - hi, quarter[1] - lo
    if x < 0:                                                               # beyond the y axis: pi - that
        lo, hi = half[0] - hi, half[1] - lo
    if y < 0:
        lo, hi = -hi, -lo
    return lo * (1 << f), hi * (1 << f)


def distance(value, enclosure):
    """how far the integer `value` can be from the enclosed number"""
    return max(abs(value - enclosure[0]), abs(value - enclosure[1]))


def centered(v, p):
    return v - p if v > p // 2 else v


# ---- operands -------------------------------------------------------------------------------------------------------------------
def r1_extremes(limits):
    """all-zero and all-ones r1 for every truncation: the two ends of what trunc_pr can add"""
    return [[0] * len(limits), [(1 << m) - 1 for m in limits]]


def quadrant_pairs(k, f):
    """(y, x): the origin, the axes, the diagonals, |x| = |y| +- 1, both tiny, one tiny and one huge, in all four quadrants"""
    top, one = (1 << (k - 1)) - 1, 1 << f
    mags = [(0, 0), (0, 1), (0, one), (0, top), (1, 0), (one, 0), (top, 0), (1, 1), (one, one), (top, top), (one, one + 1), (one, one - 1), (one + 1, one),
            (one - 1, one), (top, top - 1), (top - 1, top), (1, 2), (2, 1), (3, 2), (1, top), (top, 1), (2, top), (top, 3), (one, top), (top, one), (1, one), (one, 1)]
    return [(sy * a, sx * b) for a, b in mags for sy in (1, -1) for sx in (1, -1) if (sy == 1 or a) and (sx == 1 or b)]


def structured(rnd, k, f, extra):
    """quadrant_pairs and `extra` random pairs: half of them of random bit lengths, so that small and lopsided quotients are there"""
    lim = 1 << (k - 1)
    out = quadrant_pairs(k, f)
    for i in range(extra):
        if i & 1:
            out.append((rnd.randrange(-lim + 1, lim), rnd.randrange(-lim + 1, lim)))
        else:
            a, b = (rnd.randrange(1 << rnd.randrange(1, k)) for _ in range(2))
            out.append((rnd.choice((1, -1)) * a, rnd.choice((1, -1)) * b))
    return out


def e2e_pairs(rnd, k, f, count):
    """`count` pairs (y, x): (0, 0), the four half axes, the four diagonals, a neighbour of a diagonal in every quadrant, then random"""
    one, top = 1 << f, (1 << (k - 1)) - 1
    out = [(0, 0), (0, one), (0, -top), (one, 0), (-1, 0), (one, one), (top, -top), (-3, 3), (-one, -one), (one + 1, one), (one, -one - 1), (-top + 1, top), (-2, -3)]
    lim = 1 << (k - 1)
    while len(out) < count:
        out.append((rnd.randrange(-lim + 1, lim), rnd.randrange(-lim + 1, lim)))
    return out[:count]


# ---- the steps on Python ints -----------------------------------------------------------------------------------------------------
def _pairs_masked(p, pairs, ta, tb, count):
    out = []
    for r, (first, second) in enumerate(pairs):
        out += [(first[i] - ta[r * count + i]) % p for i in range(count)] + [(second[i] - tb[r * count + i]) % p for i in range(count)]
    return out


def _beaver_row(p, opened, ta, tb, tab, r, count):
    return [bc.beaver(opened[2 * r * count + i], opened[(2 * r + 1) * count + i], ta[r * count + i], tb[r * count + i], tab[r * count + i], p) for i in range(count)]


def sign_mask_on_ints(p, s, x, y, ta, tb, count):
    sx, sy = s[:count], s[count:]
    return _pairs_masked(p, [(sx, x), (sy, y), ([(1 - 2 * v) % p for v in sy], sx)], ta, tb, count)


def abs_on_ints(p, opened, ta, tb, tab, x, y, bits, k, kappa, count):
    """-> (masked [count], kept [5 count])"""
    prods = [_beaver_row(p, opened, ta, tb, tab, r, count) for r in range(3)]
    ax = [(v - 2 * q) % p for v, q in zip(x, prods[0])]
    ay = [(v - 2 * q) % p for v, q in zip(y, prods[1])]
    w = [(a - b) % p for a, b in zip(ax, ay)]
    m, nbits = k - 1, k + kappa
    r1 = [sum(bits[r * count + i] << r for r in range(m)) % p for i in range(count)]
    r2 = [sum(bits[r * count + i] << (r - m) for r in range(m, nbits)) for i in range(count)]
    masked = [(w[i] + (1 << (k - 1)) + r1[i] + (r2[i] << m)) % p for i in range(count)]
    return masked, ax + ay + prods[2] + w + r1


def select_mask_on_ints(p, c, w, sx, ta, tb, count):
    return _pairs_masked(p, [(c, w), ([(1 - 2 * v) % p for v in c], [(1 - 2 * v) % p for v in sx])], ta, tb, count)


def select_on_ints(p, opened, ta, tb, tab, ax, ay, count):
    cw, e1 = (_beaver_row(p, opened, ta, tb, tab, r, count) for r in range(2))
    return [(a + q) % p for a, q in zip(ay, cw)] + [(a - q) % p for a, q in zip(ax, cw)] + e1


def first_on_ints(p, q, shift, sy, e1, ta, tb, count):
    """-> (masked [4 count], t [count])"""
    t = [(v << shift) % p for v in q]
    return _pairs_masked(p, [(t, t), ([(1 - 2 * v) % p for v in sy], e1)], ta, tb, count), t


def trunc_on_ints(p, s, opened, m):
    inv = pow(2, -m, p)
    return [(a - c % (1 << m)) * inv % p for a, c in zip(s, opened)]


def level_on_ints(p, level, d, opened, s, m, ta, tb, powers, count):
    """-> (masked [2 next count], powers [(d + 1) / 2 count] updated)"""
    half = 1 << (level - 1) if level else 0
    powers = list(powers)
    new = trunc_on_ints(p, s, opened, m)
    done = level_products(level, d)
    for q in range(done - 1):
        powers[(half + q) * count:(half + q + 1) * count] = new[q * count:(q + 1) * count]
    square = new[(done - 1) * count:done * count]
    pairs = [(powers[q * count:(q + 1) * count], square) for q in range(len(level_odd(level + 1, d)))]
    if level_square(level + 1, d):
        pairs.append((square, square))
    return _pairs_masked(p, pairs, ta, tb, count), powers


def poly_mask_on_ints(p, d, opened, s, m_in, powers, coef, bits, width, m_out, kappa, count):
    """-> (masked [count], s_out [count])"""
    last = levels(d)
    half = 1 << (last - 1)
    powers = list(powers)
    new = trunc_on_ints(p, s, opened, m_in)
    for q in range(len(level_odd(last, d))):
        powers[(half + q) * count:(half + q + 1) * count] = new[q * count:(q + 1) * count]
    nbits = width + kappa
    masked, kept = [], []
    for i in range(count):
        poly = sum(coef[j] * powers[j * count + i] for j in range((d + 1) // 2)) % p
        r1 = sum(bits[r * count + i] << r for r in range(m_out))
        r2 = sum(bits[r * count + i] << (r - m_out) for r in range(m_out, nbits))
        masked.append((poly + (1 << (width - 1)) + r1 + (r2 << m_out)) % p)
        kept.append((poly + r1) % p)
    return masked, kept


def assemble_on_ints(p, opened, s, m, eopened, ea, eb, eab, sy, g, consts, ta, tb, count):
    """-> (masked [2 count], c [count])"""
    a = trunc_on_ints(p, s, opened, m)
    e = _beaver_row(p, eopened, ea, eb, eab, 0, count)
    c = [(consts[0] * g[i] + consts[1] * (1 - 2 * sy[i] - e[i])) % p for i in range(count)]
    return _pairs_masked(p, [(e, a)], ta, tb, count), c


def finish_on_ints(p, opened, ta, tb, tab, c, count):
    return [(v + q) % p for v, q in zip(c, _beaver_row(p, opened, ta, tb, tab, 0, count))]


# ---- the bodies on the host ---------------------------------------------------------------------------------------------------
SLOTS = 12                                                              # the assemble step's operands


def run_atan(p, nl, what, operands, params, outs, count):
    """hb_selftest_fxatan over lists of ints (bitdec_cases._run with room for twelve operands): params as the header lists them; outs: a
    row count (zero-filled), a list of ints (an array the step updates in place) or None -> (rc, [out lists])"""
    import numpy as np

    from honeybadgermpc_amd._capi import ints_to_limbs, limbs_to_ints, load_library, np_ptr

    nb = 8 * nl
    arrays = [None if o is None else ints_to_limbs(list(o) or [0], p, nb) for o in operands]
    ptrs = (ctypes.c_void_p * SLOTS)(*([None if x is None else x.ctypes.data for x in arrays] + [None] * (SLOTS - len(arrays))))
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
    rc = load_library().hb_selftest_fxatan(np_ptr(ints_to_limbs([p], p + 1, nb)), nl, what, ptrs, prm, optrs, count)
    return rc, [None if b is None else limbs_to_ints(b[:s], nb) for b, s in zip(bufs, sizes)]


ok = dc.ok


# ---- GPU side -------------------------------------------------------------------------------------------------------------------
def selftest_on_tensors(ctx, what, operands, params, out_rows, count, preset=()):
    """hb_selftest_fxatan over the limbs of device tensors (None: absent; a list of ints: constants in host memory), no Python ints in
    between -> [(rows, count, limbs) int64 tensors on the host], one an entry of out_rows (0: absent); preset: {index of an out: a
    tensor it starts from} for the arrays a step updates in place"""
    import numpy as np

    from honeybadgermpc_amd._capi import ints_to_limbs, load_library, np_ptr

    p, nl = ctx.modulus, ctx.n_limbs
    preset = dict(preset)
    keep = [None if o is None else (ints_to_limbs(list(o), p, 8 * nl) if isinstance(o, list) else np.ascontiguousarray(o.cpu().numpy())) for o in operands]
    ptrs = (ctypes.c_void_p * SLOTS)(*([None if a is None else a.ctypes.data for a in keep] + [None] * (SLOTS - len(keep))))
    outs = [np.zeros((max(r * count, 1), nl), dtype=np.int64) if r else None for r in out_rows]
    for i, t in preset.items():
        outs[i][:out_rows[i] * count] = t.cpu().numpy().reshape(-1, nl)
    optrs = (ctypes.c_void_p * 2)(*([None if o is None else o.ctypes.data for o in outs] + [None] * (2 - len(outs))))
    prm = (ctypes.c_int64 * 5)(*(list(params) + [0] * (5 - len(params))))
    rc = load_library().hb_selftest_fxatan(np_ptr(ints_to_limbs([p], p + 1, 8 * nl)), nl, what, ptrs, prm, optrs, count)
    assert rc == 0, rc
    return [None if o is None else ctx.torch.from_numpy(o[:r * count]).view(r, count, nl) for o, r in zip(outs, out_rows)]


def truncation_planes(lay, kappa):
    """-> [first plane of every truncation in step order] from an atan_layout: the division's (every range of its layout but the bit
    decomposition's), then the ladder's and L's"""
    base = lay["planes"]["div"][0]
    starts = [base + start for name, (start, stop) in sorted(lay["div"]["planes"].items(), key=lambda kv: kv[1]) if name != "bit_decompose"]
    nb = lay["width"] + kappa
    for name, (start, stop) in sorted(lay["planes"].items(), key=lambda kv: kv[1]):
        if name.startswith("level") or name == "poly":
            starts += list(range(start, stop, nb))
    return starts

"""
Sine and cosine of shared fixed-point numbers on the device (csrc/hb_fxtrig.hip, the demultiplexer of csrc/hb_demux.hip): cis(t) = cos t +
i sin t is multiplicative over the bits of t, as 2^x is, so the sine and cosine of an angle given in TURNS are a product of a few PUBLIC
table reads at one-hot vectors of groups of its fraction bits -- a product of complex factors -- on the (count, limbs) share arrays of
progs/fixedpoint.py.  The range reduction costs nothing: only the fraction bits of the turn count enter, the integer bits are never
decomposed, and the quadrant is the top two bits of the top group's index.  The reference has no circular functions; the pin here is
the mathematics: sincos_turns_model on Python ints, and the same steps composed from bit_decompose, demux, demux.lookup,
share_arithmetic and fixedpoint.trunc_mask / trunc_pr_finish.

Inputs are shares of a signed k-bit x with f fractional bits, value X = x / 2^f; ANY such x is in the contract.  sincos_turns gives shares
of sin(2 pi X) 2^f and cos(2 pi X) 2^f; sincos takes radians.  With ft the fraction bits of the turn count (f for turns, f + TURN_GUARD
for radians), s = ft + TRIG_GUARD the scale of the factors and g the largest width of a group:

    0 turns     (radians) y = trunc_pr(x L, m) with the public L = round(2^fl / (2 pi)), fl = k + FL_EXTRA, m = fl - TURN_GUARD: ft bits of
                the turn's fraction are left in y                                                      1 open, no triple
    a bits      bit_decompose(v, kv, ft), kv the declared signed width of v (k for turns).  Two's complement makes the low planes of a
                negative angle the fraction of its floor, which is the right one                       bit_opens(ft) opens
    b groups    the ft planes in G = ceil(ft / g) groups of widths as equal as possible, the wider ones first, least significant
                first, demultiplexed together, a level of all of them ONE open (demux_mask / demux_finish)    max demux_levels(w) opens
    c tables    PUBLIC, from Python ints, rounded exactly.  A group at bit offset o: C[j] = round(cos(2 pi j 2^(o-ft)) 2^s), S[j] likewise.
                The top group's entries are signed; finish_lookup_mask reads both tables through the SAME one-hot vector in the launch
                that finishes the group's last level, and writes the factor's rows of the first product's masked operands
    d tree      over the G complex factors: neighbours are paired, an odd last one is carried.  A complex product is Karatsuba over
                THREE ordinary Beaver triples, a.re b.re, a.im b.im, (a.re + a.im)(b.re + b.im); re and im are formed BEFORE truncation:
                two truncations a product.  A level is one open of the masked operands (6 rows a product), ONE launch
                cproducts_trunc, one open of the masked truncations, ONE launch tree_step                2 ceil(log2 G) opens
    e scales    inner levels truncate by s, the last by 2 s - f, straight to the result's scale.  With `want` of one component the last
                level keeps that component alone, ONE truncation; the cosine needs the first TWO triples only, the sine all three -- so a
                component asked for alone is, share for share, the one computed beside the other
    f G = 1     the tables are at scale f and the lookup IS the result

trig_opens = [1 for radians] + bit_opens(ft) + max_w demux_levels(w) + 2 ceil(log2 G).  The constants are set by rule (DESIGN.md section
3ae has the derivation and the table of bounds): TRIG_GUARD is the smallest value for which the table roundings and every inner
truncation contribute at most 1/4 ulp at 16 factors (_guard_rule); TURN_GUARD and FL_EXTRA the smallest for which the turn's
truncation and the rounding of L at |x| = 2^(k-1) contribute at most 1 ulp (_turn_rule).  trig_error_bound is an exact Fraction against
the real sine and cosine.

Preprocessing is handed in as tensors, consumed in step order from row 0; trig_layout names the row ranges.  `bits`: [radians: W_turn +
kappa,] kv + kappa for the bit decomposition, then width + kappa for every truncation of every tree level (re, then im, product after
product).  `triples = (p, q, pq)`: bit_triples(ft), then three a complex product (two on a last level that keeps the cosine alone).
`demux_triples`: one (ta, tab) a demultiplexer level as trig_demux_rows lists them (generate_trig_demux_triples).

Tensor level, one launch each on torch's current stream, nothing synchronises: finish_lookup_mask, cproducts_trunc, tree_step.
Protocol level, coroutines over an OpenCoalescer: sincos_turns, sincos, sin, cos, generate_trig_demux_triples.  Inputs and preprocessing
are left untouched; ValueError before anything is opened.
"""
from fractions import Fraction
from functools import lru_cache

import numpy as np

from ..share_arithmetic import mul as _ew_mul
from . import demux as dm
from .bit_decomposition import MAX_PLANES, bit_decompose, bit_opens, bit_triples
from .fixedpoint import F, K, KAPPA, _int, _inv2m, _planes, _planes_out, _triples, check_params, trunc_mask, trunc_pr_finish
from .fixedpoint_division import _open_rows, _ranges, _Rows
from .fixedpoint_exp import _centered, _fraction_groups, _signed, _tr, _tree, table_rows

TRIG_GUARD = 7                                                   # s = ft + TRIG_GUARD (_guard_rule)
TURN_GUARD = 3                                                   # radians: ft = f + TURN_GUARD (_turn_rule)
FL_EXTRA = 3                                                     # radians: fl = k + FL_EXTRA
MAX_GROUP_WIDTH = dm.MAX_BITS
MAX_GROUPS_A_LAUNCH, MAX_PRODUCTS = 8, 64                        # hb_fxtrig.hip's FXTRIG_MAX_GROUPS, FXTRIG_MAX_PRODUCTS
SPLITS = (1, 2, 4, 8, 16)                                        # lanes an element's table entries may be spread over
MODE_BOTH, MODE_COS, MODE_SIN = 0, 1, 2
_ROOT2 = Fraction(17, 12)                                        # >= sqrt(2): 289 / 144 > 2


# ---- host functions: exact constants -------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _pi(prec):
    """-> (lo, hi) ints enclosing pi 2^prec, by Machin: pi = 16 atan(1/5) - 4 atan(1/239), every term floored (below 1 short each)"""
    work = prec + 32

    def atan_inv(x):
        total, power, n, terms = 0, (1 << work) // x, 0, 0
        while power:
            total += -(power // (2 * n + 1)) if n & 1 else power // (2 * n + 1)
            power //= x * x
            n, terms = n + 1, terms + 1
        return total, 2 * terms + 2                                         # the sum and a bound of its error in units of 2^-work

    a, ea = atan_inv(5)
    b, eb = atan_inv(239)
    mid, err = 16 * a - 4 * b, 16 * ea + 4 * eb
    return (mid - err) >> 32, ((mid + err) >> 32) + 1


def _series(theta, work):
    """-> (sin, cos) of theta / 2^work for an int 0 <= theta <= 2^work, in units of 2^-work, each within 2^20 units: the alternating
    Taylor series until a term floors to 0; every term is off by at most three units more than the one before it"""
    t2 = theta * theta >> work
    sin = term = theta
    n = 1
    while term:
        term = (term * t2 >> work) // ((n + 1) * (n + 2))
        sin += term if n & 2 else -term
        n += 2
    cos = term = 1 << work
    n = 0
    while term:
        term = (term * t2 >> work) // ((n + 1) * (n + 2))
        cos += term if n & 2 else -term
        n += 2
    return sin, cos


def _cis(num, bits, prec):
    """-> ((cos lo, cos hi), (sin lo, sin hi)) enclosing cos and sin of 2 pi num / 2^bits, times 2^prec: the angle is reduced to the
    first octant, where the sine grows and the cosine falls, so the ends of the angle's enclosure give the ends of theirs"""
    if bits < 3:
        num, bits = num << (3 - bits), 3
    work, n = prec + 64, 1 << bits
    a = num % n
    quadrant, r = divmod(a, n >> 2)
    swap = r > n >> 3
    if swap:
        r = (n >> 2) - r
    plo, phi = _pi(work)
    tlo, thi = (2 * plo * r) >> bits, ((2 * phi * r) >> bits) + 1
    slack = 1 << 21
    (s_lo, c_hi), (s_hi, c_lo) = _series(tlo, work), _series(thi, work)
    sin = ((s_lo - slack) >> 64, ((s_hi + slack) >> 64) + 1)
    cos = ((c_lo - slack) >> 64, ((c_hi + slack) >> 64) + 1)
    if swap:
        sin, cos = cos, sin
    neg = lambda iv: (-iv[1], -iv[0])
    return [(cos, sin), (neg(sin), cos), (neg(cos), neg(sin)), (sin, neg(cos))][quadrant]


def _round_cis(num, bits, s):
    """(round(cos(2 pi num / 2^bits) 2^s), round(sin ...)), exactly: the enclosure is widened until both ends round alike.  (The only
    rational values are 0 and +-1, at the quarter turns, which are no rounding boundary.)"""
    prec = s + 64
    while True:
        out = []
        for lo, hi in _cis(num, bits, prec):
            a, b = ((lo >> (prec - s - 1)) + 1) >> 1, ((hi >> (prec - s - 1)) + 1) >> 1
            out.append(a if a == b else None)
        if None not in out:
            return tuple(out)
        prec *= 2


@lru_cache(maxsize=None)
def turn_factor(k):
    """(L, fl, m): the public L = round(2^fl / (2 pi)) of the radian forms, fl = k + FL_EXTRA, and the shift m = fl - TURN_GUARD"""
    fl = _int(k, "k") + FL_EXTRA
    lo, hi = _pi(fl + 64)
    top = 1 << (2 * fl + 128)                                                   # 2^fl / (2 pi) = top / (pi 2^(fl + 64)) / 2^65
    a, b = ((top // hi >> 64) + 1) >> 1, ((top // lo + 1 >> 64) + 1) >> 1       # rounded from either end of the enclosure
    if a != b:
        raise ArithmeticError("2^fl / (2 pi) lies on a rounding boundary")
    return a, fl, fl - TURN_GUARD


# ---- host functions: groups, tables, counts --------------------------------------------------------------------------------
def _check_kf(k, f):
    k, f = _int(k, "k"), _int(f, "f")
    if k < 2 or not 1 <= f <= k - 1:
        raise ValueError(f"needs k >= 2 and 1 <= f <= k - 1, got k = {k}, f = {f}")
    if f + TURN_GUARD > MAX_PLANES:
        raise ValueError(f"at most {MAX_PLANES} bits are decomposed, got {f + TURN_GUARD}")


def _ft(f, radians):
    return f + TURN_GUARD if radians else f


def _g(k, f, g, radians):
    if g is None:
        return default_group_width(k, f, radians)
    if not 1 <= _int(g, "g") <= MAX_GROUP_WIDTH:
        raise ValueError(f"needs 1 <= g <= {MAX_GROUP_WIDTH}, got {g}")
    return g


def _mode(want):
    try:
        names = tuple(want)
    except TypeError:
        names = None
    if not names or len(set(names)) != len(names) or any(n not in ("sin", "cos") for n in names):
        raise ValueError(f"want: expected one or both of 'sin' and 'cos', each once, got {want!r}")
    return names, (MODE_BOTH if len(names) == 2 else MODE_COS if names[0] == "cos" else MODE_SIN)


def mode_triples(mode):
    return 2 if mode == MODE_COS else 3


def mode_comps(mode):
    return 2 if mode == MODE_BOTH else 1


def _open_count(k, ft, g, radians):
    widths = [w for _, w in _fraction_groups(ft, g)]
    return (1 if radians else 0) + bit_opens(ft) + max(dm.demux_levels(w) for w in widths) + 2 * len(_tree(len(widths)))


@lru_cache(maxsize=None)
def default_group_width(k=K, f=F, radians=False):
    """the smallest g among those with the fewest opens"""
    _check_kf(k, f)
    ft = _ft(f, radians)
    return min(range(1, min(ft, MAX_GROUP_WIDTH) + 1), key=lambda g: (_open_count(k, ft, g, radians), g))


def trig_groups(k=K, f=F, g=None, radians=False):
    """-> [(bit offset, width)] of the G = ceil(ft / g) groups of the turn's fraction, least significant first"""
    _check_kf(k, f)
    return _fraction_groups(_ft(f, radians), _g(k, f, g, radians))


@lru_cache(maxsize=None)
def _tables(ft, f, g):
    groups = _fraction_groups(ft, g)
    s = ft + TRIG_GUARD if len(groups) > 1 else f
    out = []
    for o, w in groups:
        pairs = [_round_cis(j << o, ft, s) for j in range(1 << w)]
        out.append(([c for c, _ in pairs], [v for _, v in pairs]))
    return out


def trig_tables(k=K, f=F, g=None, radians=False):
    """-> [(C, S)] a group: C[j] = round(cos(2 pi j 2^(o-ft)) 2^s), S[j] likewise with sin, signed Python ints, j < 2^w; s = ft + TRIG_GUARD,
    or f where there is ONE group (the lookup is the result)"""
    _check_kf(k, f)
    return [(list(c), list(s)) for c, s in _tables(_ft(f, radians), f, _g(k, f, g, radians))]


def trig_width(k=K, f=F, radians=False):
    """the signed width of every truncation of the tree: a component of a product of two factors of modulus about 2^s is below 2^(2s+1)"""
    return 2 * (_ft(f, radians) + TRIG_GUARD) + 2


def _turn_widths(k):
    """(W, kv): the signed widths of x L and of y = trunc_pr(x L, m), from L and m"""
    L, _, m = turn_factor(k)
    top = L << (k - 1)
    return top.bit_length() + 1, ((top >> m) + 2).bit_length() + 1


def trig_demux_rows(k=K, f=F, g=None, radians=False):
    """-> [[(group, opened rows, products)]] level by level: what the (ta, tab) of that level of demux_triples must hold, in this order"""
    _check_kf(k, f)
    widths = [w for _, w in _fraction_groups(_ft(f, radians), _g(k, f, g, radians))]
    return [[(j, dm.demux_opened(w, l), dm.demux_products(w, l)) for j, w in enumerate(widths) if l < dm.demux_levels(w)]
            for l in range(max(dm.demux_levels(w) for w in widths))]


def trig_layout(k=K, f=F, kappa=KAPPA, g=None, radians=False, want=("sin", "cos")):
    """-> {"g", "ft", "s", "groups", "width", "kv", "tree", "modes", "shifts", "planes": {name: (start, stop)}, "triples": {...}, "n_planes",
    "n_triples", "demux_rows", "demux_opened", "demux_products", "opens"}: the rows of `bits` and of the triple tensors each step consumes,
    in step order from row 0 ([turns,] bit_decompose, tree<i>), the complex products, the mode and the shift of every tree level, and
    what the demultiplexer triples hold"""
    _check_kf(k, f)
    _int(kappa, "kappa")
    _, mode = _mode(want)
    g = _g(k, f, g, radians)
    ft = _ft(f, radians)
    groups = _fraction_groups(ft, g)
    s = ft + TRIG_GUARD
    tree = _tree(len(groups))
    modes = [MODE_BOTH] * (len(tree) - 1) + [mode] if tree else []
    shifts = [s] * (len(tree) - 1) + [2 * s - f] if tree else []
    width = trig_width(k, f, radians)
    wt, kv = _turn_widths(k) if radians else (0, k)
    planes = ([("turns", wt + kappa)] if radians else []) + [("bit_decompose", kv + kappa)]
    triples = [("bit_decompose", bit_triples(ft))]
    for i, (products, md) in enumerate(zip(tree, modes)):
        planes.append((f"tree{i}", products * mode_comps(md) * (width + kappa)))
        triples.append((f"tree{i}", products * mode_triples(md)))
    p_ranges, n_planes = _ranges(planes)
    t_ranges, n_triples = _ranges(triples)
    rows = trig_demux_rows(k, f, g, radians)
    return {"g": g, "ft": ft, "s": s if tree else f, "groups": groups, "width": width, "kv": kv, "turn_width": wt, "tree": tree, "modes": modes, "shifts": shifts,
            "planes": p_ranges, "triples": t_ranges, "n_planes": n_planes, "n_triples": n_triples, "demux_rows": rows,
            "demux_opened": sum(o for lv in rows for _, o, _ in lv), "demux_products": sum(q for lv in rows for _, _, q in lv),
            "opens": _open_count(k, ft, g, radians)}


def trig_planes(k=K, f=F, kappa=KAPPA, g=None, radians=False, want=("sin", "cos")):
    return trig_layout(k, f, kappa, g, radians, want)["n_planes"]


def trig_triples(k=K, f=F, g=None, radians=False, want=("sin", "cos")):
    return trig_layout(k, f, 0, g, radians, want)["n_triples"]


def trig_opens(k=K, f=F, g=None, radians=False):
    return trig_layout(k, f, 0, g, radians)["opens"]


def trig_shifts(k=K, f=F, g=None, radians=False, want=("sin", "cos")):
    """m of every truncation in step order: [radians: the turn's,] then level by level, product by product, re before im"""
    lay = trig_layout(k, f, 0, g, radians, want)
    out = [turn_factor(k)[2]] if radians else []
    for products, md, m in zip(lay["tree"], lay["modes"], lay["shifts"]):
        out += [m] * (products * mode_comps(md))
    return out


# ---- host functions: bounds ------------------------------------------------------------------------------------------------------
def _tree_error(n_factors, guard, ft):
    """>= 2^ft times the Euclidean error of the product of n_factors factors before the LAST level's truncation, an exact Fraction, with
    s = ft + guard: a table entry is off by at most 1/2 in either component, sqrt(2) / 2 at scale s; a product of two unit factors off by
    a and b is off by a + b + a b, and an inner truncation adds less than 1 to either component, sqrt(2) at scale s.  17 / 12 >= sqrt(2)."""
    unit = Fraction(1, 1 << guard)                                              # 2^ft 2^-s
    eps = [_ROOT2 * unit / 2] * n_factors
    while len(eps) > 1:
        last = len(eps) <= 2
        nxt = [eps[2 * q] + eps[2 * q + 1] + eps[2 * q] * eps[2 * q + 1] / (1 << ft) + (0 if last else _ROOT2 * unit) for q in range(len(eps) // 2)]
        eps = nxt + ([eps[-1]] if len(eps) & 1 else [])
    return eps[0]


def _guard_rule(guard, n_factors=16):
    """TRIG_GUARD's rule: the table roundings and every inner truncation contribute at most 1/4 ulp at 16 factors (ft = 16, the fewest
    fraction bits that make 16 factors: the second-order terms are largest there)"""
    return _tree_error(n_factors, guard, n_factors) <= Fraction(1, 4)


def _two_pi_upper():
    lo, hi = _pi(128)
    return Fraction(2 * hi, 1 << 128)


def _turn_error(turn_guard, fl_extra):
    """the turn's truncation, in (-1, 1] units of 2^-ft turns, and the rounding of L, at most 1/2, at |x| = 2^(k-1): 2 pi (2^-turn_guard +
    2^(-2 - fl_extra)) ulps of the result (sine and cosine are 1-Lipschitz in the angle)"""
    return _two_pi_upper() * (Fraction(1, 1 << turn_guard) + Fraction(1, 1 << (2 + fl_extra)))


def _turn_rule(turn_guard, fl_extra):
    return _turn_error(turn_guard, fl_extra) <= 1


def trig_error_bound(k=K, f=F, g=None, radians=False):
    """|result - sin(2 pi X) 2^f| and |result - cos(2 pi X) 2^f| (radians: sin X, cos X) in ulps of 2^-f against the exact real, an exact
    Fraction, for every signed k-bit x: the tree before its last truncation, that truncation's unit and, for radians, the turn's error.
    One group: the table's rounding alone, 1/2."""
    _check_kf(k, f)
    ft = _ft(f, radians)
    n = len(_fraction_groups(ft, _g(k, f, g, radians)))
    own = Fraction(1, 2) if n == 1 else _tree_error(n, TRIG_GUARD, ft) / (1 << (ft - f)) + 1
    return own + (_turn_error(TURN_GUARD, FL_EXTRA) if radians else 0)


# ---- host functions: the models --------------------------------------------------------------------------------------------------
def _core_model(v, p, ft, f, g, r1s, mode):
    """the low ft bits of the signed int v, in two's complement, are what the bit decomposition gives -> (re, im) residues (None: dropped)"""
    groups, tables = _fraction_groups(ft, g), _tables(ft, f, g)
    s, width = ft + TRIG_GUARD, 2 * (ft + TRIG_GUARD) + 2
    frac = v % (1 << ft)
    vals = [(tables[j][0][(frac >> o) & ((1 << w) - 1)] % p, tables[j][1][(frac >> o) & ((1 << w) - 1)] % p) for j, (o, w) in enumerate(groups)]
    r1s = iter(r1s)
    while len(vals) > 1:
        last = len(vals) <= 2
        m, md = (2 * s - f, mode) if last else (s, MODE_BOTH)
        nxt = []
        for q in range(len(vals) // 2):
            (ar, ai), (br, bi) = vals[2 * q], vals[2 * q + 1]
            re = _tr((ar * br - ai * bi) % p, next(r1s), p, width, m) if md != MODE_SIN else None
            im = _tr((ar * bi + ai * br) % p, next(r1s), p, width, m) if md != MODE_COS else None
            nxt.append((re, im))
        vals = nxt + ([vals[-1]] if len(vals) & 1 else [])
    return vals[0]


@lru_cache(maxsize=64)
def _model_plan(p, k, f, g, radians, names):
    lay = trig_layout(k, f, 0, g, radians, names)
    _check_room(p, lay, k, f, 0, radians)
    return lay, trig_shifts(k, f, lay["g"], radians, names)


def _check_model(p, k, f, g, r1s, radians, want):
    names, mode = _mode(want)
    lay, limits = _model_plan(p, k, f, g, radians, names)
    r1s = [_int(r, "r1") for r in r1s]
    if len(r1s) != len(limits) or any(not 0 <= r < 1 << m for r, m in zip(r1s, limits)):
        raise ValueError(f"r1s: expected {len(limits)} values below 2^m for m = {limits}")
    return lay, r1s, names, mode


def _named(names, re_im):
    return tuple(re_im[0] if n == "cos" else re_im[1] for n in names)


def sincos_turns_model(x, p, k=K, f=F, r1s=(), g=None, want=("sin", "cos")):
    """What sincos_turns' results open to, residues mod p in the order of `want`: x a residue (or signed int) of a signed k-bit value; r1s
    the dealt r1 of every truncation in step order (trig_shifts).  Python ints only."""
    lay, r1s, names, mode = _check_model(p, k, f, g, r1s, False, want)
    return _named(names, _core_model(_signed(x, p, k), p, f, f, lay["g"], r1s, mode))


def sincos_model(x, p, k=K, f=F, r1s=(), g=None, want=("sin", "cos")):
    """What sincos' results open to: r1s[0] is the r1 of the turn's truncation, then the tree's"""
    lay, r1s, names, mode = _check_model(p, k, f, g, r1s, True, want)
    L, _, m = turn_factor(k)
    y = _centered(_tr(_signed(x, p, k) * L % p, r1s[0], p, lay["turn_width"], m), p)
    return _named(names, _core_model(y, p, lay["ft"], f, lay["g"], r1s[1:], mode))


# ---- tensor level ----------------------------------------------------------------------------------------------------------
def lookup_split(count):
    """the lanes finish_lookup_mask spreads an element's table entries over when the caller names none: the best split measured on an
    MI355X at BLS12-381 at 2^12, 2^14, 2^16, 2^18 and 2^20 elements for merges of 256 and of 16 entries (DESIGN.md section 3ae has the
    numbers: 16 lanes are 10 times faster than one at 2^12 elements, one lane is the fastest from 2^18 on); between those counts the
    rule is a guess"""
    return 16 if count <= 1 << 12 else 8 if count <= 1 << 14 else 2 if count <= 1 << 16 else 1


def finish_lookup_mask(ctx, groups, tables, pairs, kept_slots, count, mode=MODE_BOTH, split=None, bits=None, opened=None, ta=None, tab=None, nxt=None, out=None,
                       kept_out=None):
    """The last demultiplexer level of up to 8 groups, the read of their two public tables and the masks of the first complex product, ONE
    launch.  groups: [(wl, wh, open_off, prod_off, table_off, slot)] as fixedpoint_exp.finish_lookup_mask takes them; entries table_off .. of
    tables (fixedpoint_exp.table_rows) are the group's cos table, 2^(wl + wh) entries, and then its sin table.  The factor (re, im) goes to
    rows 2 slot, 2 slot + 1 of kept (2 kept_slots, count, limbs) and, for slot < 2 pairs, its masked rows as operand slot & 1 of product
    slot / 2 of a level in `mode` to masked (2 tp pairs, count, limbs), tp = mode_triples(mode); nxt = (a, b), (tp pairs, count, limbs)
    each.  split: the lanes an element's entries are spread over (SPLITS; None: lookup_split(count)); every split gives the same bits.
    -> (masked, kept); rows that no group names are left as out / kept_out had them (uninitialised without)."""
    try:
        groups = [tuple(_int(v, "groups") for v in grp) for grp in groups]
        if any(len(grp) != 6 for grp in groups):
            raise TypeError
    except TypeError:
        raise ValueError("groups: expected a list of (wl, wh, open_off, prod_off, table_off, slot)") from None
    if not 1 <= len(groups) <= MAX_GROUPS_A_LAUNCH:
        raise ValueError(f"groups: 1 .. {MAX_GROUPS_A_LAUNCH} a launch, got {len(groups)}")
    if not 0 <= _int(pairs, "pairs") <= MAX_PRODUCTS or not 1 <= _int(kept_slots, "kept_slots") <= 2 * MAX_PRODUCTS + 1 or _int(count, "count") < 0:
        raise ValueError(f"needs 0 <= pairs <= {MAX_PRODUCTS}, 1 <= kept_slots <= {2 * MAX_PRODUCTS + 1} and count >= 0, got {pairs}, {kept_slots}, {count}")
    if mode not in (MODE_BOTH, MODE_COS, MODE_SIN):
        raise ValueError(f"mode: expected 0, 1 or 2, got {mode!r}")
    split = lookup_split(count) if split is None else split
    if split not in SPLITS:
        raise ValueError(f"split: expected one of {SPLITS}, got {split!r}")
    tp = mode_triples(mode)
    tables = ctx.elems(tables, what="tables")
    need = {"bits": 0, "open": 0, "prod": 0}
    slots = set()
    for wl, wh, oo, po, to, slot in groups:
        linear = (wl, wh) == (1, 0)
        if not linear and (wl < 1 or wh < 1 or wl + wh > MAX_GROUP_WIDTH):
            raise ValueError(f"groups: a merge needs 1 <= wl, wh and wl + wh <= {MAX_GROUP_WIDTH} (or (1, 0): one bit), got ({wl}, {wh})")
        if min(oo, po, to) < 0 or not 0 <= slot < kept_slots or slot in slots:
            raise ValueError(f"groups: offsets must not be negative and every group needs a slot of its own below {kept_slots}")
        slots.add(slot)
        if to + (2 << (wl + wh)) > tables.numel() // ctx.n_limbs:
            raise ValueError(f"tables: the group at entry {to} needs {2 << (wl + wh)} entries, the tensor holds {tables.numel() // ctx.n_limbs}")
        if linear:
            need["bits"] = max(need["bits"], oo + 1)
        else:
            need["open"], need["prod"] = max(need["open"], oo + (1 << wl) + (1 << wh)), max(need["prod"], po + (1 << (wl + wh)))
    bits_t = opened_t = ta_t = tab_t = na = nb = None
    if need["bits"]:
        bits_t, _ = _planes(ctx, bits, need["bits"], count, "bits")
    if need["open"]:
        ta_t, _ = _planes(ctx, ta, need["open"], count, "ta")
        tab_t, _ = _planes(ctx, tab, need["prod"], count, "tab")
        opened_t = ctx.elems(opened, what="opened")
        if opened_t.numel() < need["open"] * count * ctx.n_limbs:
            raise ValueError(f"opened: expected at least {need['open']} rows of {count} elements, got {opened_t.numel() // ctx.n_limbs} elements")
    masks = any(slot < 2 * pairs for slot in slots)
    if masks:
        try:
            a, b = nxt
        except (TypeError, ValueError):
            raise ValueError("nxt: expected (a, b)") from None
        na, _ = _planes(ctx, a, tp * pairs, count, "nxt a")
        nb, _ = _planes(ctx, b, tp * pairs, count, "nxt b")
    o0 = _planes_out(ctx, out, 2 * tp * pairs, count, "out") if masks or out is not None else None
    o1 = _planes_out(ctx, kept_out, 2 * kept_slots, count, "kept_out")
    desc = np.ascontiguousarray([v for grp in groups for v in grp], dtype=np.int32)
    P = lambda t: None if t is None else ctx.ptr(t)
    ctx.check(ctx.lib.hb_fxtrig_finish_lookup_mask(ctx.h, P(bits_t), P(opened_t), P(ta_t), P(tab_t), P(tables), len(groups), desc.ctypes.data, P(na), P(nb), pairs, mode, split,
                                                   P(o0), P(o1), kept_slots, count, ctx.stream()), "hb_fxtrig_finish_lookup_mask")
    return (None if o0 is None else o0.view(2 * tp * pairs, count, ctx.n_limbs)), o1.view(2 * kept_slots, count, ctx.n_limbs)


def cproducts_trunc(ctx, products, mode, opened, ta, tb, tab, bits, width, m, kappa=KAPPA, out=None):
    """The complex products of a tree level to their truncation masks, ONE launch: 1 <= products <= 64 in `mode`; opened (2 tp products,
    count, limbs) or flat, the masked operands opened; ta, tb, tab (tp products, count, limbs); bits (comps products (width + kappa), count,
    limbs).  -> (masked, s), (comps products, count, limbs) each, re before im: trunc_mask of every kept component, the array to open, and
    component + r1.  out: a pair."""
    if not 1 <= _int(products, "products") <= MAX_PRODUCTS or mode not in (MODE_BOTH, MODE_COS, MODE_SIN):
        raise ValueError(f"needs 1 <= products <= {MAX_PRODUCTS} and a mode 0, 1 or 2, got {products}, {mode!r}")
    tp, comps = mode_triples(mode) * products, mode_comps(mode) * products
    ta = ctx.elems(ta, what="ta")
    if ta.dim() != 3 or ta.shape[0] != tp:
        raise ValueError(f"ta: expected shape ({tp}, count, {ctx.n_limbs}), got {tuple(ta.shape)}")
    count = ta.shape[1]
    tb, tab = (_planes(ctx, v, tp, count, w, exact=True)[0] for v, w in ((tb, "tb"), (tab, "tab")))
    opened = ctx.elems(opened, 2 * tp * count, what="opened")
    check_params(ctx.modulus, width, m, kappa)
    bits, _ = _planes(ctx, bits, comps * (width + kappa), count, "bits")
    g0, g1 = (None, None) if out is None else out
    o0, o1 = _planes_out(ctx, g0, comps, count, "out masked"), _planes_out(ctx, g1, comps, count, "out s")
    P = ctx.ptr
    ctx.check(ctx.lib.hb_fxtrig_cproducts_trunc(ctx.h, products, mode, P(opened), P(ta), P(tb), P(tab), P(bits), width, m, kappa, P(o0), P(o1), count, ctx.stream()),
              "hb_fxtrig_cproducts_trunc")
    return o0.view(comps, count, ctx.n_limbs), o1.view(comps, count, ctx.n_limbs)


def tree_step(ctx, opened, s, m, mode=MODE_BOTH, ta=None, tb=None, carry=None, final=False, out=None):
    """After the open of masked truncations, ONE launch: t_j = (s_j - (opened_j mod 2^m)) / 2^m for the rows of s (rows, count, limbs), 1 <=
    rows <= 128, and opened (flat is fine).  final: -> (None, t), the results.  Otherwise the complex values are (t_0, t_1), (t_2, t_3) ..
    and, last, carry (2, count, limbs) if given; value u is operand u & 1 of product u // 2 of the next level, in `mode`, masked against
    ta, tb ((tp pairs, count, limbs) each); an odd last value is kept (2, count, limbs).  -> (masked, kept), None where there is no pair
    or no odd value.  out: a pair."""
    if not 0 < _int(m, "m") <= ctx.modulus.bit_length() - 2:
        raise ValueError(f"needs 0 < m <= {ctx.modulus.bit_length() - 2}, got {m}")
    if mode not in (MODE_BOTH, MODE_COS, MODE_SIN):
        raise ValueError(f"mode: expected 0, 1 or 2, got {mode!r}")
    s = ctx.elems(s, what="s")
    if s.dim() != 3 or not 1 <= s.shape[0] <= 2 * MAX_PRODUCTS:
        raise ValueError(f"s: expected shape (1 <= rows <= {2 * MAX_PRODUCTS}, count, {ctx.n_limbs}), got {tuple(s.shape)}")
    rows, count = s.shape[0], s.shape[1]
    if final and carry is not None or not final and rows & 1:
        raise ValueError("a final step carries nothing; any other takes two rows a complex value")
    opened = ctx.elems(opened, rows * count, what="opened")
    carry_t = None if carry is None else _planes(ctx, carry, 2, count, "carry", exact=True)[0]
    values = 0 if final else rows // 2 + (carry is not None)
    pairs, odd, tp = values // 2, values & 1, mode_triples(mode)
    ta_t = tb_t = None
    if pairs:
        ta_t, _ = _planes(ctx, ta, tp * pairs, count, "ta", exact=True)
        tb_t, _ = _planes(ctx, tb, tp * pairs, count, "tb", exact=True)
    g0, g1 = (None, None) if out is None else out
    kept_rows = rows if final else 2
    o0 = _planes_out(ctx, g0, 2 * tp * pairs, count, "out masked") if pairs else None
    o1 = _planes_out(ctx, g1, kept_rows, count, "out kept") if odd or final else None
    inv = _inv2m(ctx, m)
    P = lambda t: None if t is None else ctx.ptr(t)
    ctx.check(ctx.lib.hb_fxtrig_tree_step(ctx.h, rows, int(bool(final)), P(opened), P(s), m, inv.ctypes.data, P(carry_t), mode, P(ta_t), P(tb_t), P(o0), P(o1), count,
                                          ctx.stream()), "hb_fxtrig_tree_step")
    return (None if o0 is None else o0.view(2 * tp * pairs, count, ctx.n_limbs)), (None if o1 is None else o1.view(kept_rows, count, ctx.n_limbs))


# ---- protocols over an OpenCoalescer ---------------------------------------------------------------------------------------
def _check_room(p, lay, k, f, kappa, radians):
    """ValueError for parameters the modulus or the 256-bit truncation width has no room for"""
    check_params(p, lay["kv"], lay["ft"], kappa, full=True)
    widths = [lay["width"]] if lay["tree"] else []
    for m in set(lay["shifts"]):
        check_params(p, lay["width"], m, kappa)
    if radians:
        check_params(p, lay["turn_width"], turn_factor(k)[2], kappa)
        widths.append(lay["turn_width"])
    if max(widths, default=0) > 256:
        raise ValueError(f"the truncations need {max(widths)} bits: at most 256")
    if max(lay["tree"], default=0) > MAX_PRODUCTS:
        raise ValueError(f"g = {lay['g']} makes {len(lay['groups'])} factors: at most {2 * MAX_PRODUCTS + 1}")
    if 1 << (lay["s"] + 1) >= p:
        raise ValueError("the table entries do not fit below the modulus")


def _demux_prep(ctx, demux_triples, lay, count):
    rows = lay["demux_rows"]
    try:
        pairs = [tuple(pair) for pair in demux_triples]
        if len(pairs) < len(rows) or any(len(pair) != 2 for pair in pairs[:len(rows)]):
            raise TypeError
    except TypeError:
        raise ValueError(f"demux_triples: expected a list of {len(rows)} pairs (ta, tab), one a level") from None
    return [(_planes(ctx, ta, sum(o for _, o, _ in lv), count, f"demux_triples[{l}] ta")[0], _planes(ctx, tab, sum(q for _, _, q in lv), count, f"demux_triples[{l}] tab")[0])
            for l, (lv, (ta, tab)) in enumerate(zip(rows, pairs))]


async def _core(co, v, rows, prep, lay, f, kappa, split):
    """steps a to f on a value whose low ft bits are the turn's fraction -> (re, im) share arrays (None: dropped)"""
    ctx, t = co.ctx, co.ctx.torch
    count, L = v.shape[0], ctx.n_limbs
    ft, width, g, groups = lay["ft"], lay["width"], lay["g"], lay["groups"]
    nb, G = width + kappa, len(groups)
    widths = [w for _, w in groups]
    planes = await bit_decompose(co, v, rows.planes(lay["kv"] + kappa), rows.take(bit_triples(ft)), lay["kv"], ft, kappa)
    group_bits = [planes[o:o + w] for o, w in groups]
    tables, table_off = table_rows(ctx, [c + s for c, s in _tables(ft, f, g)])
    tree, modes, shifts = lay["tree"], lay["modes"], lay["shifts"]
    first = rows.take(tree[0] * mode_triples(modes[0])) if tree else None
    pairs0 = tree[0] if tree else 0
    masked0 = t.empty((2 * mode_triples(modes[0]) * pairs0, count, L), dtype=t.int64, device=ctx.tdev) if tree else None
    kept = t.empty((2 * G, count, L), dtype=t.int64, device=ctx.tdev)
    # the merged groups of the levels before the last, as fixedpoint_exp keeps them: a group's last 2^w rows are never written or read
    used = [dm.demux_group_rows(w) - (1 << w) if w >= 2 else 0 for w in widths]
    pool = t.empty((sum(used) + (1 << max(widths)), count, L), dtype=t.int64, device=ctx.tdev)
    stores = [pool[sum(used[:j]):sum(used[:j]) + dm.demux_group_rows(w)] if w >= 2 else None for j, w in enumerate(widths)]
    pending = [(1, 0, groups[j][0], 0, table_off[j], j) for j, w in enumerate(widths) if w == 1]       # groups of one bit: formed by the first launch

    def lookups(descs, opened, ta, tab):
        descs = pending + descs
        pending.clear()
        for at in range(0, len(descs), MAX_GROUPS_A_LAUNCH):
            finish_lookup_mask(ctx, descs[at:at + MAX_GROUPS_A_LAUNCH], tables, pairs0, G, count, mode=modes[0] if tree else MODE_BOTH, split=split, bits=planes, opened=opened,
                               ta=ta, tab=tab, nxt=(first[0], first[1]) if tree else None, out=masked0, kept_out=kept)

    for level, (lv, (ta, tab)) in enumerate(zip(lay["demux_rows"], prep)):
        masks, oo, po, spans = [], 0, 0, []
        for j, orows, prows in lv:
            masks.append(dm.demux_mask(ctx, group_bits[j], stores[j], level, ta[oo:oo + orows]))
            spans.append((j, oo, orows, po, prows))
            oo, po = oo + orows, po + prows
        masked = masks[0] if len(masks) == 1 else t.cat(masks)
        opened = (await _open_rows(co, masked)).view(oo, count, L)
        last = []
        for j, o, orows, q, prows in spans:
            if level == dm.demux_levels(widths[j]) - 1:
                _, wl, wh = dm.demux_plan(widths[j])[level].merges[0]
                last.append((wl, wh, o, q, table_off[j], j))
            else:
                dm.demux_finish(ctx, opened[o:o + orows], stores[j], level, ta[o:o + orows], tab[q:q + prows])
        if last:
            lookups(last, opened, ta, tab)
    if pending:                                                                 # every group has one bit: no level, no open
        lookups([], None, None, None)
    if not tree:
        return kept[0], kept[1]
    trip, carry = first, (kept[2 * G - 2:2 * G] if G & 1 else None)
    for i, products in enumerate(tree):
        mode, m = modes[i], shifts[i]
        opened = await _open_rows(co, masked0)
        masked, sv = cproducts_trunc(ctx, products, mode, opened, trip[0], trip[1], trip[2], rows.planes(products * mode_comps(mode) * nb), width, m, kappa)
        opened = await _open_rows(co, masked)
        if i == len(tree) - 1:
            _, res = tree_step(ctx, opened, sv, m, final=True)
            return (res[0], res[1]) if mode == MODE_BOTH else (res[0], None) if mode == MODE_COS else (None, res[0])
        trip = rows.take(tree[i + 1] * mode_triples(modes[i + 1]))
        masked0, carry = tree_step(ctx, opened, sv, m, mode=modes[i + 1], ta=trip[0], tb=trip[1], carry=carry)


async def _sincos(co, x, bits, triples, demux_triples, f, k, kappa, g, want, radians, split):
    ctx = co.ctx
    names, _ = _mode(want)
    lay = trig_layout(k, f, kappa, g, radians, want)
    _check_room(ctx.modulus, lay, k, f, kappa, radians)
    if split is not None and split not in SPLITS:
        raise ValueError(f"split: expected one of {SPLITS}, got {split!r}")
    x = ctx.elems(x, what="x")
    count = x.numel() // ctx.n_limbs
    x = x.view(count, ctx.n_limbs)
    bits, _ = _planes(ctx, bits, lay["n_planes"], count, "bits")
    triples = _triples(ctx, triples, lay["n_triples"], count)
    prep = _demux_prep(ctx, demux_triples, lay, count)
    rows = _Rows(bits, triples)
    if radians:
        L, _, m = turn_factor(k)
        prod = _ew_mul(ctx, x, L % ctx.modulus)
        masked, r1 = trunc_mask(ctx, prod, rows.planes(lay["turn_width"] + kappa), lay["turn_width"], m, kappa)
        x = trunc_pr_finish(ctx, prod, await co.open_share_array(masked), r1, m, out=r1)
    return _named(names, await _core(co, x, rows, prep, lay, f, kappa, split))


async def sincos_turns(co, x, bits, triples, demux_triples, f=F, k=K, kappa=KAPPA, g=None, want=("sin", "cos"), split=None):
    """Shares of sin(2 pi X) 2^f and cos(2 pi X) 2^f, a tuple in the order of `want`, up to trig_error_bound(k, f, g) ulps for shares of ANY
    signed k-bit x, X = x / 2^f turns.  trig_opens opens for any count; trig_planes bit planes and trig_triples triples an element in the
    order of trig_layout, and demux_triples as trig_demux_rows lists them.  `want` of one component drops the other's last truncation and,
    for the cosine, one of the last level's three triples.  x and the preprocessing are left untouched.  ValueError before anything is opened."""
    return await _sincos(co, x, bits, triples, demux_triples, f, k, kappa, g, want, False, split)


async def sincos(co, x, bits, triples, demux_triples, f=F, k=K, kappa=KAPPA, g=None, want=("sin", "cos"), split=None):
    """Shares of sin(X) 2^f and cos(X) 2^f for X = x / 2^f radians, up to trig_error_bound(k, f, g, radians=True) ulps: sincos_turns' core on
    trunc_pr(x L, m), one more open and no triple; every count and layout function takes radians=True.  Everything else as sincos_turns."""
    return await _sincos(co, x, bits, triples, demux_triples, f, k, kappa, g, want, True, split)


async def sin(co, x, bits, triples, demux_triples, f=F, k=K, kappa=KAPPA, g=None, split=None):
    """sincos with want = ("sin",): -> the one share array"""
    return (await _sincos(co, x, bits, triples, demux_triples, f, k, kappa, g, ("sin",), True, split))[0]


async def cos(co, x, bits, triples, demux_triples, f=F, k=K, kappa=KAPPA, g=None, split=None):
    """sincos with want = ("cos",): -> the one share array"""
    return (await _sincos(co, x, bits, triples, demux_triples, f, k, kappa, g, ("cos",), True, split))[0]


async def generate_trig_demux_triples(co, count, k=K, f=F, g=None, radians=False, tag="trig_demux_triples", generator=None):
    """What sincos_turns and sincos take as demux_triples for `count` values, made among the parties with no dealer:
    demux.generate_demux_triples for every group of two bits or more, concatenated level by level in group order (trig_demux_rows)."""
    _check_kf(k, f)
    ctx = co.ctx
    widths = [w for _, w in _fraction_groups(_ft(f, radians), _g(k, f, g, radians))]
    made = {j: await dm.generate_demux_triples(co, count, w, tag=(tag, j), generator=generator) for j, w in enumerate(widths) if w >= 2}
    out = []
    for l in range(max(dm.demux_levels(w) for w in widths)):
        have = [made[j][l] for j, w in enumerate(widths) if l < dm.demux_levels(w)]
        out.append((ctx.torch.cat([ta for ta, _ in have]).contiguous(), ctx.torch.cat([tab for _, tab in have]).contiguous()))
    return out

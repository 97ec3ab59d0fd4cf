"""
Base-2 and natural exponential of shared fixed-point numbers on the device (csrc/hb_fxexp.hip, the demultiplexer of csrc/hb_demux.hip
and the last truncation of csrc/hb_div.hip): 2^x is multiplicative over the bits of x, so it is a product of a few PUBLIC table reads
at one-hot vectors of groups of those bits, on the (count, limbs) share arrays of progs/fixedpoint.py.  The reference has no
exponential; the pin here is the mathematics: exp2_model on Python ints, and the same steps composed from bit_decompose, demux,
demux.lookup, share_arithmetic and fixedpoint.trunc_mask / trunc_pr_finish.

Inputs are shares of a signed k-bit x with f fractional bits, value X = x / 2^f.  exp2 gives shares of 2^X 2^f, exp of e^X 2^f.  The
contract is a result below 2^(k-2); every negative input down to -2^(k-1) is inside it, and anything below -f gives exactly 0 and raises
nothing (the operand is secret).  Overflow is outside the contract: the model says what comes out (0: the integer table is 0 there).
With s = k + GUARD_BITS the scale of the mantissa factors, mi = bit_length(k - 3), g the largest width of a fractional group, n the
number of bits decomposed (k for exp2, k + 1 for exp):

    1 offset    x' = x + f 2^f, local.  The result is 2^(x' / 2^f) as an integer: 2^u M with u = floor(x' / 2^f) in [0, k - 2) and M =
                2^frac in [1, 2); a negative x' is a result below one ulp.
    2 bits      bit_decompose(x', n + 1, n): declared one bit wider than it is, plane n - 1 of the two's complement is the sign of
                every in-contract x'; planes 0 .. f - 1 are the fraction, planes f .. f + mi - 1 are u            bit_opens(n) opens
    3 groups    the f fraction planes in G = ceil(f / g) groups of widths as equal as possible, the wider ones first, least
                significant first; the integer group is the mi planes of u with the sign plane as its top index bit.  All G + 1
                groups are demultiplexed together, a level of all of them ONE open                  max demux_levels(w) opens
    4 tables    PUBLIC, from Python ints.  A fractional group at bit offset o: T[j] = round(2^(j 2^(o-f)) 2^s); the integer group:
                U[j] = 2^j for j < k - 2, 0 above and in the whole sign half -- underflow becomes 0 with no product and no open.  A
                group's factor F = sum_j T[j] e_j is formed by finish_lookup_mask, the launch that finishes the group's LAST level
                (its 2^w one-hot rows are never stored), with the factor's row of the first product's masked pair.
    5 tree      over the G fractional factors: neighbours are paired, an odd last one is carried.  A level is one open of the masked
                pairs, ONE launch products_trunc, one open of the masked truncations, ONE launch tree_step that finishes the
                truncations by s, pairs the results (with the carried factor) and masks the next level    2 ceil(log2 G) opens
    6 result    one more level [M U], truncated by s, ends in fixedpoint_division.trunc_step(T_RESULT); U joins last so that no
                truncation sees a value below scale s                                               2 opens

exp2_opens = bit_opens(k) + max_w demux_levels(w) + 2 (ceil(log2 G) + 1): 17 at (64, 32) with g = 8, for any count.  g trades rounds
against preprocessing; the default is the smallest g among those with the fewest opens (default_group_width).

exp: y = trunc_pr(x L, fl) with the public L = round(log2(e) 2^fl), fl = k -- one more open, no triple -- then exp2 of y with n = k + 1
bits decomposed, because y reaches 1.45 times as far down as x.  Rounding the exponent to f bits costs a RELATIVE error of about
ln 2 2^-f on the result: exp_error_bound is a function of the input, not one number.

Where this leaves the issue's schedule: groups of different widths go through the demultiplexer's own kernels group by group (a mask
and a finish a group a level) and their masked arrays are concatenated for the level's ONE open; the fused last level takes up to 8
groups of any widths a launch, so at (64, 32, g = 8) the last level of all five groups is one launch.  Equal-width groups are not
stacked along count: that would copy the bit planes and the triples once more than the concatenation of the masked rows does.

Error (DESIGN.md section 3ac has the derivation).  A table entry is off by at most 1/2 at scale s, a relative 2^-(s+1); a tree
truncation adds an absolute error below 1 to a value of at least 2^s, a relative 2^-s, and the relative errors of the two factors
compound; the last truncation adds 1 ulp.  exp2_error_bound = 2^(k-2) eps_M + 1 against the exact real 2^X 2^f (not its floor).

Preprocessing is handed in as tensors, consumed in step order from row 0; exp2_layout / exp_layout name the row ranges.  `bits` is
(exp2_planes, count, limbs): [exp: W + kappa for the exponent's truncation,] n + 1 + kappa for the bit decomposition, then W + kappa
for every product of every tree level and the result (W = exp2_width(k)).  `triples = (p, q, pq)` is (exp2_triples, count, limbs)
each: bit_triples(n), then one a product.  `demux_triples` is a list with one (ta, tab) a demultiplexer level, each the concatenation,
in group order, of what demux.demux takes for that level of every group that has it (exp2_demux_rows; generate_exp2_demux_triples).

Host functions:

    exp2_groups(k, f, g) -> [(offset, width)] of the fraction groups; exp2_group_bits(k, f, n) -> the planes of the integer group
    default_group_width(k, f); exp2_tables(k, f, g) -> [[int]], the integer group's last
    exp2_width(k), exp2_shifts(k, f, g), exp2_layout / exp2_planes / exp2_triples / exp2_opens, exp2_demux_rows; exp_layout, ...
    exp2_error_bound(k, f, g), exp_error_bound(k, f, x, g)     exact Fractions, ulps of 2^-f
    exp2_model(x, p, k, f, r1s, g), exp_model(...) -> what the result opens to for the dealt r1 of every truncation in step order

Tensor level, one launch each on torch's current stream, nothing synchronises:

    table_rows(ctx, tables)                                      the public tables on the device, entry after entry
    finish_lookup_mask(ctx, groups, tables, pairs, kept_rows, ...)  -> (masked, kept)
    products_trunc(ctx, opened, ta, tb, tab, bits, width, m, kappa) -> (masked, s)
    tree_step(ctx, opened, s, m, ta, tb, carry)                  -> (masked, kept)

Protocol level, coroutines over an OpenCoalescer: exp2, exp, generate_exp2_demux_triples.  Inputs and preprocessing are left
untouched; ValueError before anything is opened.
"""
from fractions import Fraction
from functools import lru_cache
from math import isqrt

import numpy as np

from ..share_arithmetic import add
from ..share_arithmetic import mul as _ew_mul
from . import demux as dm
from .bit_decomposition import MAX_PLANES, bit_decompose, bit_opens, bit_triples
from .fixedpoint import F, K, KAPPA, _elems_out, _int, _inv2m, _planes, _planes_out, _triples, check_params, trunc_mask, trunc_pr_finish
from .fixedpoint_division import T_RESULT, _open_rows, _ranges, _Rows, trunc_step

GUARD_BITS = 2                                                   # s = k + GUARD_BITS
MAX_GROUP_WIDTH = dm.MAX_BITS
MAX_GROUPS_A_LAUNCH, MAX_ROWS = 8, 128                           # hb_fxexp.hip's FXEXP_MAX_GROUPS, FXEXP_MAX_ROWS
_PREC = 320                                                      # bits of the enclosures the tables are rounded from


# ---- host functions: exact constants -------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _root(i, prec):
    """-> (lo, hi) ints with lo <= 2^(2^-i) 2^prec <= hi, by repeated isqrt"""
    if i == 0:
        return 2 << prec, 2 << prec
    lo, hi = _root(i - 1, prec)
    return isqrt(lo << prec), isqrt(hi << prec) + 1


def _pow2_frac(num, bits, prec):
    """-> (lo, hi) enclosing 2^(num / 2^bits) 2^prec for 0 <= num < 2^bits: the product of the roots at the set bits of num"""
    lo = hi = 1 << prec
    for b in range(bits):
        if (num >> (bits - 1 - b)) & 1:
            rl, rh = _root(b + 1, prec)
            lo, hi = (lo * rl) >> prec, -((-hi * rh) >> prec)
    return lo, hi


def _round_pow2(num, bits, s):
    """round(2^(num / 2^bits) 2^s), exactly: the enclosure is widened until both ends round alike"""
    prec = max(_PREC, s + 64)
    while True:
        lo, hi = _pow2_frac(num, bits, prec)
        a, b = ((lo >> (prec - s - 1)) + 1) >> 1, ((hi >> (prec - s - 1)) + 1) >> 1
        if a == b:
            return a
        prec *= 2


@lru_cache(maxsize=None)
def _log2e(prec):
    """-> (lo, hi) ints enclosing log2(e) 2^prec, from ln 2 = sum_{n >= 1} 1 / (n 2^n) with its remainder below the last term"""
    work = prec + 64
    total = sum((1 << work) // (n << n) for n in range(1, work))
    ln_lo, ln_hi = total, total + work + 1                      # every term floored: below 1 short each; the terms from `work` on sum below 1
    return (1 << (work + prec)) // ln_hi, (1 << (work + prec)) // ln_lo + 1


def exponent_factor(k):
    """(L, fl): the public L = round(log2(e) 2^fl) of exp, fl = k"""
    fl = _int(k, "k")
    lo, hi = _log2e(fl + 64)
    a, b = ((lo >> 63) + 1) >> 1, ((hi >> 63) + 1) >> 1
    if a != b:
        raise ArithmeticError("log2(e) 2^fl lies on a rounding boundary")
    return a, fl


# ---- host functions: groups and tables --------------------------------------------------------------------------------------
def _mi(k):
    return (k - 3).bit_length()


def _check_kf(k, f, n=None):
    k, f = _int(k, "k"), _int(f, "f")
    n = k if n is None else n
    if k < 4 or f < 1:
        raise ValueError(f"needs k >= 4 and f >= 1, got k = {k}, f = {f}")
    if f + _mi(k) > k - 1:
        raise ValueError(f"needs f + bit_length(k - 3) <= k - 1: the exponent's integer part must fit under the sign, got k = {k}, f = {f}")
    if n > MAX_PLANES + 1:
        raise ValueError(f"at most {MAX_PLANES + 1} bits are decomposed, got {n}")
    if _mi(k) + 1 > MAX_GROUP_WIDTH:
        raise ValueError(f"the integer group has {_mi(k) + 1} bits: at most {MAX_GROUP_WIDTH}")


def _g(k, f, g):
    if g is None:
        return default_group_width(k, f)
    if not 1 <= _int(g, "g") <= MAX_GROUP_WIDTH:
        raise ValueError(f"needs 1 <= g <= {MAX_GROUP_WIDTH}, got {g}")
    return g


def _fraction_groups(f, g):
    n = -(-f // g)
    base, rem = divmod(f, n)
    out, off = [], 0
    for j in range(n):
        w = base + (1 if j < rem else 0)
        out.append((off, w))
        off += w
    return out


def exp2_groups(k, f, g=None):
    """-> [(bit offset, width)] of the G = ceil(f / g) fraction groups, least significant first, widths as equal as possible (the wider
    ones first).  The integer group, exp2_group_bits, follows them in every list that is in group order."""
    _check_kf(k, f)
    return _fraction_groups(f, _g(k, f, g))


def exp2_group_bits(k, f, n=None):
    """the planes of the integer group, least significant first: the mi planes of u and the sign plane n - 1 as the top index bit (n the
    number of bits decomposed: k for exp2, k + 1 for exp)"""
    _check_kf(k, f, n)
    n = k if n is None else n
    return list(range(f, f + _mi(k))) + [n - 1]


def _widths(k, f, g):
    return [w for _, w in _fraction_groups(f, g)] + [_mi(k) + 1]


def _tree(n_factors):
    """products of every level of the tree over n_factors factors: neighbours paired, an odd last one carried"""
    out, n = [], n_factors
    while n > 1:
        out.append(n // 2)
        n = n // 2 + (n & 1)
    return out


def _open_count(k, f, g, n):
    widths = _widths(k, f, g)
    return bit_opens(n) + max(dm.demux_levels(w) for w in widths) + 2 * (len(_tree(len(widths) - 1)) + 1)


@lru_cache(maxsize=None)
def default_group_width(k, f):
    """the smallest g among those with the fewest opens"""
    _check_kf(k, f)
    return min(range(1, min(f, MAX_GROUP_WIDTH) + 1), key=lambda g: (_open_count(k, f, g, k), g))


@lru_cache(maxsize=None)
def _tables(k, f, g):
    s, mi = k + GUARD_BITS, _mi(k)
    out = [[_round_pow2(j << o, f, s) for j in range(1 << w)] for o, w in _fraction_groups(f, g)]
    out.append([(1 << j) if j < k - 2 else 0 for j in range(1 << mi)] + [0] * (1 << mi))
    return out


def exp2_tables(k, f, g=None):
    """-> [[int]]: for every fraction group at bit offset o its table T[j] = round(2^(j 2^(o-f)) 2^s), j < 2^w, and last the integer
    group's U[j] = 2^j for j < k - 2, 0 for k - 2 <= j < 2^mi and 0 in the whole sign half, 2^(mi+1) entries"""
    _check_kf(k, f)
    return [list(t) for t in _tables(k, f, _g(k, f, g))]


# ---- host functions: counts ------------------------------------------------------------------------------------------------------
def exp2_width(k):
    """the signed width of every truncation: a product of two factors whose exponents sum below 1 is below 2^(2s+1), [M U] below
    2^(s+1+k-3), and the exponent's product x L of exp is below 2^(2k); 2 s + 2 with the sign"""
    return 2 * (_int(k, "k") + GUARD_BITS) + 2


def exp2_shifts(k, f, g=None):
    """m of every truncation in step order: the products of the tree level by level, then the result: all s"""
    _check_kf(k, f)
    return [k + GUARD_BITS] * len(_fraction_groups(f, _g(k, f, g)))


def exp2_demux_rows(k, f, g=None):
    """-> [[(group, opened rows, products)]] level by level: what the (ta, tab) of that level of demux_triples must hold, in this
    order -- for every group that has the level, in group order (the integer group last), demux_opened rows of ta and
    demux_products rows of tab"""
    _check_kf(k, f)
    widths = _widths(k, f, _g(k, f, g))
    return [[(j, dm.demux_opened(w, l), dm.demux_products(w, l)) for j, w in enumerate(widths) if l < dm.demux_levels(w)]
            for l in range(max(dm.demux_levels(w) for w in widths))]


def _layout(k, f, kappa, g, natural):
    n = k + 1 if natural else k
    _check_kf(k, f, n)
    _int(kappa, "kappa")
    g = _g(k, f, g)
    nb = exp2_width(k) + kappa
    tree = _tree(len(_fraction_groups(f, g)))
    planes = ([("exponent", nb)] if natural else []) + [("bit_decompose", n + 1 + kappa)]
    triples = [("bit_decompose", bit_triples(n))]
    for i, products in enumerate(tree):
        planes.append((f"tree{i}", products * nb))
        triples.append((f"tree{i}", products))
    planes.append(("result", nb))
    triples.append(("result", 1))
    p_ranges, n_planes = _ranges(planes)
    t_ranges, n_triples = _ranges(triples)
    rows = exp2_demux_rows(k, f, g)
    return {"g": g, "groups": _fraction_groups(f, g), "width": exp2_width(k), "bits": n, "tree": tree, "planes": p_ranges, "triples": t_ranges,
            "n_planes": n_planes, "n_triples": n_triples, "demux_rows": rows, "demux_opened": sum(o for lv in rows for _, o, _ in lv),
            "demux_products": sum(q for lv in rows for _, _, q in lv), "opens": (1 if natural else 0) + _open_count(k, f, g, n)}


def exp2_layout(k=K, f=F, kappa=KAPPA, g=None):
    """-> {"g", "groups", "width", "bits", "tree", "planes": {name: (start, stop)}, "triples": {name: (start, stop)}, "n_planes", "n_triples",
    "demux_rows", "demux_opened", "demux_products", "opens"}: the rows of `bits` and of the triple tensors each step consumes, in step order
    from row 0 (bit_decompose, tree<i>, result), the products of every tree level, and what the demultiplexer triples hold -- so the
    trade g makes between opens and preprocessing can be counted"""
    return _layout(k, f, kappa, g, False)


def exp_layout(k=K, f=F, kappa=KAPPA, g=None):
    """exp2_layout for exp: the exponent's truncation first, and k + 1 bits decomposed"""
    return _layout(k, f, kappa, g, True)


def exp2_planes(k=K, f=F, kappa=KAPPA, g=None):
    return exp2_layout(k, f, kappa, g)["n_planes"]


def exp2_triples(k=K, f=F, g=None):
    return exp2_layout(k, f, 0, g)["n_triples"]


def exp2_opens(k=K, f=F, g=None):
    return exp2_layout(k, f, 0, g)["opens"]


def exp_planes(k=K, f=F, kappa=KAPPA, g=None):
    return exp_layout(k, f, kappa, g)["n_planes"]


def exp_triples(k=K, f=F, g=None):
    return exp_layout(k, f, 0, g)["n_triples"]


def exp_opens(k=K, f=F, g=None):
    return exp_layout(k, f, 0, g)["opens"]


# ---- host functions: bounds ------------------------------------------------------------------------------------------------------
def _mantissa_error(k, f, g):
    """eps_M >= the relative error of M: 2^-(s+1) a table entry, (1 + a) (1 + b) - 1 + 2^-s a product of the tree"""
    s = k + GUARD_BITS
    eps = [Fraction(1, 1 << (s + 1))] * len(_fraction_groups(f, g))
    while len(eps) > 1:
        nxt = [(1 + eps[2 * q]) * (1 + eps[2 * q + 1]) - 1 + Fraction(1, 1 << s) for q in range(len(eps) // 2)]
        eps = nxt + ([eps[-1]] if len(eps) & 1 else [])
    return eps[0]


def exp2_error_bound(k=K, f=F, g=None):
    """|result - 2^X 2^f| in ulps of 2^-f against the exact real (not its floor), an exact Fraction, for every x whose result is below
    2^(k-2): 2^(k-2) eps_M + 1, the last truncation's unit (a result below one ulp comes out as 0 or as the truncation of it)"""
    _check_kf(k, f)
    return (1 << (k - 2)) * _mantissa_error(k, f, _g(k, f, g)) + 1


def _exp_upper(x, f):
    """>= e^(x / 2^f), a Fraction: 2^t <= 2^floor(t) (1 + t - floor(t)) for t = X log2(e) rounded up"""
    lo, hi = _log2e(256)
    t = Fraction(x * (hi if x >= 0 else lo), 1 << (256 + f))
    fl = t.numerator // t.denominator
    if fl < -1024:
        return Fraction(1, 1 << 1024)
    return (Fraction(2) ** fl) * (1 + t - fl)


def exp_error_bound(k=K, f=F, x=0, g=None):
    """|result - e^X 2^f| in ulps of 2^-f for the signed k-bit x whose result is below 2^(k-2), an exact Fraction.  The exponent y is
    off by at most d = 1 + |x| / 2^(k+1) ulps (the truncation and the rounding of L), a RELATIVE error 2^(d / 2^f) - 1 <= d / 2^f of the
    result E = e^X 2^f; exp2 adds eps_M relative to what it computes, and 1: with E' = max(an upper bound of E, 1),
    E' d / 2^f + E' (1 + d / 2^f) eps_M + 1"""
    _check_kf(k, f, k + 1)
    if not -(1 << (k - 1)) <= _int(x, "x") < 1 << (k - 1):
        raise ValueError(f"x is no signed {k}-bit value")
    d = (1 + Fraction(abs(x), 1 << (k + 1))) / (1 << f)
    e = max(_exp_upper(x, f) * (1 << f), Fraction(1))
    return e * d + e * (1 + d) * _mantissa_error(k, f, _g(k, f, g)) + 1


# ---- host functions: the models --------------------------------------------------------------------------------------------------
def _centered(x, p):
    x = int(x) % p
    return x - p if x > p // 2 else x


def _tr(v, r1, p, width, m):
    return (v - (v + (1 << (width - 1)) + r1) % p % (1 << m) + r1) * pow(2, -m, p) % p


def _exp2_residue(xp, p, k, f, r1s, g, n):
    """x' a signed int; its low n bits in two's complement are what the bit decomposition gives"""
    s, mi, width = k + GUARD_BITS, _mi(k), exp2_width(k)
    tables = _tables(k, f, g)
    v = xp % (1 << n)
    vals = [tables[j][(v >> o) & ((1 << w) - 1)] for j, (o, w) in enumerate(_fraction_groups(f, g))]
    u = tables[-1][((v >> f) & ((1 << mi) - 1)) | ((v >> (n - 1)) << mi)]
    r1s = iter(r1s)
    while len(vals) > 1:
        nxt = [_tr(vals[2 * q] * vals[2 * q + 1] % p, next(r1s), p, width, s) for q in range(len(vals) // 2)]
        vals = nxt + ([vals[-1]] if len(vals) & 1 else [])
    return _tr(vals[0] * u % p, next(r1s), p, width, s)


def _check_model(p, k, f, g, r1s, limits, n):
    _check_kf(k, f, n)
    g = _g(k, f, g)
    check_params(p, n + 1, n, 0, full=True)
    check_params(p, exp2_width(k), k + GUARD_BITS, 0)
    r1s = [_int(r, "r1") for r in r1s]
    limits = limits + exp2_shifts(k, f, g)
    if len(r1s) != len(limits) or any(not 0 <= r < 1 << m for r, m in zip(r1s, limits)):
        raise ValueError(f"r1s: expected {len(limits)} values below 2^m for m = {limits}")
    return g, r1s


def _signed(x, p, k):
    x = _centered(x, p)
    if not -(1 << (k - 1)) <= x < 1 << (k - 1):
        raise ValueError(f"x is no signed {k}-bit value")
    return x


def exp2_model(x, p, k=K, f=F, r1s=(), g=None):
    """What exp2's result opens to, a residue mod p: x a residue (or signed int) of a signed k-bit value; r1s the dealt r1 of every
    truncation in step order, below 2^s each (exp2_shifts).  Python ints only; r2 does not matter (no masked value wraps)."""
    g, r1s = _check_model(p, k, f, g, r1s, [], k)
    return _exp2_residue(_signed(x, p, k) + (f << f), p, k, f, r1s, g, k)


def exp_model(x, p, k=K, f=F, r1s=(), g=None):
    """What exp's result opens to: r1s[0] is the r1 of the exponent's truncation (below 2^k), then exp2's"""
    L, fl = exponent_factor(k)
    g, r1s = _check_model(p, k, f, g, r1s, [fl], k + 1)
    y = _centered(_tr(_signed(x, p, k) * L % p, r1s[0], p, exp2_width(k), fl), p)
    return _exp2_residue(y + (f << f), p, k, f, r1s[1:], g, k + 1)


# ---- tensor level ----------------------------------------------------------------------------------------------------------
def table_rows(ctx, tables):
    """the public tables on the device, entry after entry: -> ((entries, limbs) tensor, [first entry of every table])"""
    flat, offs = [], []
    for t in tables:
        offs.append(len(flat))
        flat += [int(v) % ctx.modulus for v in t]
    if not flat:
        raise ValueError("tables: expected at least one entry")
    return ctx.upload_ints(flat).view(len(flat), ctx.n_limbs), offs


def finish_lookup_mask(ctx, groups, tables, pairs, kept_rows, count, bits=None, opened=None, ta=None, tab=None, nxt=None, out=None, kept_out=None):
    """The last demultiplexer level of up to 8 groups, the read of their public tables and the mask of the first product, ONE launch.
    groups: [(wl, wh, open_off, prod_off, table_off, slot)] -- the last merge of the group joins a low factor of wl bits and a high
    one of wh bits; rows open_off .. of opened (the level's array, opened; flat is fine) and of ta hold its 2^wl + 2^wh rows in
    demux_mask's order, rows prod_off .. of tab its 2^(wl + wh) products, entries table_off .. of tables (table_rows) its table T;
    (1, 0, plane, 0, table_off, slot) is a group of ONE bit, plane its row of bits.  The group's factor F = sum_y T[y] e_y goes to row slot
    of kept (kept_rows, count, limbs) and, for slot < 2 pairs, F - (slot even ? nxt[0] : nxt[1])[slot / 2] to row slot of masked (2 pairs,
    count, limbs); nxt = (a, b), (pairs, count, limbs) each.  -> (masked, kept); rows that no group names are left as out / kept_out
    had them (uninitialised without)."""
    try:
        groups = [tuple(_int(v, "groups") for v in grp) for grp in groups]
        if any(len(grp) != 6 for grp in groups):
            raise TypeError
    except TypeError:
        raise ValueError("groups: expected a list of (wl, wh, open_off, prod_off, table_off, slot)") from None
    if not 1 <= len(groups) <= MAX_GROUPS_A_LAUNCH:
        raise ValueError(f"groups: 1 .. {MAX_GROUPS_A_LAUNCH} a launch, got {len(groups)}")
    if not 0 <= _int(pairs, "pairs") <= MAX_ROWS or not 1 <= _int(kept_rows, "kept_rows") <= 2 * MAX_ROWS + 1 or _int(count, "count") < 0:
        raise ValueError(f"needs 0 <= pairs <= {MAX_ROWS}, 1 <= kept_rows <= {2 * MAX_ROWS + 1} and count >= 0, got {pairs}, {kept_rows}, {count}")
    tables = ctx.elems(tables, what="tables")
    need = {"bits": 0, "open": 0, "prod": 0}
    slots = set()
    for wl, wh, oo, po, to, slot in groups:
        linear = (wl, wh) == (1, 0)
        if not linear and (wl < 1 or wh < 1 or wl + wh > MAX_GROUP_WIDTH):
            raise ValueError(f"groups: a merge needs 1 <= wl, wh and wl + wh <= {MAX_GROUP_WIDTH} (or (1, 0): one bit), got ({wl}, {wh})")
        if min(oo, po, to) < 0 or not 0 <= slot < kept_rows or slot in slots:
            raise ValueError(f"groups: offsets must not be negative and every group needs a slot of its own below {kept_rows}")
        slots.add(slot)
        if to + (1 << (wl + wh)) > tables.numel() // ctx.n_limbs:
            raise ValueError(f"tables: the group at entry {to} needs {1 << (wl + wh)} entries, the tensor holds {tables.numel() // ctx.n_limbs}")
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
        na, _ = _planes(ctx, a, pairs, count, "nxt a")
        nb, _ = _planes(ctx, b, pairs, count, "nxt b")
    o0 = _planes_out(ctx, out, 2 * pairs, count, "out") if masks or out is not None else None
    o1 = _planes_out(ctx, kept_out, kept_rows, count, "kept_out")
    desc = np.ascontiguousarray([v for grp in groups for v in grp], dtype=np.int32)
    P = lambda t: None if t is None else ctx.ptr(t)
    ctx.check(ctx.lib.hb_fxexp_finish_lookup_mask(ctx.h, P(bits_t), P(opened_t), P(ta_t), P(tab_t), P(tables), len(groups), desc.ctypes.data, P(na), P(nb), pairs,
                                                  P(o0), P(o1), kept_rows, count, ctx.stream()), "hb_fxexp_finish_lookup_mask")
    return (None if o0 is None else o0.view(2 * pairs, count, ctx.n_limbs)), o1.view(kept_rows, count, ctx.n_limbs)


def products_trunc(ctx, opened, ta, tb, tab, bits, width, m, kappa=KAPPA, out=None):
    """The products of a tree level to their truncation masks, ONE launch: opened (2 products, count, limbs) or flat, the masked pairs
    opened; ta, tb, tab (products, count, limbs), 1 <= products <= 128; bits (products (width + kappa), count, limbs).  -> (masked, s),
    (products, count, limbs) each: trunc_mask of every product, the array to open, and product + r1.  out: a pair."""
    ta = ctx.elems(ta, what="ta")
    if ta.dim() != 3 or not 1 <= ta.shape[0] <= MAX_ROWS:
        raise ValueError(f"ta: expected shape (1 <= products <= {MAX_ROWS}, count, {ctx.n_limbs}), got {tuple(ta.shape)}")
    products, count = ta.shape[0], ta.shape[1]
    tb, tab = (_planes(ctx, v, products, count, w, exact=True)[0] for v, w in ((tb, "tb"), (tab, "tab")))
    opened = ctx.elems(opened, 2 * products * count, what="opened")
    check_params(ctx.modulus, width, m, kappa)
    bits, _ = _planes(ctx, bits, products * (width + kappa), count, "bits")
    g0, g1 = (None, None) if out is None else out
    o0, o1 = _planes_out(ctx, g0, products, count, "out masked"), _planes_out(ctx, g1, products, count, "out s")
    P = ctx.ptr
    ctx.check(ctx.lib.hb_fxexp_products_trunc(ctx.h, products, P(opened), P(ta), P(tb), P(tab), P(bits), width, m, kappa, P(o0), P(o1), count, ctx.stream()),
              "hb_fxexp_products_trunc")
    return o0.view(products, count, ctx.n_limbs), o1.view(products, count, ctx.n_limbs)


def tree_step(ctx, opened, s, m, ta=None, tb=None, carry=None, out=None):
    """After the open of masked truncations, ONE launch: t_j = (s_j - (opened_j mod 2^m)) / 2^m for the rows of s (rows, count, limbs), 1 <=
    rows <= 128, and opened (flat is fine); the values are t_0 .. and, last, carry (count, limbs) if given.  Pair q of them is masked
    against ta[q], tb[q] ((values // 2, count, limbs) each): rows 2q, 2q + 1 of masked; an odd last value is kept.  -> (masked, kept),
    None where there is no pair or no odd value.  out: a pair."""
    if not 0 < _int(m, "m") <= ctx.modulus.bit_length() - 2:
        raise ValueError(f"needs 0 < m <= {ctx.modulus.bit_length() - 2}, got {m}")
    s = ctx.elems(s, what="s")
    if s.dim() != 3 or not 1 <= s.shape[0] <= MAX_ROWS:
        raise ValueError(f"s: expected shape (1 <= rows <= {MAX_ROWS}, count, {ctx.n_limbs}), got {tuple(s.shape)}")
    rows, count = s.shape[0], s.shape[1]
    opened = ctx.elems(opened, rows * count, what="opened")
    carry_t = None if carry is None else ctx.elems(carry, count, what="carry")
    values = rows + (carry is not None)
    pairs, odd = values // 2, values & 1
    ta_t = tb_t = None
    if pairs:
        ta_t, _ = _planes(ctx, ta, pairs, count, "ta", exact=True)
        tb_t, _ = _planes(ctx, tb, pairs, count, "tb", exact=True)
    g0, g1 = (None, None) if out is None else out
    o0 = _planes_out(ctx, g0, 2 * pairs, count, "out masked") if pairs else None
    o1 = _elems_out(ctx, g1, count, "out kept") if odd else None
    inv = _inv2m(ctx, m)
    P = lambda t: None if t is None else ctx.ptr(t)
    ctx.check(ctx.lib.hb_fxexp_tree_step(ctx.h, rows, P(opened), P(s), m, inv.ctypes.data, P(carry_t), P(ta_t), P(tb_t), P(o0), P(o1), count, ctx.stream()),
              "hb_fxexp_tree_step")
    return (None if o0 is None else o0.view(2 * pairs, count, ctx.n_limbs)), o1


# ---- protocols over an OpenCoalescer ---------------------------------------------------------------------------------------
def _check_protocol(ctx, lay, k, f, kappa, natural):
    n, width = lay["bits"], lay["width"]
    check_params(ctx.modulus, n + 1, n, kappa, full=True)
    check_params(ctx.modulus, width, k + GUARD_BITS, kappa)
    if natural:
        check_params(ctx.modulus, width, k, kappa)
    if width > 256:
        raise ValueError(f"the truncations need {width} bits: at most 256")
    if max(lay["tree"], default=0) > MAX_ROWS:
        raise ValueError(f"g = {lay['g']} makes {len(lay['groups'])} factors: at most {2 * MAX_ROWS + 1}")
    if (f << f) + (1 << (k - 1)) >= ctx.modulus:
        raise ValueError("the offset f 2^f does not fit below the modulus")


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


async def _exp2_core(co, xp, rows, prep, lay, k, f, kappa):
    """steps 2 to 6 on x' = x + f 2^f"""
    ctx, t = co.ctx, co.ctx.torch
    count, L = xp.shape[0], ctx.n_limbs
    n, width, s, g = lay["bits"], lay["width"], k + GUARD_BITS, lay["g"]
    nb = width + kappa
    fractions, mi = lay["groups"], _mi(k)
    G = len(fractions)
    widths = [w for _, w in fractions] + [mi + 1]
    planes = await bit_decompose(co, xp, rows.planes(n + 1 + kappa), rows.take(bit_triples(n)), n + 1, n, kappa)
    group_bits = [planes[o:o + w] for o, w in fractions]
    group_bits.append(planes[f:f + mi + 1] if f + mi == n - 1 else t.cat([planes[f:f + mi], planes[n - 1:n]]))
    tables, table_off = table_rows(ctx, _tables(k, f, g))
    # the first product's triple: level 0 of the tree, or [M U] itself where there is one fraction group
    tree = lay["tree"]
    first = rows.take(tree[0] if tree else 1)
    pairs0 = first[0].shape[0]
    masked0 = ctx.torch.empty((2 * pairs0, count, L), dtype=t.int64, device=ctx.tdev)
    kept = ctx.torch.empty((G + 1, count, L), dtype=t.int64, device=ctx.tdev)
    # the merged groups of the levels before the last: the last level's 2^w rows of a group are never written or read, so its array (the
    # shape demux_mask and demux_finish ask for) runs on into the next group's, and only the last one has that tail allocated
    used = [dm.demux_group_rows(w) - (1 << w) if w >= 2 else 0 for w in widths]
    pool = ctx.torch.empty((sum(used) + (1 << max(widths)), count, L), dtype=t.int64, device=ctx.tdev)
    stores = [pool[sum(used[:j]):sum(used[:j]) + dm.demux_group_rows(w)] if w >= 2 else None for j, w in enumerate(widths)]
    pending = [(1, 0, j, 0, table_off[j], j) for j, w in enumerate(widths) if w == 1]        # groups of one bit: formed by the first launch
    plane_of = {j: fractions[j][0] for j, w in enumerate(widths) if w == 1}

    def lookups(descs, opened, ta, tab):
        descs = pending + descs
        pending.clear()
        for at in range(0, len(descs), MAX_GROUPS_A_LAUNCH):
            chunk = [(wl, wh, plane_of[j] if (wl, wh) == (1, 0) else oo, po, to, j) for wl, wh, oo, po, to, j in descs[at:at + MAX_GROUPS_A_LAUNCH]]
            finish_lookup_mask(ctx, chunk, tables, pairs0, G + 1, count, bits=planes, opened=opened, ta=ta, tab=tab, nxt=(first[0], first[1]), out=masked0, kept_out=kept)

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
    # the tree over the fraction factors, then [M U]
    trip, values = first, G
    carry = kept[G - 1] if G > 1 and G & 1 else None
    for i, products in enumerate(tree):
        opened = await _open_rows(co, masked0)
        masked, sv = products_trunc(ctx, opened, trip[0], trip[1], trip[2], rows.planes(products * nb), width, s, kappa)
        opened = await _open_rows(co, masked)
        values = products + (carry is not None)
        last_level = i == len(tree) - 1
        trip = rows.take(1 if last_level else tree[i + 1])
        masked0, odd = tree_step(ctx, opened, sv, s, trip[0], trip[1], carry=kept[G] if last_level else carry)
        carry = None if last_level else odd
    opened = await _open_rows(co, masked0)
    masked, sv = products_trunc(ctx, opened, trip[0], trip[1], trip[2], rows.planes(nb), width, s, kappa)
    opened = await _open_rows(co, masked)
    return trunc_step(ctx, T_RESULT, opened, sv, s)


async def _exp(co, x, bits, triples, demux_triples, f, k, kappa, g, natural):
    ctx = co.ctx
    lay = _layout(k, f, kappa, g, natural)
    _check_protocol(ctx, lay, k, f, kappa, natural)
    x = ctx.elems(x, what="x")
    count = x.numel() // ctx.n_limbs
    x = x.view(count, ctx.n_limbs)
    bits, _ = _planes(ctx, bits, lay["n_planes"], count, "bits")
    triples = _triples(ctx, triples, lay["n_triples"], count)
    prep = _demux_prep(ctx, demux_triples, lay, count)
    rows = _Rows(bits, triples)
    if natural:
        L, fl = exponent_factor(k)
        prod = _ew_mul(ctx, x, L % ctx.modulus)
        masked, r1 = trunc_mask(ctx, prod, rows.planes(lay["width"] + kappa), lay["width"], fl, kappa)
        x = trunc_pr_finish(ctx, prod, await co.open_share_array(masked), r1, fl, out=r1)
    return await _exp2_core(co, add(ctx, x, (f << f) % ctx.modulus), rows, prep, lay, k, f, kappa)


async def exp2(co, x, bits, triples, demux_triples, f=F, k=K, kappa=KAPPA, g=None):
    """Shares of 2^X 2^f up to exp2_error_bound(k, f, g) ulps for shares of a signed k-bit x whose result is below 2^(k-2); below -f the
    result is exactly 0.  exp2_opens opens for any count; exp2_planes bit planes and exp2_triples triples an element in the order of
    exp2_layout, and demux_triples as exp2_demux_rows lists them.  x and the preprocessing are left untouched.  ValueError before
    anything is opened."""
    return await _exp(co, x, bits, triples, demux_triples, f, k, kappa, g, False)


async def exp(co, x, bits, triples, demux_triples, f=F, k=K, kappa=KAPPA, g=None):
    """Shares of e^X 2^f up to exp_error_bound(k, f, x, g) ulps: exp2 of trunc_pr(x L, k), one more open.  The contract is e^X 2^f (1 +
    2^(1-f)) < 2^(k-2): the rounding of the exponent may not carry the result past the integer table's end.  exp_opens, exp_planes,
    exp_triples, exp_layout; demux_triples as for exp2.  Everything else as exp2."""
    return await _exp(co, x, bits, triples, demux_triples, f, k, kappa, g, True)


async def generate_exp2_demux_triples(co, count, k=K, f=F, g=None, tag="exp2_demux_triples", generator=None):
    """What exp2 and exp take as demux_triples for `count` values, made among the parties with no dealer: demux.generate_demux_triples
    for every group of two bits or more, one after another, concatenated level by level in group order (exp2_demux_rows)."""
    _check_kf(k, f)
    ctx = co.ctx
    widths = _widths(k, f, _g(k, f, g))
    made = {j: await dm.generate_demux_triples(co, count, w, tag=(tag, j), generator=generator) for j, w in enumerate(widths) if w >= 2}
    out = []
    for l in range(max(dm.demux_levels(w) for w in widths)):
        have = [made[j][l] for j, w in enumerate(widths) if l < dm.demux_levels(w)]
        out.append((ctx.torch.cat([ta for ta, _ in have]).contiguous(), ctx.torch.cat([tab for _, tab in have]).contiguous()))
    return out

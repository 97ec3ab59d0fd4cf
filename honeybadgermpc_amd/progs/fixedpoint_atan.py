"""
Arctangent and atan2 of shared fixed-point numbers on the device (csrc/hb_fxatan.hip, the comparison of csrc/hb_fxp.hip, the division of
csrc/hb_div.hip and the products-to-masks step of csrc/hb_fxexp.hip): the octant from three sign bits, the quotient of the smaller
magnitude by the larger, and its arctangent on [0, 1] as a truncated Chebyshev series -- an ODD polynomial, evaluated from the odd powers
of a shared value alone -- for signed k-bit values with f fractional bits, on the (count, limbs) share arrays of progs/fixedpoint.py.
The reference has no arctangent; the pin here is the mathematics: atan2_model on Python ints, and the same steps composed from
share_arithmetic and fixedpoint.trunc_mask / trunc_pr_finish.

Inputs are shares of signed k-bit y and x with |x|, |y| < 2^(k-1); k / 2 <= f <= k - 3: the quotient can be exactly 1 and div asks for
|a 2^f / b| < 2^(k-2).  (f = k - 2 is not allowed: the quotient 2^f = 2^(k-2) is the very value div's contract excludes, and div_width's
bound on [a w] has no bit to spare for it.)  The result is shares of atan2(Y, X) 2^f in (-pi, pi], or with turns=True of atan2(Y, X) /
(2 pi) 2^f in (-1/2, 1/2], the unit of fixedpoint_trig.sincos_turns.  A sign bit s stands for sigma = 1 - 2 s.  With N = k - 1, beta =
2^N, g = f + GUARD_BITS, d = atan_degree(k, f, turns), J = (d - 1) / 2 and W = atan_width(k, f, turns) the width of the ladder's
truncations:

    1 signs     (sx, sy) = ltz of (x, y) as ONE array of 2 count values                             1 + carry_levels(N) opens
    2 abs       sign_mask, then abs_step: |x| = x - 2 [sx x], |y| = y - 2 [sy y], G = [sigma_y sx]; the same launch forms w = |x| - |y| and
                the mask of its comparison (trunc_mask at (k, N))                                   1 open, 3 products
    3 swap      c = [w < 0] = [|x| < |y|]: ltl_leaves, the carry tree and div2m_finish(NEG_TRUNC) of fixedpoint.py, as ltz runs them
                                                                                                    1 + carry_levels(N) opens
    4 select    select_mask, then select: [c w], e1 = [sigma_c sigma_x]; num = |y| + [c w] = min, den = |x| - [c w] = max
                                                                                                    1 open, 2 products
    5 quotient  q = div(num, den, signed=False), fixedpoint_division's coroutine, unchanged: q in [0, 2^f + delta], delta =
                quotient_error_bound(k, f): div_error_bound's recurrences at |Q| <= 1              div_opens(k, f, None, False) opens
    6 ladder    atan_first: t = 2^(N-f) q at scale beta; the masked pairs of u = [t t] and of E = [sigma_y e1] in ONE open.  Level 0 forms
                u; level l = 1 .. levels = bit_length(J) forms t^(2j+1) = [t^(2j+1-2^l) u^(2^(l-1))], 2^(l-1) <= j < min(2^l, J + 1), and,
                while a later level needs it, u^(2^l) = [u^(2^(l-1))]^2; every product goes through fixedpoint_exp.products_trunc by N
                (one open of the masked pairs, one of the masked truncations) and ONE launch atan_level finishes a level and masks the
                next                                                                                2 (levels + 1) opens
    7 polynomial atan_poly_mask: L = sum_j A_j t^(2j+1) with the PUBLIC integers A_j = round(a_j 2^g) (atan_coefficients): no product;
                masked for a truncation by m = N + GUARD_BITS                                       1 open
    8 assemble  atan_assemble: a = trunc_pr(L, m); E by the Beaver combine of the pair step 6 opened; the masked pair of [E a]; C = Pi G +
                H h with h = sigma_y sigma_x c = (sigma_y - 2 G - E) / 2.  atan_finish: C + [E a]; E = +-1, so no truncation follows
                                                                                                    1 open, 1 product

atan2_opens = 2 (1 + carry_levels(N)) + 2 + div_opens(unsigned) + 2 (levels + 1) + 1 + 1.  atan2(Y, X) = pi G + (pi / 2) h + E atan(min / max):
G = sigma_y sx says "beyond the y axis", h "past the diagonal", E the direction the octant's angle runs in.  Pi = round(pi 2^f) and H =
round(pi 2^(f-1)) are rounded each on its own (turns: 2^(f-1) and 2^(f-2), exact).  sigma_y - 2 G - E is twice a bit, so the FIELD's inverse
of 2 halves it exactly: C = (Pi - H) G + (H / 2 mod p) (sigma_y - E), two public constants and no product.  (0, 0) gives den = 0, div gives
0 for a zero divisor, every power and L are 0, G = c = 0: the result is 0, as math.atan2; y = 0, x < 0 has sy = 0, G = 1: +Pi.  Nothing raises
on secret values.  No masked value wraps.

The series (DESIGN.md section 3af has the derivation).  atan T = 2 sum_{n >= 0} (-1)^n r^(2n+1) T_{2n+1}(T) / (2n + 1) with r = sqrt 2 - 1 and
T_n the Chebyshev polynomials: |T_n| <= 1 on [-1, 1], so the series cut at degree d is off by at most 2 r^(d+2) / ((d + 2) (1 - r^2))
(series_tail).  atan_degree is the smallest odd d whose tail is at most 1/4 ulp of the result (turns: the tail over 2 pi).  r and pi are
enclosed by rationals from integer arithmetic, the series is converted to monomials over Fractions and every coefficient is rounded once
to 2^-g.  The monomial coefficients stay below 1 in magnitude: there is no cancellation to fear.

Error, in ulps of 2^-f of the result (atan_error_bound, exact Fractions), S = 1 or 1 / (2 pi): the quotient's delta times S max(1, |P'|) --
atan's slope is at most 1, and where T = q / 2^f exceeds 1, by at most eps = delta / 2^f, the polynomial's slope on [1, 1 + eps] takes its
place --; the tail; the coefficient roundings; the power truncations, 2^(f-N) sum_j |A_j| 2^-g E_j; the last trunc_pr, 1; the roundings
of Pi and H, 1/2 each (turns: none); 2^-64 for the enclosures.

Preprocessing is handed in as tensors, consumed in step order from row 0; atan_layout names the row ranges.  `bits` is (atan_planes,
count, limbs): 2 (k + kappa) for the signs, planes 2 i and 2 i + 1 being bit i of x's and of y's mask (viewed as k + kappa planes of 2 count
elements: no copy); k + kappa for the swap; div_planes(unsigned); then W + kappa a truncation in step order: u, then level by level the
odd powers and the square, then L.  `triples = (p, q, pq)` is (atan_triples, count, limbs) each: 2 carry_triples(N) for the signs,
interleaved likewise; 3 (abs); carry_triples(N) (swap); 2 (select); div_triples(unsigned); 2 (u, E); one a product of every level; 1
(assemble).

Host functions:

    atan_degree(k, f, turns), series_tail(d), atan_coefficients(k, f, turns, d), atan_constants(f, turns) -> (Pi, H)
    quotient_error_bound(k, f), atan_error_bound(k, f, turns, d), atan_width(k, f, turns, d)     exact; ulps of 2^-f
    atan_shifts, atan_layout, atan_planes, atan_triples, atan_opens
    atan2_model(y, x, p, k, f, r1s, turns) -> what the protocol opens to for the dealt r1 of every truncation in step order

Tensor level, one launch each on torch's current stream, nothing synchronises: sign_mask, abs_step, select_mask, select, atan_first,
atan_level, atan_poly_mask, atan_assemble, atan_finish.  Protocol level, coroutines over an OpenCoalescer: atan2, atan.  Inputs and
preprocessing are left untouched; ValueError before anything is opened.
"""
from fractions import Fraction
from functools import lru_cache
from math import isqrt

from .bit_decomposition import MAX_PLANES
from .fixedpoint import (F, K, KAPPA, NEG_TRUNC, _carry_tree, _elems_out, _int, _inv2m, _pair, _planes, _planes_out, _triples, carry_levels, carry_triples, check_params,
                         div2m_finish, ltl_leaves, ltz)
from .fixedpoint_division import _ceil, _div_residues, _open_rows, _ranges, _Rows, div, div_layout, div_width, goldschmidt_iterations, initial_residual_bound
from .fixedpoint_exp import _centered, _signed, _tr, products_trunc
from .fixedpoint_log import _chebyshev, _round
from .fixedpoint_trig import _pi

GUARD_BITS = 3                                                   # the coefficients carry the result's bits and these
MAX_DEGREE = 63                                                  # hb_fxatan.hip's
_PREC = 448                                                      # bits of the enclosures the constants are rounded from
_SLACK = Fraction(1, 1 << 64)                                    # ulps: what the enclosures can add, f <= 255, with room to spare

_R_LO = Fraction(isqrt(2 << (2 * _PREC)), 1 << _PREC) - 1          # r = sqrt 2 - 1 from below and from above, 2^-_PREC apart
_R_HI = Fraction(isqrt(2 << (2 * _PREC)) + 1, 1 << _PREC) - 1
_R = (_R_LO + _R_HI) / 2
_PI_LO, _PI_HI = (Fraction(v, 1 << _PREC) for v in _pi(_PREC))
_PI = (_PI_LO + _PI_HI) / 2


# ---- host functions: exact constants -------------------------------------------------------------------------------------------
def _check_kf(k, f):
    k, f = _int(k, "k"), _int(f, "f")
    if not (k <= 2 * f and f <= k - 3):
        raise ValueError(f"needs k / 2 <= f <= k - 3, got k = {k}, f = {f}")
    if k - 1 > MAX_PLANES:
        raise ValueError(f"at most {MAX_PLANES} planes, got k - 1 = {k - 1}")


def series_tail(d):
    """>= |atan T - the series cut at degree d| on [-1, 1] for odd d: 2 r^(d+2) / ((d + 2) (1 - r^2)), with r from above; a Fraction"""
    if _int(d, "d") < 1 or not d & 1:
        raise ValueError(f"the degree must be odd and positive, got {d}")
    return 2 * _R_HI ** (d + 2) / ((d + 2) * (1 - _R_HI ** 2))


def _unit(turns):
    """what a radian is in the result's unit, from above: 1, or 1 / (2 pi)"""
    return 1 / (2 * _PI_LO) if turns else Fraction(1)


def _tail_ulps(d, f, turns):
    return series_tail(d) * (1 << f) * _unit(turns)


@lru_cache(maxsize=None)
def atan_degree(k=K, f=F, turns=False):
    """the smallest odd d >= 3 whose series tail is at most 1/4 ulp of 2^-f of the result"""
    _check_kf(k, f)
    d = 3
    while _tail_ulps(d, f, bool(turns)) > Fraction(1, 4):
        d += 2
    return d


def _degree(k, f, turns, d):
    if d is None:
        return atan_degree(k, f, turns)
    if _int(d, "d") < 3 or not d & 1:
        raise ValueError(f"the degree must be odd and at least 3, got {d}")
    return d


@lru_cache(maxsize=None)
def _monomials(d, turns):
    """the series cut at the odd degree d as monomials: [a_0 .. a_J], a_j the coefficient of T^(2j+1), Fractions (from the constants'
    midpoints); turns: over 2 pi"""
    polys = _chebyshev(d)
    a = [Fraction(0)] * (d + 1)
    for n in range(1, d + 1, 2):
        cn = 2 * (-1) ** (n // 2) * _R ** n / n
        for j, c in enumerate(polys[n]):
            a[j] += cn * c
    if any(a[j] for j in range(0, d + 1, 2)):
        raise ArithmeticError("an odd series has an even term")
    return [c / (2 * _PI) if turns else c for c in a[1::2]]


@lru_cache(maxsize=None)
def atan_coefficients(k=K, f=F, turns=False, d=None):
    """the PUBLIC integers A_0 .. A_J at scale 2^g, g = f + GUARD_BITS: sum_j A_j T^(2j+1) is atan(T) 2^g (turns: over 2 pi) cut at degree d =
    2 J + 1, every coefficient rounded once"""
    _check_kf(k, f)
    d = _degree(k, f, turns, d)
    return [_round(c * (1 << (f + GUARD_BITS))) for c in _monomials(d, bool(turns))]


@lru_cache(maxsize=None)
def atan_constants(f=F, turns=False):
    """(Pi, H): round(pi 2^f) and round(pi 2^(f-1)), each rounded on its own from the enclosure of pi; turns: 2^(f-1) and 2^(f-2), exact"""
    if _int(f, "f") < 2:
        raise ValueError(f"needs f >= 2, got {f}")
    if turns:
        return 1 << (f - 1), 1 << (f - 2)
    out = []
    for e in (f, f - 1):
        a, b = _round(_PI_LO * (1 << e)), _round(_PI_HI * (1 << e))
        if a != b:
            raise ArithmeticError("pi 2^f lies on a rounding boundary")
        out.append(a)
    return tuple(out)


# ---- host functions: bounds ------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def quotient_error_bound(k=K, f=F):
    """delta >= |q - Q 2^f| in ulps of 2^-f for q = div(num, den, signed=False) with 0 <= Q = num / den <= 1 and div's default theta:
    div_error_bound's recurrences (fixedpoint_division._schedule) with the quotient's bound 2^f in place of 2^(k-2) -- y_i = Q (1 - E_i) +
    eta_i, |eta_0| < 1, |eta_{i+1}| <= |eta_i| (1 + eps_i) + 1 + 2^f 2^-2f, eps_{i+1} = eps_i^2 + 2^-2f, and at the end 2^f eps^2 + eta (1 + eps)
    + 1.  eps_0 is every k-bit divisor's (initial_residual_bound).  An exact Fraction.  The recurrence is RESTATED here, not shared:
    fixedpoint_division stays untouched, so a change to _schedule or div_error_bound there must be made here too
    (tests/test_fixedpoint_atan_host.py holds delta against every quotient at (8, 4) and below div_error_bound at the other shapes)."""
    _check_kf(k, f)
    theta = goldschmidt_iterations(k, f)
    eps, eta = initial_residual_bound(k, f), Fraction(1)
    qx, ulp = Fraction(1 << f, 1 << (2 * f)), Fraction(1, 1 << (2 * f))
    for _ in range(theta - 1):
        eta = eta * (1 + eps) + 1 + qx
        eps = eps ** 2 + ulp
    return eta * (1 + eps) + 1 + (1 << f) * eps ** 2


def _level_count(d):
    return ((d - 1) // 2).bit_length()


def _level_odd(level, d):
    """the j of the odd powers t^(2j+1) level `level` >= 1 forms"""
    J = (d - 1) // 2
    return list(range(1 << (level - 1), min(1 << level, J + 1)))


def _level_square(level, d):
    """whether level `level` forms u^(2^level): only while a later level needs it"""
    return 1 <= level < _level_count(d)


def _level_products(level, d):
    return 1 if level == 0 else len(_level_odd(level, d)) + int(_level_square(level, d))


def _ladder(k, f, d):
    """-> (mag, err): for every value of the ladder, keyed ("t", j) for t^(2j+1) and ("u", l) for u^(2^l), mag >= beta |T|^n, its true size
    for |T| <= 1 + delta / 2^f, and err >= |the value as computed - beta T^n|: t is exact, and [a b] truncated adds less than 1 to (A + E_a)
    (B + E_b) / beta"""
    beta = 1 << (k - 1)
    top = 1 + quotient_error_bound(k, f) / (1 << f)
    mag, err = {("t", 0): beta * top}, {("t", 0): Fraction(0)}

    def product(key, a, b, n):
        mag[key] = beta * top ** n
        err[key] = 1 + (mag[a] * err[b] + mag[b] * err[a] + err[a] * err[b]) / beta

    product(("u", 0), ("t", 0), ("t", 0), 2)
    for level in range(1, _level_count(d) + 1):
        for j in _level_odd(level, d):
            product(("t", j), ("t", j - (1 << (level - 1))), ("u", level - 1), 2 * j + 1)
        if _level_square(level, d):
            product(("u", level), ("u", level - 1), ("u", level - 1), 2 << level)
    return mag, err


def atan_error_bound(k=K, f=F, turns=False, d=None):
    """|result - atan2(Y, X) 2^f| (turns: over 2 pi) in ulps of 2^-f for every signed k-bit pair, an exact Fraction: the module docstring
    lists the terms"""
    _check_kf(k, f)
    turns = bool(turns)
    d = _degree(k, f, turns, d)
    beta, g, J = 1 << (k - 1), f + GUARD_BITS, (d - 1) // 2
    delta = quotient_error_bound(k, f)
    eps = delta / (1 << f)
    a = _monomials(d, turns)
    # the polynomial's slope on [1, 1 + eps], against atan's (at most 1 radian a unit): P'(1) exactly, P'' term by term
    slope = abs(sum((2 * j + 1) * a[j] for j in range(J + 1))) + eps * sum((2 * j + 1) * (2 * j) * abs(a[j]) * (1 + eps) ** (2 * j) for j in range(1, J + 1))
    quotient = delta * max(_unit(turns), slope)
    mag, err = _ladder(k, f, d)
    coef = atan_coefficients(k, f, turns, d)
    rounding = sum(Fraction(1, 2) * (mag["t", j] + err["t", j]) / beta for j in range(J + 1)) / (1 << GUARD_BITS)
    powers = sum(abs(coef[j]) * err["t", j] for j in range(J + 1)) * Fraction(1 << f, beta << g)
    return quotient + _tail_ulps(d, f, turns) + rounding + powers + 1 + (0 if turns else 1) + _SLACK


@lru_cache(maxsize=None)
def atan_width(k=K, f=F, turns=False, d=None):
    """the signed width of the ladder's truncations: what holds every product, |a b| <= (A + E_a) (B + E_b), and L, |L| <= sum_j |A_j|
    (beta |T|^(2j+1) + E_j); at least 2 k"""
    _check_kf(k, f)
    d = _degree(k, f, turns, d)
    mag, err = _ladder(k, f, d)
    coef = atan_coefficients(k, f, turns, d)
    top = max(mag[key] + err[key] for key in mag)
    bounds = [_ceil(top ** 2), _ceil(sum(abs(c) * (mag["t", j] + err["t", j]) for j, c in enumerate(coef)))]
    return max(2 * k, max(bounds).bit_length() + 1)


# ---- host functions: counts ------------------------------------------------------------------------------------------------------
def _div_shifts(k, f):
    theta = goldschmidt_iterations(k, f)
    return [2 * (k - 1 - f), f] + [2 * f] * (2 * theta - 1)


def atan_shifts(k=K, f=F, turns=False, d=None):
    """m of every truncation in step order: the division's 2 theta + 1 (div_model's), the ladder's products by N, then L by N + GUARD_BITS"""
    _check_kf(k, f)
    d = _degree(k, f, turns, d)
    products = sum(_level_products(l, d) for l in range(_level_count(d) + 1))
    return _div_shifts(k, f) + [k - 1] * products + [k - 1 + GUARD_BITS]


def atan_layout(k=K, f=F, kappa=KAPPA, turns=False, d=None):
    """-> {"degree", "width", "levels", "products", "planes": {name: (start, stop)}, "triples": {name: (start, stop)}, "n_planes", "n_triples",
    "opens", "div"}: the rows of `bits` and of the triple tensors each step consumes, in step order from row 0.  Planes: signs, swap, div,
    level<l> (l = 0 .. levels: one truncation a product), poly.  Triples: signs, abs, swap, select, div, level<l> (level0: u, then E),
    assemble.  "div" is div_layout(k, f, kappa, None, False)."""
    _check_kf(k, f)
    _int(kappa, "kappa")
    d = _degree(k, f, turns, d)
    width, n, levels = atan_width(k, f, turns, d), k - 1, _level_count(d)
    nb = width + kappa
    dlay = div_layout(k, f, kappa, None, False)
    planes = [("signs", 2 * (k + kappa)), ("swap", k + kappa), ("div", dlay["n_planes"])]
    triples = [("signs", 2 * carry_triples(n)), ("abs", 3), ("swap", carry_triples(n)), ("select", 2), ("div", dlay["n_triples"])]
    products = [_level_products(l, d) for l in range(levels + 1)]
    for level, c in enumerate(products):
        planes.append((f"level{level}", c * nb))
        triples.append((f"level{level}", c + (1 if level == 0 else 0)))
    planes.append(("poly", nb))
    triples.append(("assemble", 1))
    p_ranges, n_planes = _ranges(planes)
    t_ranges, n_triples = _ranges(triples)
    return {"degree": d, "width": width, "levels": levels, "products": products, "planes": p_ranges, "triples": t_ranges, "n_planes": n_planes, "n_triples": n_triples,
            "opens": 2 * (1 + carry_levels(n)) + 2 + dlay["opens"] + 2 * (levels + 1) + 1 + 1, "div": dlay}


def atan_planes(k=K, f=F, kappa=KAPPA, turns=False, d=None):
    return atan_layout(k, f, kappa, turns, d)["n_planes"]


def atan_triples(k=K, f=F, turns=False, d=None):
    return atan_layout(k, f, 0, turns, d)["n_triples"]


def atan_opens(k=K, f=F, turns=False, d=None):
    return atan_layout(k, f, 0, turns, d)["opens"]


atan2_opens = atan_opens


# ---- host functions: the model ---------------------------------------------------------------------------------------------------
def assemble_constants(p, f=F, turns=False):
    """(A, B) mod p with C = A G + B (sigma_y - E): A = Pi - H, B = H / 2 in the field"""
    big, half = atan_constants(f, turns)
    return (big - half) % p, half * pow(2, -1, p) % p


@lru_cache(maxsize=64)
def _model_plan(p, k, f, turns, d):
    """the model's parameter checks and constants, once a shape"""
    _check_kf(k, f)
    d = _degree(k, f, turns, d)
    width, dwidth = atan_width(k, f, turns, d), div_width(k, f)
    check_params(p, k, k - 1, 0, full=True)
    limits = atan_shifts(k, f, turns, d)
    n_div = len(_div_shifts(k, f))
    for m in set(limits[:n_div]):
        check_params(p, dwidth, m, 0)
    for m in set(limits[n_div:]):
        check_params(p, width, m, 0)
    return d, width, dwidth, limits, n_div, atan_coefficients(k, f, turns, d), assemble_constants(p, f, turns)


def atan2_model(y, x, p, k=K, f=F, r1s=(), turns=False, d=None):
    """What the protocol's result opens to, a residue mod p: y, x residues (or signed ints) of signed k-bit values with |x|, |y| < 2^(k-1);
    r1s the dealt r1 of every truncation in step order, below 2^m for m of atan_shifts (the comparisons are exact and take none).
    Python ints only; r2 does not matter (no masked value wraps for operands in the documented range)."""
    turns = bool(turns)
    d, width, dwidth, limits, n_div, coef, (ca, cb) = _model_plan(p, k, f, turns, d)
    r1s = [_int(r, "r1") for r in r1s]
    if len(r1s) != len(limits) or any(not 0 <= r < 1 << m for r, m in zip(r1s, limits)):
        raise ValueError(f"r1s: expected {len(limits)} values below 2^m for m = {limits}")
    ys, xs = _signed(y, p, k), _signed(x, p, k)
    if min(xs, ys) == -(1 << (k - 1)):
        raise ValueError("|x| and |y| must be below 2^(k-1)")
    sx, sy, c = int(xs < 0), int(ys < 0), int(abs(xs) < abs(ys))
    num, den = min(abs(xs), abs(ys)), max(abs(xs), abs(ys))
    q = _div_residues(num, den, p, k, f, r1s[:n_div], goldschmidt_iterations(k, f), False, dwidth)
    n = k - 1
    rest = iter(r1s[n_div:])

    def tr(v, m=n):
        return _tr(v % p, next(rest), p, width, m)

    t = {0: (q << (n - f)) % p}
    u = tr(t[0] * t[0])
    for level in range(1, _level_count(d) + 1):
        for j in _level_odd(level, d):
            t[j] = tr(t[j - (1 << (level - 1))] * u)
        if _level_square(level, d):
            u = tr(u * u)
    a = tr(sum(coef[j] * t[j] for j in range(len(coef))), n + GUARD_BITS)
    sig_y = 1 - 2 * sy
    g, e = sig_y * sx, sig_y * (1 - 2 * sx) * (1 - 2 * c)
    return (ca * g + cb * (sig_y - e) + e * a) % p


# ---- tensor level ----------------------------------------------------------------------------------------------------------
def coefficient_rows(ctx, k, f, turns=False, d=None):
    """atan_coefficients mod p on the device, (J + 1, limbs)"""
    return ctx.to_device(ctx.host_elems([c % ctx.modulus for c in atan_coefficients(k, f, turns, d)]))


def _check_degree(d):
    if not 3 <= _int(d, "d") <= MAX_DEGREE or not d & 1:
        raise ValueError(f"needs an odd 3 <= d <= {MAX_DEGREE}, got {d}")
    return d


def _check_shift(ctx, m, what="m"):
    if not 0 < _int(m, what) <= ctx.modulus.bit_length() - 2:
        raise ValueError(f"needs 0 < {what} <= {ctx.modulus.bit_length() - 2}, got {m}")
    return m


def _rows3(ctx, v, rows, count, what):
    return _planes(ctx, v, rows, count, what, exact=True)[0]


def sign_mask(ctx, s, x, y, ta, tb, out=None):
    """The masked pairs of the abs step, ONE launch after the signs' comparison: s (2 count, limbs) = (sx, sy), the comparison's result on
    the array (x, y); ta, tb (3, count, limbs).  -> (6, count, limbs): sx - ta[0], x - tb[0], sy - ta[1], y - tb[1], sigma_y - ta[2], sx -
    tb[2], the array to open"""
    x = ctx.elems(x, what="x")
    count = x.numel() // ctx.n_limbs
    y, s = ctx.elems(y, count, what="y"), ctx.elems(s, 2 * count, what="s")
    ta, tb = _rows3(ctx, ta, 3, count, "ta"), _rows3(ctx, tb, 3, count, "tb")
    o = _planes_out(ctx, out, 6, count)
    P = ctx.ptr
    ctx.check(ctx.lib.hb_fxatan_sign_mask(ctx.h, P(s), P(x), P(y), P(ta), P(tb), P(o), count, ctx.stream()), "hb_fxatan_sign_mask")
    return o.view(6, count, ctx.n_limbs)


def abs_step(ctx, opened, ta, tb, tab, x, y, bits, k=K, kappa=KAPPA, out=None):
    """The abs step, ONE launch after sign_mask's open: opened (6, count, limbs) or flat; ta, tb, tab (3, count, limbs); bits (k + kappa,
    count, limbs) -> (masked, kept): masked (1, count, limbs) = trunc_mask(w, k, k - 1), the comparison's array to open; kept (5, count,
    limbs) = |x|, |y|, G = [sigma_y sx], w = |x| - |y|, r1.  out: a pair."""
    check_params(ctx.modulus, _int(k, "k"), k - 1, kappa, full=True)
    x = ctx.elems(x, what="x")
    count = x.numel() // ctx.n_limbs
    y, opened = ctx.elems(y, count, what="y"), ctx.elems(opened, 6 * count, what="opened")
    ta, tb, tab = (_rows3(ctx, v, 3, count, w) for v, w in ((ta, "ta"), (tb, "tb"), (tab, "tab")))
    bits, _ = _planes(ctx, bits, k + kappa, count, "bits")
    g0, g1 = _pair(out)
    o0, o1 = _planes_out(ctx, g0, 1, count, "out masked"), _planes_out(ctx, g1, 5, count, "out kept")
    P = ctx.ptr
    ctx.check(ctx.lib.hb_fxatan_abs(ctx.h, P(opened), P(ta), P(tb), P(tab), P(x), P(y), P(bits), k, kappa, P(o0), P(o1), count, ctx.stream()), "hb_fxatan_abs")
    return o0.view(1, count, ctx.n_limbs), o1.view(5, count, ctx.n_limbs)


def select_mask(ctx, c, w, sx, ta, tb, out=None):
    """The masked pairs of the select step, ONE launch after the swap's comparison: c = [w < 0], w, sx (count, limbs); ta, tb (2, count,
    limbs) -> (4, count, limbs): c - ta[0], w - tb[0], sigma_c - ta[1], sigma_x - tb[1], the array to open"""
    c = ctx.elems(c, what="c")
    count = c.numel() // ctx.n_limbs
    w, sx = ctx.elems(w, count, what="w"), ctx.elems(sx, count, what="sx")
    ta, tb = _rows3(ctx, ta, 2, count, "ta"), _rows3(ctx, tb, 2, count, "tb")
    o = _planes_out(ctx, out, 4, count)
    P = ctx.ptr
    ctx.check(ctx.lib.hb_fxatan_select_mask(ctx.h, P(c), P(w), P(sx), P(ta), P(tb), P(o), count, ctx.stream()), "hb_fxatan_select_mask")
    return o.view(4, count, ctx.n_limbs)


def select(ctx, opened, ta, tb, tab, ax, ay, out=None):
    """The select step, ONE launch after select_mask's open: opened (4, count, limbs) or flat; ta, tb, tab (2, count, limbs); ax = |x|, ay =
    |y| -> (3, count, limbs): num = |y| + [c w], den = |x| - [c w], e1 = [sigma_c sigma_x]"""
    ax = ctx.elems(ax, what="ax")
    count = ax.numel() // ctx.n_limbs
    ay, opened = ctx.elems(ay, count, what="ay"), ctx.elems(opened, 4 * count, what="opened")
    ta, tb, tab = (_rows3(ctx, v, 2, count, w) for v, w in ((ta, "ta"), (tb, "tb"), (tab, "tab")))
    o = _planes_out(ctx, out, 3, count)
    P = ctx.ptr
    ctx.check(ctx.lib.hb_fxatan_select(ctx.h, P(opened), P(ta), P(tb), P(tab), P(ax), P(ay), P(o), count, ctx.stream()), "hb_fxatan_select")
    return o.view(3, count, ctx.n_limbs)


def atan_first(ctx, q, shift, sy, e1, ta, tb, d, out=None):
    """The ladder's first step, ONE launch after the division: q, sy, e1 (count, limbs); ta, tb (2, count, limbs); t = 2^shift q ->
    (masked, powers): masked (4, count, limbs) = t - ta[0], t - tb[0], sigma_y - ta[1], e1 - tb[1], the array to open for u = [t t] and E =
    [sigma_y e1]; powers ((d + 1) / 2, count, limbs) with row 0 = t and the other rows for atan_level to fill.  out: a pair."""
    _check_degree(d)
    if not 0 <= _int(shift, "shift") <= 255:
        raise ValueError(f"needs 0 <= shift <= 255, got {shift}")
    q = ctx.elems(q, what="q")
    count = q.numel() // ctx.n_limbs
    sy, e1 = ctx.elems(sy, count, what="sy"), ctx.elems(e1, count, what="e1")
    ta, tb = _rows3(ctx, ta, 2, count, "ta"), _rows3(ctx, tb, 2, count, "tb")
    g0, g1 = _pair(out)
    rows = (d + 1) // 2
    o0, o1 = _planes_out(ctx, g0, 4, count, "out masked"), _planes_out(ctx, g1, rows, count, "out powers")
    P = ctx.ptr
    ctx.check(ctx.lib.hb_fxatan_first(ctx.h, P(q), shift, P(sy), P(e1), P(ta), P(tb), P(o0), P(o1), count, ctx.stream()), "hb_fxatan_first")
    return o0.view(4, count, ctx.n_limbs), o1.view(rows, count, ctx.n_limbs)


def atan_level(ctx, level, d, opened, s, m, ta, tb, powers, out=None):
    """One level of the ladder, ONE launch after the open of level `level`'s masked truncations, 0 <= level < levels: s, opened (n, count,
    limbs) (opened flat is fine), n the products of the level in step order (the odd powers, then the square): t^(2j+1) = (s - (opened mod
    2^m)) / 2^m goes to row j of `powers` ((d + 1) / 2, count, limbs), IN PLACE; ta, tb (products of level + 1, count, limbs) -> masked
    (2 products, count, limbs), rows 2q, 2q + 1 = first operand - ta[q], u^(2^level) - tb[q], the array to open."""
    _check_degree(d)
    if not 0 <= _int(level, "level") < _level_count(d):
        raise ValueError(f"needs 0 <= level < {_level_count(d)} for d = {d}, got {level}")
    _check_shift(ctx, m)
    done, nxt = _level_products(level, d), _level_products(level + 1, d)
    s, count = _planes(ctx, s, done, None, "s", exact=True)
    opened = ctx.elems(opened, done * count, what="opened")
    ta, tb = _rows3(ctx, ta, nxt, count, "ta"), _rows3(ctx, tb, nxt, count, "tb")
    if not isinstance(powers, ctx.torch.Tensor) or not powers.is_contiguous():
        raise ValueError("powers: must be a contiguous tensor, it is updated in place")
    powers = ctx.elems(powers, (d + 1) // 2 * count, what="powers")
    o = _planes_out(ctx, out, 2 * nxt, count)
    inv = _inv2m(ctx, m)
    P = ctx.ptr
    ctx.check(ctx.lib.hb_fxatan_level(ctx.h, level, d, P(opened), P(s), m, inv.ctypes.data, P(ta), P(tb), P(o), P(powers), count, ctx.stream()), "hb_fxatan_level")
    return o.view(2 * nxt, count, ctx.n_limbs)


def atan_poly_mask(ctx, d, opened, s, m_in, powers, coef, bits, width, m_out, kappa=KAPPA, out=None):
    """The polynomial and its truncation mask, ONE launch after the open of the LAST level's masked truncations: s, opened (n, count,
    limbs) of that level finish its powers; the older powers are rows of `powers` ((d + 1) / 2, count, limbs), which is only read.  L =
    sum_j coef[j] t^(2j+1) with coef ((d + 1) / 2, limbs) public; bits (width + kappa, count, limbs) -> (masked, s): trunc_mask(L) to open
    and L + r1, (1, count, limbs) each.  out: a pair."""
    _check_degree(d)
    _check_shift(ctx, m_in, "m_in")
    check_params(ctx.modulus, width, m_out, kappa)
    done = _level_products(_level_count(d), d)
    s, count = _planes(ctx, s, done, None, "s", exact=True)
    opened = ctx.elems(opened, done * count, what="opened")
    powers = _rows3(ctx, powers, (d + 1) // 2, count, "powers")
    coef = ctx.elems(coef, (d + 1) // 2, what="coef")
    bits, _ = _planes(ctx, bits, width + kappa, count, "bits")
    g0, g1 = _pair(out)
    o0, o1 = _planes_out(ctx, g0, 1, count, "out masked"), _planes_out(ctx, g1, 1, count, "out kept")
    inv = _inv2m(ctx, m_in)
    P = ctx.ptr
    ctx.check(ctx.lib.hb_fxatan_poly_mask(ctx.h, d, P(opened), P(s), m_in, inv.ctypes.data, P(powers), P(coef), P(bits), width, m_out, kappa, P(o0), P(o1), count, ctx.stream()),
              "hb_fxatan_poly_mask")
    return o0.view(1, count, ctx.n_limbs), o1.view(1, count, ctx.n_limbs)


def atan_assemble(ctx, opened, s, m, eopened, ea, eb, eab, sy, g, consts, ta, tb, out=None):
    """The assemble step, ONE launch after the open of L's masked truncation: a = (s - (opened mod 2^m)) / 2^m; E = [sigma_y e1] by the
    Beaver combine of eopened (2, count, limbs) or flat, rows 2, 3 of atan_first's array opened, with its triple (ea, eb, eab); consts = (A,
    B) residues; ta, tb the next triple's factors -> (masked, c): masked (2, count, limbs) = E - ta, a - tb, the array to open; c (count,
    limbs) = A g + B (sigma_y - E).  out: a pair."""
    _check_shift(ctx, m)
    sy = ctx.elems(sy, what="sy")
    count = sy.numel() // ctx.n_limbs
    g, s, opened = ctx.elems(g, count, what="g"), ctx.elems(s, count, what="s"), ctx.elems(opened, count, what="opened")
    eopened = ctx.elems(eopened, 2 * count, what="eopened")
    ea, eb, eab, ta, tb = (ctx.elems(v, count, what=w) for v, w in ((ea, "ea"), (eb, "eb"), (eab, "eab"), (ta, "ta"), (tb, "tb")))
    try:
        ca, cb = consts
    except (TypeError, ValueError):
        raise ValueError("consts: expected (A, B)") from None
    cst = ctx.host_elems([_int(ca, "A") % ctx.modulus, _int(cb, "B") % ctx.modulus])
    g0, g1 = _pair(out)
    o0, o1 = _planes_out(ctx, g0, 2, count, "out masked"), _elems_out(ctx, g1, count, "out c")
    inv = _inv2m(ctx, m)
    P = ctx.ptr
    ctx.check(ctx.lib.hb_fxatan_assemble(ctx.h, P(opened), P(s), m, inv.ctypes.data, P(eopened), P(ea), P(eb), P(eab), P(sy), P(g), cst.ctypes.data, P(ta), P(tb), P(o0), P(o1),
                                         count, ctx.stream()), "hb_fxatan_assemble")
    return o0.view(2, count, ctx.n_limbs), o1


def atan_finish(ctx, opened, ta, tb, tab, c, out=None):
    """The last step, ONE launch: c + [E a] by the Beaver combine of opened (2, count, limbs) or flat with (ta, tb, tab), (count, limbs)"""
    c = ctx.elems(c, what="c")
    count = c.numel() // ctx.n_limbs
    opened = ctx.elems(opened, 2 * count, what="opened")
    ta, tb, tab = (ctx.elems(v, count, what=w) for v, w in ((ta, "ta"), (tb, "tb"), (tab, "tab")))
    o = _elems_out(ctx, out, count)
    P = ctx.ptr
    ctx.check(ctx.lib.hb_fxatan_finish(ctx.h, P(opened), P(ta), P(tb), P(tab), P(c), P(o), count, ctx.stream()), "hb_fxatan_finish")
    return o


# ---- protocols over an OpenCoalescer ---------------------------------------------------------------------------------------
def _check_room(ctx, lay, k, f, kappa):
    """ValueError for parameters the modulus, the 256-bit truncation width or the kernels' degree have no room for"""
    p, d, width, dwidth = ctx.modulus, lay["degree"], lay["width"], lay["div"]["width"]
    check_params(p, k, k - 1, kappa, full=True)
    if d > MAX_DEGREE:
        raise ValueError(f"f = {f} needs a polynomial of degree {d}: at most {MAX_DEGREE}")
    if max(width, dwidth) > 256:
        raise ValueError(f"the truncations need {max(width, dwidth)} bits: at most 256")
    for m in set(_div_shifts(k, f)):
        check_params(p, dwidth, m, kappa)
    for m in (k - 1, k - 1 + GUARD_BITS):
        check_params(p, width, m, kappa)


async def atan2(co, y, x, bits, triples, f=F, k=K, kappa=KAPPA, turns=False):
    """Shares of atan2(Y, X) 2^f in (-pi, pi] (turns=True: of atan2(Y, X) / (2 pi) 2^f in (-1/2, 1/2]) up to atan_error_bound(k, f, turns)
    ulps, for shares of signed k-bit y and x with |x|, |y| < 2^(k-1), Y = y / 2^f, X = x / 2^f; (0, 0) gives 0 and y = 0, x < 0 gives +pi.
    atan_opens opens for any count; atan_planes bit planes and atan_triples triples an element, in the order of atan_layout.  y, x, bits
    and triples are left untouched.  ValueError before anything is opened; nothing raises on secret values."""
    ctx, t = co.ctx, co.ctx.torch
    turns = bool(turns)
    lay = atan_layout(k, f, kappa, turns)
    _check_room(ctx, lay, k, f, kappa)
    d, width, levels, products, dlay = lay["degree"], lay["width"], lay["levels"], lay["products"], lay["div"]
    n, nb, m_out, L = k - 1, width + kappa, k - 1 + GUARD_BITS, ctx.n_limbs
    y = ctx.elems(y, what="y")
    count = y.numel() // L
    y, x = y.view(count, L), ctx.elems(x, count, what="x").view(count, L)
    bits, _ = _planes(ctx, bits, lay["n_planes"], count, "bits")
    triples = _triples(ctx, triples, lay["n_triples"], count)
    rows = _Rows(bits, triples)
    coef = coefficient_rows(ctx, k, f, turns, d)
    consts = assemble_constants(ctx.modulus, f, turns)

    # 1 signs: ONE comparison over (x, y); planes and triples 2 i, 2 i + 1 viewed as row i of 2 count elements
    ct = carry_triples(n)
    s = await ltz(co, t.cat([x, y]), rows.planes(2 * (k + kappa)).view(k + kappa, 2 * count, L), tuple(v.view(ct, 2 * count, L) for v in rows.take(2 * ct)), k, kappa)
    sx, sy = s[:count], s[count:]
    # 2 abs
    trip = rows.take(3)
    opened = await _open_rows(co, sign_mask(ctx, s, x, y, trip[0], trip[1]))
    swap_bits = rows.planes(k + kappa)
    masked, kept = abs_step(ctx, opened, trip[0], trip[1], trip[2], x, y, swap_bits, k, kappa)            # kept: |x|, |y|, G, w, r1
    # 3 swap: the comparison after its mask, as fixedpoint._div2m runs it
    c_open = await _open_rows(co, masked)
    leaves_g, leaves_p = ltl_leaves(ctx, c_open, swap_bits, n)
    carry = await _carry_tree(co, leaves_g, leaves_p, rows.take(ct), n)
    c = div2m_finish(ctx, kept[3], c_open, kept[4], carry, n, NEG_TRUNC, out=carry)
    # 4 select
    trip = rows.take(2)
    opened = await _open_rows(co, select_mask(ctx, c, kept[3], sx, trip[0], trip[1]))
    nde = select(ctx, opened, trip[0], trip[1], trip[2], kept[0], kept[1])                               # num, den, e1
    # 5 quotient
    q = await div(co, nde[0], nde[1], rows.planes(dlay["n_planes"]), rows.take(dlay["n_triples"]), f, k, kappa, None, False)
    # 6 ladder
    trip = rows.take(2)
    e_trip = tuple(v[1] for v in trip)
    masked, powers = atan_first(ctx, q, n - f, sy, nde[2], trip[0], trip[1], d)
    e_opened = None
    for level in range(levels + 1):
        c_level = products[level]
        opened = await _open_rows(co, masked)
        if level == 0:
            e_opened = opened[2 * count:]
        masked, sv = products_trunc(ctx, opened[:2 * c_level * count], trip[0][:c_level], trip[1][:c_level], trip[2][:c_level], rows.planes(c_level * nb), width, n, kappa)
        opened = await _open_rows(co, masked)
        if level < levels:
            trip = rows.take(products[level + 1])
            masked = atan_level(ctx, level, d, opened, sv, n, trip[0], trip[1], powers)
        else:
            # 7 polynomial
            masked, sv = atan_poly_mask(ctx, d, opened, sv, n, powers, coef, rows.planes(nb), width, m_out, kappa)
    # 8 assemble
    opened = await _open_rows(co, masked)
    trip = rows.take(1)
    masked, cst = atan_assemble(ctx, opened, sv, m_out, e_opened, e_trip[0], e_trip[1], e_trip[2], sy, kept[2], consts, trip[0][0], trip[1][0])
    opened = await _open_rows(co, masked)
    return atan_finish(ctx, opened, trip[0][0], trip[1][0], trip[2][0], cst)


async def atan(co, x, bits, triples, f=F, k=K, kappa=KAPPA, turns=False):
    """Shares of atan(X) 2^f in (-pi / 2, pi / 2) (turns: over 2 pi): atan2(x, one) with `one` the public 2^f as shares.  The opens and the
    preprocessing layout of atan2."""
    ctx = co.ctx
    _check_kf(k, f)
    x = ctx.elems(x, what="x")
    count = x.numel() // ctx.n_limbs
    one = ctx.to_device(ctx.host_elems([(1 << f) % ctx.modulus])).expand(count, ctx.n_limbs).contiguous()
    return await atan2(co, x, one, bits, triples, f, k, kappa, turns)

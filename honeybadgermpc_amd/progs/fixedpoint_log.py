"""
Base-2, natural and public-base logarithm of shared fixed-point numbers on the device (csrc/hb_fxlog.hip, the scale step of
csrc/hb_fxsqrt.hip and the products-to-masks step of csrc/hb_fxexp.hip): the normalised mantissa's logarithm as a truncated Chebyshev
series, evaluated from the powers of a shared value, for unsigned k-bit values with f fractional bits, on the (count, limbs) share
arrays of progs/fixedpoint.py.  The reference has no logarithm; the pin here is the mathematics: log_model on Python ints, and the same
steps composed from share_arithmetic and fixedpoint.trunc_mask / trunc_pr_finish.

Inputs are shares of x with 0 < x < 2^(k-1), value X = x / 2^f; k / 2 <= f <= k - 2.  A negative x is outside the contract (its low
k - 1 bits are what the bit decomposition sees).  With N = k - 1, beta = 2^N, g = f + GUARD_BITS, d = log_degree(k, f, base) and W =
log_width(k, f, d, base) the width of every truncation:

    1 bits      bit_decompose(x, k, N): N planes, least significant first                          bit_opens(N) opens
    2 prefix OR y_i = OR_{l >= i} x_l in place (fixedpoint_division's network, unchanged)          preor_levels(N) opens
    3 scale     fixedpoint_sqrt.sqrt_norm_mask, unchanged, with two PUBLIC weight sets (log_weights): z_i = y_i - y_{i+1} is one-hot at
                the top bit e of x; v = sum 2^(N-1-i) z_i, I = sum W_i z_i with W_i = round((i + 1 - f) 2^f / log2(base)) -- the
                integer part at the result's scale, no product, exact for base 2 -- and Y = beta y_0 = beta [x != 0].
                c = [x v] in [beta / 2, beta)                                                      1 open
    4 first     t = 4 c - 3 Y in [-beta, beta), signed; C = c / beta = (3 + T) / 4 with T = t / beta, so
                log2 X = (e + 1 - f) + log2(3/4) + log2(1 + T / 3).  t is power 1; the masked pair of [t t]
    5 powers    level l = 1, 2, .. forms t^j, 2^(l-1) < j <= min(2^l, d), as trunc_pr([t^(2^(l-1)) t^(j - 2^(l-1))], N): every power
                stays at scale beta.  ceil(log2 d) levels, d - 1 products and d - 1 truncations      2 ceil(log2 d) opens
    6 polynomial L = A_0 Y + sum_{j >= 1} A_j t^j with the PUBLIC integers A_j = round(a_j 2^g) (log_coefficients): no product;
                masked for a truncation by m = N + g - f                                            1 open
    7 result    I + trunc_pr(L, m)

log_opens = bit_opens(N) + preor_levels(N) + 1 + 2 ceil(log2 d) + 1.  The base only changes the public constants W_i and A_j.
x = 0 raises nothing -- the operand is secret --: every bit is 0, so v = I = Y = 0, c = t = 0, every power and L are 0 and the result
is 0 + trunc_pr(0, m) = 0 for any r1: what log_model gives.  No masked value wraps.

Where this leaves the issue's sketch: "products to truncation masks" between the two opens of a level is
fixedpoint_exp.products_trunc, which takes up to 128 products in one launch; fixedpoint_division.product_step(TRUNC) takes two, and a
level has up to d / 2.

The series (DESIGN.md section 3ad has the derivation).  With q = 3 - sqrt 8, 1 + T / 3 = (1 + 2 q T + q^2) / (1 + q^2) and 1 + q^2 =
6 q, so ln(1 + T / 3) = -ln(6 q) - 2 sum_{n >= 1} (-q)^n T_n(T) / n, T_n the Chebyshev polynomials: |T_n| <= 1 on [-1, 1], so the
series cut at degree d is off by at most 2 q^(d+1) / ((d + 1) (1 - q)) (series_tail).  log_degree is the smallest d >= 2 whose tail is
at most 1/4 ulp of the result.  The constants q, ln 2, ln(6 q), ln(3/4) and ln(base) are enclosed by rationals 2^-440 apart from
integer arithmetic (isqrt and the atanh series with its remainder), the series is converted to monomials over Fractions, ln(3/4) -
ln(6 q) joins the constant term, everything is divided by ln(base) and every coefficient is rounded once to 2^-g.  The monomial
coefficients decay like 0.41^j: there is no cancellation to fear.

Error, in ulps of 2^-f of the result, for 0 < x < 2^(k-1) (log_error_bound, exact Fractions): the series tail; the coefficient roundings,
(d + 1) 2^-(GUARD_BITS+1); the power truncations, 2^(f-N) sum_j |A_j| 2^-g E_j with E_j <= 1 + E_a + E_b + E_a E_b / beta for t^j = [t^a
t^b] (E_1 = 0, so E_j is about j - 1): negligible at k = 2 f, where 2^(f-N) is tiny, and NOT at f = k - 2, where it is 1/2 of about
sum_j (j - 1) |a_j|; the rounding of W_i, 1/2 for bases other than 2; the last trunc_pr, 1; and 2^-64 for the enclosures.

Preprocessing is handed in as tensors, consumed in step order from row 0; log_layout names the row ranges.  `bits` is (log_planes,
count, limbs): bit decomposition k + kappa, then W + kappa for every truncation in step order: the powers 2 .. d, then L.  `triples =
(p, q, pq)` is (log_triples, count, limbs) each: bit_triples(N), preor_triples(N), the scale 1, then one a power 2 .. d.

Host functions:

    log_degree(k, f, base), series_tail(d), log_coefficients(k, f, base), log_weights(k, f, base)
    log_error_bound(k, f, d, base), log_width(k, f, d, base)        exact; ulps of 2^-f
    log_shifts, log_layout, log_planes, log_triples, log_opens
    log_model(x, p, k, f, r1s, base) -> what the protocol opens to for the dealt r1 of every truncation in step order

Tensor level, one launch each on torch's current stream, nothing synchronises:

    log_first(ctx, opened, ta, tb, tab, ybig, nxt, d)      -> (masked, powers): t, row 0 of powers (d, count, limbs); masked t - a, t - b
    log_level(ctx, level, d, opened, s, m, ta, tb, powers) -> masked: finishes the level's powers into `powers`, masks the next level
    log_poly_mask(ctx, d, opened, s, m_in, powers, ybig, coef, bits, width, m_out, kappa) -> (masked, s): L's truncation mask
    log_finish(ctx, opened, s, m, ipart)                   -> the result
    (the scale step is fixedpoint_sqrt.sqrt_norm_mask, products to truncation masks fixedpoint_exp.products_trunc)

Protocol level, coroutines over an OpenCoalescer: log2, log, log_base.  From the scale's open on, ONE launch between consecutive
opens.  Inputs and preprocessing are left untouched; ValueError before anything is opened.
"""
from fractions import Fraction
from functools import lru_cache
from math import isqrt

from .bit_decomposition import bit_decompose, bit_opens, bit_triples
from .fixedpoint import F, K, KAPPA, _elems_out, _int, _inv2m, _pair, _planes, _planes_out, _triples, check_params
from .fixedpoint_division import _ceil, _check_kf, _check_norm, _open_rows, _prefix_or_in_place, _ranges, _Rows, norm_model, preor_levels, preor_triples
from .fixedpoint_exp import products_trunc
from .fixedpoint_sqrt import sqrt_norm_mask

GUARD_BITS = 3                                                   # the coefficients carry the result's bits and these
MAX_DEGREE = 64                                                  # hb_fxlog.hip's
E = "e"                                                          # the base of the natural logarithm, for the `base` arguments
_PREC = 448                                                      # bits of the enclosures the constants are rounded from
_SLACK = Fraction(1, 1 << 64)                                    # ulps: what the enclosures' 2^-440 can add, f <= 255, with room to spare


# ---- host functions: exact constants -------------------------------------------------------------------------------------------
def _atanh_bounds(z, prec):
    """-> (lo, hi) Fractions around atanh(z) for a rational 0 <= z <= 1/2, less than 2^-prec apart: the partial sums of z^(2n+1) / (2n +
    1) in integers at prec + 32 bits, every operation rounded down for lo (from z rounded down) and up for hi (from z rounded up), and
    for hi the remainder, below z^(2n+3) / ((2n + 3) (1 - z^2)) <= 2 z^(2n+3)"""
    w = prec + 32
    floor_z = (z.numerator << w) // z.denominator

    def run(zi, up):
        z2, term, total, n = (zi * zi >> w) + up, zi, 0, 0
        while term >> 30:
            total += term // (2 * n + 1) + up
            term, n = (term * z2 >> w) + up, n + 1
        return Fraction(total + (2 * term + 1 if up else 0), 1 << w)

    return run(floor_z, 0), run(floor_z + 1, 1)


@lru_cache(maxsize=None)
def _ln_bounds(y, prec=_PREC):
    """-> (lo, hi) Fractions around ln(y) for a rational y > 0, less than 2^-(prec-8) apart for |log2 y| < 64: y = 2^e w with 2/3 <= w
    <= 4/3, ln w = 2 atanh((w - 1) / (w + 1)), ln 2 = 2 atanh(1/3)"""
    y = Fraction(y)
    e = 0
    while y > Fraction(4, 3):
        y, e = y / 2, e + 1
    while y < Fraction(2, 3):
        y, e = y * 2, e - 1
    z = (y - 1) / (y + 1)
    lo, hi = _atanh_bounds(abs(z), prec)
    lo, hi = (2 * lo, 2 * hi) if z >= 0 else (-2 * hi, -2 * lo)
    if e:
        l2, h2 = _atanh_bounds(Fraction(1, 3), prec)
        lo, hi = (lo + 2 * e * l2, hi + 2 * e * h2) if e > 0 else (lo + 2 * e * h2, hi + 2 * e * l2)
    return lo, hi


def _mid(pair):
    return (pair[0] + pair[1]) / 2


_Q_LO = 3 - Fraction(isqrt(8 << (2 * _PREC)) + 1, 1 << _PREC)      # q = 3 - sqrt 8 from below and from above, 2^-_PREC apart
_Q_HI = 3 - Fraction(isqrt(8 << (2 * _PREC)), 1 << _PREC)
_Q = (_Q_LO + _Q_HI) / 2


def _base(base):
    if base == E:
        return base
    if not isinstance(base, int) or isinstance(base, bool) or base < 2:
        raise ValueError(f"base must be an integer >= 2 or E, got {base!r}")
    return base


@lru_cache(maxsize=None)
def _ln_base(base):
    """ln(base) to 2^-440, a Fraction"""
    return Fraction(1) if base == E else _mid(_ln_bounds(Fraction(base)))


@lru_cache(maxsize=None)
def _ln_6q():
    return (_ln_bounds(6 * _Q_LO)[0] + _ln_bounds(6 * _Q_HI)[1]) / 2


def _chebyshev(d):
    """-> [T_0 .. T_d] as lists of integer monomial coefficients, lowest first"""
    polys = [[1], [0, 1]]
    for n in range(2, d + 1):
        a, b = polys[-1], polys[-2]
        nxt = [0] + [2 * c for c in a]
        for i, c in enumerate(b):
            nxt[i] -= c
        polys.append(nxt)
    return polys[:d + 1]


def series_tail(d):
    """>= |ln(1 + T / 3) - the series cut at degree d| on [-1, 1]: 2 q^(d+1) / ((d + 1) (1 - q)), with q from above; a Fraction"""
    return 2 * _Q_HI ** (d + 1) / ((d + 1) * (1 - _Q_HI))


def _tail_ulps(d, f, base):
    return series_tail(d) * (1 << f) / (_ln_base(base) - Fraction(1, 1 << 400))


@lru_cache(maxsize=None)
def log_degree(k=K, f=F, base=2):
    """the smallest d >= 2 whose series tail is at most 1/4 ulp of 2^-f of the result"""
    _check_kf(k, f)
    base = _base(base)
    d = 2
    while _tail_ulps(d, f, base) > Fraction(1, 4):
        d += 1
    return d


def _degree(k, f, d, base):
    if d is None:
        return log_degree(k, f, base)
    if _int(d, "d") < 2:
        raise ValueError(f"the degree must be at least 2, got {d}")
    return d


@lru_cache(maxsize=None)
def _monomials(d, base):
    """the series cut at degree d, ln(3/4) folded in, over ln(base): [a_0 .. a_d], Fractions (from the constants' midpoints)"""
    polys = _chebyshev(d)
    a = [Fraction(0)] * (d + 1)
    for n in range(1, d + 1):
        cn = -2 * (-_Q) ** n / n
        for j, c in enumerate(polys[n]):
            a[j] += cn * c
    a[0] += _mid(_ln_bounds(Fraction(3, 4))) - _ln_6q()
    return [c / _ln_base(base) for c in a]


def _round(q):
    return (2 * q.numerator + q.denominator) // (2 * q.denominator)


@lru_cache(maxsize=None)
def log_coefficients(k=K, f=F, base=2, d=None):
    """the PUBLIC integers A_0 .. A_d at scale 2^g, g = f + GUARD_BITS: the polynomial in T = t / beta whose value is log_base(C) 2^g for
    the mantissa C = (3 + T) / 4, every coefficient rounded once"""
    _check_kf(k, f)
    base = _base(base)
    d = _degree(k, f, d, base)
    return [_round(c * (1 << (f + GUARD_BITS))) for c in _monomials(d, base)]


@lru_cache(maxsize=None)
def log_weights(k=K, f=F, base=2):
    """the PUBLIC weights of the scale step, W_i for i = 0 .. k - 2 (the top bit at i), two sets: round((i + 1 - f) 2^f / log2(base)),
    the integer part at the result's scale (exact for base 2), and beta for every i, which makes Y = beta [x != 0]"""
    _check_kf(k, f)
    base = _base(base)
    if base == 2:
        first = [(i + 1 - f) << f for i in range(k - 1)]
    else:
        r = _mid(_ln_bounds(Fraction(2))) / _ln_base(base)
        first = [_round((i + 1 - f) * (1 << f) * r) for i in range(k - 1)]
    return first, [1 << (k - 1)] * (k - 1)


def _level_count(d):
    return (d - 1).bit_length()


def _level_powers(level, d):
    """the powers level `level` >= 1 forms: half < j <= min(2 half, d)"""
    half = 1 << (level - 1)
    return list(range(half + 1, min(2 * half, d) + 1))


def _power_errors(k, d):
    """E_j >= |t^j as computed - beta T^j|: E_1 = 0, and t^(a+b) = trunc_pr([t^a t^b], N) adds less than 1 to (beta T^a + E_a) (beta T^b +
    E_b) / beta"""
    beta = 1 << (k - 1)
    err = {1: Fraction(0)}
    for level in range(1, _level_count(d) + 1):
        half = 1 << (level - 1)
        for j in _level_powers(level, d):
            err[j] = 1 + err[half] + err[j - half] + err[half] * err[j - half] / beta
    return err


def log_error_bound(k=K, f=F, d=None, base=2):
    """|result - log_base(x / 2^f) 2^f| in ulps of 2^-f for 0 < x < 2^(k-1), an exact Fraction: the series tail, the coefficient
    roundings, the power truncations (negligible at k = 2 f and not at f = k - 2: the module docstring), the rounding of W_i, the last
    trunc_pr and the enclosures"""
    _check_kf(k, f)
    base = _base(base)
    d = _degree(k, f, d, base)
    beta, g = 1 << (k - 1), f + GUARD_BITS
    err = _power_errors(k, d)
    coef = log_coefficients(k, f, base, d)
    rounding = sum(Fraction(1, 2) * (1 + err.get(j, 0) / beta) for j in range(d + 1)) / (1 << GUARD_BITS)
    powers = sum(abs(coef[j]) * err[j] for j in range(1, d + 1)) * Fraction(1 << f, beta << g)
    return _tail_ulps(d, f, base) + rounding + powers + (0 if base == 2 else Fraction(1, 2)) + 1 + _SLACK


@lru_cache(maxsize=None)
def log_width(k=K, f=F, d=None, base=2):
    """the signed width of the truncations: what holds every product, |t^a t^b| <= (beta + E_a) (beta + E_b), and L, |L| <= sum_j |A_j|
    (beta + E_j); at least 2 k"""
    _check_kf(k, f)
    base = _base(base)
    d = _degree(k, f, d, base)
    beta = 1 << (k - 1)
    err = _power_errors(k, d)
    coef = log_coefficients(k, f, base, d)
    top = max(err.values())
    bounds = [_ceil((beta + top) ** 2), _ceil(sum(abs(c) * (beta + err.get(j, 0)) for j, c in enumerate(coef)))]
    return max(2 * k, max(bounds).bit_length() + 1)


# ---- host functions: counts ------------------------------------------------------------------------------------------------------
def log_shifts(k=K, f=F, d=None, base=2):
    """m of every truncation in step order: the powers 2 .. d by N, then L by N + GUARD_BITS"""
    _check_kf(k, f)
    d = _degree(k, f, d, _base(base))
    return [k - 1] * (d - 1) + [k - 1 + GUARD_BITS]


def log_layout(k=K, f=F, kappa=KAPPA, d=None, base=2):
    """-> {"degree", "width", "levels", "planes": {name: (start, stop)}, "triples": {name: (start, stop)}, "n_planes", "n_triples", "opens"}:
    the rows of `bits` and of the triple tensors each step consumes, in step order from row 0.  Planes: bit_decompose, level<l> (l = 1 ..
    levels: one truncation a power), poly.  Triples: bit_decompose, prefix_or, norm, level<l>."""
    _check_kf(k, f)
    _int(kappa, "kappa")
    base = _base(base)
    d = _degree(k, f, d, base)
    width, n, levels = log_width(k, f, d, base), k - 1, _level_count(d)
    nb = width + kappa
    planes = [("bit_decompose", k + kappa)]
    triples = [("bit_decompose", bit_triples(n)), ("prefix_or", preor_triples(n)), ("norm", 1)]
    for level in range(1, levels + 1):
        c = len(_level_powers(level, d))
        planes.append((f"level{level}", c * nb))
        triples.append((f"level{level}", c))
    planes.append(("poly", nb))
    p_ranges, n_planes = _ranges(planes)
    t_ranges, n_triples = _ranges(triples)
    return {"degree": d, "width": width, "levels": levels, "planes": p_ranges, "triples": t_ranges, "n_planes": n_planes, "n_triples": n_triples,
            "opens": bit_opens(n) + preor_levels(n) + 1 + 2 * levels + 1}


def log_planes(k=K, f=F, kappa=KAPPA, d=None, base=2):
    return log_layout(k, f, kappa, d, base)["n_planes"]


def log_triples(k=K, f=F, d=None, base=2):
    return log_layout(k, f, 0, d, base)["n_triples"]


def log_opens(k=K, f=F, d=None, base=2):
    return log_layout(k, f, 0, d, base)["opens"]


# ---- host functions: the model ---------------------------------------------------------------------------------------------------
def log_model(x, p, k=K, f=F, r1s=(), base=2, d=None):
    """What the protocol's result opens to, a residue mod p: x a residue of an unsigned value below 2^(k-1); r1s the dealt r1 of every
    truncation in step order, below 2^m for m of log_shifts.  Python ints only; r2 does not matter (no masked value wraps for operands
    in the documented range).  x = 0 gives 0."""
    _check_kf(k, f)
    base = _base(base)
    d = _degree(k, f, d, base)
    width = log_width(k, f, d, base)
    check_params(p, k, k - 1, 0, full=True)
    limits = log_shifts(k, f, d, base)
    for m in set(limits):
        check_params(p, width, m, 0)
    r1s = [_int(r, "r1") for r in r1s]
    if len(r1s) != len(limits) or any(not 0 <= r < 1 << m for r, m in zip(r1s, limits)):
        raise ValueError(f"r1s: expected {len(limits)} values below 2^m for m = {limits}")
    x = int(x) % p
    if x >> (k - 1):
        raise ValueError(f"x must be below 2^(k-1), got {x}")
    beta = 1 << (k - 1)
    c, _ = norm_model(x, k, signed=False)
    top = x.bit_length() - 1
    big, ipart = (beta, log_weights(k, f, base)[0][top]) if x else (0, 0)
    r1s, shifts = iter(r1s), iter(limits)

    def tr(v):
        m, r1 = next(shifts), next(r1s)
        return (v - (v + (1 << (width - 1)) + r1) % p % (1 << m) + r1) * pow(2, -m, p) % p

    powers = {1: (4 * c - 3 * big) % p}
    for level in range(1, _level_count(d) + 1):
        half = 1 << (level - 1)
        for j in _level_powers(level, d):
            powers[j] = tr(powers[half] * powers[j - half] % p)
    coef = log_coefficients(k, f, base, d)
    poly = (coef[0] * big + sum(coef[j] * powers[j] for j in range(1, d + 1))) % p
    return (ipart + tr(poly)) % p


# ---- tensor level ----------------------------------------------------------------------------------------------------------
def weight_rows(ctx, k, f, base=2):
    """the scale step's public constants on the device, (2, k - 1, limbs): D_i = W_i - W_{i-1} mod p for the two sets of log_weights, so
    that sum_i D_i y_i = sum_i W_i (y_i - y_{i+1}); the second set is beta, 0, 0, .."""
    flat = [(w - (ws[i - 1] if i else 0)) % ctx.modulus for ws in log_weights(k, f, base) for i, w in enumerate(ws)]
    return ctx.to_device(ctx.host_elems(flat)).view(2, k - 1, ctx.n_limbs)


def coefficient_rows(ctx, k, f, base=2, d=None):
    """log_coefficients mod p on the device, (d + 1, limbs)"""
    return ctx.to_device(ctx.host_elems([c % ctx.modulus for c in log_coefficients(k, f, base, d)]))


def _check_degree(d):
    if not 2 <= _int(d, "d") <= MAX_DEGREE:
        raise ValueError(f"needs 2 <= d <= {MAX_DEGREE}, got {d}")
    return d


def _check_shift(ctx, m, what="m"):
    if not 0 < _int(m, what) <= ctx.modulus.bit_length() - 2:
        raise ValueError(f"needs 0 < {what} <= {ctx.modulus.bit_length() - 2}, got {m}")
    return m


def log_first(ctx, opened, ta, tb, tab, ybig, nxt, d, out=None):
    """The first step, ONE launch after the scale's open: opened (2, count, limbs) or flat, the masked pair of [x v]; ta, tb, tab (1,
    count, limbs) its triple; ybig (count, limbs) = Y = beta [x != 0], kept by the scale step; nxt = (a, b) the next triple's factors.
    c = [x v], t = 4 c - 3 Y -> (masked, powers): masked rows t - a, t - b, the array to open for [t t]; powers (d, count, limbs) with
    row 0 = t and the other rows for log_level to fill.  out: a pair."""
    _check_degree(d)
    ta = ctx.elems(ta, what="ta")
    if ta.dim() != 3 or ta.shape[0] != 1:
        raise ValueError(f"ta: expected shape (1, count, {ctx.n_limbs}), got {tuple(ta.shape)}")
    count = ta.shape[1]
    tb, tab = (_planes(ctx, v, 1, count, w, exact=True)[0] for v, w in ((tb, "tb"), (tab, "tab")))
    opened = ctx.elems(opened, 2 * count, what="opened")
    ybig = ctx.elems(ybig, count, what="ybig")
    na, nb = _pair(nxt)
    na, nb = ctx.elems(na, count, what="nxt a"), ctx.elems(nb, count, what="nxt b")
    g0, g1 = _pair(out)
    o0, o1 = _planes_out(ctx, g0, 2, count, "out masked"), _planes_out(ctx, g1, d, count, "out powers")
    P = ctx.ptr
    ctx.check(ctx.lib.hb_fxlog_first(ctx.h, P(opened), P(ta), P(tb), P(tab), P(ybig), P(na), P(nb), P(o0), P(o1), count, ctx.stream()), "hb_fxlog_first")
    return o0.view(2, count, ctx.n_limbs), o1.view(d, count, ctx.n_limbs)


def log_level(ctx, level, d, opened, s, m, ta, tb, powers, out=None):
    """One level of the powers, ONE launch after the open of level `level`'s masked truncations, 1 <= level < ceil(log2 d): s, opened
    (n, count, limbs) (opened flat is fine), n the powers of the level: power half + 1 + q = (s_q - (opened_q mod 2^m)) / 2^m goes to row
    half + q of `powers` (d, count, limbs), IN PLACE, half = 2^(level-1); ta, tb (products of level + 1, count, limbs): -> masked (2
    products, count, limbs), rows 2q, 2q + 1 = t^(2 half) - ta[q], t^(q+1) - tb[q], the array to open."""
    _check_degree(d)
    if not 1 <= _int(level, "level") < _level_count(d):
        raise ValueError(f"needs 1 <= level < {_level_count(d)} for d = {d}, got {level}")
    _check_shift(ctx, m)
    done, nxt = len(_level_powers(level, d)), len(_level_powers(level + 1, d))
    s, count = _planes(ctx, s, done, None, "s", exact=True)
    opened = ctx.elems(opened, done * count, what="opened")
    ta, tb = (_planes(ctx, v, nxt, count, w, exact=True)[0] for v, w in ((ta, "ta"), (tb, "tb")))
    if not isinstance(powers, ctx.torch.Tensor) or not powers.is_contiguous():
        raise ValueError("powers: must be a contiguous tensor, it is updated in place")
    powers = ctx.elems(powers, d * count, what="powers")
    o = _planes_out(ctx, out, 2 * nxt, count)
    inv = _inv2m(ctx, m)
    P = ctx.ptr
    ctx.check(ctx.lib.hb_fxlog_level(ctx.h, level, d, P(opened), P(s), m, inv.ctypes.data, P(ta), P(tb), P(o), P(powers), count, ctx.stream()), "hb_fxlog_level")
    return o.view(2 * nxt, count, ctx.n_limbs)


def log_poly_mask(ctx, d, opened, s, m_in, powers, ybig, coef, bits, width, m_out, kappa=KAPPA, out=None):
    """The polynomial and its truncation mask, ONE launch after the open of the LAST level's masked truncations: s, opened (n, count,
    limbs) of that level finish its powers; the older powers are rows of `powers` (d, count, limbs), which is only read.  L = coef[0] ybig
    + sum_j coef[j] t^j with coef (d + 1, limbs) public; bits (width + kappa, count, limbs) -> (masked, s): trunc_mask(L) to open and L +
    r1, (1, count, limbs) each.  out: a pair."""
    _check_degree(d)
    _check_shift(ctx, m_in, "m_in")
    check_params(ctx.modulus, width, m_out, kappa)
    last = _level_count(d)
    done = len(_level_powers(last, d))
    s, count = _planes(ctx, s, done, None, "s", exact=True)
    opened = ctx.elems(opened, done * count, what="opened")
    powers, _ = _planes(ctx, powers, d, count, "powers", exact=True)
    ybig = ctx.elems(ybig, count, what="ybig")
    coef = ctx.elems(coef, d + 1, what="coef")
    bits, _ = _planes(ctx, bits, width + kappa, count, "bits")
    g0, g1 = _pair(out)
    o0, o1 = _planes_out(ctx, g0, 1, count, "out masked"), _planes_out(ctx, g1, 1, count, "out kept")
    inv = _inv2m(ctx, m_in)
    P = ctx.ptr
    ctx.check(ctx.lib.hb_fxlog_poly_mask(ctx.h, d, P(opened), P(s), m_in, inv.ctypes.data, P(powers), P(ybig), P(coef), P(bits), width, m_out, kappa, P(o0), P(o1), count,
                                         ctx.stream()), "hb_fxlog_poly_mask")
    return o0.view(1, count, ctx.n_limbs), o1.view(1, count, ctx.n_limbs)


def log_finish(ctx, opened, s, m, ipart, out=None):
    """The last step, ONE launch: (s - (opened mod 2^m)) / 2^m + ipart, (count, limbs); s (1, count, limbs) or flat"""
    _check_shift(ctx, m)
    ipart = ctx.elems(ipart, what="ipart")
    count = ipart.numel() // ctx.n_limbs
    s, opened = ctx.elems(s, count, what="s"), ctx.elems(opened, count, what="opened")
    o = _elems_out(ctx, out, count)
    inv = _inv2m(ctx, m)
    P = ctx.ptr
    ctx.check(ctx.lib.hb_fxlog_finish(ctx.h, P(opened), P(s), m, inv.ctypes.data, P(ipart), P(o), count, ctx.stream()), "hb_fxlog_finish")
    return o


# ---- protocols over an OpenCoalescer ---------------------------------------------------------------------------------------
async def log_base(co, x, bits, triples, f=F, k=K, kappa=KAPPA, base=2):
    """Shares of the fixed-point logarithm to the PUBLIC base `base` (an integer >= 2, or E), log_base(x / 2^f) 2^f up to log_error_bound(k,
    f, None, base) ulps, for shares of unsigned x with 0 < x < 2^(k-1) (a negative x is outside the contract).  log_opens opens for any
    count; log_planes bit planes and log_triples triples an element, in the order of log_layout.  x, bits and triples are left
    untouched.  ValueError before anything is opened.  x = 0 raises nothing and gives what log_model gives."""
    ctx = co.ctx
    lay = log_layout(k, f, kappa, None, base)
    d, width, levels = lay["degree"], lay["width"], lay["levels"]
    _check_norm(ctx, k, kappa)
    if d > MAX_DEGREE:
        raise ValueError(f"f = {f} needs a polynomial of degree {d}: at most {MAX_DEGREE}")
    if width > 256:
        raise ValueError(f"the truncations need {width} bits: at most 256")
    n, nb, m_out = k - 1, width + kappa, k - 1 + GUARD_BITS
    for m in (n, m_out):
        check_params(ctx.modulus, width, m, kappa)
    x = ctx.elems(x, what="x")
    count = x.numel() // ctx.n_limbs
    x = x.view(count, ctx.n_limbs)
    bits, _ = _planes(ctx, bits, lay["n_planes"], count, "bits")
    triples = _triples(ctx, triples, lay["n_triples"], count)
    rows = _Rows(bits, triples)
    weights, coef = weight_rows(ctx, k, f, base), coefficient_rows(ctx, k, f, base, d)

    y = await bit_decompose(co, x, rows.planes(k + kappa), rows.take(bit_triples(n)), k, n, kappa)
    await _prefix_or_in_place(co, y, rows)
    t = rows.take(1)
    masked, kept = sqrt_norm_mask(ctx, x, y, weights, t[0], t[1])          # kept rows: v, I, Y
    opened = await _open_rows(co, masked)
    trip = rows.take(1)
    masked, powers = log_first(ctx, opened, t[0], t[1], t[2], kept[2], (trip[0][0], trip[1][0]), d)
    for level in range(1, levels + 1):
        products = len(_level_powers(level, d))
        opened = await _open_rows(co, masked)
        masked, s = products_trunc(ctx, opened, trip[0], trip[1], trip[2], rows.planes(products * nb), width, n, kappa)
        opened = await _open_rows(co, masked)
        if level < levels:
            trip = rows.take(len(_level_powers(level + 1, d)))
            masked = log_level(ctx, level, d, opened, s, n, trip[0], trip[1], powers)
        else:
            masked, s = log_poly_mask(ctx, d, opened, s, n, powers, kept[2], coef, rows.planes(nb), width, m_out, kappa)
    opened = await _open_rows(co, masked)
    return log_finish(ctx, opened, s, m_out, kept[1])


async def log2(co, x, bits, triples, f=F, k=K, kappa=KAPPA):
    """Shares of log2(x / 2^f) 2^f: log_base with base 2, where the integer part is exact"""
    return await log_base(co, x, bits, triples, f, k, kappa, 2)


async def log(co, x, bits, triples, f=F, k=K, kappa=KAPPA):
    """Shares of the natural logarithm ln(x / 2^f) 2^f: log_base with base E; the opens and the preprocessing of log2 (the degree may
    differ by one: log_degree(k, f, E))"""
    return await log_base(co, x, bits, triples, f, k, kappa, E)

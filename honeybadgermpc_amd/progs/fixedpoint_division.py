"""
Division of shared fixed-point numbers by a SHARED divisor on the device (csrc/hb_div.hip): Catrina and Saxena's FPDiv / AppRcr / Norm
("Secure Computation With Fixed-Point Numbers", http://www.ifca.ai/pub/fc10/31_47.pdf) for signed k-bit values with f fractional
bits, on the (count, limbs) share arrays of progs/fixedpoint.py.  The reference stops at division by a public number
(FixedPoint.div, fixedpoint.py:277-280); the pin here is the mathematics: norm_model and div_model on Python ints, and the same steps
composed from share_arithmetic and fixedpoint.trunc_mask / trunc_pr_finish.

Inputs are shares of a and b, signed k-bit residues, with b != 0, |b| < 2^(k-1) and |a 2^f / b| < 2^(k-2); k / 2 <= f <= k - 2.  With
N = k - 1, alpha = 2^(2f), alpha' = int(2.9142 * 2^(k-1)) and W = div_width(k, f, theta) the width of every truncation:

    1 sign      (signed only) u = ltz(b), x = b - 2 [u b] = |b|                                     1 + carry_levels(k-1) opens, then 1
    2 bits      bit_decompose(x, k, k - 1): N planes, least significant first                       bit_opens(k-1) opens
    3 prefix OR y_i = OR_{j >= i} x_j in place over the bit planes: a Sklansky network with the wiring of
                bit_decomposition.prefix_nodes, network plane r = bit N - 1 - r; a node is y_j <- y_j + y_q - [y_j y_q]
                                                                                                    preor_levels(N) opens
    4 scale     v = sum_i 2^(N-1-i) (y_i - y_{i+1}) (no product) = 2^(N-1-top bit of x); c = [x v] in [2^(k-2), 2^(k-1)) and, signed,
                v' = v - 2 [u v]                                                                     1 open
    5 AppRcr    d = alpha' - 2 c, W = [d v'], w = trunc_pr(W, 2 (k - 1 - f)) ~ 2^(2f) / b            2 opens
    6 Goldschmidt   x0 = alpha - [b w], Y = [a w]; y = trunc_pr(Y, f); theta - 1 times Y = [y (alpha + x)], X = [x x] in one open of four
                rows and y, x = trunc_pr(., 2f) in one open of two; last Y = [y (alpha + x)], trunc_pr(Y, 2f)
                                                                                                    2 + 2 (theta - 1) + 2 opens

b = 0 raises nothing -- the divisor is secret --: every bit is 0, so v = 0, w = 0, Y = 0, and the result is 0, as div_model gives.

Error and widths (DESIGN.md section 3t has the derivation).  With E_i = x_i / alpha the residual and Q = a 2^f / b:
E_0 = 1 - b w / alpha, |E_0| <= eps0 = 0.0858 + 2^(1-k) + 2^(divisor_bits - 2f) -- the linear approximation of 1 / c on [1/2, 1), the
rounding of alpha', and the one-unit rounding of w against 2^(2f) / |b| > 2^(2f - divisor_bits) -- which is 0.586 for k = 2f, not the
paper's 2^-3.5; y_i = Q (1 - E_i) + eta_i with |eta_0| < 1, |eta_{i+1}| <= |eta_i| (1 + eps_i) + 1 + 2^(k-2-2f), eps_{i+1} = eps_i^2 +
2^(-2f); the result is off by at most 2^(k-2) eps_{theta-1}^2 + eta_{theta-1} (1 + eps_{theta-1}) + 1 ulps.  The products to truncate
stay below alpha (2^(k-2) + eta (1 + eps)) [Y], alpha^2 eps0^2 [X], 2^(f+k-2) (1 + eps0) [a w] and 2^(2k-2) [W]: div_width is the
signed width that holds them all, 2 k when k = 2f and more when f > k / 2.

Preprocessing is handed in as tensors, consumed in step order from row 0; div_layout names the row ranges.  `bits` is (div_planes,
count, limbs): ltz k + kappa (signed only), bit decomposition k + kappa, then W + kappa each for w, y0, (y, x) of every iteration and
the last y.  `triples = (p, q, pq)` is (div_triples, count, limbs) each: ltz 2 k - 3 and the sign product 1 (signed only),
bit_triples(k-1), preor_triples(k-1), the scale 2 (unsigned 1), W 1, (b w, a w) 2, (Y, X) 2 an iteration, the last Y 1.

Host functions:

    preor_levels(N) = ceil(log2 N), preor_nodes(N, level) -> [(j, q)] network planes, preor_level_triples(N, level), preor_triples(N)
    initial_residual_bound(k, f, divisor_bits), div_error_bound(k, f, theta, divisor_bits)     exact Fractions; ulps of 2^-f
    goldschmidt_iterations(k, f, divisor_bits)    the smallest theta with 2^(k-2) eps0^(2^theta) <= 1; the default theta
    div_width(k, f, theta), div_planes, div_triples, div_opens, div_layout; norm_planes, norm_triples, norm_opens for normalize
    norm_model(b, k) -> (c, v');  div_model(a, b, p, k, f, r1s, theta, signed) -> what div opens to for the dealt r1 of each of the
    2 theta + 1 truncations in step order (w, y0, then y, x of every iteration, the last y); r2 does not matter.

Tensor level, one launch each on torch's current stream, nothing synchronises:

    pair_mask(ctx, x, y, ta, tb)                        (x - ta, y - tb), (2, count, limbs): one product's array to open
    or_mask(ctx, y, level, ta, tb, from_top)            the level's array to open, (2 triples, count, limbs)
    or_combine(ctx, opened, y, level, ta, tb, tab, from_top)   IN PLACE -> y
    norm_mask(ctx, x, y, u, ta, tb)                     -> (masked, v): rows x - a1, v - b1 and, with u, u - a2, v - b2
    product_step(ctx, mode, opened, ta, tb, tab, ...)   products to truncation mask: SIGN, NORM, FIRST, TRUNC (csrc/hb_div.hip)
    trunc_step(ctx, mode, opened, s, m, ...)            truncation to product masks: T_RESULT, T_RECIP, T_GOLD

Protocol level, coroutines over an OpenCoalescer:

    async prefix_or(co, planes, triples, from_top)      preor_levels(N) opens, 2 launches a level (and one copy)
    async normalize(co, b, bits, triples, k, kappa, signed)   -> (c, v')
    async div(co, a, b, bits, triples, f, k, kappa, theta, signed), async reciprocal(co, b, ...)

div takes, signed, (3 + 2 carry_levels(k-1)) + 2 + (4 + 2 prefix_levels(k-1)) + 2 preor_levels(k-1) + 1 + (2 theta + 5) launches for any
count, unsigned (4 + 2 prefix_levels(k-1)) + 2 preor_levels(k-1) + 1 + (2 theta + 5): from the scale's open on, ONE launch between
consecutive opens.  Inputs and preprocessing are left untouched; ValueError before anything is opened.
"""
from fractions import Fraction
from functools import lru_cache

from .._capi import (HB_DIV_FIRST, HB_DIV_NORM, HB_DIV_SIGN, HB_DIV_T_GOLD, HB_DIV_T_RECIP, HB_DIV_T_RESULT, HB_DIV_TRUNC)
from .bit_decomposition import MAX_PLANES, bit_decompose, bit_opens, bit_triples, prefix_nodes
from .fixedpoint import F, K, KAPPA, _elems_out, _int, _inv2m, _pair, _planes, _planes_out, _triples, carry_levels, carry_triples, check_params, ltz

SIGN, NORM, FIRST, TRUNC = HB_DIV_SIGN, HB_DIV_NORM, HB_DIV_FIRST, HB_DIV_TRUNC
T_RESULT, T_RECIP, T_GOLD = HB_DIV_T_RESULT, HB_DIV_T_RECIP, HB_DIV_T_GOLD
APPROXIMATION_ERROR = Fraction(858, 10000)                       # max |1 - c (2.9142 - 2 c)| on [1/2, 1], attained at c = 1


# ---- host functions: the prefix OR network -----------------------------------------------------------------------------------
def _n(n_planes):
    if not 1 <= _int(n_planes, "n_planes") <= MAX_PLANES:
        raise ValueError(f"needs 1 <= n_planes <= {MAX_PLANES}, got {n_planes}")
    return n_planes


def preor_levels(n_planes):
    """levels of the prefix OR over n_planes planes: ceil(log2 n_planes), none for one plane"""
    return (_n(n_planes) - 1).bit_length()


def preor_nodes(n_planes, level):
    """-> [(j, q)] for node t = 0, 1, ...: network plane j takes y_j + y_q - y_j y_q; the wiring of bit_decomposition.prefix_nodes"""
    return [(j, q) for j, q, _ in prefix_nodes(_n(n_planes), level)]


def preor_level_triples(n_planes, level):
    """triples an element level `level` consumes: one a node, the planes j < n_planes with bit `level` set"""
    if not 0 <= _int(level, "level") < preor_levels(n_planes):
        raise ValueError(f"level must be in 0 .. {preor_levels(n_planes) - 1}, got {level}")
    return len(preor_nodes(n_planes, level))


def preor_triples(n_planes):
    return sum(preor_level_triples(n_planes, l) for l in range(preor_levels(n_planes)))


# ---- host functions: bounds ------------------------------------------------------------------------------------------------------
def _check_kf(k, f):
    k, f = _int(k, "k"), _int(f, "f")
    if not (k <= 2 * f and f <= k - 2):
        raise ValueError(f"needs k / 2 <= f <= k - 2, got k = {k}, f = {f}")
    if k - 1 > MAX_PLANES:
        raise ValueError(f"at most {MAX_PLANES} planes, got k - 1 = {k - 1}")


def _divisor_bits(k, divisor_bits):
    if divisor_bits is None:
        return k - 1
    if not 1 <= _int(divisor_bits, "divisor_bits") <= k - 1:
        raise ValueError(f"needs 1 <= divisor_bits <= k - 1, got {divisor_bits}")
    return divisor_bits


def _theta(k, f, theta, divisor_bits=None):
    if theta is None:
        return goldschmidt_iterations(k, f, divisor_bits)
    if _int(theta, "theta") < 1:
        raise ValueError(f"theta must be positive, got {theta}")
    return theta


def alpha_prime(k):
    """int(2.9142 * 2^(k-1)), in integers"""
    return (29142 << (k - 1)) // 10000


def initial_residual_bound(k, f, divisor_bits=None):
    """eps0 >= |1 - b w / 2^(2f)| for every 0 < |b| < 2^divisor_bits (default k - 1): the approximation error 0.0858 of 2.9142 - 2 c for
    1 / c on [1/2, 1), 2^(1-k) for the rounding of alpha', and 2^(divisor_bits - 2f) for the rounding of w (less than one unit)
    relative to 2^(2f) / |b|.  An exact Fraction."""
    _check_kf(k, f)
    return APPROXIMATION_ERROR + Fraction(1, 1 << (k - 1)) + Fraction(1 << _divisor_bits(k, divisor_bits), 1 << (2 * f))


def _schedule(k, f, theta, divisor_bits=None):
    """-> (eps, eta): eps[i] >= |x_i / alpha| and eta[i] >= |y_i - Q (1 - x_i / alpha)| for i < theta"""
    eps, eta = [initial_residual_bound(k, f, divisor_bits)], [Fraction(1)]
    qx, ulp = Fraction(1 << (k - 2), 1 << (2 * f)), Fraction(1, 1 << (2 * f))
    for _ in range(theta - 1):
        eta.append(eta[-1] * (1 + eps[-1]) + 1 + qx)
        eps.append(eps[-1] ** 2 + ulp)
    return eps, eta


def div_error_bound(k, f, theta, divisor_bits=None):
    """|result - a 2^f / b| in ulps of 2^-f, an exact Fraction: the accumulated rounding of the 2 theta + 1 truncations,
    eta_{theta-1} (1 + eps_{theta-1}) + 1, plus 2^(k-2) eps_{theta-1}^2, which is 2^(k-2) eps0^(2^theta) and what the roundings of x add to
    it.  For 0 < |b| < 2^divisor_bits (default k - 1) and |a 2^f / b| < 2^(k-2)."""
    _check_kf(k, f)
    eps, eta = _schedule(k, f, _theta(k, f, theta), divisor_bits)
    return eta[-1] * (1 + eps[-1]) + 1 + (1 << (k - 2)) * eps[-1] ** 2


@lru_cache(maxsize=None)
def goldschmidt_iterations(k, f, divisor_bits=None):
    """the smallest theta with 2^(k-2) eps0^(2^theta) <= 1 ulp for every divisor below 2^divisor_bits (default: every k-bit divisor)"""
    eps0 = initial_residual_bound(k, f, divisor_bits)
    theta, e = 1, eps0 ** 2
    while (1 << (k - 2)) * e > 1:
        theta, e = theta + 1, e * e
    return theta


def _ceil(q):
    return -((-q.numerator) // q.denominator)


@lru_cache(maxsize=None)
def div_width(k, f, theta=None):
    """the signed width of the truncations: max(2 k, what the products need) -- |W| < 2^(2k-2), |a w| <= 2^(f+k-2) (1 + eps0),
    |Y| <= alpha (2^(k-2) + eta (1 + eps)), X <= alpha^2 eps0^2 for operands in the documented range and every k-bit divisor"""
    _check_kf(k, f)
    eps, eta = _schedule(k, f, _theta(k, f, theta))
    alpha = 1 << (2 * f)
    bounds = [(alpha_prime(k) - (1 << (k - 1))) << (k - 2), _ceil((1 << (f + k - 2)) * (1 + eps[0])),
              alpha * ((1 << (k - 2)) + _ceil(max(h * (1 + e) for h, e in zip(eta, eps)))), _ceil(alpha * alpha * eps[0] ** 2)]
    return max(2 * k, max(bounds).bit_length() + 1)


# ---- host functions: counts ------------------------------------------------------------------------------------------------------
def _ranges(sizes):
    out, off = {}, 0
    for name, n in sizes:
        out[name] = (off, off + n)
        off += n
    return out, off


def _norm_sizes(k, kappa, signed):
    planes = ([("ltz", k + kappa)] if signed else []) + [("bit_decompose", k + kappa)]
    triples = ([("ltz", carry_triples(k - 1)), ("sign", 1)] if signed else []) + [("bit_decompose", bit_triples(k - 1)), ("prefix_or", preor_triples(k - 1)),
                                                                                 ("norm", 2 if signed else 1)]
    return planes, triples


def _norm_open_count(k, signed):
    return (1 + carry_levels(k - 1) + 1 if signed else 0) + bit_opens(k - 1) + preor_levels(k - 1) + 1


def div_layout(k=K, f=F, kappa=KAPPA, theta=None, signed=True):
    """-> {"theta", "width", "planes": {name: (start, stop)}, "triples": {name: (start, stop)}, "n_planes", "n_triples", "opens"}: the rows
    of `bits` and of the triple tensors each step consumes, in step order from row 0.  Planes: ltz (signed), bit_decompose, w, y0,
    iter<i>.y, iter<i>.x (i = 1 .. theta - 1), last.  Triples: ltz, sign (signed), bit_decompose, prefix_or, norm, w, first, iter<i>, last."""
    _check_kf(k, f)
    _int(kappa, "kappa")
    theta = _theta(k, f, theta)
    width = div_width(k, f, theta)
    planes, triples = _norm_sizes(k, kappa, bool(signed))
    planes += [("w", width + kappa), ("y0", width + kappa)]
    triples += [("w", 1), ("first", 2)]
    for i in range(1, theta):
        planes += [(f"iter{i}.y", width + kappa), (f"iter{i}.x", width + kappa)]
        triples.append((f"iter{i}", 2))
    planes.append(("last", width + kappa))
    triples.append(("last", 1))
    p_ranges, n_planes = _ranges(planes)
    t_ranges, n_triples = _ranges(triples)
    return {"theta": theta, "width": width, "planes": p_ranges, "triples": t_ranges, "n_planes": n_planes, "n_triples": n_triples,
            "opens": _norm_open_count(k, bool(signed)) + 2 + 2 + 2 * (theta - 1) + 2}


def div_planes(k=K, f=F, kappa=KAPPA, theta=None, signed=True):
    return div_layout(k, f, kappa, theta, signed)["n_planes"]


def div_triples(k=K, f=F, theta=None, signed=True):
    return div_layout(k, f, 0, theta, signed)["n_triples"]


def div_opens(k=K, f=F, theta=None, signed=True):
    return div_layout(k, f, 0, theta, signed)["opens"]


def norm_planes(k=K, kappa=KAPPA, signed=True):
    return _ranges(_norm_sizes(k, kappa, bool(signed))[0])[1]


def norm_triples(k=K, signed=True):
    return _ranges(_norm_sizes(k, 0, bool(signed))[1])[1]


def norm_opens(k=K, signed=True):
    return _norm_open_count(k, bool(signed))


# ---- host functions: models ------------------------------------------------------------------------------------------------------
def norm_model(b, k, signed=True):
    """(c, v') as Python ints for the signed k-bit integer b: v = 2^(k-2-top bit of |b|), c = |b| v in [2^(k-2), 2^(k-1)), v' = v with the
    sign of b (signed=False: b > 0 is the caller's promise and v' = v); b = 0 -> (0, 0)"""
    k, b = _int(k, "k"), _int(b, "b")
    if not -(1 << (k - 1)) < b < 1 << (k - 1):
        raise ValueError(f"|b| must be below 2^(k-1), got {b}")
    x = abs(b) if signed else b % (1 << (k - 1))                 # unsigned: the low k - 1 bits, as the bit decomposition gives them
    if x == 0:
        return 0, 0
    v = 1 << (k - 2 - (x.bit_length() - 1))
    return x * v, -v if signed and b < 0 else v


def _centered(x, p):
    x = int(x) % p
    return x - p if x > p // 2 else x


def _trunc(x, r1, p, width, m):
    """trunc_pr_model with r2 = 0 on a residue, its parameter checks left to the caller"""
    c2 = (x + (1 << (width - 1)) + r1) % p % (1 << m)
    return (x - c2 + r1) * pow(2, -m, p) % p


def _div_residues(a, b, p, k, f, r1s, theta, signed, width):
    c, v = norm_model(_centered(b, p), k, signed)
    alpha = 1 << (2 * f)
    inv = {m: pow(2, -m, p) for m in (2 * (k - 1 - f), f, 2 * f)}

    def tr(x, r1, m):
        return (x - (x + (1 << (width - 1)) + r1) % p % (1 << m) + r1) * inv[m] % p

    w = tr((alpha_prime(k) - 2 * c) * v % p, r1s[0], 2 * (k - 1 - f))
    x = (alpha - b * w) % p
    y = tr(a * w % p, r1s[1], f)
    at = 2
    for _ in range(theta - 1):
        y, x = tr(y * (alpha + x) % p, r1s[at], 2 * f), tr(x * x % p, r1s[at + 1], 2 * f)
        at += 2
    return tr(y * (alpha + x) % p, r1s[at], 2 * f)


def div_model(a, b, p, k=K, f=F, r1s=(), theta=None, signed=True):
    """What div's result opens to, a residue mod p: a, b residues (or signed ints) of signed k-bit values; r1s the dealt r1 of the
    2 theta + 1 truncations in step order: w [below 2^(2 (k-1-f))], y0 [below 2^f], then y, x of every iteration and the last y [below
    2^(2f)].  Python ints only; r2 does not matter (no masked value wraps for operands in the documented range)."""
    _check_kf(k, f)
    theta = _theta(k, f, theta)
    width = div_width(k, f, theta)
    check_params(p, k, k - 1, 0, full=True)
    for m in (2 * (k - 1 - f), f, 2 * f):
        check_params(p, width, m, 0)
    r1s = [_int(r, "r1") for r in r1s]
    limits = [2 * (k - 1 - f), f] + [2 * f] * (2 * theta - 1)
    if len(r1s) != len(limits) or any(not 0 <= r < 1 << m for r, m in zip(r1s, limits)):
        raise ValueError(f"r1s: expected {len(limits)} values below 2^m for m = {limits}")
    return _div_residues(int(a) % p, int(b) % p, p, k, f, r1s, theta, bool(signed), width)


# ---- tensor level ----------------------------------------------------------------------------------------------------------
def _or_args(ctx, y, level, in_place=False):
    if in_place and isinstance(y, ctx.torch.Tensor) and not y.is_contiguous():
        raise ValueError("y: must be contiguous (it is updated in place)")
    y = ctx.elems(y, what="y")
    if y.dim() != 3 or not 1 <= y.shape[0] <= MAX_PLANES:
        raise ValueError(f"y: expected shape (1 <= planes <= {MAX_PLANES}, count, {ctx.n_limbs}), got {tuple(y.shape)}")
    return y, y.shape[0], y.shape[1], preor_level_triples(y.shape[0], level)


def pair_mask(ctx, x, y, ta, tb, out=None):
    """(x - ta, y - tb) as ONE array to open, (2, count, limbs): the masked pair of the product [x y]"""
    x = ctx.elems(x, what="x")
    count = x.numel() // ctx.n_limbs
    y, ta, tb = (ctx.elems(v, count, what=w) for v, w in ((y, "y"), (ta, "ta"), (tb, "tb")))
    out = _planes_out(ctx, out, 2, count)
    ctx.check(ctx.lib.hb_div_pair_mask(ctx.h, ctx.ptr(x), ctx.ptr(y), ctx.ptr(ta), ctx.ptr(tb), ctx.ptr(out), count, ctx.stream()), "hb_div_pair_mask")
    return out.view(2, count, ctx.n_limbs)


def or_mask(ctx, y, level, ta, tb, from_top=True, out=None):
    """One level of the prefix OR before its open.  y (N, count, limbs); ta, tb (preor_level_triples(N, level), count, limbs).
    -> (2 triples, count, limbs): rows 2t, 2t + 1 = y_j - ta[t], y_q - tb[t] for node t = (j, q) of preor_nodes, network plane r being
    plane N - 1 - r of y (from_top) or plane r."""
    y, n, count, triples = _or_args(ctx, y, level)
    ta, _ = _planes(ctx, ta, triples, count, "ta", exact=True)
    tb, _ = _planes(ctx, tb, triples, count, "tb", exact=True)
    out = _planes_out(ctx, out, 2 * triples, count)
    ctx.check(ctx.lib.hb_div_or_mask(ctx.h, ctx.ptr(y), n, level, int(bool(from_top)), ctx.ptr(ta), ctx.ptr(tb), ctx.ptr(out), count, ctx.stream()), "hb_div_or_mask")
    return out.view(2 * triples, count, ctx.n_limbs)


def or_combine(ctx, opened, y, level, ta, tb, tab, from_top=True):
    """One level of the prefix OR after its open, IN PLACE: y_j <- y_j + y_q - [y_j y_q] at the level's nodes; every other plane is left
    untouched.  y must be contiguous.  -> y"""
    y, n, count, triples = _or_args(ctx, y, level, in_place=True)
    opened = ctx.elems(opened, 2 * triples * count, what="opened")
    ta, tb, tab = (_planes(ctx, v, triples, count, w, exact=True)[0] for v, w in ((ta, "ta"), (tb, "tb"), (tab, "tab")))
    ctx.check(ctx.lib.hb_div_or_combine(ctx.h, ctx.ptr(opened), ctx.ptr(y), n, level, int(bool(from_top)), ctx.ptr(ta), ctx.ptr(tb), ctx.ptr(tab), count, ctx.stream()),
              "hb_div_or_combine")
    return y


def norm_mask(ctx, x, y, u, ta, tb, out=None, v_out=None):
    """The scale step before its open.  x (count, limbs); y (N, count, limbs) the prefix OR from the top of the bits of x; u the sign
    bit or None (unsigned); ta, tb (2, count, limbs), unsigned (1, count, limbs).  -> (masked, v): v = sum_i 2^(N-1-i) (y_i - y_{i+1}),
    masked rows x - ta[0], v - tb[0] and, with u, u - ta[1], v - tb[1]: ONE array to open."""
    x = ctx.elems(x, what="x")
    count = x.numel() // ctx.n_limbs
    y = ctx.elems(y, what="y")
    if y.dim() != 3 or not 1 <= y.shape[0] <= MAX_PLANES or y.shape[1] != count:
        raise ValueError(f"y: expected shape (1 <= planes <= {MAX_PLANES}, {count}, {ctx.n_limbs}), got {tuple(y.shape)}")
    products = 1 if u is None else 2
    if u is not None:
        u = ctx.elems(u, count, what="u")
    ta, _ = _planes(ctx, ta, products, count, "ta", exact=True)
    tb, _ = _planes(ctx, tb, products, count, "tb", exact=True)
    out, v = _planes_out(ctx, out, 2 * products, count), _elems_out(ctx, v_out, count, "v_out")
    ctx.check(ctx.lib.hb_div_norm_mask(ctx.h, ctx.ptr(x), ctx.ptr(y), y.shape[0], None if u is None else ctx.ptr(u), ctx.ptr(ta), ctx.ptr(tb), ctx.ptr(out), ctx.ptr(v),
                                       count, ctx.stream()), "hb_div_norm_mask")
    return out.view(2 * products, count, ctx.n_limbs), v


def product_step(ctx, mode, opened, ta, tb, tab, aux=None, cst=None, nxt=None, bits=None, width=None, m=None, kappa=KAPPA, out=None):
    """Products to what the next open needs, ONE launch: the Beaver combine of the products whose masked pairs were just opened
    (opened (2 products, count, limbs) or flat; ta, tb, tab (products, count, limbs)), the step's affine map, and

        SIGN   [u b], aux = b                       -> x = b - 2 [u b], (count, limbs)
        NORM   [x v], [u v] (one product: unsigned), aux = v: c = [x v], v' = v - 2 [u v] (unsigned: v).  With nxt = (a, b), the next
               triple's factors, and cst = alpha' -> (alpha' - 2 c - a, v' - b), (2, count, limbs), the array to open; else -> (c, v')
        FIRST  [b w], [a w], cst = alpha = 2^(2f), bits (width + kappa, count, limbs) -> (masked, kept): masked (1, count, limbs) =
               trunc_mask([a w]) to open, kept (2, count, limbs) = [a w] + r1, alpha - [b w]
        TRUNC  one or two products, bits (products (width + kappa), count, limbs) -> (masked, s), (products, count, limbs) each:
               trunc_mask of every product and product + r1

    out: one tensor (SIGN, NORM) or a pair; arrays of their own."""
    if mode not in (SIGN, NORM, FIRST, TRUNC) or isinstance(mode, bool):
        raise ValueError(f"mode must be SIGN, NORM, FIRST or TRUNC, got {mode!r}")
    ta = ctx.elems(ta, what="ta")
    if ta.dim() != 3 or ta.shape[0] not in ((1,) if mode == SIGN else (2,) if mode == FIRST else (1, 2)):
        raise ValueError(f"ta: expected shape (products, count, {ctx.n_limbs}) with a product count the mode takes, got {tuple(ta.shape)}")
    products, count = ta.shape[0], ta.shape[1]
    tb, tab = (_planes(ctx, v, products, count, w, exact=True)[0] for v, w in ((tb, "tb"), (tab, "tab")))
    opened = ctx.elems(opened, 2 * products * count, what="opened")
    aux_t = ctx.elems(aux, count, what="aux") if mode in (SIGN, NORM) else None
    na = nb = bits_t = cst_h = None
    if mode == NORM and nxt is not None:
        na, nb = _pair(nxt)
        na, nb = ctx.elems(na, count, what="nxt a"), ctx.elems(nb, count, what="nxt b")
    if mode == FIRST or na is not None:
        cst_h = ctx.host_elems([_int(cst, "cst") % ctx.modulus])
    sets = 1 if mode == FIRST else products if mode == TRUNC else 0
    if sets:
        check_params(ctx.modulus, width, m, kappa)
        bits_t, _ = _planes(ctx, bits, sets * (width + kappa), count, "bits")
    else:
        width, m, kappa = 0, 0, 0
    if mode in (SIGN, NORM):
        o0 = _elems_out(ctx, out, count) if mode == SIGN else _planes_out(ctx, out, 2, count)
        o1 = None
    else:
        g0, g1 = _pair(out)
        o0, o1 = _planes_out(ctx, g0, sets, count, "out masked"), _planes_out(ctx, g1, 2 if mode == FIRST else sets, count, "out kept")
    P = ctx.ptr
    ctx.check(ctx.lib.hb_div_product_step(ctx.h, mode, products, P(opened), P(ta), P(tb), P(tab), None if aux_t is None else P(aux_t),
                                          None if cst_h is None else cst_h.ctypes.data, None if na is None else P(na), None if nb is None else P(nb),
                                          None if bits_t is None else P(bits_t), width, m, kappa, P(o0), None if o1 is None else P(o1), count, ctx.stream()),
              "hb_div_product_step")
    if mode == SIGN:
        return o0
    if mode == NORM:
        return o0.view(2, count, ctx.n_limbs)
    return o0.view(sets, count, ctx.n_limbs), o1.view(2 if mode == FIRST else sets, count, ctx.n_limbs)


def trunc_step(ctx, mode, opened, s, m, ta=None, tb=None, x=None, ext=None, alpha=None, out=None):
    """Truncation to what the next open needs, ONE launch: t_r = (s_r - (opened_r mod 2^m)) / 2^m for the one or two rows of s (rows,
    count, limbs) and opened (the masked values, opened; flat is fine), and

        T_RESULT  one row                                   -> t_0, (count, limbs)
        T_RECIP   one row, ext = (b, a), ta, tb (2, ...)    -> (b - ta[0], t_0 - tb[0], a - ta[1], t_0 - tb[1]): the pairs of [b w], [a w]
        T_GOLD    x = t_1 (two rows) or the kept x (one row), alpha = 2^(2f), ta, tb (1 or 2, ...)
                                                            -> (t_0 - ta[0], alpha + x - tb[0]) and, with two triples, (x - ta[1], x - tb[1])

    -> (2 products, count, limbs), the array to open."""
    if mode not in (T_RESULT, T_RECIP, T_GOLD) or isinstance(mode, bool):
        raise ValueError(f"mode must be T_RESULT, T_RECIP or T_GOLD, got {mode!r}")
    if not 0 < _int(m, "m") <= ctx.modulus.bit_length() - 2:
        raise ValueError(f"needs 0 < m <= {ctx.modulus.bit_length() - 2}, got {m}")
    s = ctx.elems(s, what="s")
    if s.dim() != 3 or s.shape[0] not in ((1, 2) if mode == T_GOLD else (1,)):
        raise ValueError(f"s: expected shape (rows, count, {ctx.n_limbs}) with a row count the mode takes, got {tuple(s.shape)}")
    rows, count = s.shape[0], s.shape[1]
    opened = ctx.elems(opened, rows * count, what="opened")
    products, x_t, e0, e1, alpha_h = 0, None, None, None, None
    if mode != T_RESULT:
        ta = ctx.elems(ta, what="ta")
        if ta.dim() != 3 or ta.shape[1] != count or ta.shape[0] not in ((2,) if mode == T_RECIP else (1, 2)):
            raise ValueError(f"ta: expected shape (products, {count}, {ctx.n_limbs}) with a product count the mode takes, got {tuple(ta.shape)}")
        products = ta.shape[0]
        tb, _ = _planes(ctx, tb, products, count, "tb", exact=True)
    if mode == T_RECIP:
        e0, e1 = _pair(ext)
        e0, e1 = ctx.elems(e0, count, what="ext b"), ctx.elems(e1, count, what="ext a")
    if mode == T_GOLD:
        alpha_h = ctx.host_elems([_int(alpha, "alpha") % ctx.modulus])
        if rows == 1:
            x_t = ctx.elems(x, count, what="x")
    o = _planes_out(ctx, out, 2 * products, count) if products else _elems_out(ctx, out, count)
    inv = _inv2m(ctx, m)
    P = ctx.ptr
    ctx.check(ctx.lib.hb_div_trunc_step(ctx.h, mode, rows, products, P(opened), P(s), m, inv.ctypes.data, None if alpha_h is None else alpha_h.ctypes.data,
                                        None if x_t is None else P(x_t), None if e0 is None else P(e0), None if e1 is None else P(e1), P(ta) if products else None,
                                        P(tb) if products else None, P(o), count, ctx.stream()), "hb_div_trunc_step")
    return o.view(2 * products, count, ctx.n_limbs) if products else o


# ---- protocols over an OpenCoalescer ---------------------------------------------------------------------------------------
class _Rows:
    """the preprocessing, handed out in step order"""

    def __init__(self, bits, triples):
        self.bits, self.triples, self.plane, self.row = bits, triples, 0, 0

    def planes(self, n):
        self.plane += n
        return self.bits[self.plane - n:self.plane]

    def take(self, n):
        self.row += n
        return tuple(v[self.row - n:self.row] for v in self.triples)


async def _open_rows(co, masked):
    return await co.open_share_array(masked.view(masked.shape[0] * masked.shape[1], co.ctx.n_limbs))


async def _prefix_or_in_place(co, y, rows, from_top=True):
    ctx = co.ctx
    n = y.shape[0]
    for level in range(preor_levels(n)):
        a, b, ab = rows.take(preor_level_triples(n, level))
        opened = await _open_rows(co, or_mask(ctx, y, level, a, b, from_top))
        or_combine(ctx, opened, y, level, a, b, ab, from_top)
    return y


async def prefix_or(co, planes, triples, from_top=True):
    """Shares of the prefix OR of 1 .. 256 planes of bit shares, (N, count, limbs): plane i of the result is OR_{j >= i} (from_top) or
    OR_{j <= i}.  New planes; preor_levels(N) opens, preor_triples(N) rows of triples.  ValueError before anything is opened."""
    ctx = co.ctx
    planes = ctx.elems(planes, what="planes")
    if planes.dim() != 3 or not 1 <= planes.shape[0] <= MAX_PLANES:
        raise ValueError(f"planes: expected shape (1 <= planes <= {MAX_PLANES}, count, {ctx.n_limbs}), got {tuple(planes.shape)}")
    triples = _triples(ctx, triples, preor_triples(planes.shape[0]), planes.shape[1])
    return await _prefix_or_in_place(co, planes.clone(), _Rows(None, triples), from_top)


def _check_norm(ctx, k, kappa):
    _int(k, "k")
    if k - 1 > MAX_PLANES:
        raise ValueError(f"at most {MAX_PLANES} planes, got k - 1 = {k - 1}")
    check_params(ctx.modulus, k, k - 1, kappa, full=True)


async def _normalize(co, b, rows, k, kappa, signed):
    """steps 1 to 4 up to the scale's open -> (x, u, v, the scale's triples, its array opened)"""
    ctx = co.ctx
    u, x = None, b
    if signed:
        u = await ltz(co, b, rows.planes(k + kappa), rows.take(carry_triples(k - 1)), k, kappa)
        a1, b1, ab1 = rows.take(1)
        opened = await _open_rows(co, pair_mask(ctx, u, b, a1, b1))
        x = product_step(ctx, SIGN, opened, a1, b1, ab1, aux=b)
    y = await bit_decompose(co, x, rows.planes(k + kappa), rows.take(bit_triples(k - 1)), k, k - 1, kappa)
    await _prefix_or_in_place(co, y, rows)
    t = rows.take(2 if signed else 1)
    masked, v = norm_mask(ctx, x, y, u, t[0], t[1])
    return v, t, await _open_rows(co, masked)


async def normalize(co, b, bits, triples, k=K, kappa=KAPPA, signed=True):
    """-> (c, v'): shares of v' = +-2^(k-2-top bit of |b|), the sign that of b, and of c = b v' = |b| |v'| in [2^(k-2), 2^(k-1)) (Catrina and
    Saxena's Norm).  signed=False: the caller promises 0 < b, the sign step is skipped.  norm_opens(k, signed) opens, norm_planes
    bit planes and norm_triples triples an element.  b = 0 gives (0, 0)."""
    ctx = co.ctx
    signed = bool(signed)
    _check_norm(ctx, k, kappa)
    b = ctx.elems(b, what="b")
    count = b.numel() // ctx.n_limbs
    bits, _ = _planes(ctx, bits, norm_planes(k, kappa, signed), count, "bits")
    triples = _triples(ctx, triples, norm_triples(k, signed), count)
    v, t, opened = await _normalize(co, b.view(count, ctx.n_limbs), _Rows(bits, triples), k, kappa, signed)
    out = product_step(ctx, NORM, opened, t[0], t[1], t[2], aux=v)
    return out[0], out[1]


async def div(co, a, b, bits, triples, f=F, k=K, kappa=KAPPA, theta=None, signed=True):
    """Shares of the fixed-point quotient a / b, int(a 2^f / b) up to div_error_bound(k, f, theta) ulps, for shares of signed k-bit a
    and b with b != 0 and |a 2^f / b| < 2^(k-2) (signed=False: the caller promises 0 < b).  theta Goldschmidt iterations, default
    goldschmidt_iterations(k, f).  div_opens opens for any count; div_planes bit planes and div_triples triples an element, in
    the order of div_layout; (3 + 2 carry_levels(k-1)) + 2 [signed only] + (4 + 2 prefix_levels(k-1)) + 2 preor_levels(k-1) + 1 +
    (2 theta + 5) launches.  a, b, bits and triples are left untouched.  ValueError before anything is opened.  b = 0 raises nothing
    (the divisor is secret) and gives 0, as div_model does."""
    ctx = co.ctx
    signed = bool(signed)
    lay = div_layout(k, f, kappa, theta, signed)
    theta, width = lay["theta"], lay["width"]
    _check_norm(ctx, k, kappa)
    if width > 256:
        raise ValueError(f"the truncations need {width} bits: at most 256")
    shift = 2 * (k - 1 - f)
    for m in (shift, f, 2 * f):
        check_params(ctx.modulus, width, m, kappa)
    a = ctx.elems(a, what="a")
    count = a.numel() // ctx.n_limbs
    a, b = a.view(count, ctx.n_limbs), ctx.elems(b, count, what="b").view(count, ctx.n_limbs)
    bits, _ = _planes(ctx, bits, lay["n_planes"], count, "bits")
    triples = _triples(ctx, triples, lay["n_triples"], count)
    rows = _Rows(bits, triples)
    alpha, nb = 1 << (2 * f), width + kappa

    v, t, opened = await _normalize(co, b, rows, k, kappa, signed)
    tw = rows.take(1)
    opened = await _open_rows(co, product_step(ctx, NORM, opened, t[0], t[1], t[2], aux=v, cst=alpha_prime(k), nxt=(tw[0][0], tw[1][0])))
    masked, s = product_step(ctx, TRUNC, opened, tw[0], tw[1], tw[2], bits=rows.planes(nb), width=width, m=shift, kappa=kappa)
    opened = await _open_rows(co, masked)
    t = rows.take(2)
    opened = await _open_rows(co, trunc_step(ctx, T_RECIP, opened, s, shift, t[0], t[1], ext=(b, a)))
    masked, kept = product_step(ctx, FIRST, opened, t[0], t[1], t[2], cst=alpha, bits=rows.planes(nb), width=width, m=f, kappa=kappa)
    opened = await _open_rows(co, masked)
    s, x, m = kept[:1], kept[1], f
    for _ in range(theta - 1):
        t = rows.take(2)
        opened = await _open_rows(co, trunc_step(ctx, T_GOLD, opened, s, m, t[0], t[1], x=x, alpha=alpha))
        masked, s = product_step(ctx, TRUNC, opened, t[0], t[1], t[2], bits=rows.planes(2 * nb), width=width, m=2 * f, kappa=kappa)
        opened = await _open_rows(co, masked)
        x, m = None, 2 * f
    t = rows.take(1)
    opened = await _open_rows(co, trunc_step(ctx, T_GOLD, opened, s, m, t[0], t[1], x=x, alpha=alpha))
    masked, s = product_step(ctx, TRUNC, opened, t[0], t[1], t[2], bits=rows.planes(nb), width=width, m=2 * f, kappa=kappa)
    opened = await _open_rows(co, masked)
    return trunc_step(ctx, T_RESULT, opened, s, 2 * f)


async def reciprocal(co, b, bits, triples, f=F, k=K, kappa=KAPPA, theta=None, signed=True):
    """Shares of 1 / b: div with the public constant 2^f for a, so 2^(2f-k+2) < |b|.  Everything else as div."""
    ctx = co.ctx
    _check_kf(k, f)
    b = ctx.elems(b, what="b")
    count = b.numel() // ctx.n_limbs
    one = ctx.to_device(ctx.host_elems([(1 << f) % ctx.modulus])).expand(count, ctx.n_limbs).contiguous()
    return await div(co, one, b, bits, triples, f, k, kappa, theta, signed)

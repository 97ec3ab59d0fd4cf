"""
Square root and inverse square root of shared fixed-point numbers on the device (csrc/hb_fxsqrt.hip and the division's steps of
csrc/hb_div.hip): a coupled Goldschmidt iteration on the normalised mantissa, for unsigned k-bit values with f fractional bits, on the
(count, limbs) share arrays of progs/fixedpoint.py.  The reference has no square root; the pin here is the mathematics: sqrt_model on
Python ints, and the same steps composed from share_arithmetic and fixedpoint.trunc_mask / trunc_pr_finish.

Inputs are shares of x with 0 <= x < 2^(k-1), value X = x / 2^f; k / 2 <= f <= k - 2.  A negative x is outside the contract (its low
k - 1 bits are what the bit decomposition sees).  For the inverse root the contract is 2^(3f/2) / sqrt(x) < 2^(k-2), stated the way div
states |a 2^f / b| < 2^(k-2): the result must be a k-bit value with a bit to spare.  With N = k - 1, beta = 2^N, sh = GUARD_BITS = 3,
j = Y0_SHIFT = 6, and W = sqrt_width(k, f, theta, what) the width of every truncation:

    1 bits      bit_decompose(x, k, N): N planes, least significant first                          bit_opens(N) opens
    2 prefix OR y_i = OR_{l >= i} x_l in place (fixedpoint_division's network, unchanged)          preor_levels(N) opens
    3 scale     z_i = y_i - y_{i+1} is one-hot at the top bit e of x.  v = sum 2^(N-1-i) z_i and T = sum W_i z_i, W_i PUBLIC
                (sqrt_weights): floor(2^(sh + (i+1-f)/2 + f)) for the root, floor(2^(sh - (i+1-f)/2 + f)) for the inverse; no product.
                c = [x v] in [beta / 2, beta), C = c / beta, and X = C 2^(e+1-f)                    1 open
    4 first     y0 = A' - 53 c ~ C^(-1/2) beta 2^j (A' = int(1.8015 beta 2^j)): no product.  G0 = [c y0], g0 = trunc_pr(G0, N), h0 = y0:
                g0 ~ sqrt(C) beta 2^j, h0 ~ beta 2^j / sqrt(C)                                     2 opens
    5 Goldschmidt, theta times: t = trunc_pr([g h], N), r = 3 beta - t, g = trunc_pr([g r], N + 1), h = trunc_pr([h r], N + 1); the first
                iteration's shifts are N + 2 j and N + 1 + j, which takes 2^j out; the last forms only what the result needs
                                                                                                    4 theta opens
    6 result    trunc_pr([g T], N + sh) ~ sqrt(X) 2^f and / or trunc_pr([h T'], N + sh) ~ 2^f / sqrt(X)   2 opens

Where this leaves the issue's sketch: g0 is kept at scale beta 2^j like h0 (the sketch had it at beta), so that the two truncations of
the first iteration's second open share one m, N + 1 + j, and go through ONE product_step(TRUNC): j bits of width for one launch.

x = 0 raises nothing -- the operand is secret --: every bit is 0, so v = T = 0, c = 0, g = 0 throughout, and both results are 0.

Error and widths (DESIGN.md section 3ab has the derivation).  Write g = beta s sqrt(C) (1 - dg), h = beta s (1 - dh) / sqrt(C) (s the
scale, 2^j before the first iteration and 1 after).  |dh_0| <= eps_y = initial_root_error, the error of the line A - B C against
C^(-1/2) on [1/2, 1) with the rounding of A'; dg_0 - dh_0 is the rounding of g0.  One iteration maps the common part d to 3 d^2 / 2 -
d^3 / 2 and KEEPS the difference dg - dh, to which every truncation adds at most (1 + sqrt 2) / beta: the coupled iteration does not
correct the ratio g / h, so the roundings add up, linearly in theta.  _schedule carries a >= |dg|, b >= |dh|, d >= |dg - dh|; the
results are off by at most a 2^((N+f)/2) + (1 + a) 2^-sh + 2 (against floor(sqrt(x 2^f))) and b 2^(k-2) + sqrt 2 (1 + b) 2^-sh + 1 ulps.

Preprocessing is handed in as tensors, consumed in step order from row 0; sqrt_layout names the row ranges.  `bits` is (sqrt_planes,
count, limbs): bit decomposition k + kappa, then W + kappa for every truncation in step order: g0, then t, g, h of every iteration (the
last: t and what the result needs), then the result(s), the root's first.  `triples = (p, q, pq)` is (sqrt_triples, count, limbs)
each: bit_triples(N), preor_triples(N), the scale 1, G0 1, every iteration 1 + 2 (the last: 1 + 1 or 2), the result 1 or 2.

Host functions:

    sqrt_iterations(k, f)            the smallest theta with 2^(k-2) d_theta <= 1, d the common part alone; the default theta
    initial_root_error(k, f)         eps_y, an exact Fraction
    sqrt_error_bound(k, f, theta, what), sqrt_width(k, f, theta, what)    exact; ulps of 2^-f; BOTH -> a pair
    sqrt_layout, sqrt_planes, sqrt_triples, sqrt_opens; sqrt_weights(k, f, what); a_prime(k)
    sqrt_model(x, p, k, f, r1s, theta, what) -> what the protocol opens to for the dealt r1 of every truncation in step order

Tensor level, one launch each on torch's current stream, nothing synchronises:

    sqrt_norm_mask(ctx, x, y, weights, ta, tb)     -> (masked, kept): masked rows x - ta, v - tb; kept rows v, T[, T']
    sqrt_first(ctx, opened, ta, tb, tab, nxt, k)   -> (masked, h): c = [x v], y0; masked rows c - nxt a, y0 - nxt b; h = y0
    sqrt_trunc_step(ctx, mode, opened, s, m, ta, tb, kept, which, cst)    truncation to product masks: GH, R, OUT
    (products to truncation masks is fixedpoint_division.product_step(TRUNC), the last step trunc_step(T_RESULT))

Protocol level, coroutines over an OpenCoalescer: sqrt, rsqrt, sqrt_rsqrt.  From the scale's open on, ONE launch between consecutive
opens (BOTH: two launches after the last open, one a result).  Inputs and preprocessing are left untouched; ValueError before anything
is opened.
"""
from fractions import Fraction
from functools import lru_cache
from math import isqrt

from .._capi import HB_FXSQRT_GH, HB_FXSQRT_OUT, HB_FXSQRT_R
from .bit_decomposition import MAX_PLANES, bit_decompose, bit_opens, bit_triples
from .fixedpoint import F, K, KAPPA, _elems_out, _int, _inv2m, _pair, _planes, _planes_out, _triples, check_params
from .fixedpoint_division import (T_RESULT, TRUNC, _ceil, _check_kf, _check_norm, _open_rows, _prefix_or_in_place, _ranges, _Rows, norm_model, preor_levels, preor_triples,
                                  product_step, trunc_step)

GH, R, OUT = HB_FXSQRT_GH, HB_FXSQRT_R, HB_FXSQRT_OUT
SQRT, RSQRT, BOTH = 1, 2, 3                                       # bit 0: the root (g), bit 1: the inverse root (h)
GUARD_BITS = 3                                                   # sh: the weights carry the result's bits and these
Y0_SHIFT, Y0_SLOPE = 6, 53                                       # y0 = A - (53 / 64) C
_PREC = 96
SQRT2_UP = Fraction(isqrt(2 << (2 * _PREC)) + 1, 1 << _PREC)     # just above sqrt(2)


def _icbrt(n):
    lo, hi = 0, 1 << (n.bit_length() // 3 + 2)
    while lo + 1 < hi:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if mid ** 3 <= n else (lo, mid)
    return lo


# just below (2 B)^(1/3), B = 53 / 64: the line's slope meets that of C^(-1/2) where C^(-3/2) = 2 B, and there C^(-1/2) + B C = 3/2 (2 B)^(1/3)
_CBRT_2B_DOWN = Fraction(_icbrt((2 * Y0_SLOPE << (3 * _PREC)) >> Y0_SHIFT), 1 << _PREC)


# ---- host functions: bounds ------------------------------------------------------------------------------------------------------
def _what(what):
    if what not in (SQRT, RSQRT, BOTH) or isinstance(what, bool):
        raise ValueError(f"what must be SQRT, RSQRT or BOTH, got {what!r}")
    return what


def _theta(k, f, theta):
    if theta is None:
        return sqrt_iterations(k, f)
    if _int(theta, "theta") < 1:
        raise ValueError(f"theta must be positive, got {theta}")
    return theta


def a_prime(k):
    """int(1.8015 * 2^(k-1+Y0_SHIFT)), in integers: the line's constant at the scale of y0"""
    return (18015 << (k - 1 + Y0_SHIFT)) // 10000


def initial_root_error(k, f):
    """eps_y >= |C^(-1/2) - (A - B C)| on [1/2, 1) with A = a_prime(k) / 2^(k-1+Y0_SHIFT), B = 53 / 64, an exact Fraction: the error is
    convex in C, so it is largest at an end -- sqrt 2 + B / 2 - A at 1/2, 1 + B - A towards 1 -- or, negated, where the slopes meet,
    A - 3/2 (2 B)^(1/3); the irrational two are bounded by rationals 2^-96 away."""
    _check_kf(k, f)
    A, B = Fraction(a_prime(k), 1 << (k - 1 + Y0_SHIFT)), Fraction(Y0_SLOPE, 1 << Y0_SHIFT)
    return max(SQRT2_UP + B / 2 - A, 1 + B - A, A - Fraction(3, 2) * _CBRT_2B_DOWN)


def _schedule(k, f, theta):
    """-> (a, b, d): a[i] >= |dg|, b[i] >= |dh|, d[i] >= |dg - dh| after i iterations, i = 0 .. theta"""
    beta = 1 << (k - 1)
    eg, eh, et = SQRT2_UP / beta, Fraction(1, beta), Fraction(1, 2 * beta)      # one truncation of g, of h, of t (halved in r / 2 beta)
    e0 = initial_root_error(k, f)
    a, b, d = [e0 + eg / (1 << Y0_SHIFT)], [e0], [eg / (1 << Y0_SHIFT)]
    for _ in range(theta):
        x, y, z = a[-1], b[-1], d[-1]
        a.append(z / 2 + x * x / 2 + x * y + x * x * y / 2 + et * (1 + x) + eg)
        b.append(z / 2 + y * y / 2 + x * y + x * y * y / 2 + et * (1 + y) + eh)
        d.append(z * (1 + (x + y) / 2 + x * y / 2 + et) + eg + eh)
    return a, b, d


@lru_cache(maxsize=None)
def sqrt_iterations(k, f):
    """the smallest theta with 2^(k-2) d_theta <= 1 ulp, d_0 = eps_y, d_{i+1} = 3 d_i^2 / 2 + d_i^3 / 2: the iteration without its roundings"""
    d, theta = initial_root_error(k, f), 0
    while (1 << (k - 2)) * d > 1:
        d, theta = 3 * d * d / 2 + d ** 3 / 2, theta + 1
    return max(theta, 1)


def _root_max(k, f):
    """>= sqrt(x 2^f) for x < 2^(k-1)"""
    e = k - 1 + f
    return Fraction(1 << (e // 2)) * (SQRT2_UP if e & 1 else 1)


def sqrt_error_bound(k, f, theta=None, what=SQRT):
    """ulps of 2^-f, exact Fractions.  SQRT: |result - floor(sqrt(x 2^f))| for 0 <= x < 2^(k-1): a_theta sqrt(2^(k-1+f)) for the
    iteration, (1 + a_theta) 2^-sh for the floor in the weight, 1 for the last truncation and 1 for the floor compared against.  RSQRT:
    |result - 2^(3f/2) / sqrt(x)| for x with 2^(3f/2) / sqrt(x) < 2^(k-2): b_theta 2^(k-2) + sqrt 2 (1 + b_theta) 2^-sh + 1.  BOTH: the pair."""
    _check_kf(k, f)
    a, b, _ = _schedule(k, f, _theta(k, f, theta))
    root = a[-1] * _root_max(k, f) + (1 + a[-1]) / (1 << GUARD_BITS) + 2
    inverse = b[-1] * (1 << (k - 2)) + SQRT2_UP * (1 + b[-1]) / (1 << GUARD_BITS) + 1
    return {SQRT: root, RSQRT: inverse, BOTH: (root, inverse)}[_what(what)]


def sqrt_weights(k, f, what=SQRT):
    """the PUBLIC weights of the scale step, W_i for i = 0 .. k - 2 (the top bit at i): floor(2^(sh + (i+1-f)/2 + f)) = isqrt(2^(2 sh + i +
    1 + f)) for the root, floor(2^(sh - (i+1-f)/2 + f)) = isqrt(2^(2 sh + 3 f - i - 1)) for the inverse; BOTH -> the pair of lists"""
    _check_kf(k, f)
    root = [isqrt(1 << (2 * GUARD_BITS + i + 1 + f)) for i in range(k - 1)]
    inverse = [isqrt(1 << (2 * GUARD_BITS + 3 * f - i - 1)) for i in range(k - 1)]
    return {SQRT: root, RSQRT: inverse, BOTH: (root, inverse)}[_what(what)]


@lru_cache(maxsize=None)
def sqrt_width(k, f, theta=None, what=SQRT):
    """the signed width of the truncations: what the products need, at least 2 k -- G0 = c y0 < beta (A' - 53 beta / 2), g h <= (beta s)^2
    (1 + a) (1 + b), g r and h r with r <= beta (3 - (1 - a) (1 - b)) + 1, h <= sqrt 2 beta s (1 + b), and g T, h T' at the largest weight"""
    _check_kf(k, f)
    what = _what(what)
    theta = _theta(k, f, theta)
    a, b, _ = _schedule(k, f, theta)
    beta = 1 << (k - 1)
    bounds = [beta * (a_prime(k) - Y0_SLOPE * (beta >> 1))]
    for i in range(theta):
        s = beta << Y0_SHIFT if i == 0 else beta
        r = beta * (3 - (1 - a[i]) * (1 - b[i])) + 1
        bounds += [_ceil(s * s * (1 + a[i]) * (1 + b[i])), _ceil(s * SQRT2_UP * (1 + b[i]) * r)]
    if what & SQRT:
        bounds.append(_ceil(beta * (1 + a[-1]) * max(sqrt_weights(k, f, SQRT))))
    if what & RSQRT:
        bounds.append(_ceil(beta * SQRT2_UP * (1 + b[-1]) * max(sqrt_weights(k, f, RSQRT))))
    return max(2 * k, max(bounds).bit_length() + 1)


# ---- host functions: counts ------------------------------------------------------------------------------------------------------
def _results(what):
    return 2 if what == BOTH else 1


def sqrt_shifts(k, theta, what=SQRT):
    """m of every truncation in step order: g0; t, g, h of every iteration (the last: t and what the result needs); the result(s)"""
    n, res = k - 1, _results(_what(what))
    out = [n]
    for i in range(theta):
        j = Y0_SHIFT if i == 0 else 0
        out += [n + 2 * j] + [n + 1 + j] * (2 if i < theta - 1 else res)
    return out + [n + GUARD_BITS] * res


def sqrt_layout(k=K, f=F, kappa=KAPPA, theta=None, what=SQRT):
    """-> {"theta", "width", "planes": {name: (start, stop)}, "triples": {name: (start, stop)}, "n_planes", "n_triples", "opens"}: the rows
    of `bits` and of the triple tensors each step consumes, in step order from row 0.  Planes: bit_decompose, g0, iter<i>.t, iter<i>.gh
    (i = 1 .. theta; two truncations, the last iteration one for SQRT or RSQRT), result.  Triples: bit_decompose, prefix_or, norm, g0,
    iter<i>.t, iter<i>.gh, result."""
    _check_kf(k, f)
    _int(kappa, "kappa")
    what = _what(what)
    theta = _theta(k, f, theta)
    width, res, n = sqrt_width(k, f, theta, what), _results(what), k - 1
    nb = width + kappa
    planes = [("bit_decompose", k + kappa), ("g0", nb)]
    triples = [("bit_decompose", bit_triples(n)), ("prefix_or", preor_triples(n)), ("norm", 1), ("g0", 1)]
    for i in range(1, theta + 1):
        pr = 2 if i < theta else res
        planes += [(f"iter{i}.t", nb), (f"iter{i}.gh", pr * nb)]
        triples += [(f"iter{i}.t", 1), (f"iter{i}.gh", pr)]
    planes.append(("result", res * nb))
    triples.append(("result", res))
    p_ranges, n_planes = _ranges(planes)
    t_ranges, n_triples = _ranges(triples)
    return {"theta": theta, "width": width, "planes": p_ranges, "triples": t_ranges, "n_planes": n_planes, "n_triples": n_triples,
            "opens": bit_opens(n) + preor_levels(n) + 1 + 2 + 4 * theta + 2}


def sqrt_planes(k=K, f=F, kappa=KAPPA, theta=None, what=SQRT):
    return sqrt_layout(k, f, kappa, theta, what)["n_planes"]


def sqrt_triples(k=K, f=F, theta=None, what=SQRT):
    return sqrt_layout(k, f, 0, theta, what)["n_triples"]


def sqrt_opens(k=K, f=F, theta=None, what=SQRT):
    return sqrt_layout(k, f, 0, theta, what)["opens"]


# ---- host functions: the model ---------------------------------------------------------------------------------------------------
def _sqrt_residues(x, p, k, f, r1s, theta, what, width):
    n = k - 1
    beta = 1 << n
    c, _ = norm_model(x, k, signed=False)
    top = (x % beta).bit_length() - 1
    r1s, shifts = iter(r1s), iter(sqrt_shifts(k, theta, what))

    def tr(v):
        m, r1 = next(shifts), next(r1s)
        return (v - (v + (1 << (width - 1)) + r1) % p % (1 << m) + r1) * pow(2, -m, p) % p

    h = (a_prime(k) - Y0_SLOPE * c) % p
    g = tr(c * h % p)
    for i in range(theta):
        r = (3 * beta - tr(g * h % p)) % p
        last = i == theta - 1
        g, h = (tr(g * r % p) if not last or what & SQRT else g), (tr(h * r % p) if not last or what & RSQRT else h)
    out = []
    if what & SQRT:
        out.append(tr(g * (sqrt_weights(k, f, SQRT)[top] if top >= 0 else 0) % p))
    if what & RSQRT:
        out.append(tr(h * (sqrt_weights(k, f, RSQRT)[top] if top >= 0 else 0) % p))
    return tuple(out) if what == BOTH else out[0]


def sqrt_model(x, p, k=K, f=F, r1s=(), theta=None, what=SQRT):
    """What the protocol's result opens to, a residue mod p (BOTH: the pair, the root first): x a residue of an unsigned value below
    2^(k-1); r1s the dealt r1 of every truncation in step order, below 2^m for m of sqrt_shifts(k, theta, what).  Python ints only; r2
    does not matter (no masked value wraps for operands in the documented range)."""
    _check_kf(k, f)
    what = _what(what)
    theta = _theta(k, f, theta)
    width = sqrt_width(k, f, theta, what)
    check_params(p, k, k - 1, 0, full=True)
    limits = sqrt_shifts(k, theta, what)
    for m in set(limits):
        check_params(p, width, m, 0)
    r1s = [_int(r, "r1") for r in r1s]
    if len(r1s) != len(limits) or any(not 0 <= r < 1 << m for r, m in zip(r1s, limits)):
        raise ValueError(f"r1s: expected {len(limits)} values below 2^m for m = {limits}")
    x = int(x) % p
    if x >> (k - 1):
        raise ValueError(f"x must be below 2^(k-1), got {x}")
    return _sqrt_residues(x, p, k, f, r1s, theta, what, width)


# ---- tensor level ----------------------------------------------------------------------------------------------------------
def weight_rows(ctx, k, f, what=SQRT):
    """the scale step's public constants on the device, (sets, k - 1, limbs): D_i = W_i - W_{i-1} mod p, so that sum_i D_i y_i = sum_i W_i
    (y_i - y_{i+1})"""
    sets = sqrt_weights(k, f, what)
    sets = sets if what == BOTH else (sets,)
    flat = [(w - (ws[i - 1] if i else 0)) % ctx.modulus for ws in sets for i, w in enumerate(ws)]
    return ctx.to_device(ctx.host_elems(flat)).view(len(sets), k - 1, ctx.n_limbs)


def sqrt_norm_mask(ctx, x, y, weights, ta, tb, out=None, kept_out=None):
    """The scale step before its open.  x (count, limbs); y (N, count, limbs) the prefix OR from the top of the bits of x; weights (sets,
    N, limbs) from weight_rows; ta, tb (1, count, limbs).  -> (masked, kept): kept rows v = sum_i 2^(N-1-i) (y_i - y_{i+1}) and T_s =
    sum_i weights[s][i] y_i, (1 + sets, count, limbs); masked rows x - ta, v - tb: ONE array to open."""
    x = ctx.elems(x, what="x")
    count = x.numel() // ctx.n_limbs
    y = ctx.elems(y, what="y")
    if y.dim() != 3 or not 1 <= y.shape[0] <= MAX_PLANES or y.shape[1] != count:
        raise ValueError(f"y: expected shape (1 <= planes <= {MAX_PLANES}, {count}, {ctx.n_limbs}), got {tuple(y.shape)}")
    weights = ctx.elems(weights, what="weights")
    if weights.dim() != 3 or weights.shape[0] not in (1, 2) or weights.shape[1] != y.shape[0]:
        raise ValueError(f"weights: expected shape (1 or 2, {y.shape[0]}, {ctx.n_limbs}), got {tuple(weights.shape)}")
    sets = weights.shape[0]
    ta, _ = _planes(ctx, ta, 1, count, "ta", exact=True)
    tb, _ = _planes(ctx, tb, 1, count, "tb", exact=True)
    out, kept = _planes_out(ctx, out, 2, count), _planes_out(ctx, kept_out, 1 + sets, count, "kept_out")
    ctx.check(ctx.lib.hb_fxsqrt_norm_mask(ctx.h, ctx.ptr(x), ctx.ptr(y), y.shape[0], ctx.ptr(weights), sets, ctx.ptr(ta), ctx.ptr(tb), ctx.ptr(out), ctx.ptr(kept), count,
                                          ctx.stream()), "hb_fxsqrt_norm_mask")
    return out.view(2, count, ctx.n_limbs), kept.view(1 + sets, count, ctx.n_limbs)


def sqrt_first(ctx, opened, ta, tb, tab, nxt, k, out=None):
    """The first approximation, ONE launch after the scale's open: opened (2, count, limbs) or flat, the masked pair of [x v]; ta, tb,
    tab (1, count, limbs) its triple; nxt = (a, b) the next triple's factors.  c = [x v], y0 = a_prime(k) - 53 c -> (masked, h): masked
    rows c - a, y0 - b, the array to open for G0 = [c y0]; h = y0, (count, limbs).  out: a pair."""
    if not 2 <= _int(k, "k") <= MAX_PLANES + 1:
        raise ValueError(f"needs 2 <= k <= {MAX_PLANES + 1}, got {k}")
    if a_prime(k) >= ctx.modulus:
        raise ValueError(f"k = {k}: the constant of the first approximation does not fit below the modulus")
    ta = ctx.elems(ta, what="ta")
    if ta.dim() != 3 or ta.shape[0] != 1:
        raise ValueError(f"ta: expected shape (1, count, {ctx.n_limbs}), got {tuple(ta.shape)}")
    count = ta.shape[1]
    tb, tab = (_planes(ctx, v, 1, count, w, exact=True)[0] for v, w in ((tb, "tb"), (tab, "tab")))
    opened = ctx.elems(opened, 2 * count, what="opened")
    na, nb = _pair(nxt)
    na, nb = ctx.elems(na, count, what="nxt a"), ctx.elems(nb, count, what="nxt b")
    g0, g1 = _pair(out)
    o0, o1 = _planes_out(ctx, g0, 2, count, "out masked"), _elems_out(ctx, g1, count, "out h")
    cst = ctx.host_elems([a_prime(k), Y0_SLOPE % ctx.modulus])
    P = ctx.ptr
    ctx.check(ctx.lib.hb_fxsqrt_first(ctx.h, P(opened), P(ta), P(tb), P(tab), cst[0:1].ctypes.data, cst[1:2].ctypes.data, P(na), P(nb), P(o0), P(o1), count, ctx.stream()),
              "hb_fxsqrt_first")
    return o0.view(2, count, ctx.n_limbs), o1


def sqrt_trunc_step(ctx, mode, opened, s, m, ta, tb, kept=None, which=BOTH, cst=None, out=None):
    """Truncation to what the next open needs, ONE launch: t_r = (s_r - (opened_r mod 2^m)) / 2^m for the one or two rows of s (rows,
    count, limbs) and opened (the masked values, opened; flat is fine), and

        GH    g = t_0, h = t_1 (two rows) or kept (one row; (count, limbs))   -> (masked, (g, h)): masked (2, count, limbs) = g - ta[0], h - tb[0]
        R     one row, kept = (g, h) (2, count, limbs), cst = 3 beta: r = cst - t_0; which = SQRT: (g - ta[0], r - tb[0]); RSQRT: (h - ta[0],
              r - tb[0]); BOTH: both pairs, g's first, ta, tb (2, ...)               -> (2 products, count, limbs)
        OUT   one row (which = SQRT or RSQRT) or two (BOTH), kept = the kept weights (rows, count, limbs): rows 2q, 2q + 1 = t_q - ta[q],
              kept[q] - tb[q]                                                      -> (2 rows, count, limbs)

    the array to open.  out: GH a pair (masked, kept), else one tensor; arrays of their own."""
    if mode not in (GH, R, OUT) or isinstance(mode, bool):
        raise ValueError(f"mode must be GH, R or OUT, got {mode!r}")
    which = BOTH if mode == GH else _what(which)
    if not 0 < _int(m, "m") <= ctx.modulus.bit_length() - 2:
        raise ValueError(f"needs 0 < m <= {ctx.modulus.bit_length() - 2}, got {m}")
    s = ctx.elems(s, what="s")
    want = (1, 2) if mode == GH else (1,) if mode == R else (_results(which),)
    if s.dim() != 3 or s.shape[0] not in want:
        raise ValueError(f"s: expected shape (rows, count, {ctx.n_limbs}) with a row count the mode takes, got {tuple(s.shape)}")
    rows, count = s.shape[0], s.shape[1]
    opened = ctx.elems(opened, rows * count, what="opened")
    products = 1 if mode == GH else _results(which) if mode == R else rows
    ta, _ = _planes(ctx, ta, products, count, "ta", exact=True)
    tb, _ = _planes(ctx, tb, products, count, "tb", exact=True)
    kin = (1 if rows == 1 else 0) if mode == GH else 2 if mode == R else rows
    kept_t = ctx.elems(kept, kin * count, what="kept") if kin else None
    cst_h = ctx.host_elems([_int(cst, "cst") % ctx.modulus]) if mode == R else None
    if mode == GH:
        g0, g1 = _pair(out)
        o0, o1 = _planes_out(ctx, g0, 2, count, "out masked"), _planes_out(ctx, g1, 2, count, "out kept")
    else:
        o0, o1 = _planes_out(ctx, out, 2 * products, count), None
    inv = _inv2m(ctx, m)
    P = ctx.ptr
    ctx.check(ctx.lib.hb_fxsqrt_trunc_step(ctx.h, mode, rows, which, P(opened), P(s), m, inv.ctypes.data, None if cst_h is None else cst_h.ctypes.data,
                                           None if kept_t is None else P(kept_t), P(ta), P(tb), P(o0), None if o1 is None else P(o1), count, ctx.stream()),
              "hb_fxsqrt_trunc_step")
    if mode == GH:
        return o0.view(2, count, ctx.n_limbs), o1.view(2, count, ctx.n_limbs)
    return o0.view(2 * products, count, ctx.n_limbs)


# ---- protocols over an OpenCoalescer ---------------------------------------------------------------------------------------
async def _roots(co, x, bits, triples, f, k, kappa, theta, what):
    ctx = co.ctx
    lay = sqrt_layout(k, f, kappa, theta, what)
    theta, width = lay["theta"], lay["width"]
    _check_norm(ctx, k, kappa)
    if width > 256:
        raise ValueError(f"the truncations need {width} bits: at most 256")
    shifts = sqrt_shifts(k, theta, what)
    for m in set(shifts):
        check_params(ctx.modulus, width, m, kappa)
    x = ctx.elems(x, what="x")
    count = x.numel() // ctx.n_limbs
    x = x.view(count, ctx.n_limbs)
    bits, _ = _planes(ctx, bits, lay["n_planes"], count, "bits")
    triples = _triples(ctx, triples, lay["n_triples"], count)
    rows = _Rows(bits, triples)
    n, nb, res, beta = k - 1, width + kappa, _results(what), 1 << (k - 1)
    weights = weight_rows(ctx, k, f, what)
    shifts = iter(shifts)

    async def truncate(opened, t, products):
        """the products whose pairs were opened -> their truncations' masks opened, product + r1 kept, and m"""
        m = next(shifts)
        for _ in range(products - 1):
            next(shifts)
        masked, s = product_step(ctx, TRUNC, opened, t[0], t[1], t[2], bits=rows.planes(products * nb), width=width, m=m, kappa=kappa)
        return await _open_rows(co, masked), s, m

    y = await bit_decompose(co, x, rows.planes(k + kappa), rows.take(bit_triples(n)), k, n, kappa)
    await _prefix_or_in_place(co, y, rows)
    t = rows.take(1)
    masked, kept = sqrt_norm_mask(ctx, x, y, weights, t[0], t[1])
    opened = await _open_rows(co, masked)
    tw = kept[1:]
    t2 = rows.take(1)
    masked, h = sqrt_first(ctx, opened, t[0], t[1], t[2], (t2[0][0], t2[1][0]), k)
    opened, s, m = await truncate(await _open_rows(co, masked), t2, 1)
    gh = h
    for i in range(theta):
        t = rows.take(1)
        masked, gh = sqrt_trunc_step(ctx, GH, opened, s, m, t[0], t[1], kept=gh if s.shape[0] == 1 else None)
        opened, s, m = await truncate(await _open_rows(co, masked), t, 1)
        which = BOTH if i < theta - 1 else what
        t = rows.take(_results(which))
        masked = sqrt_trunc_step(ctx, R, opened, s, m, t[0], t[1], kept=gh, which=which, cst=3 * beta)
        opened, s, m = await truncate(await _open_rows(co, masked), t, _results(which))
    t = rows.take(res)
    masked = sqrt_trunc_step(ctx, OUT, opened, s, m, t[0], t[1], kept=tw, which=what)
    opened, s, m = await truncate(await _open_rows(co, masked), t, res)
    opened = opened.view(res, count, ctx.n_limbs)
    return tuple(trunc_step(ctx, T_RESULT, opened[q], s[q:q + 1], m) for q in range(res))


async def sqrt(co, x, bits, triples, f=F, k=K, kappa=KAPPA, theta=None):
    """Shares of the fixed-point square root, floor(sqrt(x 2^f)) up to sqrt_error_bound(k, f, theta, SQRT) ulps, for shares of unsigned x
    with 0 <= x < 2^(k-1) (a negative x is outside the contract).  theta Goldschmidt iterations, default sqrt_iterations(k, f).
    sqrt_opens opens for any count; sqrt_planes bit planes and sqrt_triples triples an element, in the order of sqrt_layout.  x, bits
    and triples are left untouched.  ValueError before anything is opened.  x = 0 gives 0, as sqrt_model does."""
    return (await _roots(co, x, bits, triples, f, k, kappa, theta, SQRT))[0]


async def rsqrt(co, x, bits, triples, f=F, k=K, kappa=KAPPA, theta=None):
    """Shares of the inverse square root, 2^(3f/2) / sqrt(x) up to sqrt_error_bound(k, f, theta, RSQRT) ulps, for shares of unsigned x
    below 2^(k-1) with 2^(3f/2) / sqrt(x) < 2^(k-2).  Everything else as sqrt; x = 0 raises nothing (the operand is secret) and gives 0."""
    return (await _roots(co, x, bits, triples, f, k, kappa, theta, RSQRT))[0]


async def sqrt_rsqrt(co, x, bits, triples, f=F, k=K, kappa=KAPPA, theta=None):
    """-> (root, inverse) from ONE chain: the opens of either, one more truncation in the last iteration and in the result"""
    return await _roots(co, x, bits, triples, f, k, kappa, theta, BOTH)

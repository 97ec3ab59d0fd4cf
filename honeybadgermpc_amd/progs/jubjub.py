"""
The Jubjub curve on the device (csrc/hb_jj.hip): the reference's progs/jubjub.py (SharedPoint, share_mul) and the point arithmetic of
elliptic_curve.py (Point.__mul__, the doubling chain), on the (count, limbs) int64 tensors the rest of the package speaks.  A batch of
points is a pair of such tensors `(xs, ys)`; the host model is honeybadgermpc_amd.elliptic_curve (Jubjub, Point, Ideal).

`curve` is a host Jubjub over the context's modulus (None: the default curve, BLS12-381 Fr only; a host Point brings its own).  It must
be complete (a a square, d a non-square): the kernels use the unified law and never meet a zero denominator on such a curve.

Cleartext, asynchronous on torch's current stream:

    scalar_mul(ctx, ns, point, curve=None, out=None)     ns[i] * point[i] in ONE launch -> (xs, ys).  ns: an int (any sign) or a tensor of
                                                         1 or `count` canonical residues; point: a host Point or a tensor pair of 1 or
                                                         `count` points.  n = 0 gives (0, 1), the group's neutral element.
    double_table(ctx, point, K, curve=None)              -> (xs, ys), each (K, B, limbs): row j holds 2^j * point[i].  Four launches: the
                                                         projective rows, one batched inversion, two products.

The addition of m pairs of SHARED points (SharedPoint.add, progs/jubjub.py:87-113; curves with a = -1, as the reference's law reads):

    x3 = (x1 y2 + y1 x2) / (1 + d x1 x2 y1 y2)           y3 = (y1 y2 + x1 x2) / (1 - d x1 x2 y1 y2)

Each numerator rides with the blinding of its denominator -- num / den = (num r) / (den r), and den r is what gets opened -- so an addition
is four opens and six launches, where the reference's line-by-line schedule takes five opens.  A pair consumes 9 Beaver triples and 2
random shares: `triples = (p, q, pq)`, each (9, m, limbs), `rs` (2, m, limbs).  Triple k of a pair multiplies
0 x1 x2, 1 y1 y2, 2 x1 y2, 3 y1 x2, 4 xp yp, 5 nx rx, 6 ny ry, 7 dx rx, 8 dy ry   (xp = x1 x2, yp = y1 y2, nx = x1 y2 + y1 x2, ny = yp + xp,
dx = 1 + d xp yp, dy = 1 - d xp yp).  The five stage functions are one call of the C ABI each and nothing synchronises:

    add_mask(ctx, P, Q, triples)                         -> A (8 m, limbs), to open
    add_stage1(ctx, a_open, triples, rs)                 -> B (6 m, limbs), to open
    add_stage2(ctx, b_open, triples, rs, curve=None)     -> (uv (2 m, limbs) kept, C (4 m, limbs) to open)
    add_stage3(ctx, c_open, triples)                     -> D (2 m, limbs), to open: the shares of sig_x, sig_y
    add_finish(ctx, d_open, uv, check=True)              -> (x3, y3); check=True reads the zero counter of the batched inversion back --
                                                         the one synchronisation -- and raises ZeroDivisionError("Cannot invert zero") if a
                                                         sig was zero (r = 0, probability 1 / p, or operands off the curve), as
                                                         invert_share_array does; check=False -> ((x3, y3), counter tensor)

Protocol level, coroutines over an OpenCoalescer (every party runs the same one, so the opens meet batch for batch); inputs are left untouched:

    async shared_add(co, P, Q, triples, rs, curve=None)             4 coalesced opens, 6 launches
    shared_neg(ctx, P)                                              local: (-xs, ys)
    async shared_sub(co, P, Q, triples, rs, curve=None)             shared_add(P, shared_neg(Q))
    async shared_double(co, P, triples, rs, curve=None)             shared_add(P, P): the unified law is complete, so doubling is an addition
    async shared_mul(co, P, n, triples, rs, curve=None)             n an int: double-and-add as SharedPoint.mul (:118-142); consumes
                                                                    shared_mul_pairs(n) additions of m pairs each, from the front of
                                                                    triples / rs ((9, pairs * m, limbs) and (2, pairs * m, limbs))
    async share_mul(co, bits, point, triples, rs, curve=None)       [x] * point from bit shares of x (share_mul, :258-294), batched: bits
                                                                    (K, B, limbs) least significant first, point a host Point for all or
                                                                    a tensor pair of B points.  4 ceil(log2 K) opens, (K - 1) B pairs.
"""
from .._capi import HB_JJ_POINT_BROADCAST, HB_JJ_SCALAR_BROADCAST  # noqa: F401  (the selftest's flags, re-exported for the tests)
from ..elliptic_curve import Ideal, Jubjub, Point
from ..share_arithmetic import _out, add, mul, neg, sub


def _curve(ctx, curve, point=None):
    if curve is None:
        curve = point.curve if isinstance(point, Point) else Jubjub()
    if not isinstance(curve, Jubjub):
        raise TypeError(f"curve: expected a Jubjub, got {type(curve).__name__}")
    if isinstance(point, Point) and point.curve != curve:
        raise ValueError("point: lies on another curve than `curve`")
    if curve.p != ctx.modulus:
        raise ValueError(f"curve: defined over {curve.p}, the context's modulus is {ctx.modulus}")
    if not curve.is_complete():
        raise ValueError("curve: the addition law is not complete (a must be a square and d a non-square)")
    return curve


def _shared_curve(ctx, curve):
    curve = _curve(ctx, curve)
    if curve.a != ctx.modulus - 1:
        raise ValueError("curve: the addition of shared points is the reference's law, which holds for a = -1")
    return curve


def _points(ctx, point, what="point", count=None):
    """a tensor pair -> (xs, ys, count)"""
    try:
        xs, ys = point
    except (TypeError, ValueError):
        raise TypeError(f"{what}: expected a Point or a pair of tensors (xs, ys)") from None
    xs = ctx.elems(xs, count, what=f"{what} xs")
    have = xs.numel() // ctx.n_limbs
    ys = ctx.elems(ys, have, what=f"{what} ys")
    return xs, ys, have


def _point_operand(ctx, point, curve):
    """-> (xs, ys, count, broadcast)"""
    if isinstance(point, Ideal):
        raise ValueError("point: the point at infinity has no tensor form")
    if isinstance(point, Point):
        return ctx.upload_ints([point.x]), ctx.upload_ints([point.y]), 1, 1
    xs, ys, have = _points(ctx, point)
    return xs, ys, have, 1 if have == 1 else 0


def _out_pair(ctx, out, count):
    if out is None:
        return ctx.empty(count), ctx.empty(count)
    try:
        ox, oy = out
    except (TypeError, ValueError):
        raise TypeError("out: expected a pair of tensors") from None
    ox, oy = _out(ctx, ox, None, count), _out(ctx, oy, None, count)
    if count and ox.data_ptr() == oy.data_ptr():
        raise ValueError("out: the two tensors must be distinct")
    return ox, oy


# ---- cleartext ---------------------------------------------------------------------------------------------------------
def scalar_mul(ctx, ns, point, curve=None, out=None):
    """ns[i] * point[i] -> (xs, ys) in one launch: extended coordinates in registers, one inversion an element at the end.
    A negative int negates the point, as Point.__mul__ does; 0 gives (0, 1) where the reference answers Ideal."""
    curve = _curve(ctx, curve, point)
    px, py, n_points, p_bcast = _point_operand(ctx, point, curve)
    negate = False
    if isinstance(ns, int) and not isinstance(ns, bool):
        negate = ns < 0
        if abs(ns) >= ctx.modulus:
            raise ValueError("ns: an int scalar must be below the modulus in absolute value (scalars are canonical residues)")
        n_dev, n_scalars, n_bcast = ctx.upload_ints([abs(ns)]), 1, 1
    else:
        n_dev = ctx.elems(ns, what="ns")
        n_scalars = n_dev.numel() // ctx.n_limbs
        n_bcast = 1 if n_scalars == 1 else 0
    count = max(n_scalars, n_points)
    if n_scalars not in (1, count) or n_points not in (1, count):
        raise ValueError(f"ns and point: {n_scalars} scalars against {n_points} points")
    if n_scalars == 0 or n_points == 0:
        count = 0
    if negate:
        px = neg(ctx, px)
    ox, oy = _out_pair(ctx, out, count)
    a, d = ctx.host_elems([curve.a]), ctx.host_elems([curve.d])
    ctx.check(ctx.lib.hb_jj_scalar_mul(ctx.h, ctx.ptr(n_dev), n_bcast, ctx.ptr(px), ctx.ptr(py), p_bcast, a.ctypes.data, d.ctypes.data, ctx.ptr(ox), ctx.ptr(oy),
                                       count, ctx.stream()), "hb_jj_scalar_mul")
    return ox, oy


def double_table(ctx, point, K, curve=None):
    """-> (xs, ys), each (K, B, limbs): row j is 2^j * point[i] (B = 1 for a host Point).  The rows come from the doubling body of
    scalar_mul in projective form and are made affine together: one batched inversion, not one an element and row."""
    if not isinstance(K, int) or isinstance(K, bool) or not 1 <= K < 1 << 31:
        raise ValueError(f"K must be an integer in [1, 2^31), got {K!r}")
    curve = _curve(ctx, curve, point)
    px, py, count, _ = _point_operand(ctx, point, curve)
    t = ctx.torch
    xs, ys, zs = (t.empty((K, count, ctx.n_limbs), dtype=t.int64, device=ctx.tdev) for _ in range(3))
    a = ctx.host_elems([curve.a])
    ctx.check(ctx.lib.hb_jj_double_table(ctx.h, ctx.ptr(px), ctx.ptr(py), a.ctypes.data, K, ctx.ptr(xs), ctx.ptr(ys), ctx.ptr(zs), count, None, ctx.stream()),
              "hb_jj_double_table")
    return xs, ys


# ---- the stages of a shared addition -------------------------------------------------------------------------------------
def _triples(ctx, triples, m, rows=9):
    """-> ((p, q, pq) tensors, the row stride in elements): (rows, m, limbs) tensors whose rows are contiguous -- a column slice
    [:, a:b] of a larger (rows, M, limbs) tensor is taken as it is, no copy"""
    t = ctx.torch
    try:
        p, q, pq = triples
    except (TypeError, ValueError):
        raise ValueError("triples: expected (p, q, pq)") from None
    for v, w in ((p, "triples p"), (q, "triples q"), (pq, "triples pq")):
        if not isinstance(v, t.Tensor):
            raise TypeError(f"{w}: expected a torch tensor, got {type(v).__name__}")
        if v.dtype != t.int64:
            raise TypeError(f"{w}: dtype must be int64, got {v.dtype}")
        if v.dim() != 3 or tuple(v.shape) != (rows, m, ctx.n_limbs):
            raise ValueError(f"{w}: expected a tensor of shape ({rows}, {m}, {ctx.n_limbs}), got {tuple(v.shape)}")
        if not v.is_cuda or v.device.index != ctx.device:
            raise ValueError(f"{w}: must live on cuda:{ctx.device}, is on {v.device}")
    def rows_contiguous(v):
        return v.stride(2) == 1 and v.stride(1) == ctx.n_limbs and v.stride(0) % ctx.n_limbs == 0 and v.stride(0) >= m * ctx.n_limbs

    if m and all(rows_contiguous(v) for v in (p, q, pq)) and len({v.stride(0) for v in (p, q, pq)}) == 1:
        return (p, q, pq), p.stride(0) // ctx.n_limbs
    return (p.contiguous(), q.contiguous(), pq.contiguous()), m


def _rs(ctx, rs):
    """-> (rx, ry, m) from the (2, m, limbs) random shares (a column slice of a larger tensor is taken as it is)"""
    t = ctx.torch
    if not isinstance(rs, t.Tensor):
        raise TypeError(f"rs: expected a torch tensor, got {type(rs).__name__}")
    if rs.dim() != 3 or rs.shape[0] != 2 or rs.shape[2] != ctx.n_limbs:
        raise ValueError(f"rs: expected a tensor of shape (2, m, {ctx.n_limbs}), got {tuple(rs.shape)}")
    m = int(rs.shape[1])
    return ctx.elems(rs[0], m, what="rs"), ctx.elems(rs[1], m, what="rs"), m


def _pairs(ctx, P, Q):
    x1, y1, m = _points(ctx, P, "P")
    x2, y2, _ = _points(ctx, Q, "Q", m)
    return x1, y1, x2, y2, m


def _opened(ctx, v, rows, m, what):
    return ctx.elems(v, rows * m, what=what)


def add_mask(ctx, P, Q, triples):
    """the first array a shared addition opens: the eight masked factors of x1 x2, y1 y2, x1 y2, y1 x2, rows of m"""
    x1, y1, x2, y2, m = _pairs(ctx, P, Q)
    (p, q, _), stride = _triples(ctx, triples, m)
    out = ctx.empty(8 * m)
    ctx.check(ctx.lib.hb_jj_add_mask(ctx.h, ctx.ptr(x1), ctx.ptr(y1), ctx.ptr(x2), ctx.ptr(y2), ctx.ptr(p), ctx.ptr(q), stride, ctx.ptr(out), m, ctx.stream()),
              "hb_jj_add_mask")
    return out


def add_stage1(ctx, a_open, triples, rs):
    rx, ry, m = _rs(ctx, rs)
    a_open = _opened(ctx, a_open, 8, m, "a_open")
    (p, q, pq), stride = _triples(ctx, triples, m)
    out = ctx.empty(6 * m)
    ctx.check(ctx.lib.hb_jj_add_stage1(ctx.h, ctx.ptr(a_open), ctx.ptr(p), ctx.ptr(q), ctx.ptr(pq), stride, ctx.ptr(rx), ctx.ptr(ry), ctx.ptr(out), m, ctx.stream()),
              "hb_jj_add_stage1")
    return out


def add_stage2(ctx, b_open, triples, rs, curve=None):
    curve = _shared_curve(ctx, curve)
    rx, ry, m = _rs(ctx, rs)
    b_open = _opened(ctx, b_open, 6, m, "b_open")
    (p, q, pq), stride = _triples(ctx, triples, m)
    uv, out = ctx.empty(2 * m), ctx.empty(4 * m)
    d = ctx.host_elems([curve.d])
    ctx.check(ctx.lib.hb_jj_add_stage2(ctx.h, ctx.ptr(b_open), ctx.ptr(p), ctx.ptr(q), ctx.ptr(pq), stride, ctx.ptr(rx), ctx.ptr(ry), d.ctypes.data, ctx.ptr(uv),
                                       ctx.ptr(out), m, ctx.stream()), "hb_jj_add_stage2")
    return uv, out


def add_stage3(ctx, c_open, triples):
    c_open = ctx.elems(c_open, what="c_open")
    count = c_open.numel() // ctx.n_limbs
    if count % 4:
        raise ValueError(f"c_open: expected 4 m elements, got {count}")
    m = count // 4
    (p, q, pq), stride = _triples(ctx, triples, m)
    out = ctx.empty(2 * m)
    ctx.check(ctx.lib.hb_jj_add_stage3(ctx.h, ctx.ptr(c_open), ctx.ptr(p), ctx.ptr(q), ctx.ptr(pq), stride, ctx.ptr(out), m, ctx.stream()), "hb_jj_add_stage3")
    return out


def add_finish(ctx, d_open, uv, check=True, out=None):
    d_open = ctx.elems(d_open, what="d_open")
    count = d_open.numel() // ctx.n_limbs
    if count % 2:
        raise ValueError(f"d_open: expected 2 m elements, got {count}")
    m = count // 2
    uv = ctx.elems(uv, 2 * m, what="uv")
    x3, y3 = _out_pair(ctx, out, m)
    inv = ctx.empty(2 * m)
    zeros = ctx.torch.zeros(1, dtype=ctx.torch.int32, device=ctx.tdev)
    ctx.check(ctx.lib.hb_jj_add_finish(ctx.h, ctx.ptr(d_open), ctx.ptr(uv), ctx.ptr(inv), ctx.ptr(x3), ctx.ptr(y3), m, ctx.ptr(zeros), ctx.stream()),
              "hb_jj_add_finish")
    if not check:
        return (x3, y3), zeros
    if int(zeros.item()):
        raise ZeroDivisionError("Cannot invert zero")
    return x3, y3


# ---- protocols over an OpenCoalescer ---------------------------------------------------------------------------------------
async def shared_add(co, P, Q, triples, rs, curve=None):
    """Shares of P[i] + Q[i] for m pairs of shared points: four coalesced opens and six launches.  Raises ZeroDivisionError on every
    party alike if an opened sig is zero (the sigs are public)."""
    ctx = co.ctx
    _shared_curve(ctx, curve)
    a_open = await co.open_share_array(add_mask(ctx, P, Q, triples))
    b_open = await co.open_share_array(add_stage1(ctx, a_open, triples, rs))
    uv, c = add_stage2(ctx, b_open, triples, rs, curve)
    c_open = await co.open_share_array(c)
    d_open = await co.open_share_array(add_stage3(ctx, c_open, triples))
    return add_finish(ctx, d_open, uv, check=True)


def shared_neg(ctx, P):
    """-P: (-xs, ys), local (SharedPoint.neg, :84-85)"""
    xs, ys, _ = _points(ctx, P, "P")
    return neg(ctx, xs), ys


async def shared_sub(co, P, Q, triples, rs, curve=None):
    return await shared_add(co, P, shared_neg(co.ctx, Q), triples, rs, curve)


async def shared_double(co, P, triples, rs, curve=None):
    return await shared_add(co, P, P, triples, rs, curve)


def shared_mul_pairs(n):
    """additions (of m pairs each) shared_mul(P, n) consumes: a doubling for every bit above the lowest, an addition for every set bit
    but the first"""
    if not isinstance(n, int) or isinstance(n, bool):
        raise TypeError("n: expected an int")
    n = abs(n)
    if n == 0:
        raise ValueError("n = 0: the point at infinity has no tensor form")
    return (n.bit_length() - 1) + (bin(n).count("1") - 1)


def _preprocessing(ctx, triples, rs, need, what):
    """-> (p, q, pq) after the checks both compositions make before they slice: three (9, >= need, limbs) tensors and rs (2, >= need, limbs)"""
    t = ctx.torch
    try:
        p, q, pq = triples
    except (TypeError, ValueError):
        raise ValueError("triples: expected (p, q, pq)") from None
    for v, w, rows in ((p, "triples p", 9), (q, "triples q", 9), (pq, "triples pq", 9), (rs, "rs", 2)):
        if not isinstance(v, t.Tensor):
            raise TypeError(f"{w}: expected a torch tensor, got {type(v).__name__}")
        if v.dim() != 3 or v.shape[0] != rows or v.shape[2] != ctx.n_limbs or v.shape[1] < need:
            raise ValueError(f"{w}: {what} take a tensor of shape ({rows}, >= {need}, {ctx.n_limbs}), got {tuple(v.shape)}")
    return p, q, pq


async def shared_mul(co, P, n, triples, rs, curve=None):
    """n * P for an int n by double-and-add, least significant bit first as SharedPoint.mul (:118-142).  A composition in Python of
    shared_add: the reference starts its product at a shared (0, 1) and doubles once more after the top bit; here the product starts
    at the first set bit's term and the last doubling is not made, so the opened result is the same and shared_mul_pairs(n)
    additions are consumed, addition j taking columns [j m, (j + 1) m) of `triples` / `rs`.  n < 0 negates P; n = 0 raises ValueError
    (the reference returns a SharedIdeal, which has no tensor form)."""
    ctx = co.ctx
    _shared_curve(ctx, curve)
    xs, ys, m = _points(ctx, P, "P")
    need = shared_mul_pairs(n)
    p, q, pq = _preprocessing(ctx, triples, rs, need * m, f"{need} additions of {m} pairs")
    current = (xs, ys) if n > 0 else shared_neg(ctx, (xs, ys))
    n = abs(n)
    used = 0

    def take():
        nonlocal used
        s = slice(used * m, (used + 1) * m)
        used += 1
        return (p[:, s], q[:, s], pq[:, s]), rs[:, s]

    product = None
    i = 1
    while i <= n:
        if n & i:
            product = current if product is None else await shared_add(co, product, current, *take(), curve)
        i <<= 1
        if i <= n:
            current = await shared_add(co, current, current, *take(), curve)
    return product


async def share_mul(co, bits, point, triples, rs, curve=None):
    """Shares of x[i] * point[i] from the bit shares of x (share_mul, progs/jubjub.py:258-294): term j of instance i is the shared point
    ([b] P2.x, [b] (P2.y - 1) + 1) with P2 = 2^j point[i] from double_table -- (0, 1) or P2 -- and the K terms are summed by a tree whose
    every level is ONE shared_add over all its pairs and all B instances: the first floor(rows / 2) rows pair with the next
    floor(rows / 2), contiguous slices, a leftover row is carried (the group is commutative: the sum is the reference's).
    4 ceil(log2 K) opens; (K - 1) B pairs of `triples` (9, >= (K - 1) B, limbs) / `rs` are consumed from the front, level by level.
    K = 1 returns the terms with no open.  A host Ideal raises ValueError."""
    ctx = co.ctx
    t = ctx.torch
    if isinstance(point, Ideal):
        raise ValueError("point: the point at infinity has no tensor form (the reference returns a SharedIdeal)")
    curve = _shared_curve(ctx, _curve(ctx, curve, point))
    if not isinstance(bits, t.Tensor) or bits.dim() != 3:
        raise ValueError("bits: expected a tensor of shape (K, B, limbs)")
    K, B = int(bits.shape[0]), int(bits.shape[1])
    if K < 1 or B < 1:
        raise ValueError("bits: expected at least one bit and one instance")
    bits = ctx.elems(bits, K * B, what="bits")
    tx, ty = double_table(ctx, point, K, curve)
    if tx.shape[1] == 1 and B > 1:
        tx, ty = tx.expand(K, B, ctx.n_limbs).contiguous(), ty.expand(K, B, ctx.n_limbs).contiguous()
    elif tx.shape[1] != B:
        raise ValueError(f"point: {tx.shape[1]} points against {B} instances")
    need = (K - 1) * B
    p, q, pq = _preprocessing(ctx, triples, rs, need, f"{K} bits of {B} instances")
    xs = mul(ctx, bits, tx).reshape(K, B, ctx.n_limbs)
    ys = add(ctx, mul(ctx, bits, sub(ctx, ty, 1, out=ty)), 1).reshape(K, B, ctx.n_limbs)
    rows, used = K, 0
    while rows > 1:
        h = rows // 2
        s = slice(used, used + h * B)
        used += h * B
        sx, sy = await shared_add(co, (xs[:h], ys[:h]), (xs[h:2 * h], ys[h:2 * h]), (p[:, s], q[:, s], pq[:, s]), rs[:, s], curve)
        sx, sy = sx.reshape(h, B, ctx.n_limbs), sy.reshape(h, B, ctx.n_limbs)
        if rows & 1:
            sx, sy = t.cat([sx, xs[2 * h:rows]]), t.cat([sy, ys[2 * h:rows]])
        xs, ys, rows = sx, sy, (rows + 1) // 2
    return xs.reshape(B, ctx.n_limbs), ys.reshape(B, ctx.n_limbs)

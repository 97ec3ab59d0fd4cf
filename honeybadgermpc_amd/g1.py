"""
BLS12-381 G1 on the device (csrc/hb_g1.hip): batches of points as tensors, over a Context whose modulus is the group order
R = Subgroup.BLS12_381 (the field every share lives in); any other context raises ValueError.  The host model is
honeybadgermpc_amd.bls12_381.G1, which writes the group multiplicatively as the reference does; the names here are additive.

A batch of points is ONE int64 tensor (count, 2, 6): x then y, six little-endian 64-bit words each, canonical residues below Q; the
identity is all zeros.  Scalars are the context's (count, 4) elements, read as plain 256-bit integers.

    upload(points, ctx=None) / download(tensor)          lists of host G1 <-> tensors (download synchronises: it copies to the host)
    scalar_mul(ctx, ks, points, out=None)                ks[i] * points[i] in one launch.  ks: an int (any sign, reduced mod R) or a
                                                         tensor of 1 or `count` scalars; points: a host G1 or a tensor of 1 or `count`
    add(ctx, P, Q, out=None), sub(...), neg(ctx, P)      element-wise; complete (identity, equal and opposite operands)
    on_curve(ctx, points) -> bool tensor                 the identity, or coordinates below Q and y^2 = x^3 + 4
    in_subgroup(ctx, points) -> bool tensor              R * P == identity, through scalar_mul's kernel.  NOTHING else checks this.
    FixedBase(ctx, base, window=8)                       owns the window table of one base (a host G1, not the identity)
    commit(ctx, tg, th, a, b, out=None)                  a[i] * g + b[i] * h from two FixedBase of one window width: 2 * 256 / window
                                                         mixed additions at most, no doubling
    eval_commitments(ctx, cs, i, out=None)               cs (B, t + 1, 2, 6), 0 <= i < 2^32 -> (B, 2, 6): sum_j i^j cs[b][j] by Horner
    verify(ctx, tg, th, cs, i, shares, witnesses)        -> (verdict (B,) int32: 1 accepted, 0 rejected; counter (1,) int32: rejected
                                                         items).  One fused launch; an item with a commitment off the curve is rejected.

Everything is asynchronous on torch's current stream and nothing synchronises, except download() and FixedBase() (the base's upload).
"""
import numpy as np

from .bls12_381 import G1, LIMBS, R

POINT_WORDS = 2 * LIMBS


def _ctx(ctx):
    if ctx.modulus != R or ctx.n_limbs != 4:
        raise ValueError(f"ctx: G1 works over the group order R = Subgroup.BLS12_381 in four limbs, the context's modulus is {ctx.modulus}")
    return ctx


def upload(points, ctx=None):
    """list of host G1 -> (count, 2, 6) tensor on the context's device (ctx=None: the context of R on torch's current device)"""
    if ctx is None:
        from ._capi import Context

        ctx = Context.get(R)
    _ctx(ctx)
    points = list(points)
    for p in points:
        if not isinstance(p, G1):
            raise TypeError(f"points: expected host G1 elements, got {type(p).__name__}")
    arr = np.array([p.to_limbs() for p in points], dtype=np.uint64).reshape(len(points), 2, LIMBS)
    return ctx.torch.from_numpy(arr.view(np.int64)).to(ctx.tdev)


def download(tensor):
    """(..., 2, 6) tensor -> flat list of host G1 (raises ValueError for a point off the curve, as G1 does).  Copies to the host."""
    import torch

    if not isinstance(tensor, torch.Tensor):
        raise TypeError(f"tensor: expected a torch tensor, got {type(tensor).__name__}")
    if tensor.dtype != torch.int64 or tensor.dim() < 2 or tuple(tensor.shape[-2:]) != (2, LIMBS):
        raise ValueError(f"tensor: expected an int64 tensor of shape (..., 2, {LIMBS}), got {tensor.dtype} {tuple(tensor.shape)}")
    arr = tensor.cpu().contiguous().numpy().view(np.uint64).reshape(-1, POINT_WORDS)
    return [G1.from_limbs(row.tolist()) for row in arr]


def _points(ctx, t, count=None, what="points"):
    torch = ctx.torch
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: expected a host G1 or a torch tensor, got {type(t).__name__}")
    if t.dtype != torch.int64:
        raise TypeError(f"{what}: dtype must be int64 (6 x u64 words a coordinate viewed as int64), got {t.dtype}")
    if t.dim() < 2 or tuple(t.shape[-2:]) != (2, LIMBS):
        raise ValueError(f"{what}: expected a tensor of shape (..., 2, {LIMBS}), got {tuple(t.shape)}")
    if not t.is_cuda or t.device.index != ctx.device:
        raise ValueError(f"{what}: must live on cuda:{ctx.device}, is on {t.device}")
    if count is not None and t.numel() != count * POINT_WORDS:
        raise ValueError(f"{what}: expected {count} points, got {t.numel() // POINT_WORDS}")
    return t if t.is_contiguous() else t.contiguous()


def _n(t):
    return t.numel() // POINT_WORDS


def _out(ctx, out, count):
    if out is None:
        return ctx.torch.empty((count, 2, LIMBS), dtype=ctx.torch.int64, device=ctx.tdev)
    # (_points hands back a contiguous COPY of a strided tensor: fine for an input, useless for an output)
    if isinstance(out, ctx.torch.Tensor) and not out.is_contiguous():
        raise ValueError("out: must be contiguous")
    return _points(ctx, out, count, what="out")


def _operand(ctx, points, what="points"):
    """-> (tensor, count)"""
    if isinstance(points, G1):
        return upload([points], ctx), 1
    t = _points(ctx, points, what=what)
    return t, _n(t)


def scalar_mul(ctx, ks, points, out=None):
    """ks[i] * points[i] -> (count, 2, 6) in one launch: Jacobian coordinates in registers, one inversion an element at the end.
    An int scalar is reduced mod R (a negative one negates); tensors of scalars are read as plain 256-bit integers."""
    _ctx(ctx)
    pts, n_points = _operand(ctx, points)
    if isinstance(ks, int) and not isinstance(ks, bool):
        k_dev, n_scalars = ctx.upload_ints([ks % R]), 1
    elif hasattr(ks, "__int__") and not isinstance(ks, ctx.torch.Tensor):
        k_dev, n_scalars = ctx.upload_ints([int(ks) % R]), 1
    else:
        k_dev = ctx.elems(ks, what="ks")
        n_scalars = k_dev.numel() // ctx.n_limbs
    count = max(n_scalars, n_points)
    if n_scalars not in (1, count) or n_points not in (1, count):
        raise ValueError(f"ks and points: {n_scalars} scalars against {n_points} points")
    if n_scalars == 0 or n_points == 0:
        count = 0
    out = _out(ctx, out, count)
    ctx.check(ctx.lib.hb_g1_scalar_mul(ctx.h, ctx.ptr(k_dev), 1 if n_scalars == 1 else 0, ctx.ptr(pts), 1 if n_points == 1 else 0, ctx.ptr(out), count,
                                       ctx.stream()), "hb_g1_scalar_mul")
    return out


def _add(ctx, P, Q, subtract, out):
    _ctx(ctx)
    p, n = _operand(ctx, P, "P")
    q, m = _operand(ctx, Q, "Q")
    if n != m:
        raise ValueError(f"P and Q: {n} points against {m}")
    out = _out(ctx, out, n)
    ctx.check(ctx.lib.hb_g1_add(ctx.h, ctx.ptr(p), ctx.ptr(q), subtract, ctx.ptr(out), n, ctx.stream()), "hb_g1_add")
    return out


def add(ctx, P, Q, out=None):
    """P[i] + Q[i]; complete: identity, equal and opposite operands give the right answer"""
    return _add(ctx, P, Q, 0, out)


def sub(ctx, P, Q, out=None):
    """P[i] - Q[i]"""
    return _add(ctx, P, Q, 1, out)


def neg(ctx, P, out=None):
    """-P[i], as identity - P[i] (the identity stays all zeros)"""
    _ctx(ctx)
    p, n = _operand(ctx, P, "P")
    return _add(ctx, ctx.torch.zeros_like(p), p, 1, out)


def on_curve(ctx, points):
    """-> bool tensor (count,): the identity, or both coordinates below Q and y^2 = x^3 + 4"""
    _ctx(ctx)
    p, n = _operand(ctx, points)
    flags = ctx.torch.empty((n,), dtype=ctx.torch.int32, device=ctx.tdev)
    ctx.check(ctx.lib.hb_g1_check(ctx.h, ctx.ptr(p), ctx.ptr(flags), n, ctx.stream()), "hb_g1_check")
    return flags != 0


def in_subgroup(ctx, points):
    """-> bool tensor (count,): on the curve and R * P the identity.  A full-width scalar multiplication an element: a recipient of
    foreign commitments decides whether to pay for it (Pedersen binding holds in the subgroup)."""
    _ctx(ctx)
    p, n = _operand(ctx, points)
    order = ctx.torch.from_numpy(np.array([[(R >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)]], dtype=np.uint64).view(np.int64)).to(ctx.tdev)
    rp = scalar_mul(ctx, order, p)                           # the order itself is no canonical residue: uploaded as words
    return on_curve(ctx, p) & (rp.reshape(n, POINT_WORDS) == 0).all(dim=1)


class FixedBase:
    """The fixed-base window table of one base: entry (w, j) = j * 2^(window w) * base, affine, for window in {4, 8}.  The table's
    layout belongs to the library.  Built by one launch that works a window a lane: once a common reference string."""

    def __init__(self, ctx, base, window=8):
        _ctx(ctx)
        if not isinstance(base, G1):
            raise TypeError(f"base: expected a host G1, got {type(base).__name__}")
        if isinstance(window, bool) or not isinstance(window, int) or window not in (4, 8):
            raise ValueError(f"window: 4 or 8, got {window!r}")
        if base.is_one():
            raise ValueError("base: the identity has no table")
        self.ctx, self.base, self.window = ctx, base, window
        nbytes = int(ctx.lib.hb_g1_table_bytes(window))
        self.table = ctx.torch.empty((nbytes // 8,), dtype=ctx.torch.int64, device=ctx.tdev)
        host = np.array(base.to_limbs(), dtype=np.uint64)
        ctx.check(ctx.lib.hb_g1_table(ctx.h, host.ctypes.data, window, ctx.ptr(self.table), ctx.stream()), "hb_g1_table")


def _tables(ctx, tg, th):
    for t, w in ((tg, "tg"), (th, "th")):
        if not isinstance(t, FixedBase):
            raise TypeError(f"{w}: expected a FixedBase, got {type(t).__name__}")
        if t.ctx is not ctx:
            raise ValueError(f"{w}: the table belongs to another context")
    if tg.window != th.window:
        raise ValueError(f"tg and th: window widths {tg.window} and {th.window} differ")
    return tg.window


def commit(ctx, tg, th, a, b, out=None):
    """a[i] * g + b[i] * h -> (count, 2, 6): the dealer's commitments, count = B (t + 1) for B polynomials"""
    _ctx(ctx)
    window = _tables(ctx, tg, th)
    a = ctx.elems(a, what="a")
    count = a.numel() // ctx.n_limbs
    b = ctx.elems(b, count, what="b")
    out = _out(ctx, out, count)
    ctx.check(ctx.lib.hb_g1_commit(ctx.h, ctx.ptr(tg.table), ctx.ptr(th.table), window, ctx.ptr(a), ctx.ptr(b), ctx.ptr(out), count, ctx.stream()), "hb_g1_commit")
    return out


def _commitments(ctx, cs):
    cs = _points(ctx, cs, what="cs")
    if cs.dim() != 4 or cs.shape[1] < 1:
        raise ValueError(f"cs: expected a tensor of shape (B, t + 1, 2, {LIMBS}) with t + 1 >= 1, got {tuple(cs.shape)}")
    return cs, int(cs.shape[0]), int(cs.shape[1])


def _index(i):
    if isinstance(i, bool) or not isinstance(i, int):
        raise TypeError(f"i: expected an int, got {type(i).__name__}")
    if not 0 <= i < 1 << 32:
        raise ValueError(f"i: the index must be in [0, 2^32), got {i}")
    return i


def eval_commitments(ctx, cs, i, out=None):
    """sum_j i^j * cs[b][j] -> (B, 2, 6), by Horner's rule: about t log2(i) doublings an item where the reference raises every
    commitment to a 255-bit power"""
    _ctx(ctx)
    cs, B, n_coef = _commitments(ctx, cs)
    i = _index(i)
    out = _out(ctx, out, B)
    ctx.check(ctx.lib.hb_g1_eval(ctx.h, ctx.ptr(cs), n_coef, i, ctx.ptr(out), B, ctx.stream()), "hb_g1_eval")
    return out


def verify(ctx, tg, th, cs, i, shares, witnesses):
    """-> (verdict (B,) int32, counter (1,) int32): verdict[b] = 1 iff every commitment of item b is on the curve and
    sum_j i^j cs[b][j] == shares[b] * g + witnesses[b] * h; the counter holds the number of rejected items.  Nothing synchronises."""
    _ctx(ctx)
    window = _tables(ctx, tg, th)
    cs, B, n_coef = _commitments(ctx, cs)
    i = _index(i)
    s = ctx.elems(shares, B, what="shares")
    w = ctx.elems(witnesses, B, what="witnesses")
    torch = ctx.torch
    verdict = torch.empty((B,), dtype=torch.int32, device=ctx.tdev)
    counter = torch.zeros((1,), dtype=torch.int32, device=ctx.tdev)
    ctx.check(ctx.lib.hb_g1_verify(ctx.h, ctx.ptr(tg.table), ctx.ptr(th.table), window, ctx.ptr(cs), n_coef, i, ctx.ptr(s), ctx.ptr(w), ctx.ptr(verdict),
                                   ctx.ptr(counter), B, ctx.stream()), "hb_g1_verify")
    return verdict, counter

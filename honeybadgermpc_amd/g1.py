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
    in_subgroup(ctx, points, method="order")             -> bool tensor.  "order": R * P == identity, through scalar_mul's kernel;
                                                         "endomorphism": phi(P) == -[x^2] P in one launch, the same verdicts.  Nothing
                                                         else checks this unless asked (decompress's and verify_batch's check_subgroup).
    decompress(ctx, data, check_subgroup=False, out=None)
                                                         48-byte encodings (device uint8 (count, 48), or host bytes) -> (points, status
                                                         (count,) int32: STATUS_*, rejected (1,) int32) in one launch (csrc/hb_g1_wire.hip)
    compress(ctx, points, out=None)                      -> uint8 (count, 48): the encodings, in one launch
    FixedBase(ctx, base, window=8)                       owns the window table of one base (a host G1, not the identity)
    commit(ctx, tg, th, a, b, out=None)                  a[i] * g + b[i] * h from two FixedBase of one window width: 2 * 256 / window
                                                         mixed additions at most, no doubling
    eval_commitments(ctx, cs, i, out=None)               cs (B, t + 1, 2, 6), 0 <= i < 2^32 -> (B, 2, 6): sum_j i^j cs[b][j] by Horner
    verify(ctx, tg, th, cs, i, shares, witnesses)        -> (verdict (B,) int32: 1 accepted, 0 rejected; counter (1,) int32: rejected
                                                         items).  One fused launch; an item with a commitment off the curve is rejected.
    msm(ctx, scalars, points, out=None, method="auto", chunk=None)
                                                         sum_k scalars[m][k] * points[m or 0][k] -> (M, 2, 6) (csrc/hb_msm.hip): the sum
                                                         over a list of points everything above lacks
    FixedBases(ctx, bases, window=8)                     owns ONE buffer with the window tables of N bases (a list of host G1, none the
                                                         identity): a common reference string.  .base(k): table k as a FixedBase
    msm_fixed(ctx, tg, a, th=None, b=None, out=None, split=None)
                                                         sum_k a[m][k] * G_k (+ b[m][k] * H_k) over the first K bases of one or two
                                                         FixedBases -> (rows, 2, 6) (csrc/hb_crs.hip): table look-ups, no doubling
    kzg_quotients(ctx, phi, xs) -> (q, rem)              phi (B, t + 1, 4), n points: q (B, n, t, 4) the coefficients of
                                                         (phi_b(X) - phi_b(x_i)) / (X - x_i), rem (B, n, 4) = phi_b(x_i)
    lagrange_scalars(xs, targets)                        host, Python ints mod R: the weights of interpolation at `targets`
    interpolate_at(ctx, xs, points, targets, out=None)   interpolation in the exponent: msm of those weights over shared bases
    interpolate_g1_at_x(coords, x, order=-1, ctx=None)   the reference's betterpairing.interpolate_g1_at_x on host objects

Everything is asynchronous on torch's current stream and nothing synchronises, except download(), FixedBase() and FixedBases() (the
bases' upload).
"""
import numpy as np

from .bls12_381 import COMPRESSED_BYTES, G1, LIMBS, R

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


def in_subgroup(ctx, points, method="order"):
    """-> bool tensor (count,): on the curve and in the subgroup of order R; both methods return the same tensor for every input.
    "order": R * P the identity, a full-width scalar multiplication an element and two more launches.  "endomorphism": one launch of
    hb_g1_subgroup, phi(P) == -[x^2] P (csrc/hb_g1_wire.hip): about a quarter of the field products, no inversion, and 3.5 times
    faster at 2^16 points (profiles/g1_wire.txt): the one to use; "order" stays the default until the default is changed on its own."""
    _ctx(ctx)
    if method not in ("order", "endomorphism"):
        raise ValueError(f"method: 'order' or 'endomorphism', got {method!r}")
    p, n = _operand(ctx, points)
    if method == "endomorphism":
        flags = ctx.torch.empty((n,), dtype=ctx.torch.int32, device=ctx.tdev)
        ctx.check(ctx.lib.hb_g1_subgroup(ctx.h, ctx.ptr(p), ctx.ptr(flags), n, ctx.stream()), "hb_g1_subgroup")
        return flags != 0
    order = ctx.torch.from_numpy(np.array([[(R >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)]], dtype=np.uint64).view(np.int64)).to(ctx.tdev)
    rp = scalar_mul(ctx, order, p)                           # the order itself is no canonical residue: uploaded as words
    return on_curve(ctx, p) & (rp.reshape(n, POINT_WORDS) == 0).all(dim=1)


# ---- points from the wire (csrc/hb_g1_wire.hip): status[i] of decompress, as the header's HB_G1_WIRE_*
STATUS_OK, STATUS_NOT_COMPRESSED, STATUS_BAD_IDENTITY, STATUS_X_NOT_BELOW_Q, STATUS_NOT_ON_CURVE, STATUS_NOT_IN_SUBGROUP = range(6)


def _wire_bytes(ctx, data):
    """-> (uint8 tensor on the device, contiguous, its storage aligned to 16 bytes; count)"""
    torch = ctx.torch
    if isinstance(data, torch.Tensor):
        if data.dtype != torch.uint8:
            raise TypeError(f"data: dtype must be uint8, got {data.dtype}")
        if not data.is_cuda or data.device.index != ctx.device:
            raise ValueError(f"data: must live on cuda:{ctx.device}, is on {data.device}")
        if data.numel() % COMPRESSED_BYTES or (data.dim() >= 2 and data.shape[-1] != COMPRESSED_BYTES):
            raise ValueError(f"data: expected a tensor of shape (count, {COMPRESSED_BYTES}), got {tuple(data.shape)}")
        t = data if data.is_contiguous() else data.contiguous()
        if t.data_ptr() % 16:
            t = t.clone()                                       # a view into the middle of a buffer: the kernel reads 16 bytes a load
    else:
        if isinstance(data, (bytes, bytearray, memoryview)):
            arr = np.frombuffer(data, dtype=np.uint8)
        elif isinstance(data, np.ndarray):
            if data.dtype != np.uint8:
                raise TypeError(f"data: dtype must be uint8, got {data.dtype}")
            arr = data.reshape(-1)
        else:
            raise TypeError(f"data: expected a uint8 tensor, bytes, a bytearray or a numpy uint8 array, got {type(data).__name__}")
        if arr.size % COMPRESSED_BYTES:
            raise ValueError(f"data: {arr.size} bytes are no multiple of {COMPRESSED_BYTES}")
        t = torch.from_numpy(np.array(arr, dtype=np.uint8, copy=True)).to(ctx.tdev)
    return t, t.numel() // COMPRESSED_BYTES


def decompress(ctx, data, check_subgroup=False, out=None):
    """48-byte compressed encodings (bls12_381.G1.compress's format) -> (points (count, 2, 6), status (count,) int32, rejected (1,)
    int32) in one launch.  data: a uint8 tensor (count, 48) on the context's device (copied when it is not contiguous or its storage
    not aligned to 16 bytes), or host bytes / bytearray / numpy uint8 of 48 * count bytes, which is uploaded.  status[i] is STATUS_OK
    or the first check the item fails, in the order G1.decompress makes them; STATUS_NOT_IN_SUBGROUP only with check_subgroup.  A
    rejected item's point is all zeros (as the identity's: the status tells), rejected[0] counts them.  Nothing synchronises."""
    _ctx(ctx)
    enc, count = _wire_bytes(ctx, data)
    torch = ctx.torch
    out = _out(ctx, out, count)
    status = torch.empty((count,), dtype=torch.int32, device=ctx.tdev)
    rejected = torch.zeros((1,), dtype=torch.int32, device=ctx.tdev)
    ctx.check(ctx.lib.hb_g1_decompress(ctx.h, ctx.ptr(enc), 1 if check_subgroup else 0, ctx.ptr(out), ctx.ptr(status), ctx.ptr(rejected), count, ctx.stream()),
              "hb_g1_decompress")
    return out, status, rejected


def compress(ctx, points, out=None):
    """points (count, 2, 6) -> uint8 (count, 48) in one launch: big-endian x with 0x80 set, 0x40 for the all-zero point, 0x20 iff
    y > (Q - 1) / 2.  The coordinates are written as they stand: on_curve tells whether they are a point."""
    _ctx(ctx)
    p, n = _operand(ctx, points)
    torch = ctx.torch
    if out is None:
        out = torch.empty((n, COMPRESSED_BYTES), dtype=torch.uint8, device=ctx.tdev)
    else:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8:
            raise TypeError("out: expected a uint8 tensor")
        if not out.is_cuda or out.device.index != ctx.device:
            raise ValueError(f"out: must live on cuda:{ctx.device}, is on {out.device}")
        if not out.is_contiguous() or out.numel() != n * COMPRESSED_BYTES or out.data_ptr() % 16:
            raise ValueError(f"out: expected a contiguous tensor of {n} x {COMPRESSED_BYTES} bytes aligned to 16, got {tuple(out.shape)}")
    ctx.check(ctx.lib.hb_g1_compress(ctx.h, ctx.ptr(p), ctx.ptr(out), n, ctx.stream()), "hb_g1_compress")
    return out


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


# ---- multi-scalar multiplication (csrc/hb_msm.hip)
MSM_CHUNK = 4096
# "auto": the bucket path from this many terms a row on (hb_msm.hip's MSM_AUTO_TERMS says the same for the C ABI's method 0).  The smallest
# K of the M = 64 rows of profiles/g1_msm.txt at which bucket beats direct: it does at every K measured (22: 7.5 ms against 10.4 ms), so
# the smallest one; below it nothing is measured and a row of a few terms keeps the direct path.
MSM_CROSSOVER = 22
_MSM_METHODS = {"direct": 1, "bucket": 2}


def msm(ctx, scalars, points, out=None, method="auto", chunk=None):
    """out[m] = sum_k scalars[m][k] * points[m or 0][k] -> (M, 2, 6).  scalars: (M, K, 4), or (K, 4) for M = 1, plain 256-bit
    integers; points: (K, 2, 6) shared by every row, or (M, K, 2, 6).  method: "direct" (a full scalar multiplication a term and a
    tree of additions), "bucket" (windows of 8 bits: one mixed addition a term a window) or "auto" (bucket from MSM_CROSSOVER terms
    on); all return the same words.  chunk (tests): the terms a workgroup of the bucket path takes, a multiple of 64 in [64, 4096].
    K = 0 gives identities.  A call is never faster than about one scalar_mul of a wave (the last step is 248 dependent doublings a
    row): the gain over scalar_mul + add is throughput at sizes that fill the device, see profiles/g1_msm.txt."""
    _ctx(ctx)
    if method != "auto" and method not in _MSM_METHODS:
        raise ValueError(f"method: 'auto', 'direct' or 'bucket', got {method!r}")
    if chunk is None:
        chunk = 0
    elif isinstance(chunk, bool) or not isinstance(chunk, int) or not 64 <= chunk <= MSM_CHUNK or chunk % 64:
        raise ValueError(f"chunk: a multiple of 64 in [64, {MSM_CHUNK}], got {chunk!r}")
    pts = _points(ctx, points)
    if pts.dim() not in (3, 4):
        raise ValueError(f"points: expected a tensor of shape (K, 2, {LIMBS}) or (M, K, 2, {LIMBS}), got {tuple(pts.shape)}")
    K = int(pts.shape[-3])
    sc = ctx.elems(scalars, what="scalars")
    if sc.dim() not in (2, 3) or sc.shape[-2] != K:
        raise ValueError(f"scalars: expected a tensor of shape (K, 4) or (M, K, 4) with K = {K}, got {tuple(sc.shape)}")
    M = int(sc.shape[0]) if sc.dim() == 3 else 1
    if pts.dim() == 4 and pts.shape[0] != M:
        raise ValueError(f"scalars and points: {M} rows of scalars against {int(pts.shape[0])} rows of points")
    code = _MSM_METHODS[method] if method != "auto" else (1 if K < MSM_CROSSOVER else 2)
    out = _out(ctx, out, M)
    nbytes = int(ctx.lib.hb_g1_msm_workspace_bytes(M, K, code, chunk))
    if nbytes <= 0:
        raise ValueError(f"msm: {M} rows of {K} terms are beyond one call")
    ws = ctx.torch.empty((nbytes // 8,), dtype=ctx.torch.int64, device=ctx.tdev)
    ctx.check(ctx.lib.hb_g1_msm(ctx.h, ctx.ptr(sc), ctx.ptr(pts), 1 if pts.dim() == 4 else 0, ctx.ptr(out), M, K, code, chunk, ctx.ptr(ws), nbytes,
                                ctx.stream()), "hb_g1_msm")
    return out


# ---- fixed bases of a common reference string (csrc/hb_crs.hip)
MAX_FIXED_BASES = 4096


class FixedBases:
    """The window tables of N fixed bases in one buffer, built by one launch (a base a workgroup): the gs or hs of a KZG common reference
    string.  Table k has FixedBase's layout: .base(k) is a FixedBase on it for commit and verify (a view: it keeps the buffer alive)."""

    def __init__(self, ctx, bases, window=8):
        _ctx(ctx)
        bases = list(bases)
        for p in bases:
            if not isinstance(p, G1):
                raise TypeError(f"bases: expected host G1 elements, got {type(p).__name__}")
        if isinstance(window, bool) or not isinstance(window, int) or window not in (4, 8):
            raise ValueError(f"window: 4 or 8, got {window!r}")
        if not 1 <= len(bases) <= MAX_FIXED_BASES:
            raise ValueError(f"bases: between 1 and {MAX_FIXED_BASES} bases, got {len(bases)}")
        if any(p.is_one() for p in bases):
            raise ValueError("bases: the identity has no table")
        self.ctx, self.bases, self.window, self.n = ctx, bases, window, len(bases)
        self.table_words = int(ctx.lib.hb_g1_table_bytes(window)) // 8
        self.tables = ctx.torch.empty((self.n * self.table_words,), dtype=ctx.torch.int64, device=ctx.tdev)
        host = np.array([p.to_limbs() for p in bases], dtype=np.uint64).reshape(self.n, POINT_WORDS)
        ctx.check(ctx.lib.hb_g1_crs_table(ctx.h, host.ctypes.data, self.n, window, ctx.ptr(self.tables), ctx.stream()), "hb_g1_crs_table")

    def __len__(self):
        return self.n

    def base(self, k):
        if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k < self.n:
            raise IndexError(f"k: a base index in [0, {self.n}), got {k!r}")
        fb = FixedBase.__new__(FixedBase)
        fb.ctx, fb.base, fb.window = self.ctx, self.bases[k], self.window
        fb.table = self.tables[k * self.table_words:(k + 1) * self.table_words]
        return fb


def msm_fixed(ctx, tg, a, th=None, b=None, out=None, split=None):
    """out[m] = sum_k a[m][k] * tg[k] (+ b[m][k] * th[k]) -> (rows, 2, 6).  tg, th: FixedBases of one window width and one length N;
    a, b: (rows, K, 4), or (K, 4) for one row, plain 256-bit integers, K <= N: the first K bases are used.  th and b come together or not
    at all.  One mixed addition a non-zero window digit, no doubling.  split (tests, measurements): the lanes that share a row, a
    power of two in [1, 256]; None: the library's rule.  Every split and both widths return the same words.  K = 0 gives identities."""
    _ctx(ctx)
    if (th is None) != (b is None):
        raise ValueError("th and b: the second family needs both its tables and its scalars")
    for t, w in ((tg, "tg"), (th, "th")):
        if t is None:
            continue
        if not isinstance(t, FixedBases):
            raise TypeError(f"{w}: expected a FixedBases, got {type(t).__name__}")
        if t.ctx is not ctx:
            raise ValueError(f"{w}: the tables belong to another context")
    if th is not None and (tg.window != th.window or tg.n != th.n):
        raise ValueError(f"tg and th: window widths {tg.window} and {th.window}, lengths {tg.n} and {th.n} differ")
    if split is None:
        split = 0
    elif isinstance(split, bool) or not isinstance(split, int) or not 1 <= split <= 256 or split & (split - 1):
        raise ValueError(f"split: a power of two in [1, 256], got {split!r}")
    a = ctx.elems(a, what="a")
    if a.dim() not in (2, 3):
        raise ValueError(f"a: expected a tensor of shape (K, 4) or (rows, K, 4), got {tuple(a.shape)}")
    rows, K = (int(a.shape[0]) if a.dim() == 3 else 1), int(a.shape[-2])
    if K > tg.n:
        raise ValueError(f"a: {K} terms a row against {tg.n} bases")
    if b is not None:
        b = ctx.elems(b, what="b")
        if tuple(b.shape) != tuple(a.shape):
            raise ValueError(f"a and b: shapes {tuple(a.shape)} and {tuple(b.shape)} differ")
    out = _out(ctx, out, rows)
    ctx.check(ctx.lib.hb_g1_crs_msm(ctx.h, ctx.ptr(tg.tables), ctx.ptr(th.tables) if th is not None else None, tg.n, tg.window, ctx.ptr(a),
                                    ctx.ptr(b) if b is not None else None, K, split, ctx.ptr(out), rows, ctx.stream()), "hb_g1_crs_msm")
    return out


def kzg_quotients(ctx, phi, xs):
    """phi (B, t + 1, 4): B polynomials' coefficients, canonical residues, lowest first; xs: n points, a tensor (n, 4) of canonical
    residues or a list of ints (reduced mod R) -> (q (B, n, t, 4), rem (B, n, 4)): phi_b(X) - rem[b][i] = (X - xs[i]) sum_j q[b][i][j] X^j,
    so rem[b][i] = phi_b(xs[i]) and q[b][i] are the exponents of the KZG witness at xs[i].  One launch, a lane a (b, i)."""
    _ctx(ctx)
    phi = ctx.elems(phi, what="phi")
    if phi.dim() != 3 or phi.shape[1] < 1:
        raise ValueError(f"phi: expected a tensor of shape (B, t + 1, {ctx.n_limbs}) with t + 1 >= 1, got {tuple(phi.shape)}")
    if isinstance(xs, ctx.torch.Tensor):
        xs = ctx.elems(xs, what="xs")
        if xs.dim() != 2:
            raise ValueError(f"xs: expected a tensor of shape (n, {ctx.n_limbs}), got {tuple(xs.shape)}")
    else:
        xs = ctx.upload_ints([int(x) % R for x in xs]).reshape(-1, ctx.n_limbs)
    B, n_coef, n = int(phi.shape[0]), int(phi.shape[1]), int(xs.shape[0])
    torch = ctx.torch
    q = torch.empty((B, n, n_coef - 1, ctx.n_limbs), dtype=torch.int64, device=ctx.tdev)
    rem = torch.empty((B, n, ctx.n_limbs), dtype=torch.int64, device=ctx.tdev)
    ctx.check(ctx.lib.hb_kzg_quotient(ctx.h, ctx.ptr(phi), n_coef, ctx.ptr(xs), n, ctx.ptr(q), ctx.ptr(rem), B, ctx.stream()), "hb_kzg_quotient")
    return q, rem


def _batch_inverse(values):
    """1 / v mod R for every v (none zero) with ONE modular inversion: prefix products, then back"""
    prefix, run = [], 1
    for v in values:
        prefix.append(run)
        run = run * v % R
    inv, out = pow(run, -1, R), [0] * len(values)
    for k in range(len(values) - 1, -1, -1):
        out[k] = inv * prefix[k] % R
        inv = inv * values[k] % R
    return out


def lagrange_scalars(xs, targets, shortcut=True):
    """-> rows[i][k] = prod_{j != k} (targets[i] - xs[j]) / (xs[k] - xs[j]) mod R, Python ints: sum_k rows[i][k] f(xs[k]) = f(targets[i])
    for every polynomial f of degree below len(xs).  A target that is a node gives a unit row (its numerators vanish but one).
    Nodes that are consecutive integers (the reference's 0 .. K - 1) take their denominators from factorials,
    (xs[k] - xs[j]) over j != k = k! (K - 1 - k)! (-1)^(K - 1 - k): O(K); any other distinct nodes O(K^2) (shortcut=False forces this
    path).  Either way one modular inversion.  Duplicate nodes (mod R) raise ValueError."""
    raw = [int(x) for x in xs]
    nodes = [x % R for x in raw]
    K = len(nodes)
    if len(set(nodes)) != K:
        raise ValueError("xs: the nodes must be distinct mod R")
    if K == 0:
        return [[] for _ in targets]
    if shortcut and K < R and all(raw[k] == raw[0] + k for k in range(K)):
        fact = [1] * K
        for k in range(1, K):
            fact[k] = fact[k - 1] * k % R
        dens = [fact[k] * fact[K - 1 - k] * (-1 if (K - 1 - k) & 1 else 1) % R for k in range(K)]
    else:
        dens = []
        for k in range(K):
            d = 1
            for j in range(K):
                if j != k:
                    d = d * (nodes[k] - nodes[j]) % R
            dens.append(d)
    inv = _batch_inverse(dens)
    rows = []
    for t in targets:
        t = int(t) % R
        # numerator k = (the product before k) * (the product after k): no division by t - xs[k], which may be zero
        before, run = [], 1
        for k in range(K):
            before.append(run)
            run = run * (t - nodes[k]) % R
        row, run = [0] * K, 1
        for k in range(K - 1, -1, -1):
            row[k] = before[k] * run % R * inv[k] % R
            run = run * (t - nodes[k]) % R
        rows.append(row)
    return rows


def interpolate_at(ctx, xs, points, targets, out=None):
    """points[k] = f(xs[k]) * G for an unknown polynomial f of degree below K -> (len(targets), 2, 6): f(targets[i]) * G, as msm of
    lagrange_scalars(xs, targets) over the shared bases `points` (K, 2, 6).  The n Lagrange combinations of HbAvssBatch's share
    recovery (hbavss.py:499-512) are ONE call."""
    _ctx(ctx)
    xs, targets = list(xs), list(targets)
    pts = _points(ctx, points, len(xs))
    rows = lagrange_scalars(xs, targets)
    sc = ctx.upload_ints([v for row in rows for v in row]).reshape(len(targets), len(xs), 4)
    return msm(ctx, sc, pts.reshape(len(xs), 2, LIMBS), out=out)


def interpolate_g1_at_x(coords, x, order=-1, ctx=None):
    """The reference's betterpairing.interpolate_g1_at_x (:800) on host objects: coords = [(x_k, host G1)], sorted by x_k, the first
    `order` of them (all by default) interpolated at x -> a host G1.  One msm of one row; download synchronises."""
    if ctx is None:
        from ._capi import Context

        ctx = Context.get(R)
    _ctx(ctx)
    coords = sorted(((int(c[0]), c[1]) for c in coords), key=lambda c: c[0])
    if order == -1:
        order = len(coords)
    coords = coords[:order]
    if not coords:
        return G1.one()
    pts = upload([c[1] for c in coords], ctx)
    return download(interpolate_at(ctx, [c[0] for c in coords], pts, [int(x)]))[0]

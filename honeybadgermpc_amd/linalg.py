"""
Products of share matrices on the device (csrc/hb_mat.hip): the GF(p) GEMM that regression, a linear layer and the reference
tutorial's dot_product need, on the limb tensors the rest of the package speaks.  A matrix is an int64 tensor (m, k, limbs), a batch of
them (batch, m, k, limbs); row-major, canonical residues.

Tensor level -- one call each on torch's current stream, nothing synchronises:

    matmul(ctx, a, b, add=None, sub=None, out=None)     a b, a b + add or a b - sub; the epilogue is part of the launch; out may be add / sub
    dot(ctx, x, y)                                      inner products: (k, limbs) vectors -> (1, limbs); (batch, k, limbs) -> (batch, limbs)

    TILE_M, TILE_N, TILE_K        the kernel's output tile and the depth of one staged step
    LAZY_GROUP, LAZY_L            products between two carry passes / two reductions, per element width: {limbs: value}
    SPLIT_MIN_K, SPLIT_MAX_WORKGROUPS, SPLIT_TARGET_WORKGROUPS
                                  the inner dimension is cut into slices when the output gives at most SPLIT_MAX_WORKGROUPS tiles
                                  over all batches and k >= SPLIT_MIN_K (hbmpc_hip.h): takes_split(batch, m, k, n)
    (all read from the library: hb_mat_constants)

Protocol level -- coroutines over an OpenCoalescer, tensors in and out.  Degree reduction is linear, so a product of share matrices
needs one open per OUTPUT (or per input), not one per scalar product:

    double_sharing_matmul(co, X, Y, r_t, r_2t)          open(X Y - r_2t, degree 2t) + r_t: m n opened elements, no triple
    beaver_matmul(co, X, Y, (P, Q, PQ))                 D = open(X - P), E = open(Y - Q) in ONE batch; D (E + Q) + (P E + PQ):
                                                        m k + k n opened elements, one matrix triple
    count_opens(method, m, k, n, batch=1)               opened elements of one call
    count_triples(method, m, k, n, batch=1)             scalar Beaver triples of one call: none by either method (the element-wise
                                                        route, share_arithmetic.beaver_multiply_arrays on the expanded array, is
                                                        count_opens("elementwise", ...) = 2 m k n and count_triples(...) = m k n)
    count_matrix_triples(method, batch=1)               matrix triples (P, Q, P Q) of one call: batch for BEAVER, else 0
    count_double_sharings(method, m, k, n, batch=1)     pairs (r_t, r_2t) of one call: m n for DOUBLE_SHARING, else 0

Preprocessing is handed in as tensors (offline.randousha, offline.generate_matrix_triples).  A mask may be given in the product's
shape or flat, (m n, limbs), as randousha returns it.
"""
import ctypes

from ._capi import HB_MAT_ADD, HB_MAT_CONSTANTS, HB_MAT_NONE, HB_MAT_SUB, load_library
from .share_arithmetic import add as _add
from .share_arithmetic import sub as _sub

DOUBLE_SHARING, BEAVER, ELEMENTWISE = "double_sharing", "beaver", "elementwise"


def _constants(n_limbs):
    out = (ctypes.c_int32 * HB_MAT_CONSTANTS)()
    rc = load_library().hb_mat_constants(n_limbs, out)
    if rc:
        raise RuntimeError(f"hb_mat_constants({n_limbs}) failed: {rc}")
    return list(out)


_W, _N = _constants(4), _constants(1)
TILE_M, TILE_N, TILE_K = _W[0], _W[1], _W[2]
LAZY_GROUP = {4: _W[3], 1: _N[3]}
LAZY_L = {4: _W[4], 1: _N[4]}
SPLIT_MIN_K, SPLIT_MAX_WORKGROUPS, SPLIT_TARGET_WORKGROUPS = _W[5], _W[6], _W[7]


def workgroups(batch, m, n):
    """output tiles of one call"""
    return batch * (-(-m // TILE_M)) * (-(-n // TILE_N))


def takes_split(batch, m, k, n):
    """does hb_mat_mul cut the inner dimension of this shape into slices (two launches, partial products in the context's per-stream
    scratch)?  The rule hbmpc_hip.h states: few enough output tiles, a long enough inner dimension."""
    return 1 <= workgroups(batch, m, n) <= SPLIT_MAX_WORKGROUPS and k >= SPLIT_MIN_K


# ---- tensor level ------------------------------------------------------------------------------------------------------------
def _matrix(ctx, t, what):
    t = ctx.elems(t, what=what)
    if t.dim() not in (3, 4):
        raise ValueError(f"{what}: expected shape (rows, columns, {ctx.n_limbs}) or (batch, rows, columns, {ctx.n_limbs}), got {tuple(t.shape)}")
    return t


def _shaped(ctx, t, shape, what):
    """a tensor of the product's shape (returned as it is when contiguous), or flat with as many elements -> viewed in that shape"""
    t = ctx.elems(t, what=what)
    count = 1
    for d in shape[:-1]:
        count *= d
    if tuple(t.shape) != tuple(shape) and tuple(t.shape) != (count, ctx.n_limbs):
        raise ValueError(f"{what}: expected shape {tuple(shape)} or ({count}, {ctx.n_limbs}), got {tuple(t.shape)}")
    return t if tuple(t.shape) == tuple(shape) else t.view(shape)


def matmul(ctx, a, b, add=None, sub=None, out=None):
    """a b (+ add | - sub): a (m, k, limbs) or (batch, m, k, limbs), b (k, n, limbs) or (batch, k, n, limbs) -> (m, n, limbs) or
    (batch, m, n, limbs).  add and sub are mutually exclusive and have the result's shape (or are flat).  out may be add or sub, never
    a or b.  One launch (two when the inner dimension is split), on torch's current stream; nothing synchronises."""
    if add is not None and sub is not None:
        raise ValueError("add and sub are mutually exclusive")
    a, b = _matrix(ctx, a, "a"), _matrix(ctx, b, "b")
    if b.dim() != a.dim():
        raise ValueError(f"b: expected {a.dim()} dimensions as a has, got shape {tuple(b.shape)}")
    batch = a.shape[0] if a.dim() == 4 else 1
    m, k = a.shape[-3], a.shape[-2]
    if b.shape[-3] != k or (b.dim() == 4 and b.shape[0] != batch):
        raise ValueError(f"b: expected shape {tuple(a.shape[:-3]) + (k, 'n', ctx.n_limbs)} to go with a {tuple(a.shape)}, got {tuple(b.shape)}")
    n = b.shape[-2]
    shape = tuple(a.shape[:-3]) + (m, n, ctx.n_limbs)
    c, op, name = None, HB_MAT_NONE, None
    if add is not None:
        c, op, name = _shaped(ctx, add, shape, "add"), HB_MAT_ADD, "add"
    elif sub is not None:
        c, op, name = _shaped(ctx, sub, shape, "sub"), HB_MAT_SUB, "sub"
    if out is None:
        res = ctx.torch.empty(shape, dtype=ctx.torch.int64, device=ctx.tdev)
    else:
        if isinstance(out, ctx.torch.Tensor) and not out.is_contiguous():
            raise ValueError("out: must be contiguous")
        res = _shaped(ctx, out, shape, "out")
        if res.numel() and res.data_ptr() in (a.data_ptr(), b.data_ptr()):
            raise ValueError("out: must not be a or b")
    if batch * m * n == 0:
        return res
    rc = ctx.lib.hb_mat_mul(ctx.h, ctx.ptr(a), ctx.ptr(b), None if c is None else ctx.ptr(c), op, ctx.ptr(res), batch, m, k, n, ctx.stream())
    ctx.check(rc, f"hb_mat_mul({name})" if name else "hb_mat_mul")
    return res


def dot(ctx, x, y):
    """inner products of share vectors: x, y (k, limbs) -> (1, limbs); (batch, k, limbs) -> (batch, limbs).  matmul with m = n = 1:
    a long vector is cut into slices over the device (takes_split)."""
    x, y = ctx.elems(x, what="x"), ctx.elems(y, what="y")
    if x.dim() not in (2, 3):
        raise ValueError(f"x: expected shape (k, {ctx.n_limbs}) or (batch, k, {ctx.n_limbs}), got {tuple(x.shape)}")
    if tuple(y.shape) != tuple(x.shape):
        raise ValueError(f"y: expected shape {tuple(x.shape)} as x has, got {tuple(y.shape)}")
    batch, k = (x.shape[0], x.shape[1]) if x.dim() == 3 else (1, x.shape[0])
    res = matmul(ctx, x.view(batch, 1, k, ctx.n_limbs), y.view(batch, k, 1, ctx.n_limbs))
    return res.view(batch, ctx.n_limbs)


# ---- costs ---------------------------------------------------------------------------------------------------------------------
def _check_method(method):
    if method not in (DOUBLE_SHARING, BEAVER, ELEMENTWISE):
        raise ValueError(f"method: DOUBLE_SHARING, BEAVER or ELEMENTWISE, got {method!r}")


def _check_dims(*dims):
    for d in dims:
        if not isinstance(d, int) or isinstance(d, bool) or d < 0:
            raise ValueError(f"dimensions must be integers >= 0, got {d!r}")


def count_opens(method, m, k, n, batch=1):
    """opened elements of one shared product: m n (DOUBLE_SHARING, at degree 2t), m k + k n (BEAVER, one batch), 2 m k n
    (ELEMENTWISE: beaver_multiply_arrays on the expanded array)"""
    _check_method(method)
    _check_dims(m, k, n, batch)
    return batch * {DOUBLE_SHARING: m * n, BEAVER: m * k + k * n, ELEMENTWISE: 2 * m * k * n}[method]


def count_triples(method, m, k, n, batch=1):
    """scalar Beaver triples of one shared product: m k n for ELEMENTWISE, none otherwise"""
    _check_method(method)
    _check_dims(m, k, n, batch)
    return batch * m * k * n if method == ELEMENTWISE else 0


def count_matrix_triples(method, batch=1):
    """matrix triples (P, Q, P Q) of one shared product"""
    _check_method(method)
    _check_dims(batch)
    return batch if method == BEAVER else 0


def count_double_sharings(method, m, k, n, batch=1):
    """pairs (r_t, r_2t) of one shared product"""
    _check_method(method)
    _check_dims(m, k, n, batch)
    return batch * m * n if method == DOUBLE_SHARING else 0


# ---- protocols over an OpenCoalescer -------------------------------------------------------------------------------------------
def _flat(ctx, t):
    return t.view(-1, ctx.n_limbs)


async def double_sharing_matmul(co, X, Y, r_t, r_2t):
    """Shares of X Y by degree reduction: the local product of two share matrices is a degree-2t sharing of the product matrix;
    masked by r_2t it is opened at degree 2t -- m n elements, whatever the inner dimension -- and the difference is added to r_t, the
    degree-t sharing of the same random values.  One launch, one open, one add; no triple.  n >= 3t + 1 parties."""
    ctx = co.ctx
    masked = matmul(ctx, X, Y, sub=r_2t)
    shape = tuple(masked.shape)
    r_t = _shaped(ctx, r_t, shape, "r_t")
    diff = await co.open_share_array(_flat(ctx, masked), degree=2 * co.t)
    return _add(ctx, _flat(ctx, r_t), diff).view(shape)


async def beaver_matmul(co, X, Y, triple):
    """Shares of X Y from one matrix triple (P, Q, PQ = P Q), P of X's shape and Q of Y's: D = X - P and E = Y - Q are queued before
    the first await and travel as ONE batch of m k + k n elements; the result is D (E + Q) + (P E + PQ) = D E + D Q + P E + P Q: two
    matmul launches whose epilogues do both additions, and one add."""
    ctx = co.ctx
    try:
        P, Q, PQ = triple
    except (TypeError, ValueError):
        raise ValueError("triple: expected (P, Q, PQ)") from None
    X, Y = _matrix(ctx, X, "X"), _matrix(ctx, Y, "Y")
    P, Q = _shaped(ctx, P, tuple(X.shape), "triple P"), _shaped(ctx, Q, tuple(Y.shape), "triple Q")
    if Y.dim() != X.dim() or Y.shape[-3] != X.shape[-2] or (X.dim() == 4 and Y.shape[0] != X.shape[0]):
        raise ValueError(f"Y: shape {tuple(Y.shape)} does not go with X {tuple(X.shape)}")
    shape = tuple(X.shape[:-2]) + (Y.shape[-2], ctx.n_limbs)
    PQ = _shaped(ctx, PQ, shape, "triple PQ")
    f = co.open_share_array(_sub(ctx, _flat(ctx, X), _flat(ctx, P)))
    g = co.open_share_array(_sub(ctx, _flat(ctx, Y), _flat(ctx, Q)))
    D = (await f).view(X.shape)
    E = (await g).view(Y.shape)
    low = matmul(ctx, P, E, add=PQ)
    EQ = _add(ctx, _flat(ctx, E), _flat(ctx, Q)).view(Y.shape)
    return matmul(ctx, D, EQ, add=low, out=low)

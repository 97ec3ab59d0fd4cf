"""
Fixed-point arithmetic on share arrays on the device (csrc/hb_fxp.hip): the reference's progs/fixedpoint.py ("Secure Computation
With Fixed-Point Numbers", Catrina and Saxena, http://www.ifca.ai/pub/fc10/31_47.pdf), on the (count, limbs) int64 tensors the rest
of the package speaks.  A real number a is the integer int(a * 2**f), a signed k-bit value held as a residue; kappa is the
statistical security parameter of the masks.

    F = 32, KAPPA = 32, K = 64                          the reference's constants; every function takes f, k, kappa with these defaults
    to_fixed_point_repr(x, f)                           fixedpoint.py:55-56    int(x * 2**f): rounds towards zero
    from_fixed_point_repr(v, p, k, f, signed)           :66-71                 v a residue; v >= 2^(k-1) is negative when signed
    binary_repr(x, k)                                   :80-86                 k bits, least significant first
    check_params(p, k, m, kappa)                        ValueError unless 0 < m < k and k + kappa + 1 <= p.bit_length() - 1: the masked
                                                        value c = x + 2^(k-1) + r1 + 2^m r2 < 2^k + 2^m + 2^(k+kappa) < 2^(k+kappa+1) must not wrap
    trunc_pr_model, div2m_model, trunc_model, ltz_model host models on Python ints with the dealt r1, r2 as inputs (:108-120, :184-211, :266-268)

Preprocessing is handed in as tensors.  `bits` is one tensor of bit planes, (at least k + kappa, count, limbs): plane i holds this
party's shares of random bit b_i of every element; r1 = sum_{i<m} 2^i b_i, r2 = sum_{i<k+kappa-m} 2^i b_{m+i}.  `triples = (p, q, pq)`,
each (at least carry_triples(m), count, limbs).

Tensor level, one launch each on torch's current stream, nothing synchronises:

    random2m(ctx, bits, k, m, kappa)                    -> (r1, r2)                                             :91-98
    trunc_mask(ctx, x, bits, k, m, kappa)               -> (x + 2^(k-1) + r1 + 2^m r2, r1): the array to open   :114-117, :185-189
    trunc_pr_finish(ctx, x, c, r1, m)                   (x - (c mod 2^m) + r1) / 2^m                            :118-119
    ltl_leaves(ctx, c, bits, m)                         -> (g, p), (m + 1, count, limbs) each: the carry tree's leaves, no product   :143-149, :168-169
    carry_mask(ctx, g, p, ta, tb, root)                 the level's array to open                               :141
    carry_combine(ctx, opened, g, p, ta, tb, tab, root) -> the next level's (g, p); at the root g alone         :141
    div2m_finish(ctx, x, c, r1, carry, m, mode)         MOD [x mod 2^m] | TRUNC [floor(x / 2^m)] | NEG_TRUNC    :191-192, :210, :268
    carry_levels(m)  = ceil(log2(m + 1))                levels of the tree over m + 1 leaves
    carry_triples(m) = 2 m - 1                          triples an element it consumes

The carry tree.  Leaves are ordered most significant bit first, then the low carry (1, 0); a level combines planes 2j and 2j + 1 with
(g1, p1) o (g2, p2) = (g1 + p1 g2, p1 p2) and moves an odd last plane up unchanged.  The operator is associative, so pairing
adjacent planes level by level gives the same carry as the reference's len // 2 recursion (_bit_ltl_reduce): the parties' SHARES
differ from the reference's, the opened values do not.  A level over `nodes` planes consumes 2 (nodes // 2) rows of the triple
tensors, in order: row 2j multiplies p1 g2 of node j, row 2j + 1 p1 p2; the root level (two planes) consumes one row, p1 g2 (its p is
never used).  Levels take their rows one after the other from row 0.

Protocol level, coroutines over an OpenCoalescer (every party runs the same coroutine, so the opens meet batch for batch):

    async trunc_pr(co, x, bits, k, m, kappa)            1 open, 2 launches                        [x / 2^m] rounded up or down   :108-120
    async carry_tree(co, g, p, triples)                 carry_levels(nodes - 1) opens, 2 per level the root's g of given leaf planes
    async get_carry_bit(co, c, r_bits, triples)         carry_levels(m) opens, 1 + 2 per level    carry of c2 + (2^m - 1 - r) + 1   :131-150
    async bit_ltl(co, c, r_bits, triples)               the same, + 2 launches                    [c2 < r]                       :163-172
    async div2m(co, x, bits, triples, k, m, kappa)      1 + carry_levels(m) opens                 [x mod 2^m]                    :184-193
    async trunc(co, x, bits, triples, k, m, kappa)      1 + carry_levels(m) opens                 [floor(x / 2^m)]               :208-211
    async ltz(co, x, bits, triples, k, kappa)           1 + carry_levels(k - 1) opens             [x < 0]                        :266-268
    async lt(co, x, y, bits, triples, k, kappa)         the same, + 1 launch                      [x < y]                        :274-275
    async mul(co, x, y, triple, bits, f, k, kappa)      2 opens: beaver_multiply_arrays, then trunc_pr(., 2 k, f); 2 k + kappa planes   :240-251
    async matmul(co, X, Y, prep, bits, method, f, k, kappa)   the shared matrix product (linalg), then ONE trunc_pr an output at width
                                                        matmul_width(k, inner) = 2 k + ceil(log2(inner)): 2 batches, m n truncation opens

div2m and its kin take 3 + 2 carry_levels(m) launches for any count.  FixedPointArray wraps a share array with +, -, neg(), mul,
div by a public number, divide by a shared one and reciprocal (progs/fixedpoint_division.py), atan2 and atan
(progs/fixedpoint_atan.py), ltz, lt, sort (progs/sorting.py) and open() -> list[float].
"""
from .._capi import HB_FXP_MOD, HB_FXP_NEG_TRUNC, HB_FXP_TRUNC
from ..share_arithmetic import add, beaver_multiply_arrays, neg, sub
from ..share_arithmetic import mul as _ew_mul

F = 32
KAPPA = 32
K = 64
MOD, TRUNC, NEG_TRUNC = HB_FXP_MOD, HB_FXP_TRUNC, HB_FXP_NEG_TRUNC


# ---- host functions ------------------------------------------------------------------------------------------------------
def to_fixed_point_repr(x, f=F):
    """int(x * 2**f), rounding towards zero (fixedpoint.py:55-56)"""
    return int(x * 2 ** f)


def from_fixed_point_repr(v, p, k=K, f=F, signed=True):
    """the real number a residue v stands for (fixedpoint.py:66-71, whose argument is a field element)"""
    v = int(v)
    if v >= 2 ** (k - 1) and signed:
        v = -(p - v)
    return float(v) / 2 ** f


def binary_repr(x, k):
    """x in k bits (more if it needs them), least significant first (fixedpoint.py:80-86)"""
    if not isinstance(x, int):
        raise TypeError("x must be an integer")
    return [int(i) for i in f"{x:0{k}b}"[::-1]]


def _int(v, what):
    if not isinstance(v, int) or isinstance(v, bool):
        raise ValueError(f"{what} must be an integer, got {v!r}")
    return v


def check_params(p, k, m, kappa=KAPPA, full=False):
    """ValueError unless 0 < m < k and the masked value cannot wrap: k + kappa + 1 <= p.bit_length() - 1.  full=True (trunc, ltz: the
    carry tree): also m <= k - 1."""
    k, m, kappa = _int(k, "k"), _int(m, "m"), _int(kappa, "kappa")
    if not 0 < m < k:
        raise ValueError(f"needs 0 < m < k, got m = {m}, k = {k}")
    if kappa < 0:
        raise ValueError(f"kappa must not be negative, got {kappa}")
    if k + kappa + 1 > p.bit_length() - 1:
        raise ValueError(f"k + kappa + 1 = {k + kappa + 1} bits do not fit below a modulus of {p.bit_length()} bits: the masked value would wrap")
    if full and m > k - 1:
        raise ValueError(f"needs m <= k - 1, got m = {m}, k = {k}")


def _check_m(p, m):
    m = _int(m, "m")
    if not 0 < m <= p.bit_length() - 2:
        raise ValueError(f"needs 0 < m <= {p.bit_length() - 2}, got {m}")


def masked_model(x, r1, r2, p, k, m):
    """the value trunc_pr and div2m open (fixedpoint.py:117, :189)"""
    return (x + 2 ** (k - 1) + r1 + 2 ** m * r2) % p


def trunc_pr_model(x, r1, r2, p, k, m, kappa=KAPPA):
    """what trunc_pr's result opens to (fixedpoint.py:108-120) with the masks r1 < 2^m, r2 < 2^(k+kappa-m) that were dealt"""
    check_params(p, k, m, kappa)
    c2 = masked_model(x, r1, r2, p, k, m) % 2 ** m
    return (x - c2 + r1) * pow(2, -m, p) % p


def div2m_model(x, r1, r2, p, k, m, kappa=KAPPA):
    """what div2m's result opens to (fixedpoint.py:184-193): u = bit_ltl(c2, r1) = [c2 < r1]"""
    check_params(p, k, m, kappa, full=True)
    c2 = masked_model(x, r1, r2, p, k, m) % 2 ** m
    u = 1 if c2 < r1 else 0
    return (c2 - r1 + 2 ** m * u) % p


def trunc_model(x, r1, r2, p, k, m, kappa=KAPPA):
    """fixedpoint.py:208-211"""
    return (x - div2m_model(x, r1, r2, p, k, m, kappa)) * pow(2, -m, p) % p


def ltz_model(x, r1, r2, p, k=K, kappa=KAPPA):
    """FixedPoint.ltz, fixedpoint.py:266-268"""
    return -trunc_model(x, r1, r2, p, k, k - 1, kappa) % p


def carry_levels(m):
    """levels of the carry tree over m + 1 leaves: ceil(log2(m + 1))"""
    if _int(m, "m") < 1:
        raise ValueError(f"m must be positive, got {m}")
    return m.bit_length()


def _level_triples(nodes):
    return 1 if nodes == 2 else 2 * (nodes // 2)


def carry_triples(m):
    """triples an element the carry tree over m + 1 leaves consumes: two a merge, one at the root"""
    if _int(m, "m") < 1:
        raise ValueError(f"m must be positive, got {m}")
    return 2 * m - 1


# ---- tensor level ----------------------------------------------------------------------------------------------------------
def _planes(ctx, t, rows, count, what, exact=False):
    """a (rows, count, limbs) tensor (at least `rows` rows unless exact) -> contiguous, count"""
    t = ctx.elems(t, what=what)
    if t.dim() != 3 or (count is not None and t.shape[1] != count) or (t.shape[0] != rows if exact else t.shape[0] < rows):
        raise ValueError(f"{what}: expected shape ({'' if exact else 'at least '}{rows}, {'count' if count is None else count}, {ctx.n_limbs}), got {tuple(t.shape)}")
    return t, t.shape[1]


def _planes_out(ctx, out, rows, count, what="out"):
    if out is None:
        return ctx.torch.empty((rows, count, ctx.n_limbs), dtype=ctx.torch.int64, device=ctx.tdev)
    if isinstance(out, ctx.torch.Tensor) and not out.is_contiguous():
        raise ValueError(f"{what}: must be contiguous")
    return ctx.elems(out, rows * count, what=what)


def _elems_out(ctx, out, count, what="out"):
    if out is None:
        return ctx.empty(count)
    if isinstance(out, ctx.torch.Tensor) and not out.is_contiguous():
        raise ValueError(f"{what}: must be contiguous")
    return ctx.elems(out, count, what=what)


def _pair(out):
    if out is None:
        return None, None
    try:
        a, b = out
    except (TypeError, ValueError):
        raise ValueError("out: expected a pair of tensors") from None
    return a, b


def _inv2m(ctx, m):
    return ctx.host_elems([pow(2, -m, ctx.modulus)])


def random2m(ctx, bits, k, m, kappa=KAPPA, out=None):
    """-> (r1, r2) = (sum_{i<m} 2^i b_i, sum_{i<k+kappa-m} 2^i b_{m+i}): the two random2m calls of trunc_pr and div2m
    (fixedpoint.py:91-98, :114-115) in one launch.  out: a pair (r1, r2)."""
    check_params(ctx.modulus, k, m, kappa)
    bits, count = _planes(ctx, bits, k + kappa, None, "bits")
    o1, o2 = _pair(out)
    r1, r2 = _elems_out(ctx, o1, count, "out r1"), _elems_out(ctx, o2, count, "out r2")
    ctx.check(ctx.lib.hb_fxp_mask(ctx.h, None, ctx.ptr(bits), k, m, kappa, ctx.ptr(r2), ctx.ptr(r1), count, ctx.stream()), "hb_fxp_mask")
    return r1, r2


def trunc_mask(ctx, x, bits, k, m, kappa=KAPPA, out=None, r1_out=None):
    """-> (x + 2^(k-1) + r1 + 2^m r2, r1): the array to open and what the step after the open needs.  One launch reading k + kappa
    planes.  out (the masked array) may be x."""
    check_params(ctx.modulus, k, m, kappa)
    x = ctx.elems(x, what="x")
    count = x.numel() // ctx.n_limbs
    bits, _ = _planes(ctx, bits, k + kappa, count, "bits")
    masked, r1 = _elems_out(ctx, out, count), _elems_out(ctx, r1_out, count, "r1_out")
    if count and masked.data_ptr() == r1.data_ptr():
        raise ValueError("out and r1_out must be two arrays")
    ctx.check(ctx.lib.hb_fxp_mask(ctx.h, ctx.ptr(x), ctx.ptr(bits), k, m, kappa, ctx.ptr(masked), ctx.ptr(r1), count, ctx.stream()), "hb_fxp_mask")
    return masked, r1


def trunc_pr_finish(ctx, x, c, r1, m, out=None):
    """(x - (c mod 2^m) + r1) / 2^m with c the opened masked array (fixedpoint.py:118-119).  out may be any of the arrays."""
    _check_m(ctx.modulus, m)
    x = ctx.elems(x, what="x")
    count = x.numel() // ctx.n_limbs
    c, r1 = ctx.elems(c, count, what="c"), ctx.elems(r1, count, what="r1")
    out = _elems_out(ctx, out, count)
    inv = _inv2m(ctx, m)
    ctx.check(ctx.lib.hb_fxp_trunc_pr(ctx.h, ctx.ptr(x), ctx.ptr(c), ctx.ptr(r1), m, inv.ctypes.data, ctx.ptr(out), count, ctx.stream()), "hb_fxp_trunc_pr")
    return out


def ltl_leaves(ctx, c, bits, m, out=None):
    """-> (g, p), (m + 1, count, limbs) each: the leaves of the carry tree of c2 + (2^m - 1 - r) + 1, c2 = c mod 2^m public, r the
    number whose bit shares are planes 0 .. m - 1 of `bits`, most significant bit first, the low carry (1, 0) last.  No triple, no
    open: a public bit selects (the reference multiplies, fixedpoint.py:143).  out: a pair (g, p) of arrays of their own."""
    _check_m(ctx.modulus, m)
    c = ctx.elems(c, what="c")
    count = c.numel() // ctx.n_limbs
    bits, _ = _planes(ctx, bits, m, count, "bits")
    og, op = _pair(out)
    g, p = _planes_out(ctx, og, m + 1, count, "out g"), _planes_out(ctx, op, m + 1, count, "out p")
    ctx.check(ctx.lib.hb_fxp_ltl_leaves(ctx.h, ctx.ptr(c), ctx.ptr(bits), m, ctx.ptr(g), ctx.ptr(p), count, ctx.stream()), "hb_fxp_ltl_leaves")
    return g.view(m + 1, count, ctx.n_limbs), p.view(m + 1, count, ctx.n_limbs)


def _level(ctx, g, p, root):
    g = ctx.elems(g, what="g")
    if g.dim() != 3 or g.shape[0] < 2:
        raise ValueError(f"g: expected shape (nodes >= 2, count, {ctx.n_limbs}), got {tuple(g.shape)}")
    nodes, count = g.shape[0], g.shape[1]
    if nodes > 257:
        raise ValueError(f"g: at most 257 planes, got {nodes}")
    p, _ = _planes(ctx, p, nodes, count, "p", exact=True)
    root = bool(root)
    if root and nodes != 2:
        raise ValueError(f"root: the root level has two planes, got {nodes}")
    return g, p, nodes, count, root, (1 if root else 2 * (nodes // 2))


def carry_mask(ctx, g, p, ta, tb, root=False, out=None):
    """One level of the carry tree before its open.  g, p (nodes, count, limbs); ta, tb this party's shares of the first and second
    factors of the level's triples, (2 (nodes // 2), count, limbs), at the root (1, count, limbs).  -> (2 triples, count, limbs): rows
    2t, 2t + 1 = p1 - ta[t], (g2 | p2) - tb[t], ONE array to open."""
    g, p, nodes, count, root, triples = _level(ctx, g, p, root)
    ta, _ = _planes(ctx, ta, triples, count, "ta", exact=True)
    tb, _ = _planes(ctx, tb, triples, count, "tb", exact=True)
    out = _planes_out(ctx, out, 2 * triples, count)
    ctx.check(ctx.lib.hb_fxp_carry_mask(ctx.h, ctx.ptr(g), ctx.ptr(p), nodes, int(root), ctx.ptr(ta), ctx.ptr(tb), ctx.ptr(out), count, ctx.stream()),
              "hb_fxp_carry_mask")
    return out.view(2 * triples, count, ctx.n_limbs)


def carry_combine(ctx, opened, g, p, ta, tb, tab, root=False, out=None):
    """One level of the carry tree after its open: -> (g', p'), (ceil(nodes / 2), count, limbs) each; at the root -> g' alone,
    (count, limbs): the carry.  out: a pair (root: one tensor), arrays of their own."""
    g, p, nodes, count, root, triples = _level(ctx, g, p, root)
    opened = ctx.elems(opened, 2 * triples * count, what="opened")                       # (2 triples, count, limbs), or flat as an open returns it
    ta, tb, tab = (_planes(ctx, v, triples, count, w, exact=True)[0] for v, w in ((ta, "ta"), (tb, "tb"), (tab, "tab")))
    if root:
        g_out, p_out = _elems_out(ctx, out, count), None
    else:
        og, op = _pair(out)
        g_out, p_out = _planes_out(ctx, og, (nodes + 1) // 2, count, "out g"), _planes_out(ctx, op, (nodes + 1) // 2, count, "out p")
    ctx.check(ctx.lib.hb_fxp_carry_combine(ctx.h, ctx.ptr(opened), ctx.ptr(g), ctx.ptr(p), nodes, int(root), ctx.ptr(ta), ctx.ptr(tb), ctx.ptr(tab), ctx.ptr(g_out),
                                           None if root else ctx.ptr(p_out), count, ctx.stream()), "hb_fxp_carry_combine")
    if root:
        return g_out
    rows = (nodes + 1) // 2
    return g_out.view(rows, count, ctx.n_limbs), p_out.view(rows, count, ctx.n_limbs)


def div2m_finish(ctx, x, c, r1, carry, m, mode=MOD, out=None):
    """u = 1 - carry, a2 = (c mod 2^m) - r1 + 2^m u (fixedpoint.py:191-192).  mode MOD: a2 = [x mod 2^m] (x may be None);
    TRUNC: (x - a2) / 2^m (:210); NEG_TRUNC: its negation (:268, ltz when m = k - 1).  out may be any of the arrays."""
    _check_m(ctx.modulus, m)
    if mode not in (MOD, TRUNC, NEG_TRUNC) or isinstance(mode, bool):
        raise ValueError(f"mode must be MOD, TRUNC or NEG_TRUNC, got {mode!r}")
    c = ctx.elems(c, what="c")
    count = c.numel() // ctx.n_limbs
    if x is not None or mode != MOD:
        x = ctx.elems(x, count, what="x")
    r1, carry = ctx.elems(r1, count, what="r1"), ctx.elems(carry, count, what="carry")
    out = _elems_out(ctx, out, count)
    inv = _inv2m(ctx, m)
    ctx.check(ctx.lib.hb_fxp_div2m_finish(ctx.h, None if x is None else ctx.ptr(x), ctx.ptr(c), ctx.ptr(r1), ctx.ptr(carry), m, inv.ctypes.data, mode, ctx.ptr(out),
                                          count, ctx.stream()), "hb_fxp_div2m_finish")
    return out


# ---- protocols over an OpenCoalescer ---------------------------------------------------------------------------------------
def _triples(ctx, triples, rows, count):
    try:
        p, q, pq = triples
    except (TypeError, ValueError):
        raise ValueError("triples: expected (p, q, pq)") from None
    return tuple(_planes(ctx, v, rows, count, w)[0] for v, w in ((p, "triples p"), (q, "triples q"), (pq, "triples pq")))


async def trunc_pr(co, x, bits, k, m, kappa=KAPPA):
    """Shares of x / 2^m rounded up or down: floor(x / 2^m) + [(x mod 2^m) + r1 >= 2^m] (trunc_pr, fixedpoint.py:108-120).
    One open, two launches, k + kappa bit planes, no triple.  x and bits are left untouched."""
    ctx = co.ctx
    check_params(ctx.modulus, k, m, kappa)
    x = ctx.elems(x, what="x")
    bits, _ = _planes(ctx, bits, k + kappa, x.numel() // ctx.n_limbs, "bits")
    masked, r1 = trunc_mask(ctx, x, bits, k, m, kappa)
    c = await co.open_share_array(masked)
    return trunc_pr_finish(ctx, x, c, r1, m, out=r1)


async def _carry_tree(co, g, p, triples, m):
    """the root's g from the m + 1 leaf planes: one open and two launches a level"""
    ctx = co.ctx
    ta, tb, tab = triples
    nodes, off = m + 1, 0
    while True:
        root = nodes == 2
        n = _level_triples(nodes)
        a, b, ab = ta[off:off + n], tb[off:off + n], tab[off:off + n]
        masked = carry_mask(ctx, g, p, a, b, root=root)
        opened = await co.open_share_array(masked.view(masked.shape[0] * masked.shape[1], ctx.n_limbs))
        res = carry_combine(ctx, opened, g, p, a, b, ab, root=root)
        if root:
            return res
        g, p = res
        nodes, off = (nodes + 1) // 2, off + n


async def carry_tree(co, g, p, triples):
    """Shares of the g at the root of (g1, p1) o (g2, p2) = (g1 + p1 g2, p1 p2) over the leaf planes g, p, (2 <= nodes <= 257, count,
    limbs) each, most significant first: the level loop of get_carry_bit for leaves made elsewhere (share_comparison.less_than).
    carry_levels(nodes - 1) opens, carry_triples(nodes - 1) rows of triples."""
    ctx = co.ctx
    g, p, nodes, count, _, _ = _level(ctx, g, p, False)
    return await _carry_tree(co, g, p, _triples(ctx, triples, carry_triples(nodes - 1), count), nodes - 1)


async def get_carry_bit(co, c, r_bits, triples):
    """Shares of the carry bit of c2 + (2^m - 1 - r) + 1 = [c2 >= r] (get_carry_bit with the operands bit_ltl gives it,
    fixedpoint.py:131-150, :168-171): c public (its low m bits count), r_bits (m, count, limbs) the bit shares of r, least
    significant first.  carry_levels(m) opens, carry_triples(m) rows of triples."""
    ctx = co.ctx
    c = ctx.elems(c, what="c")
    count = c.numel() // ctx.n_limbs
    r_bits = ctx.elems(r_bits, what="r_bits")
    if r_bits.dim() != 3 or r_bits.shape[0] < 1 or r_bits.shape[1] != count:
        raise ValueError(f"r_bits: expected shape (m, {count}, {ctx.n_limbs}), got {tuple(r_bits.shape)}")
    m = r_bits.shape[0]
    _check_m(ctx.modulus, m)
    triples = _triples(ctx, triples, carry_triples(m), count)
    g, p = ltl_leaves(ctx, c, r_bits, m)
    return await _carry_tree(co, g, p, triples, m)


async def bit_ltl(co, c, r_bits, triples):
    """Shares of [c2 < r] = 1 - carry (bit_ltl, fixedpoint.py:163-172)"""
    carry = await get_carry_bit(co, c, r_bits, triples)
    return add(co.ctx, neg(co.ctx, carry, out=carry), 1, out=carry)


async def _div2m(co, x, bits, triples, k, m, kappa, mode):
    ctx = co.ctx
    check_params(ctx.modulus, k, m, kappa, full=True)
    x = ctx.elems(x, what="x")
    count = x.numel() // ctx.n_limbs
    bits, _ = _planes(ctx, bits, k + kappa, count, "bits")
    triples = _triples(ctx, triples, carry_triples(m), count)
    masked, r1 = trunc_mask(ctx, x, bits, k, m, kappa)
    c = await co.open_share_array(masked)
    g, p = ltl_leaves(ctx, c, bits, m)
    carry = await _carry_tree(co, g, p, triples, m)
    return div2m_finish(ctx, x, c, r1, carry, m, mode, out=carry)


async def div2m(co, x, bits, triples, k, m, kappa=KAPPA):
    """Shares of x mod 2^m (div2m, fixedpoint.py:184-193; the mathematical mod of the signed value).  1 + carry_levels(m) opens for
    any count; k + kappa bit planes and carry_triples(m) triples an element."""
    return await _div2m(co, x, bits, triples, k, m, kappa, MOD)


async def trunc(co, x, bits, triples, k, m, kappa=KAPPA):
    """Shares of floor(x / 2^m) (trunc, fixedpoint.py:208-211)"""
    return await _div2m(co, x, bits, triples, k, m, kappa, TRUNC)


async def ltz(co, x, bits, triples, k=K, kappa=KAPPA):
    """Shares of [x < 0] for signed k-bit x: -floor(x / 2^(k-1)) (FixedPoint.ltz, fixedpoint.py:266-268)"""
    _int(k, "k")
    return await _div2m(co, x, bits, triples, k, k - 1, kappa, NEG_TRUNC)


async def lt(co, x, y, bits, triples, k=K, kappa=KAPPA):
    """Shares of [x < y] = ltz(x - y) (FixedPoint.lt, fixedpoint.py:274-275)"""
    ctx = co.ctx
    check_params(ctx.modulus, _int(k, "k"), k - 1, kappa, full=True)
    x = ctx.elems(x, what="x")
    count = x.numel() // ctx.n_limbs
    y = ctx.elems(y, count, what="y")
    _planes(ctx, bits, k + kappa, count, "bits")
    _triples(ctx, triples, carry_triples(k - 1), count)
    return await ltz(co, sub(ctx, x, y), bits, triples, k, kappa)


async def mul(co, x, y, triple, bits, f=F, k=K, kappa=KAPPA):
    """Shares of the fixed-point product (FixedPoint.__mul__, fixedpoint.py:240-251): beaver_multiply_arrays with one triple an
    element, then trunc_pr(., 2 k, f).  Two batches; 2 k + kappa bit planes."""
    ctx = co.ctx
    check_params(ctx.modulus, 2 * _int(k, "k"), f, kappa)
    x = ctx.elems(x, what="x")
    count = x.numel() // ctx.n_limbs
    y = ctx.elems(y, count, what="y")
    try:
        p, q, pq = triple
    except (TypeError, ValueError):
        raise ValueError("triple: expected (p, q, pq)") from None
    triple = tuple(ctx.elems(v, count, what=w) for v, w in ((p, "triple p"), (q, "triple q"), (pq, "triple pq")))
    bits, _ = _planes(ctx, bits, 2 * k + kappa, count, "bits")
    xy = await beaver_multiply_arrays(co, x, y, triple)
    return await trunc_pr(co, xy, bits, 2 * k, f, kappa)


def matmul_width(k, inner):
    """bits of a sum of `inner` products of two signed k-bit values: 2 k + ceil(log2(inner))"""
    k, inner = _int(k, "k"), _int(inner, "inner")
    if inner < 1:
        raise ValueError(f"inner must be positive, got {inner}")
    return 2 * k + (inner - 1).bit_length()


async def matmul(co, X, Y, prep, bits, method, f=F, k=K, kappa=KAPPA):
    """Shares of the fixed-point matrix product: X (m, inner, limbs) [or (batch, m, inner, limbs)] times Y (inner, n, limbs), by
    linalg.double_sharing_matmul (method = linalg.DOUBLE_SHARING, prep = (r_t, r_2t)) or linalg.beaver_matmul (method = linalg.BEAVER,
    prep = (P, Q, PQ)) -- told apart by `method`, never guessed -- then ONE trunc_pr(., matmul_width(k, inner), f) on each of the m n
    outputs: one rounding an output instead of one a product, m n truncation opens instead of m inner n.  bits: (at least
    matmul_width(k, inner) + kappa, m n, limbs) planes.  check_params decides whether that width fits the modulus: ValueError if
    not, before anything is opened."""
    from .. import linalg

    ctx = co.ctx
    if method not in (linalg.DOUBLE_SHARING, linalg.BEAVER):
        raise ValueError(f"method: linalg.DOUBLE_SHARING or linalg.BEAVER, got {method!r}")
    X, Y = linalg._matrix(ctx, X, "X"), linalg._matrix(ctx, Y, "Y")
    if Y.dim() != X.dim() or Y.shape[-3] != X.shape[-2] or (X.dim() == 4 and Y.shape[0] != X.shape[0]):
        raise ValueError(f"Y: shape {tuple(Y.shape)} does not go with X {tuple(X.shape)}")
    inner = X.shape[-2]
    if inner < 1:
        raise ValueError("X: the inner dimension must not be empty")
    width = matmul_width(k, inner)
    check_params(ctx.modulus, width, f, kappa)
    shape = tuple(X.shape[:-2]) + (Y.shape[-2], ctx.n_limbs)
    count = 1
    for d in shape[:-1]:
        count *= d
    bits, _ = _planes(ctx, bits, width + kappa, count, "bits")
    try:
        n_prep = len(prep)
    except TypeError:
        n_prep = -1
    if n_prep != (2 if method == linalg.DOUBLE_SHARING else 3):
        raise ValueError("prep: expected (r_t, r_2t) for DOUBLE_SHARING, (P, Q, PQ) for BEAVER")
    if method == linalg.DOUBLE_SHARING:
        xy = await linalg.double_sharing_matmul(co, X, Y, prep[0], prep[1])
    else:
        xy = await linalg.beaver_matmul(co, X, Y, prep)
    return (await trunc_pr(co, xy.view(count, ctx.n_limbs), bits, width, f, kappa)).view(shape)


class FixedPointArray:
    """An array of shared fixed-point numbers (the reference's FixedPoint, fixedpoint.py:214-280, for `count` values at once).
    `shares`: a (count, limbs) tensor of shares of int(a * 2**f) mod p.  Preprocessing goes to the calls that spend it."""

    def __init__(self, co, shares, f=F, k=K, kappa=KAPPA):
        self.co, self.ctx = co, co.ctx
        self.shares = self.ctx.elems(shares, what="shares")
        self.f, self.k, self.kappa = f, k, kappa

    def _like(self, shares):
        return FixedPointArray(self.co, shares, self.f, self.k, self.kappa)

    def _other(self, x):
        if not isinstance(x, FixedPointArray):
            raise NotImplementedError
        return x.shares

    def __add__(self, x):
        return self._like(add(self.ctx, self.shares, self._other(x)))

    def __sub__(self, x):
        return self._like(sub(self.ctx, self.shares, self._other(x)))

    def neg(self):
        return self._like(neg(self.ctx, self.shares))

    async def mul(self, x, triple, bits):
        return self._like(await mul(self.co, self.shares, self._other(x), triple, bits, self.f, self.k, self.kappa))

    async def matmul(self, x, rows, inner, cols, prep, bits, method):
        """self as a (rows, inner) matrix times x as an (inner, cols) matrix, row-major -> (rows cols) values (fixedpoint.matmul)"""
        L = self.ctx.n_limbs
        if self.shares.numel() != rows * inner * L or self._other(x).numel() != inner * cols * L:
            raise ValueError(f"matmul: expected {rows * inner} and {inner * cols} values, got {self.shares.numel() // L} and {x.shares.numel() // L}")
        out = await matmul(self.co, self.shares.view(rows, inner, L), x.shares.view(inner, cols, L), prep, bits, method, self.f, self.k, self.kappa)
        return self._like(out.view(rows * cols, L))

    async def div(self, x, bits):
        """by a public number: times to_fixed_point_repr(1 / x), then trunc_pr (FixedPoint.div, fixedpoint.py:277-280; a public
        factor needs no triple)"""
        if not isinstance(x, (float, int)) or isinstance(x, bool):
            raise NotImplementedError
        prod = _ew_mul(self.ctx, self.shares, to_fixed_point_repr(1.0 / x, self.f) % self.ctx.modulus)
        return self._like(await trunc_pr(self.co, prod, bits, 2 * self.k, self.f, self.kappa))

    async def divide(self, x, bits, triples, signed=True, theta=None):
        """by a SHARED divisor (fixedpoint_division.div): x != 0 and |self / x| < 2^(k-2-f); signed=False: the caller promises 0 < x"""
        from .fixedpoint_division import div

        return self._like(await div(self.co, self.shares, self._other(x), bits, triples, self.f, self.k, self.kappa, theta, signed))

    async def reciprocal(self, bits, triples, signed=True, theta=None):
        """1 / self (fixedpoint_division.reciprocal)"""
        from .fixedpoint_division import reciprocal

        return self._like(await reciprocal(self.co, self.shares, bits, triples, self.f, self.k, self.kappa, theta, signed))

    async def sqrt(self, bits, triples, theta=None):
        """the square root of a non-negative array (fixedpoint_sqrt.sqrt): 0 <= self < 2^(k-1-f)"""
        from .fixedpoint_sqrt import sqrt

        return self._like(await sqrt(self.co, self.shares, bits, triples, self.f, self.k, self.kappa, theta))

    async def rsqrt(self, bits, triples, theta=None):
        """1 / sqrt(self) (fixedpoint_sqrt.rsqrt): 0 < self < 2^(k-1-f) and 1 / sqrt(self) < 2^(k-2-f)"""
        from .fixedpoint_sqrt import rsqrt

        return self._like(await rsqrt(self.co, self.shares, bits, triples, self.f, self.k, self.kappa, theta))

    async def exp2(self, bits, triples, demux_triples, g=None):
        """2^self (fixedpoint_exp.exp2): a result below 2^(k-2-f); below -f it is exactly 0"""
        from .fixedpoint_exp import exp2

        return self._like(await exp2(self.co, self.shares, bits, triples, demux_triples, self.f, self.k, self.kappa, g))

    async def exp(self, bits, triples, demux_triples, g=None):
        """e^self (fixedpoint_exp.exp): a result below 2^(k-2-f)"""
        from .fixedpoint_exp import exp

        return self._like(await exp(self.co, self.shares, bits, triples, demux_triples, self.f, self.k, self.kappa, g))

    async def log2(self, bits, triples):
        """log2(self) (fixedpoint_log.log2): 0 < self < 2^(k-1-f)"""
        from .fixedpoint_log import log2

        return self._like(await log2(self.co, self.shares, bits, triples, self.f, self.k, self.kappa))

    async def log(self, bits, triples):
        """ln(self) (fixedpoint_log.log): 0 < self < 2^(k-1-f)"""
        from .fixedpoint_log import log

        return self._like(await log(self.co, self.shares, bits, triples, self.f, self.k, self.kappa))

    async def sincos_turns(self, bits, triples, demux_triples, g=None, want=("sin", "cos")):
        """sin and cos of self TURNS (fixedpoint_trig.sincos_turns): a tuple in the order of `want`, for any value"""
        from .fixedpoint_trig import sincos_turns

        return tuple(self._like(v) for v in await sincos_turns(self.co, self.shares, bits, triples, demux_triples, self.f, self.k, self.kappa, g, want))

    async def sincos(self, bits, triples, demux_triples, g=None, want=("sin", "cos")):
        """sin and cos of self radians (fixedpoint_trig.sincos): a tuple in the order of `want`, for any value"""
        from .fixedpoint_trig import sincos

        return tuple(self._like(v) for v in await sincos(self.co, self.shares, bits, triples, demux_triples, self.f, self.k, self.kappa, g, want))

    async def sin(self, bits, triples, demux_triples, g=None):
        """sin(self) (fixedpoint_trig.sin), self in radians: the preprocessing of want = ("sin",)"""
        return (await self.sincos(bits, triples, demux_triples, g, ("sin",)))[0]

    async def cos(self, bits, triples, demux_triples, g=None):
        """cos(self) (fixedpoint_trig.cos), self in radians: the preprocessing of want = ("cos",)"""
        return (await self.sincos(bits, triples, demux_triples, g, ("cos",)))[0]

    async def atan2(self, x, bits, triples, turns=False):
        """atan2(self, x) in (-pi, pi] (fixedpoint_atan.atan2), self the ordinate; turns=True: in (-1/2, 1/2], sincos_turns' unit"""
        from .fixedpoint_atan import atan2

        return self._like(await atan2(self.co, self.shares, self._other(x), bits, triples, self.f, self.k, self.kappa, turns))

    async def atan(self, bits, triples, turns=False):
        """atan(self) (fixedpoint_atan.atan): atan2 against the public 1, the same preprocessing"""
        from .fixedpoint_atan import atan

        return self._like(await atan(self.co, self.shares, bits, triples, self.f, self.k, self.kappa, turns))

    async def ltz(self, bits, triples):
        """-> a (count, limbs) tensor of shares of [a < 0]"""
        return await ltz(self.co, self.shares, bits, triples, self.k, self.kappa)

    async def lt(self, x, bits, triples):
        """-> shares of [self < x]"""
        return await lt(self.co, self.shares, self._other(x), bits, triples, self.k, self.kappa)

    async def sort(self, plan, bits, carry_triples, swap_triples, payload=None):
        """-> (sorted, payload): every one of the plan's `batch` arrays of n values sorted ascending (progs/sorting.py), `payload`,
        a (plan.width - 1, count, limbs) tensor of columns (None for plan.width == 1), moved with the values.  The values must lie in
        [-2^(k-2-f), 2^(k-2-f)); equal values come out in the network's order, not the input's.  self and payload are left untouched."""
        from . import sorting

        if not isinstance(plan, sorting.SortPlan) or (plan.k, plan.kappa) != (self.k, self.kappa):
            raise ValueError(f"plan: expected a SortPlan with (k, kappa) = ({self.k}, {self.kappa})")
        L, count = self.ctx.n_limbs, self.shares.numel() // self.ctx.n_limbs
        if count != plan.batch * plan.n:
            raise ValueError(f"plan: {plan.batch} arrays of {plan.n} rows, but the array holds {count} values")
        if (payload is None) != (plan.width == 1):
            raise ValueError(f"payload: plan.width = {plan.width} takes {plan.width - 1} columns")
        columns = [self.shares.view(1, count, L)]
        if payload is not None:
            payload = self.ctx.elems(payload, what="payload")
            if payload.dim() != 3 or payload.shape[0] != plan.width - 1 or payload.shape[1] != count:
                raise ValueError(f"payload: expected shape ({plan.width - 1}, {count}, {L}), got {tuple(payload.shape)}")
            columns.append(payload)
        table = await sorting.sort(self.co, self.ctx.torch.cat(columns), plan, bits, carry_triples, swap_triples)
        return self._like(table[0]), (table[1:] if payload is not None else None)

    async def bits(self, m, bits, triples):
        """-> an (m, count, limbs) tensor of shares of the low m bits of int(a * 2**f), least significant first
        (bit_decomposition.bit_decompose)"""
        from .bit_decomposition import bit_decompose

        return await bit_decompose(self.co, self.shares, bits, triples, self.k, m, self.kappa)

    async def lookup(self, table, m, bits, bd_triples, demux_triples):
        """-> a (W, count, limbs) tensor of shares of row int(a * 2**f) of the public table (N, W), N <= 2^m, for a non-negative array
        below 2^m (an index at or above N gives 0): bit_decomposition.bit_decompose, then demux.demux, then demux.lookup"""
        from . import demux
        from .bit_decomposition import bit_decompose

        planes = await bit_decompose(self.co, self.shares, bits, bd_triples, self.k, m, self.kappa)
        return demux.lookup(self.ctx, await demux.demux(self.co, planes, demux_triples), table)

    async def open(self):
        """-> list[float], decoded with the signed rule of FixedPoint.open (fixedpoint.py:253-257)"""
        opened = await self.co.open_share_array(self.shares)
        return [from_fixed_point_repr(v, self.ctx.modulus, self.k, self.f) for v in self.ctx.download_ints(opened)]

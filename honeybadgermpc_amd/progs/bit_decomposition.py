"""
Bit decomposition of share arrays on the device (csrc/hb_bd.hip): shares of the low m bits of a signed k-bit value, Catrina and de
Hoogh's BitDec ("Improved Primitives for Secure Multiparty Integer Computation", SCN 2010) on the masks of progs/fixedpoint.py.  The
reference has no bit decomposition; the pin is the mathematics: bits_model on Python ints, and the same steps composed from
share_arithmetic.

x is a signed k-bit value held as a residue and 0 < m <= k - 1 (check_params(p, k, m, kappa, full=True); for all k bits of a k-bit
value call with k + 1).  trunc_mask opens c = x + 2^(k-1) + r1 + 2^m r2, which cannot wrap, and 2^(k-1) = 0 mod 2^m, so the bits wanted
are those of (c2 - r1) mod 2^m = c2 + (2^m - 1 - r1) + 1 mod 2^m with c2 = c mod 2^m public and b_i the bit shares of r1.  div2m runs
the carry tree of that sum and keeps its root; here a Sklansky parallel prefix network keeps every carry at the same depth:

    leaves      a_i = bit i of c2 is public: (g_i, p_i) = (1 - b_i, b_i) for a_i = 1, (0, 1 - b_i) for a_i = 0; no product.  N = m - 1
                planes (bits 0 .. m - 2: the carry out of bit m - 1 is never used), LEAST significant first; the carry-in 1 is folded
                into plane 0: (g_0 + p_0, 0).
    level l     node y = 0, 1, ... is plane j = ((y >> l) << (l + 1)) | (1 << l) | (y & ((1 << l) - 1)) while j <= N - 1, its partner
                q = ((j >> l) << l) - 1, and (g_j, p_j) <- (g_j + p_j g_q, p_j p_q).  Bit l of q is clear: q is no node of level l, so the
                level updates g and p in place.  The nodes y < 2^l lie in the block that starts at plane 0, whose p is 0 after the
                fold: they are g-only, one product, p never written.  prefix_levels(m) = ceil(log2 N) levels, none for N <= 1; after
                the last one plane i holds the carry into bit i + 1.
    sum bits    s_0 = a_0 xor b_0, a select; s_i = p_i + C_i - 2 p_i C_i with p_i the LEAF's propagate (recomputed from c and plane i
                of `bits`) and C_i = g of plane i - 1: m - 1 products in one batch.

Triple rows, from row 0: level by level; within a level the G = min(2^l, active) g-only nodes take rows 0 .. G - 1 (p_j g_q), full
node y rows G + 2 (y - G) (p_j g_q) and G + 2 (y - G) + 1 (p_j p_q); after the levels the m - 1 sum products, bit i at row
prefix_triples(m) + i - 1.  The first factor of a triple masks p (p_j or the leaf's p_i), the second g_q, p_q or C_i.

Host functions:

    prefix_levels(m)                                    ceil(log2(m - 1)), 0 for m <= 2
    prefix_nodes(n_planes, level)                       -> [(j, q, g_only)]: the wiring
    prefix_level_triples(m, level), prefix_triples(m)   triples of one level, of all levels
    bit_triples(m) = prefix_triples(m) + m - 1          triples an element the decomposition consumes (m = 64: 373)
    bit_opens(m)   = 1 + prefix_levels(m) + (m >= 2)    batches it opens (m = 64: 8)
    bits_model(x, p, k, m)                              the low m bits of the signed value of residue x, least significant first
    difference_bits_model(c, r, m)                      the bits of ((c mod 2^m) - r) mod 2^m

Tensor level, one launch each on torch's current stream, nothing synchronises:

    sub_leaves(ctx, c, bits, m)                         -> (g, p), (m - 1, count, limbs) each
    prefix_mask(ctx, g, p, level, ta, tb)               the level's array to open, (2 triples, count, limbs)
    prefix_combine(ctx, opened, g, p, level, ta, tb, tab)   IN PLACE -> (g, p)
    sum_mask(ctx, c, bits, g, m, ta, tb)                the sum step's array to open, (2 (m - 1), count, limbs)
    sum_combine(ctx, opened, c, bits, g, m, ta, tb, tab)    -> the bit planes, (m, count, limbs)

Protocol level, coroutines over an OpenCoalescer:

    async difference_bits(co, c, r_bits, triples)       bit_opens(m) - 1 opens      the bits of (c - r) mod 2^m, c public
    async bit_decompose(co, x, bits, triples, k, m, kappa)   bit_opens(m) opens     the low m bits of x

Both take 1 + 2 prefix_levels(m) + 2 launches after the open of c, for any count.
"""
from .fixedpoint import KAPPA, _check_m, _int, _planes, _planes_out, _triples, check_params, trunc_mask

MAX_PLANES = 256


# ---- host functions ------------------------------------------------------------------------------------------------------
def _m(m):
    if _int(m, "m") < 1:
        raise ValueError(f"m must be positive, got {m}")
    return m


def prefix_levels(m):
    """levels of the prefix network over m - 1 planes: ceil(log2(m - 1)), none for m <= 2"""
    return max(_m(m) - 2, 0).bit_length()


def prefix_nodes(n_planes, level):
    """-> [(j, q, g_only)] for y = 0, 1, ...: the planes level `level` updates, their partners, and whether only g is computed"""
    n, l = _int(n_planes, "n_planes"), _int(level, "level")
    if n < 0 or l < 0:
        raise ValueError(f"n_planes and level must not be negative, got {n}, {l}")
    nodes, y = [], 0
    while True:
        j = ((y >> l) << (l + 1)) | (1 << l) | (y & ((1 << l) - 1))
        if j > n - 1:
            return nodes
        nodes.append((j, ((j >> l) << l) - 1, y < (1 << l)))
        y += 1


def prefix_level_triples(m, level):
    """triples an element level `level` consumes: one a g-only node, two a full node"""
    if not 0 <= _int(level, "level") < prefix_levels(m):
        raise ValueError(f"level must be in 0 .. {prefix_levels(m) - 1}, got {level}")
    return sum(1 if g_only else 2 for _, _, g_only in prefix_nodes(m - 1, level))


def prefix_triples(m):
    return sum(prefix_level_triples(m, l) for l in range(prefix_levels(m)))


def bit_triples(m):
    """triples an element bit_decompose consumes: the network's, and one a bit above bit 0"""
    return prefix_triples(m) + m - 1


def bit_opens(m):
    """batches bit_decompose opens: c, one a level, and the sum products"""
    return 1 + prefix_levels(m) + (1 if m >= 2 else 0)


def bits_model(x, p, k, m):
    """the low m bits, least significant first, of the signed k-bit value the residue x stands for (two's complement); what
    bit_decompose's planes open to, whatever masks were dealt"""
    k, m = _int(k, "k"), _int(m, "m")
    if not 0 < m <= k - 1:
        raise ValueError(f"needs 0 < m <= k - 1, got m = {m}, k = {k}")
    x = int(x) % p
    v = x - p if x >= p - (1 << (k - 1)) else x
    if not -(1 << (k - 1)) <= v < 1 << (k - 1):
        raise ValueError(f"x is no signed {k}-bit value")
    return [(v >> i) & 1 for i in range(m)]


def difference_bits_model(c, r, m):
    """the bits of ((c mod 2^m) - r) mod 2^m, least significant first"""
    d = (int(c) % (1 << _m(m)) - int(r)) % (1 << m)
    return [(d >> i) & 1 for i in range(m)]


# ---- tensor level ----------------------------------------------------------------------------------------------------------
def _check_bd_m(p, m):
    _check_m(p, m)
    if m - 1 > MAX_PLANES:
        raise ValueError(f"at most {MAX_PLANES} planes, got m - 1 = {m - 1}")


def _network(ctx, g, p, level, in_place=False):
    """g, p (N, count, limbs) with N >= 2 planes -> contiguous g, p, m, count, the level's triples"""
    if in_place:
        for v, w in ((g, "g"), (p, "p")):
            if isinstance(v, ctx.torch.Tensor) and not v.is_contiguous():
                raise ValueError(f"{w}: must be contiguous (it is updated in place)")
    g = ctx.elems(g, what="g")
    if g.dim() != 3 or g.shape[0] < 2:
        raise ValueError(f"g: expected shape (planes >= 2, count, {ctx.n_limbs}), got {tuple(g.shape)}")
    n, count = g.shape[0], g.shape[1]
    _check_bd_m(ctx.modulus, n + 1)
    p, _ = _planes(ctx, p, n, count, "p", exact=True)
    return g, p, n + 1, count, prefix_level_triples(n + 1, level)


def sub_leaves(ctx, c, bits, m, out=None):
    """-> (g, p), (m - 1, count, limbs) each: the leaves of the prefix network of c2 + (2^m - 1 - r) + 1, c2 = c mod 2^m public, r the
    number whose bit shares are planes 0 .. m - 2 of `bits`, least significant bit first, the carry-in folded into plane 0.  No
    triple, no open.  out: a pair (g, p) of arrays of their own.  m = 1: no plane, nothing is launched."""
    _check_bd_m(ctx.modulus, m)
    c = ctx.elems(c, what="c")
    count = c.numel() // ctx.n_limbs
    bits, _ = _planes(ctx, bits, m - 1, count, "bits")
    try:
        og, op = (None, None) if out is None else out
    except (TypeError, ValueError):
        raise ValueError("out: expected a pair of tensors") from None
    g, p = _planes_out(ctx, og, m - 1, count, "out g"), _planes_out(ctx, op, m - 1, count, "out p")
    ctx.check(ctx.lib.hb_bd_leaves(ctx.h, ctx.ptr(c), ctx.ptr(bits), m, ctx.ptr(g), ctx.ptr(p), count, ctx.stream()), "hb_bd_leaves")
    return g.view(m - 1, count, ctx.n_limbs), p.view(m - 1, count, ctx.n_limbs)


def prefix_mask(ctx, g, p, level, ta, tb, out=None):
    """One level of the prefix network before its open.  g, p (m - 1, count, limbs); ta, tb this party's shares of the first and second
    factors of the level's triples, (prefix_level_triples(m, level), count, limbs).  -> (2 triples, count, limbs): rows 2t, 2t + 1 =
    p_j - ta[t], (g_q | p_q) - tb[t], ONE array to open."""
    g, p, m, count, triples = _network(ctx, g, p, level)
    ta, _ = _planes(ctx, ta, triples, count, "ta", exact=True)
    tb, _ = _planes(ctx, tb, triples, count, "tb", exact=True)
    out = _planes_out(ctx, out, 2 * triples, count)
    ctx.check(ctx.lib.hb_bd_prefix_mask(ctx.h, ctx.ptr(g), ctx.ptr(p), m, level, ctx.ptr(ta), ctx.ptr(tb), ctx.ptr(out), count, ctx.stream()), "hb_bd_prefix_mask")
    return out.view(2 * triples, count, ctx.n_limbs)


def prefix_combine(ctx, opened, g, p, level, ta, tb, tab):
    """One level of the prefix network after its open, IN PLACE: (g_j, p_j) <- (g_j + [p_j g_q], [p_j p_q]) at the level's nodes (g alone
    at the g-only ones); every other plane is left untouched.  g and p must be contiguous.  -> (g, p)"""
    g, p, m, count, triples = _network(ctx, g, p, level, in_place=True)
    opened = ctx.elems(opened, 2 * triples * count, what="opened")                       # (2 triples, count, limbs), or flat as an open returns it
    ta, tb, tab = (_planes(ctx, v, triples, count, w, exact=True)[0] for v, w in ((ta, "ta"), (tb, "tb"), (tab, "tab")))
    ctx.check(ctx.lib.hb_bd_prefix_combine(ctx.h, ctx.ptr(opened), ctx.ptr(g), ctx.ptr(p), m, level, ctx.ptr(ta), ctx.ptr(tb), ctx.ptr(tab), count, ctx.stream()),
              "hb_bd_prefix_combine")
    return g, p


def _sum_args(ctx, c, bits, g, m):
    _check_bd_m(ctx.modulus, m)
    c = ctx.elems(c, what="c")
    count = c.numel() // ctx.n_limbs
    bits, _ = _planes(ctx, bits, m, count, "bits")
    g, _ = _planes(ctx, g, m - 1, count, "g", exact=True)
    return c, bits, g, count


def sum_mask(ctx, c, bits, g, m, ta, tb, out=None):
    """The sum step before its open: g (m - 1, count, limbs) the carries after the last level, ta, tb (m - 1, count, limbs).
    -> (2 (m - 1), count, limbs): rows 2t, 2t + 1 = p_{t+1} - ta[t], g[t] - tb[t], p_i the leaf's propagate of bit i."""
    c, bits, g, count = _sum_args(ctx, c, bits, g, m)
    ta, _ = _planes(ctx, ta, m - 1, count, "ta", exact=True)
    tb, _ = _planes(ctx, tb, m - 1, count, "tb", exact=True)
    out = _planes_out(ctx, out, 2 * (m - 1), count)
    ctx.check(ctx.lib.hb_bd_sum_mask(ctx.h, ctx.ptr(c), ctx.ptr(bits), ctx.ptr(g), m, ctx.ptr(ta), ctx.ptr(tb), ctx.ptr(out), count, ctx.stream()), "hb_bd_sum_mask")
    return out.view(2 * (m - 1), count, ctx.n_limbs)


def sum_combine(ctx, opened, c, bits, g, m, ta, tb, tab, out=None):
    """The sum step after its open -> (m, count, limbs): plane 0 = a_0 xor b_0, plane i = p_i + g[i - 1] - 2 [p_i g[i - 1]].
    out: an array of its own."""
    c, bits, g, count = _sum_args(ctx, c, bits, g, m)
    opened = ctx.elems(opened, 2 * (m - 1) * count, what="opened")
    ta, tb, tab = (_planes(ctx, v, m - 1, count, w, exact=True)[0] for v, w in ((ta, "ta"), (tb, "tb"), (tab, "tab")))
    out = _planes_out(ctx, out, m, count)
    ctx.check(ctx.lib.hb_bd_sum_combine(ctx.h, ctx.ptr(opened), ctx.ptr(c), ctx.ptr(bits), ctx.ptr(g), m, ctx.ptr(ta), ctx.ptr(tb), ctx.ptr(tab), ctx.ptr(out), count,
                                        ctx.stream()), "hb_bd_sum_combine")
    return out.view(m, count, ctx.n_limbs)


# ---- protocols over an OpenCoalescer ---------------------------------------------------------------------------------------
async def _difference_bits(co, c, r_bits, triples, m):
    """c, r_bits (at least m planes) and triples (at least bit_triples(m) rows) checked by the caller"""
    ctx = co.ctx
    ta, tb, tab = triples
    g, p = sub_leaves(ctx, c, r_bits, m)
    off = 0
    for level in range(prefix_levels(m)):
        n = prefix_level_triples(m, level)
        a, b, ab = ta[off:off + n], tb[off:off + n], tab[off:off + n]
        masked = prefix_mask(ctx, g, p, level, a, b)
        opened = await co.open_share_array(masked.view(masked.shape[0] * masked.shape[1], ctx.n_limbs))
        prefix_combine(ctx, opened, g, p, level, a, b, ab)
        off += n
    n = m - 1
    a, b, ab = ta[off:off + n], tb[off:off + n], tab[off:off + n]
    if n == 0:
        return sum_combine(ctx, a, c, r_bits, g, m, a, b, ab)                            # one bit: a select, nothing to open
    masked = sum_mask(ctx, c, r_bits, g, m, a, b)
    opened = await co.open_share_array(masked.view(masked.shape[0] * masked.shape[1], ctx.n_limbs))
    return sum_combine(ctx, opened, c, r_bits, g, m, a, b, ab)


async def difference_bits(co, c, r_bits, triples):
    """Shares of the bits of ((c mod 2^m) - r) mod 2^m as (m, count, limbs) planes, least significant first: c public, r_bits (m, count,
    limbs) the bit shares of r.  The analogue of get_carry_bit that keeps every carry.  bit_opens(m) - 1 opens, bit_triples(m) rows
    of triples.  ValueError before anything is opened."""
    ctx = co.ctx
    c = ctx.elems(c, what="c")
    count = c.numel() // ctx.n_limbs
    r_bits = ctx.elems(r_bits, what="r_bits")
    if r_bits.dim() != 3 or r_bits.shape[0] < 1 or r_bits.shape[1] != count:
        raise ValueError(f"r_bits: expected shape (m, {count}, {ctx.n_limbs}), got {tuple(r_bits.shape)}")
    m = r_bits.shape[0]
    _check_bd_m(ctx.modulus, m)
    triples = _triples(ctx, triples, bit_triples(m), count)
    return await _difference_bits(co, c, r_bits, triples, m)


async def bit_decompose(co, x, bits, triples, k, m, kappa=KAPPA):
    """Shares of the low m bits (two's complement) of the signed k-bit values x as (m, count, limbs) planes, least significant first.
    bit_opens(m) opens for any count; k + kappa bit planes and bit_triples(m) triples an element.  x, bits and triples are left
    untouched.  ValueError before anything is opened."""
    ctx = co.ctx
    check_params(ctx.modulus, k, m, kappa, full=True)
    _check_bd_m(ctx.modulus, m)
    x = ctx.elems(x, what="x")
    count = x.numel() // ctx.n_limbs
    bits, _ = _planes(ctx, bits, k + kappa, count, "bits")
    triples = _triples(ctx, triples, bit_triples(m), count)
    masked, _ = trunc_mask(ctx, x, bits, k, m, kappa)
    c = await co.open_share_array(masked)
    return await _difference_bits(co, c, bits, triples, m)

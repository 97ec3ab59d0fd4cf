"""
Comparison of shared values on the device: the two mixins of the reference's progs/mixins/share_comparison.py for whole share arrays, on
the (count, limbs) int64 tensors the rest of the package speaks.  Equality (:9-80, the probabilistic Legendre-symbol test behind
Share.__eq__) is csrc/hb_eq.hip and the first half of this module; LessThan (:83-212, Reistad's comparison behind Share.__lt__) is
csrc/hb_lt.hip and the second half, below under "Less-than".  (progs.fixedpoint.lt is the ordered comparison of SIGNED k-bit values
with k + kappa + 2 <= bit_length(p); less_than compares any two residues below (p - 1) / 2.)

For a pair with diff = x - y, test bit j draws a bit share [b] and two random shares [r], [rp], opens

    c = diff r + _b rp^2,   _b = nr - (nr - 1) b in {nr, 1},   nr a public quadratic non-residue      share_comparison.py:31-48

and maps L = legendre(c) to a factor that is affine in [b]; the product of kappa factors is the result (:65-80).  Two finishing maps:

    BIT (default)   (1 - L) / 2 + L [b]                        1 where the bit says "equal", else 0.  Equal inputs -> every factor 1 ->
                                                               the result opens to exactly 1; unequal inputs -> each factor is 0 with
                                                               probability 1 / 2 -> the result opens to 0 but with probability 2^-kappa
    REFERENCE       L (nr + L) / 2 - (L (nr - 1) / 2) [b]      the reference's (L / 2) (_b + L), :61: with nr = 5 a factor is 1, -2, 3 or 0,
                                                               so equal inputs open to (-2)^(number of b = 0) -- nonzero, not 1 -- and an
                                                               unequal pair's factor is 0 with probability 1 / 4 only

Host functions:

    legendre_mod_p(a, p)                                 share_comparison.py:16-27
    smallest_nonresidue(p)                               5 for the BLS12-381 scalar field (the reference's constant, :35-37), 2 for 2^64 - 59
    check_nonresidue(p, nr)                              ValueError unless legendre(nr) == -1
    test_bit_model(diff, b, r, rp, p, nr, mode)          -> (c, factor)                                            :31-61
    equal_model(diff, bits, rs, rps, p, nr, mode)        the product of the factors                                :65-80
    equality_triples(kappa) = 4 kappa - 1                triples an element
    equality_opens(kappa)   = 3 + ceil(log2 kappa)       coalesced batches for any count

Preprocessing is handed in as tensors of planes, one row a test bit: `bits` (at least kappa, count, limbs); `rands` (at least 2 kappa,
count, limbs), rows [0, kappa) the r, rows [kappa, 2 kappa) the rp; `triples = (p, q, pq)`, each (at least 4 kappa - 1, count, limbs),
rows [0, kappa) for diff r, [kappa, 2 kappa) for rp rp, [2 kappa, 3 kappa) for _b rp^2, and the remaining kappa - 1 for the product
tree, level by level: a level over k planes multiplies planes [0, k // 2) by planes [k // 2, 2 (k // 2)) with k // 2 rows and moves an
odd last plane up unchanged.

Tensor level, one launch each on torch's current stream, nothing synchronises:

    legendre(ctx, a)                                     -> int8 tensor (count,) in {-1, 0, 1}                     :16-27
    eq_mask1(ctx, x, y, r, rp, pa, qa, pb, qb)           -> (4, rows, count, limbs): diff - pa, r - qa, rp - pb, rp - qb, ONE array to open
    eq_mid(ctx, opened, ta, tb, bits, pc, qc, nr)        -> ((2, rows, count, limbs): _b - pc, [rp^2] - qc; (rows, count, limbs): [diff r])
    eq_cshare(ctx, opened2, dr, tc)                      -> (rows, count, limbs): [c], the third array to open      :46
    eq_finish(ctx, c, bits, mode, nr)                    -> (factor planes, zero_rows): int32 (rows,), 1 where a c of the row is 0   :57-61

Protocol level, coroutines over an OpenCoalescer (every party runs the same coroutine, so the opens meet batch for batch):

    async equal(co, x, y, bits, rands, triples, kappa=32, nr=None, mode=BIT)    shares of [x == y]      :65-80
    async is_zero(co, x, bits, rands, triples, kappa=32, nr=None, mode=BIT)     shares of [x == 0]

3 opens and 4 launches for the test bits, then ceil(log2 kappa) opens for the product tree (beaver_multiply_arrays on plane slices).

A zero c.  The reference draws the test bit again (:54-59).  Here eq_finish flags the rows in which some c is 0, the coroutine reads
the flags back (one small copy: every party sees the same opened c, so all agree) and runs the flagged rows again, in one further
pass of the three opens, on the spare rows the caller supplied beyond the counts above: pass by pass and in order, f flagged rows
take the next f rows of `bits`, the next 2 f rows of `rands` (f for r, then f for rp) and the next 3 f rows of each triple plane (f for
diff r, f for rp rp, f for _b rp^2).  Without enough spares: exceptions.PreprocessingExhausted.  Over a 255-bit field this does not
happen by chance.

Less-than.  L = bit_length(p), z = a - b.  The protocol opens c = 2 z + r with r a dealt random residue whose bit shares r_0 .. r_{L-1}
are dealt with it (the reference's get_share_bits), and [a < b] = c_0 xor r_0 xor [r > c] (:206-212).  c_i is public, so the terms of
the reference's x = sum_i r_i (1 - c_i) prod_{j>i} (1 + (r_j xor c_j)) (_compute_x, :137-163) are affine in [r_i]: x is the g at the
root of fixedpoint's carry tree, (g1, p1) o (g2, p2) = (g1 + p1 g2, p1 p2), over leaves that cost no triple.  Two modes:

    DIRECT (default)  leaves c_i = 0 -> (r_i, 1 - r_i), c_i = 1 -> (0, r_i): the root's g is [r > c] itself, a bit; one product for the
                      last xor.  2 L - 2 triples, 2 + ceil(log2 L) opens.
    REFERENCE         leaves c_i = 0 -> (r_i, 1 + r_i), c_i = 1 -> (0, 2 - r_i): the root's g is the reference's x, whose least
                      significant bit is [r > c].  The reference's _extract_lsb (:167-202) follows: a second dealt s with bit
                      shares, d = s + x opened, [d_0] by a four-way select on s_{L-1}, s_{L-2}, x_0 = s_0 xor d_0.  xor is a symmetric
                      polynomial, so (c_0 xor r_0) xor (s_0 xor d_0) is evaluated as ((c_0 xor r_0) xor s_0) xor d_0 and opens to the
                      same value: the products u s_0 and s_1 s_2 do not wait for d, and their masked operands travel in d's open.
                      2 L triples, 3 + ceil(log2 L) opens.  It opens what the reference opens: c, d and the result.

The reference computes x by a chain of L - 1 dependent products and L more, one open each: about 2 L = 510 triples and more than 255
rounds a comparison over the BLS12-381 scalar field, against 508 triples and 10 rounds (DIRECT) here.

    less_than_model(a, b, r, s, p, mode)                 -> {"c", "x" | "w", "d" (REFERENCE), "out"}: the reference line by line on ints
    less_than_triples(L, mode) = 2 L - 2 | 2 L           triples an element
    less_than_opens(L, mode)   = 2 | 3 + ceil(log2 L)    coalesced batches for any count: 10 | 11 over BLS12-381, 8 | 9 over 64 bits

    lt_mask(ctx, a, b, r)                                -> 2 (a - b) + r, the array to open (b None: 2 a + r)
    lt_leaves(ctx, c, r_bits, mode)                      -> (g, p), (L, count, limbs) each, most significant bit first; no product
    lt_xor_mask(ctx, c, r0, w, pa, qa)                   DIRECT -> (u, (2, count, limbs): u - pa, w - qa); u = c_0 xor r_0, r0 = r_bits[0]
    lt_dmask(ctx, c, r0, x, s, s_bits, pa, qa, pb, qb)   REFERENCE -> (u, (5, count, limbs): s + x, u - pa, s_0 - qa, s_1 - pb, s_2 - qb)
    lt_mid(ctx, opened, u, s_bits, ta, tb, pc, qc)       REFERENCE -> (v, d_0, (2, count, limbs): v - pc, d_0 - qc); v = u xor s_0
    lt_xor_finish(ctx, opened, u, v, t)                  -> u + v - 2 [u v]

    async less_than(co, a, b, r, r_bits, triples, s=None, s_bits=None, mode=DIRECT)     shares of [a < b]      :206-212

r, s are (count, limbs); r_bits, s_bits (L, count, limbs), least significant bit first; `triples = (p, q, pq)`, each (at least
less_than_triples, count, limbs): rows [0, 2 L - 3) are the tree's, in the order progs.fixedpoint documents for L leaves; then DIRECT
takes one row for the last xor, REFERENCE three: u s_0, s_1 s_2, the last xor.
"""
from ._capi import HB_EQ_BIT, HB_EQ_REFERENCE, HB_LT_DIRECT, HB_LT_REFERENCE
from .exceptions import PreprocessingExhausted
from .progs.fixedpoint import carry_tree
from .share_arithmetic import beaver_multiply_arrays

KAPPA = 32
BIT, REFERENCE = HB_EQ_BIT, HB_EQ_REFERENCE
DIRECT = HB_LT_DIRECT
assert HB_LT_REFERENCE == REFERENCE


# ---- host functions ------------------------------------------------------------------------------------------------------
def legendre_mod_p(a, p):
    """the Legendre symbol of a modulo the odd prime p: 1, -1 or 0 (share_comparison.py:16-27)"""
    if p % 2 != 1:
        raise ValueError("the modulus must be odd")
    b = pow(a % p, (p - 1) // 2, p)
    if b == 1:
        return 1
    if b == p - 1:
        return -1
    return 0


def smallest_nonresidue(p):
    """the smallest quadratic non-residue modulo the odd prime p"""
    for z in range(2, p):
        if legendre_mod_p(z, p) == -1:
            return z
    raise ValueError(f"no quadratic non-residue below {p}")


def check_nonresidue(p, nr):
    """ValueError unless nr is a quadratic non-residue modulo p"""
    if not isinstance(nr, int) or isinstance(nr, bool):
        raise ValueError(f"nr must be an integer, got {nr!r}")
    if legendre_mod_p(nr, p) != -1:
        raise ValueError(f"nr = {nr} is not a quadratic non-residue modulo the field's prime")


def _check_mode(mode):
    if mode not in (BIT, REFERENCE) or isinstance(mode, bool):
        raise ValueError(f"mode must be BIT or REFERENCE, got {mode!r}")


def test_bit_model(diff, b, r, rp, p, nr, mode=BIT):
    """one test bit on Python ints with the dealt b, r, rp -> (c, factor): the opened c (share_comparison.py:46) and what the factor
    share holds (:61, or the BIT map); a zero c gives factor None (the bit is drawn again)"""
    _check_mode(mode)
    if b not in (0, 1):
        raise ValueError(f"b must be 0 or 1, got {b!r}")
    _b = (nr - (nr - 1) * b) % p
    c = (diff * r + _b * rp * rp) % p
    leg = legendre_mod_p(c, p)
    if leg == 0:
        return c, None
    if mode == BIT:
        return c, ((1 - leg) * pow(2, -1, p) + leg * b) % p
    return c, leg * pow(2, -1, p) * (_b + leg) % p


test_bit_model.__test__ = False            # a model OF a test bit, not a test


def equal_model(diff, bits, rs, rps, p, nr, mode=BIT):
    """what equal's result opens to for one element: the product of the factors of the test bits (share_comparison.py:70-80); None
    if some c is zero"""
    out = 1
    for b, r, rp in zip(bits, rs, rps):
        _, f = test_bit_model(diff, b, r, rp, p, nr, mode)
        if f is None:
            return None
        out = out * f % p
    return out


def _kappa(kappa):
    if not isinstance(kappa, int) or isinstance(kappa, bool) or kappa < 1:
        raise ValueError(f"kappa must be a positive integer, got {kappa!r}")
    return kappa


def equality_triples(kappa):
    """triples an element: three a test bit and kappa - 1 for the product tree"""
    return 4 * _kappa(kappa) - 1


def equality_opens(kappa):
    """coalesced batches of one equal(): three for the test bits and ceil(log2 kappa) for the product tree"""
    return 3 + (_kappa(kappa) - 1).bit_length()


# ---- tensor level ----------------------------------------------------------------------------------------------------------
MAX_ROWS = 4096


def _planes(ctx, t, rows, count, what, exact=True):
    """a (rows, count, limbs) tensor (at least `rows` rows unless exact) -> contiguous"""
    t = ctx.elems(t, what=what)
    if t.dim() != 3 or t.shape[1] != count or (t.shape[0] != rows if exact else t.shape[0] < rows):
        raise ValueError(f"{what}: expected shape ({'' if exact else 'at least '}{rows}, {count}, {ctx.n_limbs}), got {tuple(t.shape)}")
    return t


def _rows_of(ctx, t, what):
    t = ctx.elems(t, what=what)
    if t.dim() != 3 or not 1 <= t.shape[0] <= MAX_ROWS:
        raise ValueError(f"{what}: expected shape (1 <= rows <= {MAX_ROWS}, count, {ctx.n_limbs}), got {tuple(t.shape)}")
    return t, t.shape[0], t.shape[1]


def _triple(ctx, triple, rows, count, what):
    try:
        p, q, pq = triple
    except (TypeError, ValueError):
        raise ValueError(f"{what}: expected (p, q, pq)") from None
    return tuple(_planes(ctx, v, rows, count, f"{what} {w}") for v, w in ((p, "p"), (q, "q"), (pq, "pq")))


def _new(ctx, *shape):
    return ctx.torch.empty(shape + (ctx.n_limbs,), dtype=ctx.torch.int64, device=ctx.tdev)


def _nr(ctx, nr):
    """nr (None: the smallest non-residue) checked -> (nr, its host element)"""
    if nr is None:
        nr = _nr_cache.get(ctx.modulus)
        if nr is None:
            nr = _nr_cache[ctx.modulus] = smallest_nonresidue(ctx.modulus)
    else:
        check_nonresidue(ctx.modulus, nr)
    return nr % ctx.modulus, ctx.host_elems([nr % ctx.modulus])


_nr_cache = {}


def legendre(ctx, a):
    """the Legendre symbol of every element: -> int8 tensor (count,) in {-1, 0, 1} (share_comparison.py:16-27).  One launch: a
    sliding-window chain for the exponent (p - 1) / 2 whose schedule is the same for every lane."""
    a = ctx.elems(a, what="a")
    count = a.numel() // ctx.n_limbs
    out = ctx.torch.empty((count,), dtype=ctx.torch.int8, device=ctx.tdev)
    ctx.check(ctx.lib.hb_legendre(ctx.h, ctx.ptr(a), ctx.ptr(out), count, ctx.stream()), "hb_legendre")
    return out


def eq_mask1(ctx, x, y, r, rp, pa, qa, pb, qb):
    """diff = x - y (y None: diff = x) against `rows` test bits: r, rp and the first factors (pa, pb) and second factors (qa, qb) of
    the triples for diff r and rp rp, (rows, count, limbs) each.  -> (4, rows, count, limbs) = diff - pa, r - qa, rp - pb, rp - qb, ONE
    array to open.  The inputs are left untouched."""
    r, rows, count = _rows_of(ctx, r, "r")
    x = ctx.elems(x, count, what="x")
    if y is not None:
        y = ctx.elems(y, count, what="y")
    rp, pa, qa, pb, qb = (_planes(ctx, v, rows, count, w) for v, w in ((rp, "rp"), (pa, "pa"), (qa, "qa"), (pb, "pb"), (qb, "qb")))
    out = _new(ctx, 4, rows, count)
    ctx.check(ctx.lib.hb_eq_mask1(ctx.h, ctx.ptr(x), None if y is None else ctx.ptr(y), ctx.ptr(r), ctx.ptr(rp), ctx.ptr(pa), ctx.ptr(qa), ctx.ptr(pb), ctx.ptr(qb),
                                  ctx.ptr(out), rows, count, ctx.stream()), "hb_eq_mask1")
    return out


def eq_mid(ctx, opened, ta, tb, bits, pc, qc, nr=None):
    """After the first open.  opened: the array of eq_mask1, opened ((4, rows, count, limbs), or flat as an open returns it);
    ta, tb = (p, q, pq): the triples for diff r and rp rp; bits the bit planes; pc, qc the factors of the triples for _b rp^2.
    -> (masked2, dr): (2, rows, count, limbs) = _b - pc, [rp^2] - qc, the next array to open, and (rows, count, limbs) = [diff r]."""
    bits, rows, count = _rows_of(ctx, bits, "bits")
    opened = ctx.elems(opened, 4 * rows * count, what="opened")
    ta, tb = _triple(ctx, ta, rows, count, "ta"), _triple(ctx, tb, rows, count, "tb")
    pc, qc = _planes(ctx, pc, rows, count, "pc"), _planes(ctx, qc, rows, count, "qc")
    _, nr_h = _nr(ctx, nr)
    masked2, dr = _new(ctx, 2, rows, count), _new(ctx, rows, count)
    ctx.check(ctx.lib.hb_eq_mid(ctx.h, ctx.ptr(opened), *(ctx.ptr(v) for v in ta), *(ctx.ptr(v) for v in tb), ctx.ptr(bits), ctx.ptr(pc), ctx.ptr(qc), nr_h.ctypes.data,
                                ctx.ptr(masked2), ctx.ptr(dr), rows, count, ctx.stream()), "hb_eq_mid")
    return masked2, dr


def eq_cshare(ctx, opened2, dr, tc):
    """After the second open: -> (rows, count, limbs) = [c] = [diff r] + [_b rp^2], the third array to open
    (share_comparison.py:46).  opened2: masked2 opened; tc = (p, q, pq): the triples for _b rp^2."""
    dr, rows, count = _rows_of(ctx, dr, "dr")
    opened2 = ctx.elems(opened2, 2 * rows * count, what="opened2")
    tc = _triple(ctx, tc, rows, count, "tc")
    out = _new(ctx, rows, count)
    ctx.check(ctx.lib.hb_eq_cshare(ctx.h, ctx.ptr(opened2), ctx.ptr(dr), *(ctx.ptr(v) for v in tc), ctx.ptr(out), rows, count, ctx.stream()), "hb_eq_cshare")
    return out


def eq_finish(ctx, c, bits, mode=BIT, nr=None):
    """After the third open: the Legendre symbol of every opened c and the mode's affine map of the bit share, in one launch.
    -> (factors (rows, count, limbs), zero_rows): an int32 tensor (rows,) holding 1 where some c of the row is 0 (the factor written
    there is 0) once the stream has got there.  Nothing synchronises."""
    _check_mode(mode)
    bits, rows, count = _rows_of(ctx, bits, "bits")
    c = ctx.elems(c, rows * count, what="c")
    _, nr_h = _nr(ctx, nr)
    out = _new(ctx, rows, count)
    zero_rows = ctx.torch.zeros((rows,), dtype=ctx.torch.int32, device=ctx.tdev)
    ctx.check(ctx.lib.hb_eq_finish(ctx.h, ctx.ptr(c), ctx.ptr(bits), mode, nr_h.ctypes.data, ctx.ptr(out), ctx.ptr(zero_rows), rows, count, ctx.stream()), "hb_eq_finish")
    return out, zero_rows


# ---- protocols over an OpenCoalescer ---------------------------------------------------------------------------------------
async def _test_bits(co, x, y, bits, r, rp, ta, tb, tc, nr, mode):
    """the factor planes of `rows` test bits: three opens, four launches"""
    ctx = co.ctx
    rows, count = bits.shape[0], bits.shape[1]
    flat = lambda t: t.view(-1, ctx.n_limbs)                                               # noqa: E731
    masked = eq_mask1(ctx, x, y, r, rp, ta[0], ta[1], tb[0], tb[1])
    opened = await co.open_share_array(flat(masked))
    masked2, dr = eq_mid(ctx, opened, ta, tb, bits, tc[0], tc[1], nr)
    opened2 = await co.open_share_array(flat(masked2))
    c = await co.open_share_array(flat(eq_cshare(ctx, opened2, dr, tc)))
    factors, zero_rows = eq_finish(ctx, c, bits, mode, nr)
    return factors.view(rows, count, ctx.n_limbs), zero_rows


async def equal(co, x, y, bits, rands, triples, kappa=KAPPA, nr=None, mode=BIT):
    """Shares of [x == y] element by element (Equality._prog, share_comparison.py:65-80): 1 (mode REFERENCE: a nonzero value) for an
    equal pair, 0 for an unequal one but with probability 2^-kappa (REFERENCE: (3 / 4)^kappa).  equality_opens(kappa) batches for any
    count; kappa rows of bits, 2 kappa of rands and equality_triples(kappa) of triples an element, and spare rows for test bits
    whose c opens to zero (see the module's header).  nr: the public non-residue, None for the field's smallest.  y None: [x == 0].
    The inputs are left untouched."""
    ctx = co.ctx
    _check_mode(mode)
    _kappa(kappa)
    if kappa > MAX_ROWS:
        raise ValueError(f"kappa: at most {MAX_ROWS}, got {kappa}")
    nr, _ = _nr(ctx, nr)
    x = ctx.elems(x, what="x")
    count = x.numel() // ctx.n_limbs
    if y is not None:
        y = ctx.elems(y, count, what="y")
    need_t = equality_triples(kappa)
    bits = _planes(ctx, bits, kappa, count, "bits", exact=False)
    rands = _planes(ctx, rands, 2 * kappa, count, "rands", exact=False)
    try:
        tp, tq, tpq = triples
    except (TypeError, ValueError):
        raise ValueError("triples: expected (p, q, pq)") from None
    trip = tuple(_planes(ctx, v, need_t, count, w, exact=False) for v, w in ((tp, "triples p"), (tq, "triples q"), (tpq, "triples pq")))
    if count == 0:
        return ctx.empty(0)
    rows = lambda lo, n: tuple(v[lo:lo + n] for v in trip)                                  # noqa: E731
    factors, zero_rows = await _test_bits(co, x, y, bits[:kappa], rands[:kappa], rands[kappa:2 * kappa], rows(0, kappa), rows(kappa, kappa), rows(2 * kappa, kappa), nr, mode)
    used = 0                                                                               # spare test bits spent so far
    while True:
        again = [j for j, z in enumerate(zero_rows.tolist()) if z]
        if not again:
            break
        f = len(again)
        spare = min(bits.shape[0] - kappa, (rands.shape[0] - 2 * kappa) // 2, min(v.shape[0] - need_t for v in trip) // 3) - used
        if f > spare:
            raise PreprocessingExhausted(f"equal: the opened c of test bits {again} is zero and {max(spare, 0)} spare rows of preprocessing are left for {f}")
        b0, r0, t0 = kappa + used, 2 * kappa + 2 * used, need_t + 3 * used
        redo, zero_rows = await _test_bits(co, x, y, bits[b0:b0 + f], rands[r0:r0 + f], rands[r0 + f:r0 + 2 * f], rows(t0, f), rows(t0 + f, f), rows(t0 + 2 * f, f), nr, mode)
        idx = ctx.torch.tensor(again, device=ctx.tdev)
        factors.index_copy_(0, idx, redo)
        flags = ctx.torch.zeros((kappa,), dtype=ctx.torch.int32, device=ctx.tdev)            # a row that is zero again keeps its place
        zero_rows = flags.index_copy_(0, idx, zero_rows)
        used += f
    # the product of the kappa planes: lower half times upper half, an odd last plane moves up
    k, off = kappa, need_t - (kappa - 1)
    while k > 1:
        h = k // 2
        prod = await beaver_multiply_arrays(co, factors[:h].reshape(h * count, ctx.n_limbs), factors[h:2 * h].reshape(h * count, ctx.n_limbs),
                                            tuple(v[off:off + h].reshape(h * count, ctx.n_limbs) for v in trip))
        prod = prod.view(h, count, ctx.n_limbs)
        factors = ctx.torch.cat((prod, factors[2 * h:k])) if k & 1 else prod
        k, off = h + (k & 1), off + h
    return factors[0]


async def is_zero(co, x, bits, rands, triples, kappa=KAPPA, nr=None, mode=BIT):
    """Shares of [x == 0]: equal() with no second operand"""
    return await equal(co, x, None, bits, rands, triples, kappa, nr, mode)


# ---- less-than: host functions ---------------------------------------------------------------------------------------------
def _check_lt_mode(mode):
    if mode not in (DIRECT, REFERENCE) or isinstance(mode, bool):
        raise ValueError(f"mode must be DIRECT or REFERENCE, got {mode!r}")


def _bit_length(L):
    if not isinstance(L, int) or isinstance(L, bool) or L < 2:
        raise ValueError(f"L must be an integer of at least 2, got {L!r}")
    return L


def less_than_triples(L, mode=DIRECT):
    """triples an element: 2 L - 3 for the tree over L leaves, then one (DIRECT) or three (REFERENCE)"""
    _check_lt_mode(mode)
    return 2 * _bit_length(L) - (2 if mode == DIRECT else 0)


def less_than_opens(L, mode=DIRECT):
    """coalesced batches of one less_than(): c, ceil(log2 L) tree levels, (REFERENCE: d,) the last xor"""
    _check_lt_mode(mode)
    return (2 if mode == DIRECT else 3) + (_bit_length(L) - 1).bit_length()


def less_than_model(a, b, r, s, p, mode=DIRECT):
    """what less_than opens to for one pair, on Python ints with the dealt r (and s) as inputs: the reference's _prog line by line
    (share_comparison.py:117-212), no tree.  -> {"c", "x", "d", "out"} in REFERENCE, {"c", "w", "out"} in DIRECT, which ignores s:
    w = r_i at the most significant bit where r_i != c_i, that is [r > c] (:140-143)."""
    _check_lt_mode(mode)
    L = p.bit_length()
    xor = lambda u, v: (u + v - 2 * u * v) % p                                              # noqa: E731    _xor_bits, :110-113
    bits = lambda v: [(v >> i) & 1 for i in range(L)]                                       # noqa: E731    least significant first
    # _transform_comparison, :117-133
    z = (a - b) % p
    c = (2 * z + r) % p
    r_bits, c_bits = bits(r % p), bits(c)
    lead = xor(c_bits[0], r_bits[0])
    if mode == DIRECT:
        w = next((rb for rb, cb in zip(reversed(r_bits), reversed(c_bits)) if rb != cb), 0)
        return {"c": c, "w": w, "out": xor(lead, w)}
    # _compute_x, :137-163
    power_bits = [(1 + xor(rb, cb)) % p for rb, cb in zip(r_bits[1:], c_bits[1:])]
    powers = [1]
    for pb in reversed(power_bits):
        powers.insert(0, pb * powers[0] % p)
    x = 0
    for r_i, c_i, pw in zip(r_bits, c_bits, powers):
        x = (x + r_i * (1 - c_i) * pw) % p
    # _extract_lsb, :167-202
    s_bits = bits(s % p)
    d = (s + x) % p
    s_0, s_1, s_2 = s_bits[0], s_bits[L - 1], s_bits[L - 2]
    s_prod = s_1 * s_2
    d0 = d & 1
    d_xor_1 = d0 ^ (d < (1 << (L - 1)))
    d_xor_2 = d0 ^ (d < (1 << (L - 2)))
    d_xor_12 = d0 ^ (d < ((1 << (L - 1)) + (1 << (L - 2))))
    d_0 = ((1 - s_1 - s_2 + s_prod) * d0 + (s_2 - s_prod) * d_xor_2 + (s_1 - s_prod) * d_xor_1 + s_prod * d_xor_12) % p
    x_0 = xor(s_0, d_0)
    # _prog, :206-212
    return {"c": c, "x": x, "d": d, "out": xor(lead, x_0)}


# ---- less-than: tensor level -----------------------------------------------------------------------------------------------
def _lt_elems(ctx, count, *named):
    return tuple(ctx.elems(v, count, what=w) for v, w in named)


def _lt_bits(ctx, t, count, what):
    L = ctx.modulus.bit_length()
    return _planes(ctx, t, L, count, what), L


def _lt_triple(ctx, t, count, what):
    try:
        p, q, pq = t
    except (TypeError, ValueError):
        raise ValueError(f"{what}: expected (p, q, pq)") from None
    return _lt_elems(ctx, count, (p, f"{what} p"), (q, f"{what} q"), (pq, f"{what} pq"))


def lt_mask(ctx, a, b, r):
    """-> 2 (a - b) + r, the array to open (share_comparison.py:122-127); b None: 2 a + r.  The inputs are left untouched."""
    a = ctx.elems(a, what="a")
    count = a.numel() // ctx.n_limbs
    if b is not None:
        b = ctx.elems(b, count, what="b")
    r = ctx.elems(r, count, what="r")
    out = ctx.empty(count)
    ctx.check(ctx.lib.hb_lt_mask(ctx.h, ctx.ptr(a), None if b is None else ctx.ptr(b), ctx.ptr(r), ctx.ptr(out), count, ctx.stream()), "hb_lt_mask")
    return out


def lt_leaves(ctx, c, r_bits, mode=DIRECT):
    """-> (g, p), (L, count, limbs) each: the leaves of the tree for the opened c against the bit shares r_bits (L, count, limbs), least
    significant first; the leaves are ordered most significant bit first.  No triple, no open: a public bit selects."""
    _check_lt_mode(mode)
    c = ctx.elems(c, what="c")
    count = c.numel() // ctx.n_limbs
    r_bits, L = _lt_bits(ctx, r_bits, count, "r_bits")
    g, p = _new(ctx, L, count), _new(ctx, L, count)
    ctx.check(ctx.lib.hb_lt_leaves(ctx.h, ctx.ptr(c), ctx.ptr(r_bits), L, mode, ctx.ptr(g), ctx.ptr(p), count, ctx.stream()), "hb_lt_leaves")
    return g, p


def lt_xor_mask(ctx, c, r0, w, pa, qa):
    """DIRECT, after the tree: w = [r > c], r0 = r_bits[0]; pa, qa the factors of the last triple.  -> (u, masked): u = c_0 xor r_0
    (count, limbs) and (2, count, limbs) = u - pa, w - qa, the array to open."""
    c = ctx.elems(c, what="c")
    count = c.numel() // ctx.n_limbs
    r0, w, pa, qa = _lt_elems(ctx, count, (r0, "r0"), (w, "w"), (pa, "pa"), (qa, "qa"))
    u, masked = ctx.empty(count), _new(ctx, 2, count)
    ctx.check(ctx.lib.hb_lt_xor_mask(ctx.h, ctx.ptr(c), ctx.ptr(r0), ctx.ptr(w), ctx.ptr(pa), ctx.ptr(qa), ctx.ptr(u), ctx.ptr(masked), count, ctx.stream()), "hb_lt_xor_mask")
    return u, masked


def lt_dmask(ctx, c, r0, x, s, s_bits, pa, qa, pb, qb):
    """REFERENCE, after the tree: x the root's g, s and s_bits (L, count, limbs) the second mask; (pa, qa), (pb, qb) the factors of the
    triples for u s_0 and s_1 s_2.  -> (u, masked): (5, count, limbs) = s + x, u - pa, s_0 - qa, s_1 - pb, s_2 - qb with s_0, s_1, s_2
    planes 0, L - 1, L - 2 of s_bits (share_comparison.py:178-182), ONE array to open."""
    c = ctx.elems(c, what="c")
    count = c.numel() // ctx.n_limbs
    r0, x, s, pa, qa, pb, qb = _lt_elems(ctx, count, (r0, "r0"), (x, "x"), (s, "s"), (pa, "pa"), (qa, "qa"), (pb, "pb"), (qb, "qb"))
    s_bits, L = _lt_bits(ctx, s_bits, count, "s_bits")
    u, masked = ctx.empty(count), _new(ctx, 5, count)
    ctx.check(ctx.lib.hb_lt_dmask(ctx.h, ctx.ptr(c), ctx.ptr(r0), ctx.ptr(x), ctx.ptr(s), ctx.ptr(s_bits), L, ctx.ptr(pa), ctx.ptr(qa), ctx.ptr(pb), ctx.ptr(qb),
                                  ctx.ptr(u), ctx.ptr(masked), count, ctx.stream()), "hb_lt_dmask")
    return u, masked


def lt_mid(ctx, opened, u, s_bits, ta, tb, pc, qc):
    """REFERENCE, after d's open.  opened: the array of lt_dmask, opened ((5, count, limbs), or flat as an open returns it); ta, tb =
    (p, q, pq): the triples for u s_0 and s_1 s_2; pc, qc the factors of the last triple.  -> (v, d_0, masked): v = u xor s_0, [d_0] by
    the reference's select (share_comparison.py:186-199) and (2, count, limbs) = v - pc, d_0 - qc, the array to open."""
    u = ctx.elems(u, what="u")
    count = u.numel() // ctx.n_limbs
    opened = ctx.elems(opened, 5 * count, what="opened")
    s_bits, L = _lt_bits(ctx, s_bits, count, "s_bits")
    ta, tb = _lt_triple(ctx, ta, count, "ta"), _lt_triple(ctx, tb, count, "tb")
    pc, qc = _lt_elems(ctx, count, (pc, "pc"), (qc, "qc"))
    v, d0, masked = ctx.empty(count), ctx.empty(count), _new(ctx, 2, count)
    ctx.check(ctx.lib.hb_lt_mid(ctx.h, ctx.ptr(opened), ctx.ptr(u), ctx.ptr(s_bits), L, *(ctx.ptr(t) for t in ta), *(ctx.ptr(t) for t in tb), ctx.ptr(pc), ctx.ptr(qc),
                                ctx.ptr(v), ctx.ptr(d0), ctx.ptr(masked), count, ctx.stream()), "hb_lt_mid")
    return v, d0, masked


def lt_xor_finish(ctx, opened, u, v, t):
    """After the last open: -> u + v - 2 [u v] (share_comparison.py:110-113).  opened: (2, count, limbs) = u - p, v - q opened (or
    flat); t = (p, q, pq) the triple.  REFERENCE hands in lt_mid's v and d_0."""
    u = ctx.elems(u, what="u")
    count = u.numel() // ctx.n_limbs
    v, = _lt_elems(ctx, count, (v, "v"))
    opened = ctx.elems(opened, 2 * count, what="opened")
    t = _lt_triple(ctx, t, count, "t")
    out = ctx.empty(count)
    ctx.check(ctx.lib.hb_lt_xor_finish(ctx.h, ctx.ptr(opened), ctx.ptr(u), ctx.ptr(v), *(ctx.ptr(w) for w in t), ctx.ptr(out), count, ctx.stream()), "hb_lt_xor_finish")
    return out


# ---- less-than: the protocol -----------------------------------------------------------------------------------------------
async def less_than(co, a, b, r, r_bits, triples, s=None, s_bits=None, mode=DIRECT):
    """Shares of [a < b] element by element (LessThan._prog, share_comparison.py:206-212): 1 where a < b, else 0.

    Precondition: a, b < (p - 1) / 2, as the reference requires (:85, :95).  For other inputs the result is what less_than_model
    gives, which is wrong for about a quarter of the pairs drawn from the whole field.  The only other exception is a mask within
    about 2^(number of bits in which the operands differ) of the wrap -- r so close to p that c = 2 (a - b) + r wraps differently
    from the bits dealt, or (REFERENCE) s so close that s + x does -- which is negligible over a 255-bit field.

    r (count, limbs) and r_bits (L, count, limbs), least significant first, L = bit_length(p): a dealt random residue and its bit
    shares; REFERENCE needs a second pair s, s_bits (ValueError without them; DIRECT ignores them).  less_than_opens(L, mode)
    batches for any count, less_than_triples(L, mode) rows of triples an element (see the module's header for their order).
    b None: z = a, that is [a < 0] read as the reference reads it: 1 where a >= (p + 1) / 2.  The inputs are left untouched."""
    ctx = co.ctx
    _check_lt_mode(mode)
    if mode == REFERENCE and (s is None or s_bits is None):
        raise ValueError("mode REFERENCE needs the second mask: s and s_bits")
    a = ctx.elems(a, what="a")
    count = a.numel() // ctx.n_limbs
    if b is not None:
        b = ctx.elems(b, count, what="b")
    r = ctx.elems(r, count, what="r")
    r_bits, L = _lt_bits(ctx, r_bits, count, "r_bits")
    if mode == REFERENCE:
        s = ctx.elems(s, count, what="s")
        s_bits, _ = _lt_bits(ctx, s_bits, count, "s_bits")
    try:
        tp, tq, tpq = triples
    except (TypeError, ValueError):
        raise ValueError("triples: expected (p, q, pq)") from None
    trip = tuple(_planes(ctx, v, less_than_triples(L, mode), count, w, exact=False) for v, w in ((tp, "triples p"), (tq, "triples q"), (tpq, "triples pq")))
    if count == 0:
        return ctx.empty(0)
    nt = 2 * L - 3
    row = lambda k: tuple(v[k] for v in trip)                                               # noqa: E731
    c = await co.open_share_array(lt_mask(ctx, a, b, r))
    g, p = lt_leaves(ctx, c, r_bits, mode)
    root = await carry_tree(co, g, p, tuple(v[:nt] for v in trip))
    if mode == DIRECT:
        t = row(nt)
        u, masked = lt_xor_mask(ctx, c, r_bits[0], root, t[0], t[1])
        opened = await co.open_share_array(masked.view(2 * count, ctx.n_limbs))
        return lt_xor_finish(ctx, opened, u, root, t)
    ta, tb, tc = row(nt), row(nt + 1), row(nt + 2)
    u, masked = lt_dmask(ctx, c, r_bits[0], root, s, s_bits, ta[0], ta[1], tb[0], tb[1])
    opened = await co.open_share_array(masked.view(5 * count, ctx.n_limbs))
    v, d0, masked2 = lt_mid(ctx, opened, u, s_bits, ta, tb, tc[0], tc[1])
    opened2 = await co.open_share_array(masked2.view(2 * count, ctx.n_limbs))
    return lt_xor_finish(ctx, opened2, v, d0, tc)

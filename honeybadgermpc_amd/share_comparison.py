"""
Equality of shared values on the device (csrc/hb_eq.hip): the reference's Equality mixin, progs/mixins/share_comparison.py:9-80 -- the
probabilistic Legendre-symbol test behind Share.__eq__ -- for whole share arrays, on the (count, limbs) int64 tensors the rest of the
package speaks.  (LessThan, :83-212, is not here: progs.fixedpoint.lt is the ordered comparison.)

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
"""
from ._capi import HB_EQ_BIT, HB_EQ_REFERENCE
from .exceptions import PreprocessingExhausted
from .share_arithmetic import beaver_multiply_arrays

KAPPA = 32
BIT, REFERENCE = HB_EQ_BIT, HB_EQ_REFERENCE


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

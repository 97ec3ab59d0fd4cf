"""
Oblivious sort of shared values on the device (csrc/hb_sort.hip): Batcher's merge exchange (Knuth, The Art of Computer Programming
5.2.2, Algorithm M) over the comparison of progs/fixedpoint.py, on the (count, limbs) int64 tensors the rest of the package speaks.

The network.  With t = ceil(log2 n), every p = 2^(t-1), ..., 2, 1 gives the layer (p, r, d) = (p, 0, p) and then, for
q = 2^(t-1), 2^(t-2), ..., 2 p, the layers (p, p, q - p).  A layer compares rows (i, i + d) for every i < n - d with i & p == r and
leaves the smaller key at i.  It works for any n; every layer is a matching (bit log2(p) of i + d differs from that of i).  The
comparators of a layer are a dense prefix e = 0 .. cnt - 1: with a = log2 p,

    lo(e) = ((e >> a) << (a + 1)) | (e & (p - 1)) | r,    hi(e) = lo(e) + d

and, with m = max(n - d, 0) and full, rem = divmod(m, 2 p), cnt = full p + min(rem, p) for r = 0 and full p + max(rem - p, 0) for
r = p.  So a kernel takes (a, r, d, cnt) and reads no index list, and the arrays a layer opens have no holes.

    layers(n)                   -> [(a, r, d, cnt)] in order; [] for n < 2
    comparators(n)              -> [[(lo, hi), ...]] a layer
    sort_model(table, n, k)     the host model on Python ints: table = `width` columns of batch n values, column 0 the key.  A pair is
                                swapped, every column of it, where key_lo >= key_hi: ties swap, as in the protocol, so the model
                                fixes the payload's order bit for bit.  Keys lie in [-2^(k-2), 2^(k-2)): the difference of two keys
                                is a signed k-bit value, fixedpoint.lt's contract.  ValueError otherwise.
    SortPlan(n, batch, width, k, kappa)   the layout of a whole sort of `batch` independent arrays of n rows and `width` columns

The table is ONE tensor (width, batch n, limbs): column-major planes, each array contiguous inside a plane.  Slot s of a layer is
comparator s % cnt of array s // cnt; a layer has slots_l = batch cnt_l of them.  Preprocessing is one flat (elements, limbs) buffer a
kind, laid out layer after layer; layer l's block is a contiguous (rows, slots_l, limbs) array, so fixedpoint.ltl_leaves, carry_mask
and carry_combine run on views of it unchanged:

    kind "bits"    k + kappa rows a slot            this party's shares of the random bits of the comparison's mask
    kind "carry"   carry_triples(k - 1) = 2 k - 3   one buffer each for the first factors, second factors and products
    kind "swap"    width rows a slot                the same three: one triple a slot and column

Tensor level, one launch each on torch's current stream, nothing synchronises; layer = (a, r, d, cnt):

    cmp_mask(ctx, table, layer, n, batch, bits, k, kappa, out=, r1_out=)   -> (masked, r1): key[lo] - key[hi] under fixedpoint's mask
    swap_mask(ctx, table, layer, n, batch, c, r1, carry, p, q, k, out=)    -> (2 width, slots, limbs): rows 2w, 2w + 1 = u - p_w,
                                                                           (T[w][lo] - T[w][hi]) - q_w with u = 1 - [key_lo < key_hi]
    swap_finish(ctx, table, layer, n, batch, opened, p, q, pq)             T[w][lo] -= m, T[w][hi] += m in place, m = [u (lo - hi)]

Protocol level, coroutines over an OpenCoalescer (every party runs the same coroutine, so the opens meet batch for batch):

    async compare_exchange_layer(co, table, plan, l, bits, carry, swap)    cmp_mask, open, ltl_leaves, the carry tree's levels
                                                                           (carry_mask / open / carry_combine), swap_mask, open,
                                                                           swap_finish: 2 + carry_levels(k - 1) opens for any slots
    async sort(co, table, plan, bits, carry_triples, swap_triples)         every layer in order; sorts in place, returns the table

Ascending by key.  Descending order is a flip of the returned views (table.flip(1) for one array) and needs no kernel.  The sort
is not stable.
"""
from . import fixedpoint as fx

MAX_WIDTH = 256
KINDS = ("bits", "carry", "swap")


def _int(v, what, least=None):
    if not isinstance(v, int) or isinstance(v, bool):
        raise ValueError(f"{what} must be an integer, got {v!r}")
    if least is not None and v < least:
        raise ValueError(f"{what} must be at least {least}, got {v}")
    return v


# ---- the network (host) ------------------------------------------------------------------------------------------------------
def _count(n, p, r, d):
    """indices i < n - d with i & p == r"""
    full, rem = divmod(max(n - d, 0), 2 * p)
    return full * p + (min(rem, p) if r == 0 else max(rem - p, 0))


def layers(n):
    """[(a, r, d, cnt)] of the merge exchange over n rows, in order; a layer without a comparator is dropped"""
    n = _int(n, "n", 0)
    out = []
    if n < 2:
        return out
    t = (n - 1).bit_length()
    for a in range(t - 1, -1, -1):
        p = 1 << a
        steps = [(0, p)] + [(p, (1 << j) - p) for j in range(t - 1, a, -1)]
        for r, d in steps:
            cnt = _count(n, p, r, d)
            if cnt:
                out.append((a, r, d, cnt))
    return out


def _lo(e, a, r):
    return ((e >> a) << (a + 1)) | (e & ((1 << a) - 1)) | r


def comparators(n):
    """[[(lo, hi), ...]]: the pairs of every layer of layers(n), comparator e at position e"""
    return [[(_lo(e, a, r), _lo(e, a, r) + d) for e in range(cnt)] for a, r, d, cnt in layers(n)]


def sort_model(table, n, k):
    """The network on Python ints.  table: `width` columns (lists) of batch n values each, column 0 the key; every array of n rows
    is sorted by itself.  -> a new table.  A pair swaps where key_lo >= key_hi."""
    n, k = _int(n, "n", 0), _int(k, "k", 2)
    cols = [list(c) for c in table]
    if not cols or any(len(c) != len(cols[0]) for c in cols):
        raise ValueError("table: expected columns of one length, at least one")
    if (n == 0 and cols[0]) or (n and len(cols[0]) % n):
        raise ValueError(f"table: {len(cols[0])} rows are not whole arrays of {n}")
    bound = 1 << (k - 2)
    for v in cols[0]:
        if not isinstance(v, int) or isinstance(v, bool) or not -bound <= v < bound:
            raise ValueError(f"key {v!r} is outside [-2^(k-2), 2^(k-2)) for k = {k}")
    pairs = comparators(n)
    for base in range(0, len(cols[0]), n or 1):
        for layer in pairs:
            for lo, hi in layer:
                if cols[0][base + lo] >= cols[0][base + hi]:
                    for c in cols:
                        c[base + lo], c[base + hi] = c[base + hi], c[base + lo]
    return cols


class SortPlan:
    """The layout of a sort of `batch` arrays of n rows and `width` columns with (k, kappa) comparisons.

    layers [(a, r, d, cnt)], slots [batch cnt] a layer, n_layers, total_slots; opens = n_layers (2 + carry_levels(k - 1));
    bit_rows = k + kappa, carry_rows = carry_triples(k - 1), swap_rows = width: rows a slot of each kind.  size(kind) = elements of
    the kind's flat buffer, offset(kind, l) = where layer l's block begins, views(buf, kind, l) = that block as (rows, slots_l, limbs)."""

    def __init__(self, n, batch, width, k, kappa):
        self.n, self.batch, self.width = _int(n, "n", 0), _int(batch, "batch", 1), _int(width, "width", 1)
        self.k, self.kappa = _int(k, "k", 2), _int(kappa, "kappa", 0)
        if width > MAX_WIDTH:
            raise ValueError(f"width must be at most {MAX_WIDTH}, got {width}")
        if n > 1 << 31 or batch * max(n, 1) > 1 << 40:
            raise ValueError(f"n = {n}, batch = {batch}: at most 2^31 rows an array and 2^40 rows in all")
        self.layers = layers(n)
        self.slots = [batch * cnt for _, _, _, cnt in self.layers]
        self.n_layers, self.total_slots = len(self.layers), sum(self.slots)
        self.levels = fx.carry_levels(k - 1)
        self.opens = self.n_layers * (2 + self.levels)
        self.bit_rows, self.carry_rows, self.swap_rows = k + kappa, fx.carry_triples(k - 1), width
        self._before = [0]
        for s in self.slots:
            self._before.append(self._before[-1] + s)

    def rows(self, kind):
        if kind not in KINDS:
            raise ValueError(f"kind: one of {KINDS}, got {kind!r}")
        return {"bits": self.bit_rows, "carry": self.carry_rows, "swap": self.swap_rows}[kind]

    def size(self, kind):
        return self.rows(kind) * self.total_slots

    def offset(self, kind, l):
        if _int(l, "l", 0) >= self.n_layers:
            raise ValueError(f"l: the plan has {self.n_layers} layers, got {l}")
        return self.rows(kind) * self._before[l]

    def views(self, buf, kind, l):
        """layer l's block of a kind's flat (size(kind), limbs) buffer -> (rows, slots_l, limbs), a view"""
        rows, off = self.rows(kind), self.offset(kind, l)
        if len(buf.shape) != 2 or buf.shape[0] != self.size(kind):
            raise ValueError(f"{kind}: expected a flat buffer of shape ({self.size(kind)}, limbs), got {tuple(buf.shape)}")
        return buf[off:off + rows * self.slots[l]].reshape(rows, self.slots[l], buf.shape[1])


# ---- tensor level ------------------------------------------------------------------------------------------------------------
def _layer(layer, n, batch):
    try:
        a, r, d, cnt = layer
    except (TypeError, ValueError):
        raise ValueError("layer: expected (a, r, d, cnt)") from None
    a, r, d, cnt = _int(a, "a", 0), _int(r, "r", 0), _int(d, "d", 1), _int(cnt, "cnt", 0)
    n, batch = _int(n, "n", 2), _int(batch, "batch", 1)
    p = 1 << a
    if a > 30 or n > 1 << 31 or batch * n > 1 << 40 or r not in (0, p) or d >= n or d % p or not (d >> a) & 1 or cnt > _count(n, p, r, d):
        raise ValueError(f"layer {layer!r}: not a layer of comparators inside n = {n} rows")
    return (a, r, d, cnt), n, batch, batch * cnt


def _table(ctx, table, n, batch, in_place=False):
    if isinstance(table, ctx.torch.Tensor) and (table.dim() != 3 or not 1 <= table.shape[0] <= MAX_WIDTH or table.shape[1] != batch * n):
        raise ValueError(f"table: expected shape (1 <= width <= {MAX_WIDTH}, {batch * n}, {ctx.n_limbs}), got {tuple(table.shape)}")
    if in_place and isinstance(table, ctx.torch.Tensor) and not table.is_contiguous():
        raise ValueError("table: must be contiguous (it is updated in place)")
    return ctx.elems(table, what="table")


def cmp_mask(ctx, table, layer, n, batch, bits, k, kappa=fx.KAPPA, out=None, r1_out=None):
    """Before a layer's first open: for every slot d = key[lo] - key[hi] (column 0 of the table) and -> (d + 2^(k-1) + r1 +
    2^(k-1) r2, r1), the array to open and what swap_mask needs, from the slot's k + kappa bit planes.  One launch; the table is
    left untouched."""
    fx.check_params(ctx.modulus, k, _int(k, "k", 2) - 1, kappa, full=True)
    (a, r, d, cnt), n, batch, slots = _layer(layer, n, batch)
    table = _table(ctx, table, n, batch)
    bits, _ = fx._planes(ctx, bits, k + kappa, slots, "bits")
    masked, r1 = fx._elems_out(ctx, out, slots), fx._elems_out(ctx, r1_out, slots, "r1_out")
    if slots and masked.data_ptr() == r1.data_ptr():
        raise ValueError("out and r1_out must be two arrays")
    ctx.check(ctx.lib.hb_sort_cmp_mask(ctx.h, ctx.ptr(table), n, batch, a, r, d, cnt, ctx.ptr(bits), k, kappa, ctx.ptr(masked), ctx.ptr(r1), ctx.stream()),
              "hb_sort_cmp_mask")
    return masked, r1


def swap_mask(ctx, table, layer, n, batch, c, r1, carry, p, q, k, out=None):
    """After the carry tree's root: c the opened array of cmp_mask, r1 its second result, carry the root's g.  u = 1 -
    [key_lo < key_hi] once a slot, never stored; -> (2 width, slots, limbs), rows 2w, 2w + 1 = u - p[w], (T[w][lo] - T[w][hi]) - q[w]:
    ONE array to open.  p, q: (width, slots, limbs).  One launch; the table is left untouched."""
    fx._check_m(ctx.modulus, _int(k, "k", 2) - 1)
    (a, r, d, cnt), n, batch, slots = _layer(layer, n, batch)
    table = _table(ctx, table, n, batch)
    width = table.shape[0]
    c, r1, carry = (ctx.elems(v, slots, what=w) for v, w in ((c, "c"), (r1, "r1"), (carry, "carry")))
    p, q = (fx._planes(ctx, v, width, slots, w, exact=True)[0] for v, w in ((p, "p"), (q, "q")))
    out = fx._planes_out(ctx, out, 2 * width, slots)
    inv = fx._inv2m(ctx, k - 1)
    ctx.check(ctx.lib.hb_sort_swap_mask(ctx.h, ctx.ptr(table), width, n, batch, a, r, d, cnt, ctx.ptr(c), ctx.ptr(r1), ctx.ptr(carry), ctx.ptr(p), ctx.ptr(q), k,
                                        inv.ctypes.data, ctx.ptr(out), ctx.stream()), "hb_sort_swap_mask")
    return out.view(2 * width, slots, ctx.n_limbs)


def swap_finish(ctx, table, layer, n, batch, opened, p, q, pq):
    """After a layer's last open: opened = swap_mask's array opened, (p, q, pq) this party's shares of the layer's swap triples,
    (width, slots, limbs) each.  For every slot and column m = d e + d q + e p + pq, T[w][lo] -= m, T[w][hi] += m IN PLACE (a layer
    is a matching: no two slots share a row); rows no comparator touches are not written.  -> the table.  One launch."""
    (a, r, d, cnt), n, batch, slots = _layer(layer, n, batch)
    table = _table(ctx, table, n, batch, in_place=True)
    width = table.shape[0]
    opened = ctx.elems(opened, 2 * width * slots, what="opened")                         # (2 width, slots, limbs), or flat as an open returns it
    p, q, pq = (fx._planes(ctx, v, width, slots, w, exact=True)[0] for v, w in ((p, "p"), (q, "q"), (pq, "pq")))
    ctx.check(ctx.lib.hb_sort_swap_finish(ctx.h, ctx.ptr(table), width, n, batch, a, r, d, cnt, ctx.ptr(opened), ctx.ptr(p), ctx.ptr(q), ctx.ptr(pq), ctx.stream()),
              "hb_sort_swap_finish")
    return table


# ---- protocols over an OpenCoalescer -----------------------------------------------------------------------------------------
def _check_sort(ctx, table, plan, bits, carry, swap):
    """everything a sort is handed, checked before anything is opened -> (table, bits, carry, swap)"""
    if not isinstance(plan, SortPlan):
        raise ValueError("plan: expected a SortPlan")
    fx.check_params(ctx.modulus, plan.k, plan.k - 1, plan.kappa, full=True)
    if not isinstance(table, ctx.torch.Tensor) or table.dim() != 3 or table.shape[0] != plan.width or table.shape[1] != plan.batch * plan.n:
        raise ValueError(f"table: expected a tensor of shape ({plan.width}, {plan.batch * plan.n}, {ctx.n_limbs})")
    if not table.is_contiguous():
        raise ValueError("table: must be contiguous (it is sorted in place)")
    table = ctx.elems(table, what="table")

    def flat(v, kind, what):
        if not isinstance(v, ctx.torch.Tensor) or v.dim() != 2 or v.shape[0] != plan.size(kind) or not v.is_contiguous():
            raise ValueError(f"{what}: expected a contiguous tensor of shape ({plan.size(kind)}, {ctx.n_limbs})")
        return ctx.elems(v, what=what)

    def three(v, kind, what):
        try:
            x, y, z = v
        except (TypeError, ValueError):
            raise ValueError(f"{what}: expected (p, q, pq)") from None
        return tuple(flat(t, kind, f"{what} {w}") for t, w in ((x, "p"), (y, "q"), (z, "pq")))

    return table, flat(bits, "bits", "bits"), three(carry, "carry", "carry_triples"), three(swap, "swap", "swap_triples")


async def _layer_steps(co, table, plan, l, bits, carry, swap):
    ctx = co.ctx
    layer, n, batch, k = plan.layers[l], plan.n, plan.batch, plan.k
    b = plan.views(bits, "bits", l)
    masked, r1 = cmp_mask(ctx, table, layer, n, batch, b, k, plan.kappa)
    c = await co.open_share_array(masked)
    g, pr = fx.ltl_leaves(ctx, c, b, k - 1)
    root = await fx._carry_tree(co, g, pr, tuple(plan.views(v, "carry", l) for v in carry), k - 1)
    p, q, pq = (plan.views(v, "swap", l) for v in swap)
    out = swap_mask(ctx, table, layer, n, batch, c, r1, root, p, q, k)
    opened = await co.open_share_array(out.view(-1, ctx.n_limbs))
    return swap_finish(ctx, table, layer, n, batch, opened, p, q, pq)


async def compare_exchange_layer(co, table, plan, l, bits, carry, swap):
    """Layer l of the plan on the table, in place: after it, every comparator of the layer holds the smaller key in its low row,
    payload columns moved with the keys.  bits, carry = (p, q, pq), swap = (p, q, pq): the plan's flat buffers (the layer uses its
    own blocks).  2 + carry_levels(k - 1) opens; 4 + 2 carry_levels(k - 1) launches.  -> the table."""
    table, bits, carry, swap = _check_sort(co.ctx, table, plan, bits, carry, swap)
    plan.offset("bits", l)
    return await _layer_steps(co, table, plan, l, bits, carry, swap)


async def sort(co, table, plan, bits, carry_triples, swap_triples):
    """Sorts every one of the plan's `batch` arrays by column 0, ascending, in place; the other columns travel with their keys.
    table: (width, batch n, limbs) shares; keys are signed values in [-2^(k-2), 2^(k-2)).  plan.opens batches; the preprocessing
    buffers have exactly the plan's sizes and are left untouched.  -> the table."""
    table, bits, carry, swap = _check_sort(co.ctx, table, plan, bits, carry_triples, swap_triples)
    for l in range(plan.n_layers):
        await _layer_steps(co, table, plan, l, bits, carry, swap)
    return table

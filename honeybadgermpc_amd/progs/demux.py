"""
One-hot demultiplexer of shared index bits on the device (csrc/hb_demux.hip), and what follows from it: table lookup at a shared
index, histograms and group-by sums.  From shares of the m bits of s = sum_i 2^i b_i, least significant first as bit_decompose
returns them, shares of the one-hot vector e_j = [s == j], j < 2^m.  The reference has none of this; the pin is the mathematics:
demux_model and its companions on Python ints, and the same steps composed from share_arithmetic.

Neighbouring groups of bits are merged by a Beaver OUTER product: only the two factor vectors are opened, never the product entries.

    groups      level 0 starts from m groups of width 1; a level merges the groups (0, 1), (2, 3), .. counted from the least
                significant and carries an odd last group unchanged: demux_levels(m) = ceil(log2 m) levels, none for m = 1.
    a merge     of a low group of width wl with one-hot vector A and a high group of width wh with vector B writes
                out[hi 2^wl + lo] = A[lo] B[hi].  A width-1 group is never stored: its vector is (1 - b, b), read from the bit plane by
                both kernels of the level that consumes it, so the leaves cost no launch and no product.
    storage     every merged group lives in ONE array of planes, `groups` (demux_group_rows(m), count, limbs): a level writes its
                merges in order from the row where the levels before it ended (DemuxLevel.out_row), a carried group stays where it is,
                and the last level's 2^m rows are the result.
    triples     one (ta, tab) a level.  ta (demux_opened(m, level), count, limbs): for each merge in order the 2^wl rows of P, then the
                2^wh rows of Q; tab (demux_products(m, level), count, limbs): merge by merge, row hi 2^wl + lo = P[lo] Q[hi] --
                offline.generate_matrix_triples with inner dimension 1, transposed to planes.

At m = 10 an index costs 4 opens of 20 + 16 + 32 + 260 = 328 elements and 1 332 triple entries; the bit-by-bit chain composed from
share_arithmetic (one bit a round) costs 9 opens of 2 (2^m - 2) = 2 044 elements and 1 022 triple entries (counted, not measured).

Host functions:

    demux_levels(m), demux_plan(m)                      the wiring: [DemuxLevel(merges, carried, sources, out_row)]
    demux_opened(m, level), demux_products(m, level)    sum (2^wl + 2^wh), sum 2^(wl + wh)
    demux_triples(m)                                    (rows of ta, rows of tab) over all levels
    demux_group_rows(m)                                 rows of `groups`
    demux_model(s, m)                                   [s == j] for j < 2^m
    lookup_model, histogram_model, aggregate_model

Tensor level, one launch each on torch's current stream, nothing synchronises:

    demux_leaves(ctx, bits)                             m = 1 -> (2, count, limbs)
    demux_groups(ctx, m, count)                         an empty `groups`
    demux_mask(ctx, bits, groups, level, ta)            the level's array to open, (demux_opened, count, limbs)
    demux_finish(ctx, opened, groups, level, ta, tab)   IN PLACE -> the level's rows of groups, (demux_products, count, limbs)
    lookup(ctx, onehot, table)                          public table (N, W) -> (W, count, limbs) shares of T[s]; no open
    histogram(ctx, onehot)                              -> (2^m, limbs), the count of each index value; no open

Protocol level, coroutines over an OpenCoalescer:

    async demux(co, bits, triples)                      demux_levels(m) opens, two launches a level      -> (2^m, count, limbs)
    async generate_demux_triples(co, count, m)          the list of (ta, tab), among the parties with no dealer
    async lookup_shared(co, onehot, table, prep, method)    shared table (N, W) -> (W, count, limbs); one open
    async aggregate(co, onehot, values, prep, method)   (2^m, W, limbs), sum_i [s_i == j] v_i; one open
"""
import collections
import functools

from .. import linalg
from .fixedpoint import _int, _planes

MAX_BITS = 12          # a level's rows go in blockIdx.y, and preprocessing grows as 2^m an index

# merges: [(bit_offset, wl, wh)]; carried: (bit_offset, width) or None; sources: [(lo_row, hi_row)], a bit plane for a group of width
# 1, a row of `groups` for a wider one; out_row: the row of `groups` the level's products start at
DemuxLevel = collections.namedtuple("DemuxLevel", "merges carried sources out_row")


# ---- host functions ------------------------------------------------------------------------------------------------------
def _m(m):
    if not 1 <= _int(m, "m") <= MAX_BITS:
        raise ValueError(f"needs 1 <= m <= {MAX_BITS}, got {m}")
    return m


def demux_levels(m):
    """ceil(log2 m), 0 for m = 1"""
    return (_m(m) - 1).bit_length()


def demux_plan(m):
    """-> [DemuxLevel] for level 0, 1, ..: the wiring and where each group lives"""
    groups = [(i, 1, i) for i in range(_m(m))]                  # (bit offset, width, row)
    plan, base = [], 0
    while len(groups) > 1:
        merges, sources, merged, off = [], [], [], 0
        for k in range(len(groups) // 2):
            (lo_bit, wl, lo_row), (_, wh, hi_row) = groups[2 * k], groups[2 * k + 1]
            merges.append((lo_bit, wl, wh))
            sources.append((lo_row, hi_row))
            merged.append((lo_bit, wl + wh, base + off))
            off += 1 << (wl + wh)
        carried = groups[-1] if len(groups) & 1 else None
        plan.append(DemuxLevel(merges, None if carried is None else carried[:2], sources, base))
        groups = merged + ([carried] if carried else [])
        base += off
    return plan


@functools.lru_cache(maxsize=None)
def _counts(m):
    """per level (rows opened, products, out_row) of a checked m: the tensor-level calls ask at every launch"""
    return tuple((sum((1 << wl) + (1 << wh) for _, wl, wh in lv.merges), sum(1 << (wl + wh) for _, wl, wh in lv.merges), lv.out_row) for lv in demux_plan(m))


def _level(m, level):
    counts = _counts(_m(m))
    if not 0 <= _int(level, "level") < len(counts):
        raise ValueError(f"level must be in 0 .. {len(counts) - 1}, got {level}")
    return counts[level]


def demux_opened(m, level):
    """elements an index level `level` opens: the two factor vectors of every merge"""
    return _level(m, level)[0]


def demux_products(m, level):
    """triple products an index level `level` consumes: the outer product of every merge"""
    return _level(m, level)[1]


def demux_triples(m):
    """-> (rows of ta, rows of tab) an index over all levels (m = 10: 328, 1 332)"""
    counts = _counts(_m(m))
    return sum(c[0] for c in counts), sum(c[1] for c in counts)


def demux_group_rows(m):
    """rows of `groups`: the products of every level"""
    return demux_triples(m)[1]


def demux_model(s, m):
    """[s == j] for j < 2^m"""
    if not 0 <= _int(s, "s") < 1 << _m(m):
        raise ValueError(f"needs 0 <= s < 2^{m}, got {s}")
    return [1 if j == s else 0 for j in range(1 << m)]


def lookup_model(s, table, m, p):
    """row s of table ((N, W) ints, N <= 2^m) mod p; zeros for an index at or above N"""
    demux_model(s, m)
    if len(table) > 1 << m:
        raise ValueError(f"table: at most 2^{m} rows, got {len(table)}")
    width = len(table[0]) if len(table) else 0
    return [v % p for v in table[s]] if s < len(table) else [0] * width


def histogram_model(indices, m):
    """how often each j < 2^m occurs"""
    out = [0] * (1 << _m(m))
    for s in indices:
        demux_model(s, m)
        out[s] += 1
    return out


def aggregate_model(indices, values, m, p):
    """[j][w] = sum of values[i][w] over the i with indices[i] == j, mod p"""
    width = len(values[0]) if len(values) else 0
    out = [[0] * width for _ in range(1 << _m(m))]
    for s, row in zip(indices, values):
        demux_model(s, m)
        out[s] = [(a + b) % p for a, b in zip(out[s], row)]
    return out


# ---- tensor level ----------------------------------------------------------------------------------------------------------
_M_OF_ROWS = {demux_group_rows(m): m for m in range(2, MAX_BITS + 1)}


def _bits(ctx, bits):
    """(m, count, limbs) -> contiguous, m, count"""
    bits = ctx.elems(bits, what="bits")
    if bits.dim() != 3 or bits.shape[0] < 1:
        raise ValueError(f"bits: expected shape (m, count, {ctx.n_limbs}), got {tuple(bits.shape)}")
    return bits, _m(bits.shape[0]), bits.shape[1]


def _groups(ctx, groups, m=None, count=None):
    """the array the finish updates in place: contiguous, (demux_group_rows(m), count, limbs) -> groups, m, count"""
    if isinstance(groups, ctx.torch.Tensor) and not groups.is_contiguous():
        raise ValueError("groups: must be contiguous (it is updated in place)")
    groups = ctx.elems(groups, what="groups")
    if m is None:
        m = _M_OF_ROWS.get(groups.shape[0]) if groups.dim() == 3 else None
    if m is None or groups.dim() != 3 or groups.shape[0] != demux_group_rows(m) or (count is not None and groups.shape[1] != count):
        raise ValueError(f"groups: expected shape (demux_group_rows(m), {'count' if count is None else count}, {ctx.n_limbs}) as demux_groups makes it, "
                         f"got {tuple(groups.shape)}")
    return groups, m, groups.shape[1]


def demux_leaves(ctx, bits):
    """m = 1: bits (1, count, limbs) -> (2, count, limbs) = (1 - b, b).  No triple, no open."""
    bits, m, count = _bits(ctx, bits)
    if m != 1:
        raise ValueError(f"demux_leaves is the whole demultiplexer of ONE bit, got m = {m}")
    out = ctx.torch.empty((2, count, ctx.n_limbs), dtype=ctx.torch.int64, device=ctx.tdev)
    ctx.check(ctx.lib.hb_demux_leaves(ctx.h, ctx.ptr(bits), ctx.ptr(out), count, ctx.stream()), "hb_demux_leaves")
    return out


def demux_groups(ctx, m, count):
    """the array of merged groups of m >= 2 bits, (demux_group_rows(m), count, limbs), uninitialised"""
    if _m(m) < 2:
        raise ValueError("one bit has no merged group: demux_leaves")
    if _int(count, "count") < 0:
        raise ValueError(f"count must not be negative, got {count}")
    return ctx.torch.empty((demux_group_rows(m), count, ctx.n_limbs), dtype=ctx.torch.int64, device=ctx.tdev)


def demux_mask(ctx, bits, groups, level, ta):
    """One level before its open.  bits (m, count, limbs); groups as demux_groups makes it, holding the levels before this one (level
    0 reads bit planes alone); ta (at least demux_opened(m, level), count, limbs): P then Q of every merge.  -> (demux_opened, count,
    limbs), ONE array to open: for each merge 2^wl rows A[lo] - P[lo], then 2^wh rows B[hi] - Q[hi]."""
    bits, m, count = _bits(ctx, bits)
    rows = demux_opened(m, level)
    if groups is not None or level != 0:                                                 # level 0 reads no stored group: groups may be None
        groups, _, _ = _groups(ctx, groups, m, count)
    ta, _ = _planes(ctx, ta, rows, count, "ta")
    out = ctx.torch.empty((rows, count, ctx.n_limbs), dtype=ctx.torch.int64, device=ctx.tdev)
    ctx.check(ctx.lib.hb_demux_mask(ctx.h, ctx.ptr(bits), None if groups is None else ctx.ptr(groups), m, level, ctx.ptr(ta), ctx.ptr(out), count, ctx.stream()),
              "hb_demux_mask")
    return out


def demux_finish(ctx, opened, groups, level, ta, tab):
    """One level after its open, IN PLACE: the level's rows of groups <- d_lo e_hi + d_lo Q_hi + e_hi P_lo + PQ; every other row is left
    untouched.  opened (demux_opened, count, limbs), or flat as an open returns it; tab (at least demux_products(m, level), count,
    limbs).  -> the level's rows, a view; after the last level that is the result (2^m, count, limbs)."""
    groups, m, count = _groups(ctx, groups)
    rows, products = demux_opened(m, level), demux_products(m, level)
    opened = ctx.elems(opened, rows * count, what="opened")
    ta, _ = _planes(ctx, ta, rows, count, "ta")
    tab, _ = _planes(ctx, tab, products, count, "tab")
    ctx.check(ctx.lib.hb_demux_finish(ctx.h, ctx.ptr(opened), ctx.ptr(ta), ctx.ptr(tab), m, level, ctx.ptr(groups), count, ctx.stream()), "hb_demux_finish")
    first = _level(m, level)[2]
    return groups[first:first + products]


def _onehot(ctx, onehot):
    """(2^m, count, limbs) -> contiguous, m, count"""
    onehot = ctx.elems(onehot, what="onehot")
    rows = onehot.shape[0] if onehot.dim() == 3 else 0
    if rows < 2 or rows & (rows - 1) or rows > 1 << MAX_BITS:
        raise ValueError(f"onehot: expected shape (2^m, count, {ctx.n_limbs}) with 1 <= m <= {MAX_BITS}, got {tuple(onehot.shape)}")
    return onehot, rows.bit_length() - 1, onehot.shape[1]


def _table(ctx, table, m, shared):
    """(N, W) -> the transposed table (W, N, limbs) on the device, N, W"""
    if isinstance(table, ctx.torch.Tensor):
        table = ctx.elems(table, what="table")
        if table.dim() != 3:
            raise ValueError(f"table: expected shape (N, W, {ctx.n_limbs}), got {tuple(table.shape)}")
        n, w = table.shape[0], table.shape[1]
        t = table.transpose(0, 1).contiguous()
    elif shared:
        raise TypeError(f"table: expected a torch tensor of shares, got {type(table).__name__}")
    else:
        rows = [list(r) for r in table]
        n, w = len(rows), len(rows[0]) if rows else 0
        if any(len(r) != w for r in rows):
            raise ValueError("table: rows of different lengths")
        t = ctx.upload_ints([int(rows[j][i]) % ctx.modulus for i in range(w) for j in range(n)]).view(w, n, ctx.n_limbs)
    if not 1 <= n <= 1 << m or w < 1:
        raise ValueError(f"table: expected (N, W) with 1 <= N <= 2^{m} and W >= 1, got ({n}, {w})")
    return t, n, w


def lookup(ctx, onehot, table):
    """Shares of T[s] for a PUBLIC table: onehot (2^m, count, limbs), table (N, W) as ints or an (N, W, limbs) tensor, N <= 2^m.
    -> (W, count, limbs); an index at or above N gives 0.  Local: one linalg.matmul, no open."""
    onehot, m, count = _onehot(ctx, onehot)
    t, n, w = _table(ctx, table, m, shared=False)
    return linalg.matmul(ctx, t, onehot[:n])


def histogram(ctx, onehot):
    """-> (2^m, limbs): shares of the number of indices equal to j, for every j.  Local: one linalg.matmul against a column of ones."""
    onehot, m, count = _onehot(ctx, onehot)
    if count == 0:
        return ctx.torch.zeros((1 << m, ctx.n_limbs), dtype=ctx.torch.int64, device=ctx.tdev)
    ones = ctx.torch.zeros((count, 1, ctx.n_limbs), dtype=ctx.torch.int64, device=ctx.tdev)
    ones[:, :, 0] = 1
    return linalg.matmul(ctx, onehot, ones).view(1 << m, ctx.n_limbs)


# ---- protocols over an OpenCoalescer ---------------------------------------------------------------------------------------
def _level_triples(ctx, triples, m, count):
    """[(ta, tab)] a level, each with at least the level's rows -> the list, checked"""
    levels = demux_levels(m)
    try:
        pairs = [tuple(pair) for pair in triples]
        if len(pairs) < levels or any(len(pair) != 2 for pair in pairs[:levels]):
            raise TypeError
    except TypeError:
        raise ValueError(f"triples: expected a list of {levels} pairs (ta, tab), one a level") from None
    return [(_planes(ctx, ta, demux_opened(m, l), count, f"triples[{l}] ta")[0], _planes(ctx, tab, demux_products(m, l), count, f"triples[{l}] tab")[0])
            for l, (ta, tab) in enumerate(pairs[:levels])]


async def demux(co, bits, triples):
    """Shares of the one-hot vector of the index whose bit shares are bits (m, count, limbs), least significant first: -> (2^m, count,
    limbs), plane j a share of [s == j].  triples: a list with one (ta, tab) a level (generate_demux_triples).  Exactly
    demux_levels(m) coalesced opens at degree t and two launches a level, for any count (m = 1: one launch, no open).  bits and
    triples are left untouched.  ValueError before anything is opened."""
    ctx = co.ctx
    bits, m, count = _bits(ctx, bits)
    triples = _level_triples(ctx, triples, m, count)
    if m == 1:
        return demux_leaves(ctx, bits)
    groups = demux_groups(ctx, m, count)
    out = None
    for level, (ta, tab) in enumerate(triples):
        masked = demux_mask(ctx, bits, groups, level, ta)
        opened = await co.open_share_array(masked.view(masked.shape[0] * count, ctx.n_limbs))
        out = demux_finish(ctx, opened, groups, level, ta, tab)
    return out


async def generate_demux_triples(co, count, m, tag="demux_triples", generator=None):
    """What demux consumes for `count` indices of m bits, made among the parties with no dealer: -> [(ta, tab)], one pair a level.
    One offline.generate_matrix_triples(co, 2^wl, 1, 2^wh, count=count) a merge -- an outer product is a matrix product with inner
    dimension 1 -- transposed to planes; the merges of all levels run concurrently, each on a branch of co with its own channels and
    batch numbering.  Aborts are randousha's: anything but 2t successes raises HoneyBadgerMPCError in every party."""
    from ..offline import _branches, generate_matrix_triples

    if _int(count, "count") < 1:
        raise ValueError(f"generate_demux_triples: count >= 1, got {count}")
    ctx, plan, L = co.ctx, demux_plan(m), co.ctx.n_limbs
    if not plan:
        return []

    def source(name, wl, wh):
        return lambda kid: generate_matrix_triples(kid, 1 << wl, 1, 1 << wh, count=count, tag=(tag, name), generator=generator)

    named = [((l, k), source((l, k), wl, wh)) for l, level in enumerate(plan) for k, (_, wl, wh) in enumerate(level.merges)]
    made = dict(zip((name for name, _ in named), await _branches(co, tag, named)))
    out = []
    for l, level in enumerate(plan):
        ta, tab = [], []
        for k, (_, wl, wh) in enumerate(level.merges):
            P, Q, PQ = made[(l, k)]                              # (count, 2^wl, 1), (count, 1, 2^wh), (count, 2^wl, 2^wh)
            ta += [P.view(count, 1 << wl, L).transpose(0, 1), Q.view(count, 1 << wh, L).transpose(0, 1)]
            tab.append(PQ.permute(2, 1, 0, 3).reshape(1 << (wl + wh), count, L))
        out.append((ctx.torch.cat(ta).contiguous(), ctx.torch.cat(tab).contiguous()))
    return out


async def _shared_product(co, X, Y, prep, method):
    if method == linalg.BEAVER:
        return await linalg.beaver_matmul(co, X, Y, prep)
    if method == linalg.DOUBLE_SHARING:
        try:
            r_t, r_2t = prep
        except (TypeError, ValueError):
            raise ValueError("prep: expected (r_t, r_2t)") from None
        return await linalg.double_sharing_matmul(co, X, Y, r_t, r_2t)
    raise ValueError(f"method: linalg.BEAVER or linalg.DOUBLE_SHARING, got {method!r}")


async def lookup_shared(co, onehot, table, prep, method):
    """Shares of T[s] for a SHARED table (N, W, limbs), N <= 2^m: -> (W, count, limbs), one open.  The product T^t (W, N) times the
    first N planes (N, count) by linalg.beaver_matmul (prep = a matrix triple (P, Q, PQ) of those shapes) or
    linalg.double_sharing_matmul (prep = (r_t, r_2t), W count pairs)."""
    ctx = co.ctx
    onehot, m, count = _onehot(ctx, onehot)
    t, n, w = _table(ctx, table, m, shared=True)
    return await _shared_product(co, t, onehot[:n], prep, method)


async def aggregate(co, onehot, values, prep, method):
    """Group-by sum: values (count, W, limbs) shares -> (2^m, W, limbs), shares of sum_i [s_i == j] v_i; one open.  The product of
    the planes (2^m, count) and values (count, W); method and prep as in lookup_shared, for those shapes."""
    ctx = co.ctx
    onehot, m, count = _onehot(ctx, onehot)
    values = ctx.elems(values, what="values")
    if values.dim() != 3 or values.shape[0] != count or values.shape[1] < 1:
        raise ValueError(f"values: expected shape ({count}, W, {ctx.n_limbs}), got {tuple(values.shape)}")
    return await _shared_product(co, onehot, values, prep, method)

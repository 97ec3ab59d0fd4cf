"""GPU: honeybadgermpc_amd.progs.demux -- the kernels of csrc/hb_demux.hip bit for bit against the same level composed from
share_arithmetic (neg, add, index_select, sub, beaver_combine) and against Python ints on sampled elements, and the whole protocol over
OpenCoalescers in one process: demux opens to exactly demux_model in demux_levels(m) batches, lookup, lookup_shared, histogram and
aggregate open to their models, and the preprocessing made among the parties serves FixedPointArray.lookup.  No tolerance anywhere:
the result does not depend on the masks."""
import random

import pytest

import bitdec_cases as bc
import demux_cases as dc
from bitdec_cases import gpu_ctx, random_tensor, rows_of
from conftest import BLS

pytestmark = pytest.mark.gpu

COUNTS = (0, 1, 255, 256, 257)        # around the 256-thread workgroup


def _check_level(ctx, sa, dx, m, level, count, seed, bits, groups):
    """mask and finish of one level over planes of any residues -> groups after the level (the kernel's, checked)"""
    torch, p = ctx.torch, ctx.modulus
    lv = dx.demux_plan(m)[level]
    n_open, n_prod = dx.demux_opened(m, level), dx.demux_products(m, level)
    ta, tab, opened = (random_tensor(ctx, seed + s, count, rows=r) for s, r in enumerate((n_open + 1, n_prod + 1, n_open)))   # a row more than needed is fine
    before = groups.clone()
    keep = [v.clone() for v in (bits, ta, tab, opened)]
    masked = dx.demux_mask(ctx, bits, groups, level, ta)
    stored = any(w > 1 for _, wl, wh in lv.merges for w in (wl, wh))
    want_masked = dc.composed_mask(ctx, sa, lv, bits, groups if stored else None, ta)
    assert tuple(masked.shape) == (n_open, count, ctx.n_limbs) and torch.equal(masked, want_masked), (m, level, count)
    assert torch.equal(groups, before)
    out = dx.demux_finish(ctx, opened.view(n_open * count, ctx.n_limbs), groups, level, ta, tab)          # flat, as an open returns it
    want = dc.composed_finish(ctx, sa, lv, m, opened, ta, tab)
    assert tuple(out.shape) == (n_prod, count, ctx.n_limbs) and (count == 0 or out.data_ptr() == groups[lv.out_row].data_ptr())
    assert torch.equal(out, want), (m, level, count)
    assert torch.equal(groups[:lv.out_row], before[:lv.out_row]) and torch.equal(groups[lv.out_row + n_prod:], before[lv.out_row + n_prod:]), (m, level, count)
    assert all(torch.equal(v, w) for v, w in zip((bits, ta, tab, opened), keep))
    if count:                                                           # Python ints on sampled elements
        sel = torch.tensor(sorted({0, count // 2, count - 1}), device=ctx.tdev)
        b, g, a, ab, o, mk, res = (rows_of(ctx, v.index_select(1, sel)) for v in (bits, before, ta, tab, opened, masked, out))
        src, d, e = dc.level_rows(lv, m)
        for x in range(len(sel)):
            pool = [(1 - r[x]) % p for r in b] + [r[x] for r in b] + [r[x] for r in g]
            assert [mk[y][x] for y in range(n_open)] == [(pool[src[y]] - a[y][x]) % p for y in range(n_open)], (m, level, count, x)
            assert [res[r][x] for r in range(n_prod)] == [bc.beaver(o[d[r]][x], o[e[r]][x], a[d[r]][x], a[e[r]][x], ab[r][x], p) for r in range(n_prod)], (m, level, x)
    return groups


# ---- the kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 3, 5, 6])
@pytest.mark.parametrize("p", dc.GPU_FIELDS, ids=dc.FIELD_IDS)
def test_kernels_against_share_arithmetic(p, m):
    """a carried group (3, 5), unequal widths (2, 1) and (4, 1), several merges in one level (5, 6), a first level that reads bit
    planes and later levels that read stored groups"""
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd.progs import demux as dx

    ctx = gpu_ctx(p)
    torch = ctx.torch
    for count in COUNTS:
        bits = random_tensor(ctx, 3 + count, count, rows=m)
        if count >= 255:
            bits[:, :3] = ctx.upload_ints([0, 1, p - 1] * m).view(m, 3, ctx.n_limbs)
        if m == 1:
            keep = bits.clone()
            out = dx.demux_leaves(ctx, bits)
            assert tuple(out.shape) == (2, count, ctx.n_limbs)
            assert torch.equal(out[0], sa.add(ctx, sa.neg(ctx, bits[0]), 1)) and torch.equal(out[1], bits[0]) and torch.equal(bits, keep)
            assert ctx.download_ints(out[0][:3]) == [(1 - b) % p for b in ctx.download_ints(bits[0][:3])]
            continue
        groups = random_tensor(ctx, 4 + count, count, rows=dx.demux_group_rows(m))
        for level in range(dx.demux_levels(m)):
            groups = _check_level(ctx, sa, dx, m, level, count, 10 * level + count, bits, groups)
        assert dx.demux_mask(ctx, bits, None, 0, random_tensor(ctx, 1, count, rows=dx.demux_opened(m, 0))).shape[0] == dx.demux_opened(m, 0)


def test_kernels_at_1024_rows():
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd.progs import demux as dx

    ctx = gpu_ctx(BLS)
    m, count = 10, 3
    bits = random_tensor(ctx, 70, count, rows=m)
    groups = random_tensor(ctx, 71, count, rows=dx.demux_group_rows(m))
    for level in range(dx.demux_levels(m)):
        groups = _check_level(ctx, sa, dx, m, level, count, 72 + 10 * level, bits, groups)
    assert dx.demux_products(m, 3) == 1024


# ---- the protocol -----------------------------------------------------------------------------------------------------------
def _deal_demux_triples(ctx, dx, rnd, p, n, t, m, count):
    """-> [party] of [(ta, tab)] a level"""
    out = [[] for _ in range(n)]
    for level in range(dx.demux_levels(m)):
        ta, tab = dc.level_triples(dx, m, level, count, p, rnd)
        a, ab = bc.deal_planes(ctx, rnd, p, n, t, ta), bc.deal_planes(ctx, rnd, p, n, t, tab)
        for i in range(n):
            out[i].append((a[i], ab[i]))
    return out


def _deal_matrix(ctx, rnd, p, n, degree, rows):
    """rows: [r][c] values -> [party] tensors (r, c, limbs)"""
    dealt = bc.deal(rnd, p, n, degree, bc.flat(rows))
    return [ctx.upload_ints(d).view(len(rows), len(rows[0]), ctx.n_limbs) for d in dealt]


def _prep(ctx, rnd, p, n, t, method, r, k, c):
    """-> [party] the preprocessing of one shared (r, k) x (k, c) product"""
    from honeybadgermpc_amd import linalg

    if method == linalg.BEAVER:
        P = [[rnd.randrange(p) for _ in range(k)] for _ in range(r)]
        Q = [[rnd.randrange(p) for _ in range(c)] for _ in range(k)]
        PQ = [[sum(P[i][x] * Q[x][j] for x in range(k)) % p for j in range(c)] for i in range(r)]
        return list(zip(*(_deal_matrix(ctx, rnd, p, n, t, v) for v in (P, Q, PQ))))
    mask = [[rnd.randrange(p) for _ in range(c)] for _ in range(r)]
    return list(zip(_deal_matrix(ctx, rnd, p, n, t, mask), _deal_matrix(ctx, rnd, p, n, 2 * t, mask)))


@pytest.mark.parametrize("m", [3, 5, 8])
@pytest.mark.parametrize("p", dc.GPU_FIELDS, ids=dc.FIELD_IDS)
def test_demux_opens_to_the_model(p, m):
    from honeybadgermpc_amd.progs import demux as dx

    n, t = 4, 1
    ctx = gpu_ctx(p)
    rnd = random.Random(100 * m + p % 7)
    ss = list(range(1 << m)) if m <= 5 else [0, 1, (1 << m) - 1, (1 << m) - 2] + [rnd.randrange(1 << m) for _ in range(60)]
    count = len(ss)
    bits = bc.deal_planes(ctx, rnd, p, n, t, [[dc.bits_of(s, m)[i] for s in ss] for i in range(m)])
    triples = _deal_demux_triples(ctx, dx, rnd, p, n, t, m, count)

    async def body(co, i):
        keep = (bits[i].clone(), [(a.clone(), b.clone()) for a, b in triples[i]])
        before = co.batches
        planes = await dx.demux(co, bits[i], triples[i])
        batches = co.batches - before
        assert tuple(planes.shape) == (1 << m, count, ctx.n_limbs)
        assert ctx.torch.equal(bits[i], keep[0]) and all(ctx.torch.equal(a, c) and ctx.torch.equal(b, d) for (a, b), (c, d) in zip(triples[i], keep[1]))
        return ctx.download_ints(await co.open_share_array(planes.reshape(count << m, ctx.n_limbs))), batches

    want = bc.flat([[dx.demux_model(s, m)[j] for s in ss] for j in range(1 << m)])
    for got, batches in bc.run_parties(p, n, t, set(), rnd, body):
        assert got == want and batches == dx.demux_levels(m)


@pytest.mark.parametrize("p", dc.GPU_FIELDS, ids=dc.FIELD_IDS)
def test_lookup_histogram_and_aggregate_open_to_their_models(p):
    from honeybadgermpc_amd import linalg
    from honeybadgermpc_amd.progs import demux as dx

    n, t, m, N, W = 4, 1, 3, 5, 2                                        # a table shorter than 2^m: indices 5, 6, 7 give 0
    ctx = gpu_ctx(p)
    L = ctx.n_limbs
    rnd = random.Random(77)
    ss = list(range(1 << m)) + [3, 3, 7, 0, 6]
    count = len(ss)
    table = [[rnd.randrange(p), (j * j + 1) % p] for j in range(N)]
    full = [[rnd.randrange(p) for _ in range(W)] for _ in range(1 << m)]
    values = [[rnd.randrange(p) for _ in range(W)] for _ in range(count)]
    bits = bc.deal_planes(ctx, rnd, p, n, t, [[dc.bits_of(s, m)[i] for s in ss] for i in range(m)])
    triples = _deal_demux_triples(ctx, dx, rnd, p, n, t, m, count)
    shared_table, shared_values = _deal_matrix(ctx, rnd, p, n, t, table), _deal_matrix(ctx, rnd, p, n, t, values)
    methods = (linalg.BEAVER, linalg.DOUBLE_SHARING)
    prep_lookup = {me: _prep(ctx, rnd, p, n, t, me, W, N, count) for me in methods}
    prep_agg = {me: _prep(ctx, rnd, p, n, t, me, 1 << m, count, W) for me in methods}

    async def body(co, i):
        onehot = await dx.demux(co, bits[i], triples[i])
        keep = onehot.clone()
        got, batches = {}, {}

        async def opened(name, v, shape):
            assert tuple(v.shape) == shape + (L,), name
            got[name] = ctx.download_ints(await co.open_share_array(v.reshape(-1, L)))

        await opened("lookup", dx.lookup(ctx, onehot, table), (W, count))
        await opened("lookup tensor", dx.lookup(ctx, onehot, ctx.upload_ints(bc.flat(table)).view(N, W, L)), (W, count))
        await opened("lookup full", dx.lookup(ctx, onehot, full), (W, count))
        await opened("histogram", dx.histogram(ctx, onehot), (1 << m,))
        for me in methods:
            before = co.batches
            res = await dx.lookup_shared(co, onehot, shared_table[i], prep_lookup[me][i], me)
            agg = await dx.aggregate(co, onehot, shared_values[i], prep_agg[me][i], me)
            batches[me] = co.batches - before
            await opened(("lookup_shared", me), res, (W, count))
            await opened(("aggregate", me), agg, (1 << m, W))
        with pytest.raises(ValueError):
            await dx.lookup_shared(co, onehot, shared_table[i], prep_lookup[linalg.BEAVER][i], "elementwise")
        assert ctx.torch.equal(onehot, keep)
        return got, batches

    by_row = [dx.lookup_model(s, table, m, p) for s in ss]
    want_lookup = [by_row[e][w] for w in range(W) for e in range(count)]
    assert [by_row[e] for e in (5, 6, 7)] == [[0, 0]] * 3
    want_agg = bc.flat(dx.aggregate_model(ss, values, m, p))
    for got, batches in bc.run_parties(p, n, t, set(), rnd, body):
        assert got["lookup"] == got["lookup tensor"] == want_lookup
        assert got["lookup full"] == [full[s][w] for w in range(W) for s in ss]
        assert got["histogram"] == dx.histogram_model(ss, m)
        for me in methods:
            assert got[("lookup_shared", me)] == want_lookup and got[("aggregate", me)] == want_agg, me
            assert batches[me] == 2, me                                  # one open each


def test_preprocessing_among_the_parties_and_fixed_point_lookup():
    """generate_demux_triples with no dealer, spent by FixedPointArray.lookup of a public table of squares at m = 5"""
    from offline_support import _run_parties

    from honeybadgermpc_amd.progs import bit_decomposition as bd
    from honeybadgermpc_amd.progs import demux as dx
    from honeybadgermpc_amd.progs import fixedpoint as fx

    p, n, t, m, k, kappa = BLS, 4, 1, 5, 16, 8
    ctx = gpu_ctx(p)
    rnd = random.Random(55)
    xs = [0, 1, 31, 30, 17, 8, 5]
    count = len(xs)
    squares = [[j * j] for j in range(1 << m)]
    vals = bc.deal_planes(ctx, rnd, p, n, t, [xs])
    mask_bits = bc.deal_planes(ctx, rnd, p, n, t, [[rnd.getrandbits(1) for _ in range(count)] for _ in range(k + kappa)])
    need = bd.bit_triples(m)
    ta, tb = ([[rnd.randrange(p) for _ in range(count)] for _ in range(need)] for _ in range(2))
    tab = [[a * b % p for a, b in zip(ra, rb)] for ra, rb in zip(ta, tb)]
    bd_triples = [bc.deal_planes(ctx, rnd, p, n, t, v) for v in (ta, tb, tab)]

    async def body(co, i):
        triples = await dx.generate_demux_triples(co, count, m)
        assert [(tuple(a.shape), tuple(b.shape)) for a, b in triples] == [((dx.demux_opened(m, l), count, ctx.n_limbs), (dx.demux_products(m, l), count, ctx.n_limbs))
                                                                           for l in range(dx.demux_levels(m))]
        arr = fx.FixedPointArray(co, vals[i][0], 0, k, kappa)
        res = await arr.lookup(squares, m, mask_bits[i], tuple(v[i] for v in bd_triples), triples)
        assert tuple(res.shape) == (1, count, ctx.n_limbs)
        opened = [ctx.download_ints(await co.open_share_array(v.reshape(-1, ctx.n_limbs))) for v in (res, triples[2][0], triples[2][1])]
        return opened

    for got, a, ab in _run_parties(p, n, t, body):
        assert got == [x * x for x in xs]
        P, Q = [a[r * count:(r + 1) * count] for r in range(16)], [a[(16 + r) * count:(17 + r) * count] for r in range(2)]      # level 2: the merge (4, 1)
        assert ab == bc.flat([[P[lo][e] * Q[hi][e] % p for e in range(count)] for hi in range(2) for lo in range(16)])


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals():
    from honeybadgermpc_amd._capi import HB_ERR_BAD_ARG
    from honeybadgermpc_amd.progs import demux as dx

    p, m, count = BLS, 3, 5
    ctx = gpu_ctx(p)
    torch, L = ctx.torch, ctx.n_limbs
    bits = random_tensor(ctx, 1, count, rows=m)
    groups = random_tensor(ctx, 2, count, rows=dx.demux_group_rows(m))
    ta, tab, opened = (random_tensor(ctx, 3 + s, count, rows=r) for s, r in enumerate((6, 8, 6)))
    copies = [v.clone() for v in (bits, groups, ta, tab, opened)]
    wide = random_tensor(ctx, 6, 2 * count, rows=dx.demux_group_rows(m))
    for call in (lambda: dx.demux_mask(ctx, bits[0], groups, 1, ta),                                  # wrong shapes
                 lambda: dx.demux_mask(ctx, bits, groups[:4], 1, ta),
                 lambda: dx.demux_mask(ctx, bits, groups, 1, ta[:, :4]),
                 lambda: dx.demux_mask(ctx, bits, groups, 1, ta[:5]),                                  # too few triple rows
                 lambda: dx.demux_mask(ctx, bits, groups, 2, ta),
                 lambda: dx.demux_mask(ctx, random_tensor(ctx, 7, count, rows=13), groups, 0, ta),      # m = 13
                 lambda: dx.demux_mask(ctx, bits, wide[:, ::2], 1, ta),                                # non-contiguous in-place operand
                 lambda: dx.demux_finish(ctx, opened, wide[:, ::2], 1, ta, tab),
                 lambda: dx.demux_finish(ctx, opened, groups, 1, ta, tab[:7]),
                 lambda: dx.demux_finish(ctx, opened, groups, 1, ta[:5], tab),
                 lambda: dx.demux_finish(ctx, opened[:5], groups, 1, ta, tab),
                 lambda: dx.demux_finish(ctx, opened, groups[:11], 1, ta, tab),
                 lambda: dx.demux_finish(ctx, opened, groups, -1, ta, tab),
                 lambda: dx.demux_leaves(ctx, bits),
                 lambda: dx.demux_groups(ctx, 1, count), lambda: dx.demux_groups(ctx, 13, count), lambda: dx.demux_groups(ctx, 3, -1),
                 lambda: dx.lookup(ctx, groups[:3], [[1]]), lambda: dx.lookup(ctx, groups[:4], [[1]] * 5), lambda: dx.lookup(ctx, groups[:4], [[1, 2], [3]]),
                 lambda: dx.histogram(ctx, groups[0])):
        with pytest.raises(ValueError):
            call()
    lib, st, P = ctx.lib, ctx.stream(), ctx.ptr
    out = torch.full((8, count, L), 7, dtype=torch.int64, device=ctx.tdev)
    for rc in (lib.hb_demux_mask(ctx.h, P(bits), P(groups), 13, 0, P(ta), P(out), count, st), lib.hb_demux_mask(ctx.h, P(bits), P(groups), 0, 0, P(ta), P(out), count, st),
               lib.hb_demux_mask(ctx.h, P(bits), P(groups), m, 2, P(ta), P(out), count, st), lib.hb_demux_mask(ctx.h, P(bits), None, m, 1, P(ta), P(out), count, st),
               lib.hb_demux_mask(ctx.h, P(bits), P(groups), m, 1, P(ta), P(ta), count, st), lib.hb_demux_mask(ctx.h, P(bits), P(groups), m, 1, P(ta), P(out), -1, st),
               lib.hb_demux_finish(ctx.h, P(opened), P(ta), P(tab), 13, 0, P(groups), count, st), lib.hb_demux_finish(ctx.h, P(opened), P(ta), P(tab), m, 2, P(groups), count, st),
               lib.hb_demux_finish(ctx.h, P(opened), P(ta), None, m, 1, P(groups), count, st), lib.hb_demux_finish(ctx.h, P(groups), P(ta), P(tab), m, 1, P(groups), count, st),
               lib.hb_demux_leaves(ctx.h, None, P(out), count, st), lib.hb_demux_leaves(ctx.h, P(out), P(out), count, st)):
        assert rc == HB_ERR_BAD_ARG
    assert lib.hb_demux_mask(ctx.h, None, None, m, 1, None, None, 0, st) == 0 and lib.hb_demux_finish(ctx.h, None, None, None, m, 1, None, 0, st) == 0
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and all(torch.equal(v, w) for v, w in zip((bits, groups, ta, tab, opened), copies))

    async def refused(co, i):
        if i:
            return None
        pairs = [(ta[:4], tab[:4]), (ta, tab)]
        for coro in (lambda: dx.demux(co, bits, pairs[:1]), lambda: dx.demux(co, bits, [pairs[0], (ta[:5], tab)]), lambda: dx.demux(co, bits, [pairs[0], (ta, tab[:7])]),
                     lambda: dx.demux(co, bits, [pairs[0], (ta,)]), lambda: dx.demux(co, bits[:, :4], pairs), lambda: dx.demux(co, bits, None),
                     lambda: dx.generate_demux_triples(co, 0, 3), lambda: dx.generate_demux_triples(co, 4, 13)):
            with pytest.raises(ValueError):
                await coro()
        return co.batches

    assert bc.run_parties(p, 4, 1, set(), random.Random(3), refused)[0] == 0

"""GPU: honeybadgermpc_amd.progs.fixedpoint_exp -- every step of csrc/hb_fxexp.hip bit-equal to its host self-test row (the same row, the
same step function) and to the step composed from what the package had (demux_finish + demux.lookup + share_arithmetic.sub;
beaver_combine + trunc_mask; trunc_pr_finish + sub); inputs untouched, out= honoured, overlaps refused, nothing synchronises; and the
whole protocol among n = 4 parties in one process: exp2 and exp open to exactly the model for the dealt r1 -- no tolerance -- and their
shares are bit-equal to the same chain composed from bit_decompose, demux, demux.lookup, share_arithmetic and trunc_mask /
trunc_pr_finish, in exp2_opens batches."""
import random

import pytest

import bitdec_cases as bc
import demux_cases as xc
import exp_cases as ec
from bitdec_cases import COUNTS, gpu_ctx, random_tensor
from conftest import BLS
from exp_cases import FINISH_LOOKUP_MASK, PRODUCTS_TRUNC, TREE_STEP

pytestmark = pytest.mark.gpu


# ---- the kernels ------------------------------------------------------------------------------------------------------------
def _lookup_case(ctx, fe, chosen, count, seed, short):
    """operands of one finish_lookup_mask launch over the merges `chosen` ((1, 0): a group of one bit)"""
    p, L = ctx.modulus, ctx.n_limbs
    rnd = random.Random(seed)
    groups, tables, oo, po = [], [], 0, 0
    slots = rnd.sample(range(len(chosen) + 2), len(chosen))
    for (wl, wh), slot in zip(chosen, slots):
        top = min(p, 1 << 67) if short else p
        table = [0 if rnd.random() < 0.25 else rnd.randrange(top) for _ in range(1 << (wl + wh))]
        if wh == 0:
            groups.append((1, 0, rnd.randrange(3), 0, len(tables), slot))
        else:
            groups.append((wl, wh, oo, po, len(tables), slot))
            oo, po = oo + (1 << wl) + (1 << wh), po + (1 << (wl + wh))
        tables += table
    tdev, _ = fe.table_rows(ctx, [tables])
    ops = dict(bits=random_tensor(ctx, seed + 1, count, rows=3), opened=random_tensor(ctx, seed + 2, count, rows=max(oo, 1)), ta=random_tensor(ctx, seed + 3, count, rows=max(oo, 1)),
               tab=random_tensor(ctx, seed + 4, count, rows=max(po, 1)))
    return groups, tables, tdev, ops


@pytest.mark.parametrize("p", bc.GPU_FIELDS, ids=bc.GPU_FIELD_IDS)
def test_finish_lookup_mask_equals_its_selftest_row_and_the_composed_step(p):
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd.progs import demux as dx
    from honeybadgermpc_amd.progs import fixedpoint_exp as fe

    ctx = gpu_ctx(p)
    torch, L = ctx.torch, ctx.n_limbs
    same = lambda got, want: torch.equal(got.cpu(), want)
    launches = [[m] for m in ec.MERGES] + [[(1, 0)], [(2, 2), (1, 0)], [(4, 3), (1, 1), (2, 1)]]
    for count in COUNTS:
        for li, chosen in enumerate(launches):
            if count == 5000 and sum(1 << (wl + wh) for wl, wh in chosen) > 64 and p >> 64 and chosen != [(4, 4)]:
                continue                                                    # the wide merges at the large count once: (4, 4)
            groups, tables, tdev, ops = _lookup_case(ctx, fe, chosen, count, 500 + 7 * li + count, li & 1)
            pairs, kept_rows = 1, len(chosen) + 2
            nxt = (random_tensor(ctx, 600 + count, count, rows=pairs), random_tensor(ctx, 601 + count, count, rows=pairs))
            m0, k0 = random_tensor(ctx, 602 + count, count, rows=2 * pairs), random_tensor(ctx, 603 + count, count, rows=kept_rows)
            inputs = [tdev, nxt[0], nxt[1]] + list(ops.values())
            copies = [t.clone() for t in inputs]
            masked, kept = fe.finish_lookup_mask(ctx, groups, tdev, pairs, kept_rows, count, nxt=nxt, out=m0.clone(), kept_out=k0.clone(), **ops)
            assert tuple(masked.shape) == (2 * pairs, count, L) and tuple(kept.shape) == (kept_rows, count, L)
            want = ec.selftest_on_tensors(ctx, FINISH_LOOKUP_MASK, [ops["bits"], ops["opened"], ops["ta"], ops["tab"], tdev, nxt[0], nxt[1]],
                                          [len(groups), pairs, kept_rows] + [v for grp in groups for v in grp], [2 * pairs, kept_rows], count, outs_in=[m0, k0])
            assert same(masked, want[0]) and same(kept, want[1]), (chosen, count)
            if count in (1, 257):                                               # ... and the composed step: the level's products, the table read, one sub
                for wl, wh, oo, po, to, slot in groups:
                    table = tables[to:to + (1 << (wl + wh))]
                    if wh == 0:
                        f = sa.add(ctx, sa.mul(ctx, ops["bits"][oo], (table[1] - table[0]) % p), table[0])
                    else:
                        rows = (1 << wl) + (1 << wh)
                        d = [oo + (y & ((1 << wl) - 1)) for y in range(1 << (wl + wh))]
                        e = [oo + (1 << wl) + (y >> wl) for y in range(1 << (wl + wh))]
                        di, ei = (torch.tensor(v, dtype=torch.int64, device=ctx.tdev) for v in (d, e))
                        flat = [v.index_select(0, i).reshape(-1, L) for v, i in ((ops["opened"], di), (ops["opened"], ei), (ops["ta"], di), (ops["ta"], ei))]
                        onehot = sa.beaver_combine(ctx, *flat, ops["tab"][po:po + (1 << (wl + wh))].reshape(-1, L)).view(1 << (wl + wh), count, L)
                        f = dx.lookup(ctx, onehot, [[t] for t in table])[0]
                    assert torch.equal(kept[slot], f), (chosen, slot, count)
                    if slot < 2 * pairs:
                        assert torch.equal(masked[slot], sa.sub(ctx, f, nxt[slot & 1][slot >> 1]))
            assert all(torch.equal(t, cp) for t, cp in zip(inputs, copies))


@pytest.mark.parametrize("p", bc.GPU_FIELDS, ids=bc.GPU_FIELD_IDS)
def test_products_trunc_and_tree_step_equal_their_selftest_rows_and_the_composed_steps(p):
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd.progs import fixedpoint as fx
    from honeybadgermpc_amd.progs import fixedpoint_exp as fe

    ctx = gpu_ctx(p)
    torch, L = ctx.torch, ctx.n_limbs
    same = lambda got, want: torch.equal(got.cpu(), want)
    width, kappa = (134, 32) if p >> 64 else (38, 8)
    nb = width + kappa
    for count in COUNTS:
        opened = random_tensor(ctx, 700 + count, count, rows=10)
        ta, tb, tab, s = (random_tensor(ctx, 701 + i + count, count, rows=5) for i in range(4))
        carry = random_tensor(ctx, 706 + count, count)
        inputs = [opened, ta, tb, tab, s, carry]
        copies = [t.clone() for t in inputs]
        for products in (1, 2, 3, 4, 5) if count <= 257 else (1, 5):
            planes = random_tensor(ctx, 710 + products + count, count, rows=products * nb)
            m = width // 2
            masked, sv = fe.products_trunc(ctx, opened[:2 * products], ta[:products], tb[:products], tab[:products], planes, width, m, kappa)
            want = ec.selftest_on_tensors(ctx, PRODUCTS_TRUNC, [opened[:2 * products], ta[:products], tb[:products], tab[:products], planes], [products, width, m, kappa],
                                          [products, products], count)
            assert same(masked, want[0]) and same(sv, want[1]), (products, count)
            if count in (1, 257):
                for r in range(products):
                    v = sa.beaver_combine(ctx, opened[2 * r], opened[2 * r + 1], ta[r], tb[r], tab[r])
                    mk, r1 = fx.trunc_mask(ctx, v, planes[r * nb:(r + 1) * nb], width, m, kappa)
                    assert torch.equal(masked[r], mk) and torch.equal(sv[r], sa.add(ctx, v, r1)), (products, r, count)
        for rows in (1, 2, 3, 4, 5) if count <= 257 else (1, 5):
            for carried in (False, True):
                for m in (1, 8, 61) + ((64, 127, 140) if p >> 64 else ()):
                    values = rows + carried
                    pairs = values // 2
                    masked, kept = fe.tree_step(ctx, opened[:rows], s[:rows], m, ta[:pairs] if pairs else None, tb[:pairs] if pairs else None, carry=carry if carried else None)
                    want = ec.selftest_on_tensors(ctx, TREE_STEP, [opened[:rows], s[:rows], [pow(2, -m, p)], carry if carried else None, ta[:pairs] if pairs else None,
                                                                   tb[:pairs] if pairs else None], [rows, m], [2 * pairs, values & 1], count)
                    assert (masked is None) == (pairs == 0) and (kept is None) == (values % 2 == 0)
                    assert (pairs == 0 or same(masked, want[0])) and (kept is None or same(kept.view(1, count, L), want[1])), (rows, carried, m, count)
                    if count in (1, 257) and m in (8, 127):
                        zero = ctx.upload_ints([0] * count)
                        vals = [fx.trunc_pr_finish(ctx, s[j], opened[j], zero, m) for j in range(rows)] + ([carry] if carried else [])
                        for q in range(pairs):
                            assert torch.equal(masked[2 * q], sa.sub(ctx, vals[2 * q], ta[q])) and torch.equal(masked[2 * q + 1], sa.sub(ctx, vals[2 * q + 1], tb[q]))
                        if values & 1:
                            assert torch.equal(kept, vals[-1])
        assert all(torch.equal(t, cp) for t, cp in zip(inputs, copies))


def test_out_honoured_overlap_refused_and_asynchronous():
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd._capi import HB_ERR_BAD_ARG, HbmpcBackendError
    from honeybadgermpc_amd.progs import fixedpoint_exp as fe

    p, count, width, kappa, m = BLS, 600, 134, 32, 66
    ctx = gpu_ctx(p)
    torch, L = ctx.torch, ctx.n_limbs
    groups, tables, tdev, ops = _lookup_case(ctx, fe, [(2, 2), (1, 0), (2, 1)], count, 800, True)
    nxt = (random_tensor(ctx, 801, count, rows=1), random_tensor(ctx, 802, count, rows=1))
    opened, ta, tb, tab, s = (random_tensor(ctx, 803 + i, count, rows=4) for i in range(5))
    planes = random_tensor(ctx, 810, count, rows=2 * (width + kappa))
    carry = random_tensor(ctx, 811, count)
    m0, k0 = random_tensor(ctx, 812, count, rows=2), random_tensor(ctx, 813, count, rows=5)

    def run():
        a = fe.finish_lookup_mask(ctx, groups, tdev, 1, 5, count, nxt=nxt, out=m0.clone(), kept_out=k0.clone(), **ops)
        b = fe.products_trunc(ctx, opened, ta[:2], tb[:2], tab[:2], planes, width, m, kappa)
        c = fe.tree_step(ctx, opened[:2], s[:2], m, ta[:1], tb[:1], carry=carry)
        return [a[0], a[1], b[0], b[1], c[0], c[1]]

    first = run()
    assert torch.equal(sa.sub(ctx, sa.add(ctx, first[4][0], first[4][0]), first[4][0]), first[4][0])      # consumed on the current stream without a synchronise
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        second = run()
    side.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    # out given: written where asked, and handed back
    b0, b1 = torch.empty_like(first[2]), torch.empty_like(first[3])
    got = fe.products_trunc(ctx, opened, ta[:2], tb[:2], tab[:2], planes, width, m, kappa, out=(b0, b1))
    assert got[0].data_ptr() == b0.data_ptr() and got[1].data_ptr() == b1.data_ptr() and torch.equal(b0, first[2]) and torch.equal(b1, first[3])
    c0, c1 = torch.empty_like(first[4]), torch.empty_like(first[5])
    got = fe.tree_step(ctx, opened[:2], s[:2], m, ta[:1], tb[:1], carry=carry, out=(c0, c1))
    assert got[0].data_ptr() == c0.data_ptr() and got[1].data_ptr() == c1.data_ptr() and torch.equal(c0, first[4]) and torch.equal(c1, first[5])
    a0, a1 = m0.clone(), k0.clone()
    got = fe.finish_lookup_mask(ctx, groups, tdev, 1, 5, count, nxt=nxt, out=a0, kept_out=a1, **ops)
    assert got[0].data_ptr() == a0.data_ptr() and got[1].data_ptr() == a1.data_ptr() and torch.equal(a0, first[0]) and torch.equal(a1, first[1])
    # ValueError before C for shapes
    c0.fill_(7)
    for i, call in enumerate([
            lambda: fe.products_trunc(ctx, opened[:3], ta[:2], tb[:2], tab[:2], planes, width, m, kappa),
            lambda: fe.products_trunc(ctx, opened, ta[:2], tb[:1], tab[:2], planes, width, m, kappa),
            lambda: fe.products_trunc(ctx, opened, ta[:2], tb[:2], tab[:2], planes[:-1], width, m, kappa),
            lambda: fe.products_trunc(ctx, opened, ta[:2], tb[:2], tab[:2], planes, width, width, kappa),
            lambda: fe.products_trunc(ctx, opened, ta[:2], tb[:2], tab[:2], planes, 250, m, kappa),
            lambda: fe.tree_step(ctx, opened[:2], s[:2], 0, ta[:1], tb[:1], carry=carry),
            lambda: fe.tree_step(ctx, opened[:2], s[:2], 254, ta[:1], tb[:1], carry=carry),
            lambda: fe.tree_step(ctx, opened[:2], s[:2], m, ta[:2], tb[:1], carry=carry),
            lambda: fe.tree_step(ctx, opened[:1], s[:2], m, ta[:1], tb[:1]),
            lambda: fe.tree_step(ctx, opened[:2], s[:2], m, ta[:1], tb[:1], carry=carry[:-1]),
            lambda: fe.tree_step(ctx, opened[:2], s[:2], m, ta[:1], tb[:1], carry=carry, out=(c0[:-1], c1)),
            lambda: fe.finish_lookup_mask(ctx, [], tdev, 1, 5, count, nxt=nxt, **ops),
            lambda: fe.finish_lookup_mask(ctx, groups * 3, tdev, 1, 5, count, nxt=nxt, **ops),
            lambda: fe.finish_lookup_mask(ctx, [(7, 6, 0, 0, 0, 0)], tdev, 1, 5, count, nxt=nxt, **ops),
            lambda: fe.finish_lookup_mask(ctx, [(2, 0, 0, 0, 0, 0)], tdev, 1, 5, count, nxt=nxt, **ops),
            lambda: fe.finish_lookup_mask(ctx, groups, tdev, 1, 2, count, nxt=nxt, **ops),
            lambda: fe.finish_lookup_mask(ctx, groups[:1] * 2, tdev, 1, 5, count, nxt=nxt, **ops),
            lambda: fe.finish_lookup_mask(ctx, groups, tdev[:5], 1, 5, count, nxt=nxt, **ops),
            lambda: fe.finish_lookup_mask(ctx, groups, tdev, 1, 5, count, nxt=nxt[:1], **ops),
            lambda: fe.finish_lookup_mask(ctx, groups, tdev, 1, 5, count, nxt=nxt, **dict(ops, tab=ops["tab"][:-1])),
            lambda: fe.finish_lookup_mask(ctx, groups, tdev, 1, 5, count - 1, nxt=nxt, **ops)]):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"bad call {i} was accepted")
    # an output laid over an input is refused by the C ABI, through Python too
    for call in (lambda: fe.products_trunc(ctx, opened, ta[:2], tb[:2], tab[:2], planes, width, m, kappa, out=(opened[:2], b1)),
                 lambda: fe.products_trunc(ctx, opened, ta[:2], tb[:2], tab[:2], planes, width, m, kappa, out=(b0, b0)),
                 lambda: fe.products_trunc(ctx, opened, ta[:2], tb[:2], tab[:2], planes, width, m, kappa, out=(b0, planes[3:5])),
                 lambda: fe.tree_step(ctx, opened[:2], s[:2], m, ta[:1], tb[:1], carry=carry, out=(s[:2], c1)),
                 lambda: fe.tree_step(ctx, opened[:2], s[:2], m, ta[:1], tb[:1], carry=carry, out=(c0, carry)),
                 lambda: fe.finish_lookup_mask(ctx, groups, tdev, 1, 5, count, nxt=nxt, out=ops["opened"][:2], kept_out=a1, **ops),
                 lambda: fe.finish_lookup_mask(ctx, groups, tdev, 1, 5, count, nxt=nxt, out=a0, kept_out=ops["tab"][:5], **ops),
                 lambda: fe.finish_lookup_mask(ctx, groups, tdev, 1, 5, count, nxt=nxt, out=a1[:2], kept_out=a1, **ops)):
        with pytest.raises(HbmpcBackendError):
            call()
    # count == 0: a successful call that launches nothing
    lib, st, P = ctx.lib, ctx.stream(), ctx.ptr
    one = ctx.host_elems([1])
    assert lib.hb_fxexp_products_trunc(ctx.h, 2, P(opened), P(ta), P(tb), P(tab), P(planes), width, m, kappa, P(b0), P(b1), 0, st) == 0
    assert lib.hb_fxexp_tree_step(ctx.h, 2, P(opened), P(s), m, one.ctypes.data, P(carry), P(ta), P(tb), P(c0), P(c1), 0, st) == 0
    assert lib.hb_fxexp_products_trunc(ctx.h, 0, P(opened), P(ta), P(tb), P(tab), P(planes), width, m, kappa, P(b0), P(b1), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxexp_tree_step(ctx.h, 2, P(opened), P(s), m, None, P(carry), P(ta), P(tb), P(c0), P(c1), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxexp_tree_step(ctx.h, 2, P(opened), P(s), m, one.ctypes.data, P(carry), P(ta), P(tb), P(c0), P(c1), -1, st) == HB_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert bool((c0 == 7).all()) and torch.equal(b0, first[2]) and torch.equal(b1, first[3])


# ---- the protocol, end to end ---------------------------------------------------------------------------------------------------
async def _composed(co, x, bits, triples, demux_triples, f, k, kappa, g, natural):
    """the chain of fixedpoint_exp from what the package offered before: bit_decompose, demux, demux.lookup, share_arithmetic and
    fixedpoint.trunc_mask / trunc_pr_finish; the same preprocessing in the same order, the same opens -> the result shares"""
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd.progs import bit_decomposition as bd
    from honeybadgermpc_amd.progs import demux as dx
    from honeybadgermpc_amd.progs import fixedpoint as fx
    from honeybadgermpc_amd.progs import fixedpoint_division as fd
    from honeybadgermpc_amd.progs import fixedpoint_exp as fe

    ctx = co.ctx
    torch, L, p = ctx.torch, ctx.n_limbs, ctx.modulus
    lay = fe.exp_layout(k, f, kappa, g) if natural else fe.exp2_layout(k, f, kappa, g)
    n, width, s, nb = lay["bits"], lay["width"], k + fe.GUARD_BITS, lay["width"] + kappa
    count = x.shape[0]
    rows = fd._Rows(bits, triples)
    fractions, mi = lay["groups"], (k - 3).bit_length()
    G = len(fractions)
    widths = [w for _, w in fractions] + [mi + 1]

    async def truncate(vals, m):
        masks = [fx.trunc_mask(ctx, v, rows.planes(nb), width, m, kappa) for v in vals]
        opened = await co.open_share_array(torch.cat([mk for mk, _ in masks]))
        return [fx.trunc_pr_finish(ctx, v, opened[q * count:(q + 1) * count], masks[q][1], m) for q, v in enumerate(vals)]

    async def products(pairs, t):
        opened = await co.open_share_array(torch.cat([mk for q, (u, v) in enumerate(pairs) for mk in (sa.sub(ctx, u, t[0][q]), sa.sub(ctx, v, t[1][q]))]))
        return [sa.beaver_combine(ctx, opened[2 * q * count:(2 * q + 1) * count], opened[(2 * q + 1) * count:(2 * q + 2) * count], t[0][q], t[1][q], t[2][q]) for q in range(len(pairs))]

    if natural:
        Lc, fl = fe.exponent_factor(k)
        x, = await truncate([sa.mul(ctx, x, Lc % p)], fl)
    xp = sa.add(ctx, x, (f << f) % p)
    planes = await bd.bit_decompose(co, xp, rows.planes(n + 1 + kappa), rows.take(bd.bit_triples(n)), n + 1, n, kappa)
    group_bits = [planes[o:o + w].contiguous() for o, w in fractions] + [torch.cat([planes[f:f + mi], planes[n - 1:n]])]
    tables = fe.exp2_tables(k, f, g)
    first = rows.take(lay["tree"][0] if lay["tree"] else 1)
    stores = [dx.demux_groups(ctx, w, count) if w >= 2 else None for w in widths]
    onehot = [dx.demux_leaves(ctx, group_bits[j]) if w == 1 else None for j, w in enumerate(widths)]
    for level, (lv, (ta, tab)) in enumerate(zip(lay["demux_rows"], demux_triples)):      # the demultiplexer's own two launches a group a level, ONE open a level
        masks, spans, oo, po = [], [], 0, 0
        for j, orows, prows in lv:
            masks.append(dx.demux_mask(ctx, group_bits[j], stores[j], level, ta[oo:oo + orows]))
            spans.append((j, oo, orows, po, prows))
            oo, po = oo + orows, po + prows
        opened = (await co.open_share_array(torch.cat(masks).view(oo * count, L))).view(oo, count, L)
        for j, o, orows, q, prows in spans:
            onehot[j] = dx.demux_finish(ctx, opened[o:o + orows].contiguous(), stores[j], level, ta[o:o + orows], tab[q:q + prows])
    factors = [dx.lookup(ctx, onehot[j], [[t] for t in tables[j]])[0] for j in range(G + 1)]
    vals, u, t = factors[:G], factors[G], first
    for i, n_products in enumerate(lay["tree"]):
        prods = await products([(vals[2 * q], vals[2 * q + 1]) for q in range(n_products)], t)
        vals = await truncate(prods, s) + ([vals[-1]] if len(vals) & 1 else [])
        t = rows.take(1 if i == len(lay["tree"]) - 1 else lay["tree"][i + 1])
    out, = await truncate(await products([(vals[0], u)], t), s)
    return out


SMALL = [(8, 4, 8, 2), (16, 8, 8, 3)]
E2E = [(p, shape) for p in bc.GPU_FIELDS for shape in SMALL] + [(BLS, (64, 32, 32, 8))]
E2E_IDS = [f"{bc.GPU_FIELD_IDS[bc.GPU_FIELDS.index(p)]}-k{k}-f{f}-g{g}" for p, (k, f, kappa, g) in E2E]


def _deal(ctx, fe, dx, rnd, p, n, t, lay, k, kappa, count, natural):
    """bit planes with an all-ones r1 planted under the first and the last truncation of element 1, triples, demultiplexer triples, each
    with a canary row after its last -> (bits, trip, demux [party], r1s [element])"""
    n_planes, n_triples = lay["n_planes"], lay["n_triples"]
    bit_rows = [[rnd.getrandbits(1) for _ in range(count)] for _ in range(n_planes)]
    starts = ec.truncation_planes(lay, kappa)
    limits = ([k] if natural else []) + [k + fe.GUARD_BITS] * (len(starts) - (1 if natural else 0))
    for which in (0, len(starts) - 1):
        for i in range(limits[which]):
            bit_rows[starts[which] + i][1] = 1
    r1s = [[sum(bit_rows[s + i][e] << i for i in range(m)) for s, m in zip(starts, limits)] for e in range(count)]
    bit_rows.append([rnd.randrange(p) for _ in range(count)])              # a canary plane and canary rows: reading one would spoil the results
    ta, tb = ([[rnd.randrange(p) for _ in range(count)] for _ in range(n_triples)] for _ in range(2))
    tab = [[a * b % p for a, b in zip(ra, rb)] for ra, rb in zip(ta, tb)]
    for v in (ta, tb, tab):
        v.append([rnd.randrange(p) for _ in range(count)])
    widths = [w for _, w in lay["groups"]] + [(k - 3).bit_length() + 1]
    return (bc.deal_planes(ctx, rnd, p, n, t, bit_rows), [bc.deal_planes(ctx, rnd, p, n, t, v) for v in (ta, tb, tab)],
            ec.deal_demux_triples(ctx, fe, dx, rnd, p, n, t, lay, widths, count), r1s)


@pytest.mark.parametrize("natural", [False, True], ids=["exp2", "exp"])
@pytest.mark.parametrize("p, shape", E2E, ids=E2E_IDS)
def test_protocol_end_to_end(p, shape, natural):
    from fractions import Fraction

    from honeybadgermpc_amd.progs import demux as dx
    from honeybadgermpc_amd.progs import fixedpoint_exp as fe

    k, f, kappa, g = shape
    n, t, count = 4, 1, 16
    ctx = gpu_ctx(p)
    torch = ctx.torch
    rnd = random.Random(100 * k + f + natural + p % 7)
    bad = set(rnd.sample(range(n), 1))
    honest = [i for i in range(n) if i not in bad]
    lay = fe.exp_layout(k, f, kappa, g) if natural else fe.exp2_layout(k, f, kappa, g)
    n_planes, n_triples = lay["n_planes"], lay["n_triples"]
    pool = ec.operands(fe, rnd, k, f, g, natural, 8)
    xs = pool[:12] + rnd.sample(pool[12:], count - 12)
    bits, trip, demux_prep, r1s = _deal(ctx, fe, dx, rnd, p, n, t, lay, k, kappa, count, natural)
    vals = bc.deal_planes(ctx, rnd, p, n, t, [[x % p for x in xs]])
    fn = fe.exp if natural else fe.exp2

    async def body(co, i):
        x = vals[i][0]
        triples = tuple(tr[i] for tr in trip)
        exact_bits, exact_triples = bits[i][:n_planes], tuple(v[:n_triples] for v in triples)
        exact_demux = [(ta[:-1], tab[:-1]) for ta, tab in demux_prep[i]]
        keep = (vals[i].clone(), bits[i].clone(), [v.clone() for v in triples], [(a.clone(), b.clone()) for a, b in demux_prep[i]])
        for short in (lambda: fn(co, x, exact_bits, tuple(v[:n_triples - 1] for v in triples), exact_demux, f, k, kappa, g),
                      lambda: fn(co, x, exact_bits[:n_planes - 1], exact_triples, exact_demux, f, k, kappa, g),
                      lambda: fn(co, x, exact_bits, exact_triples, exact_demux[:-1], f, k, kappa, g),
                      lambda: fn(co, x, exact_bits, exact_triples, [(ta[:-1], tab) for ta, tab in exact_demux], f, k, kappa, g),
                      lambda: fn(co, x, exact_bits, exact_triples, exact_demux, f, k, kappa, 0),
                      lambda: fn(co, x, exact_bits, exact_triples, exact_demux, f, k, kappa, 13),
                      lambda: fn(co, x, exact_bits, exact_triples, exact_demux, k - 2, k, kappa, g)):
            with pytest.raises(ValueError):
                await short()
        assert co.batches == 0                                             # refused before anything was opened
        fused = await fn(co, x, bits[i], triples, demux_prep[i], f, k, kappa, g)
        batches = co.batches
        exact = await fn(co, x, exact_bits, exact_triples, exact_demux, f, k, kappa, g)
        before = co.batches
        composed = await _composed(co, x, exact_bits, exact_triples, exact_demux, f, k, kappa, g, natural)
        assert co.batches - before == batches                               # the same opens, composed or fused
        assert torch.equal(fused, exact) and torch.equal(fused, composed), i          # share for share
        opened = ctx.download_ints(await co.open_share_array(fused))
        assert torch.equal(vals[i], keep[0]) and torch.equal(bits[i], keep[1]) and all(torch.equal(v, w) for v, w in zip(triples, keep[2]))
        assert all(torch.equal(a, c) and torch.equal(b, d) for (a, b), (c, d) in zip(demux_prep[i], keep[3]))
        return opened, batches

    results = bc.run_parties(p, n, t, bad, rnd, body)
    model = fe.exp_model if natural else fe.exp2_model
    want = [model(xs[e], p, k, f, r1s[e], g) for e in range(count)]
    for e, w in enumerate(want):                                            # the inputs are in contract: the model is within the bound
        bound = fe.exp_error_bound(k, f, xs[e], g) if natural else fe.exp2_error_bound(k, f, g)
        assert ec.error_ulps(w, (ec.exp_enclosure if natural else ec.exp2_enclosure)(xs[e], f)) <= bound * (1 << ec.EXTRA), (e, xs[e], Fraction(w))
    for i in honest:
        opened, batches = results[i]
        assert opened == want, i
        assert batches == lay["opens"] == (fe.exp_opens if natural else fe.exp2_opens)(k, f, g)


def test_fixed_point_array_exp2_and_exp():
    from honeybadgermpc_amd.progs import demux as dx
    from honeybadgermpc_amd.progs import fixedpoint as fx
    from honeybadgermpc_amd.progs import fixedpoint_exp as fe

    p, (k, f, kappa, g), n, t, count = BLS, (16, 8, 8, 3), 4, 1, 16
    ctx = gpu_ctx(p)
    rnd = random.Random(169)
    xs = ec.operands(fe, rnd, k, f, g, True, 4)[:count]
    vals = bc.deal_planes(ctx, rnd, p, n, t, [[x % p for x in xs]])
    prep = {nat: _deal(ctx, fe, dx, rnd, p, n, t, fe.exp_layout(k, f, kappa, g) if nat else fe.exp2_layout(k, f, kappa, g), k, kappa, count, nat) for nat in (False, True)}

    async def body(co, i):
        arr = fx.FixedPointArray(co, vals[i][0], f, k, kappa)
        out = []
        for nat in (False, True):
            bits, trip, demux_prep, _ = prep[nat]
            res = await (arr.exp if nat else arr.exp2)(bits[i], tuple(tr[i] for tr in trip), demux_prep[i], g)
            assert isinstance(res, fx.FixedPointArray) and (res.f, res.k, res.kappa) == (f, k, kappa)
            out.append(ctx.download_ints(await co.open_share_array(res.shares)))
        return out

    for got in bc.run_parties(p, n, t, set(), rnd, body):
        assert got[0] == [fe.exp2_model(xs[e], p, k, f, prep[False][3][e], g) for e in range(count)]
        assert got[1] == [fe.exp_model(xs[e], p, k, f, prep[True][3][e], g) for e in range(count)]

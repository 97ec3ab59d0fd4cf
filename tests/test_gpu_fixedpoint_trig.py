"""GPU: honeybadgermpc_amd.progs.fixedpoint_trig -- every step of csrc/hb_fxtrig.hip bit-equal to its host self-test row (the same row, the
same step function), for every lane split, and to the step composed from what the package had (demux_finish + two demux.lookup + sub;
three beaver_combine + sub + trunc_mask; trunc_pr_finish + sub); inputs untouched, out= honoured, overlaps refused, nothing
synchronises; and the whole protocol among n = 4 parties in one process: sincos_turns and sincos open to exactly the model for the
dealt r1 -- no tolerance -- and their shares are bit-equal to the same chain composed from bit_decompose, demux, demux.lookup,
share_arithmetic and trunc_mask / trunc_pr_finish, in trig_opens batches."""
import random

import pytest

import bitdec_cases as bc
import exp_cases as ec
import trig_cases as tc
from bitdec_cases import COUNTS, gpu_ctx, random_tensor
from conftest import BLS
from trig_cases import BOTH, COS, CPRODUCTS_TRUNC, FINISH_LOOKUP_MASK, SIN, TREE_STEP

pytestmark = pytest.mark.gpu


# ---- the kernels ------------------------------------------------------------------------------------------------------------
def _lookup_case(ctx, fe, chosen, count, seed, kind):
    """operands of one finish_lookup_mask launch over the merges `chosen` ((1, 0): a group of one bit); kind 0: tables of arbitrary residues,
    1: short entries of both signs with zeros among them"""
    p = ctx.modulus
    rnd = random.Random(seed)
    groups, tables, oo, po = [], [], 0, 0
    slots = rnd.sample(range(len(chosen) + 2), len(chosen))
    top = min(p // 2, 1 << 67)
    for (wl, wh), slot in zip(chosen, slots):
        entries = 2 << (wl + wh)                                            # the cos table and, after it, the sin table
        table = [rnd.randrange(p) for _ in range(entries)] if kind == 0 else [0 if rnd.random() < 0.2 else rnd.choice((-1, 1)) * rnd.randrange(1, top + 1) for _ in range(entries)]
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


def _masked_rows(ctx, sa, re, im, mode, q, side, nxt):
    """{row of masked: tensor}: the composed masks of the value (re, im) as operand `side` of product q of a level in `mode`"""
    tp = tc.triples_of(mode)
    vals = [re, im] + ([sa.add(ctx, re, im)] if tp == 3 else [])
    return {2 * (tp * q + t) + side: sa.sub(ctx, vals[t], nxt[side][tp * q + t]) for t in range(tp)}


@pytest.mark.parametrize("p", bc.GPU_FIELDS, ids=bc.GPU_FIELD_IDS)
def test_finish_lookup_mask_equals_its_selftest_row_and_the_composed_step(p):
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd.progs import demux as dx
    from honeybadgermpc_amd.progs import fixedpoint_exp as fe
    from honeybadgermpc_amd.progs import fixedpoint_trig as ft

    ctx = gpu_ctx(p)
    torch, L = ctx.torch, ctx.n_limbs
    same = lambda got, want: torch.equal(got.cpu(), want)
    launches = [[m] for m in tc.MERGES] + [[(1, 0)], [(2, 2), (1, 0)], [(4, 3), (1, 1), (2, 1)]]
    for count in COUNTS:
        for li, chosen in enumerate(launches):
            if count == 5000 and sum(1 << (wl + wh) for wl, wh in chosen) > 64 and p >> 64 and chosen != [(4, 4)]:
                continue                                                    # the wide merges at the large count once: (4, 4)
            mode = (li + count) % 3
            tp = tc.triples_of(mode)
            groups, tables, tdev, ops = _lookup_case(ctx, fe, chosen, count, 500 + 7 * li + count, li & 1)
            pairs, kept_slots = 1, len(chosen) + 2
            nxt = (random_tensor(ctx, 600 + count, count, rows=tp * pairs), random_tensor(ctx, 601 + count, count, rows=tp * pairs))
            m0, k0 = random_tensor(ctx, 602 + count, count, rows=2 * tp * pairs), random_tensor(ctx, 603 + count, count, rows=2 * kept_slots)
            inputs = [tdev, nxt[0], nxt[1]] + list(ops.values())
            copies = [t.clone() for t in inputs]
            want = tc.selftest_on_tensors(ctx, FINISH_LOOKUP_MASK, [ops["bits"], ops["opened"], ops["ta"], ops["tab"], tdev, nxt[0], nxt[1]],
                                          [len(groups), pairs, kept_slots, mode, 1] + [v for grp in groups for v in grp], [2 * tp * pairs, 2 * kept_slots], count, outs_in=[m0, k0])
            for split in tc.SPLITS:                                             # every lane split: the bits of the host row
                masked, kept = ft.finish_lookup_mask(ctx, groups, tdev, pairs, kept_slots, count, mode=mode, split=split, nxt=nxt, out=m0.clone(), kept_out=k0.clone(), **ops)
                assert tuple(masked.shape) == (2 * tp * pairs, count, L) and tuple(kept.shape) == (2 * kept_slots, count, L)
                assert same(masked, want[0]) and same(kept, want[1]), (chosen, count, split)
            if count in (1, 257):                                               # ... and the composed step: the level's products, two table reads, the subs
                for wl, wh, oo, po, to, slot in groups:
                    n = 1 << (wl + wh)
                    ctab, stab = tables[to:to + n], tables[to + n:to + 2 * n]
                    if wh == 0:
                        re, im = (sa.add(ctx, sa.mul(ctx, ops["bits"][oo], (t[1] - t[0]) % p), t[0] % p) for t in (ctab, stab))
                    else:
                        d = [oo + (y & ((1 << wl) - 1)) for y in range(n)]
                        e = [oo + (1 << wl) + (y >> wl) for y in range(n)]
                        di, ei = (torch.tensor(v, dtype=torch.int64, device=ctx.tdev) for v in (d, e))
                        flat = [v.index_select(0, i).reshape(-1, L) for v, i in ((ops["opened"], di), (ops["opened"], ei), (ops["ta"], di), (ops["ta"], ei))]
                        onehot = sa.beaver_combine(ctx, *flat, ops["tab"][po:po + n].reshape(-1, L)).view(n, count, L)
                        re, im = dx.lookup(ctx, onehot, [[t % p] for t in ctab])[0], dx.lookup(ctx, onehot, [[t % p] for t in stab])[0]
                    assert torch.equal(kept[2 * slot], re) and torch.equal(kept[2 * slot + 1], im), (chosen, slot, count)
                    if slot < 2 * pairs:
                        for row, v in _masked_rows(ctx, sa, re, im, mode, slot >> 1, slot & 1, nxt).items():
                            assert torch.equal(masked[row], v), (chosen, slot, row, mode)
            assert all(torch.equal(t, cp) for t, cp in zip(inputs, copies))


@pytest.mark.parametrize("p", bc.GPU_FIELDS, ids=bc.GPU_FIELD_IDS)
def test_cproducts_trunc_and_tree_step_equal_their_selftest_rows_and_the_composed_steps(p):
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd.progs import fixedpoint as fx
    from honeybadgermpc_amd.progs import fixedpoint_trig as ft

    ctx = gpu_ctx(p)
    torch, L = ctx.torch, ctx.n_limbs
    same = lambda got, want: torch.equal(got.cpu(), want)
    width, kappa = (134, 32) if p >> 64 else (38, 8)
    nb = width + kappa
    for count in COUNTS:
        opened = random_tensor(ctx, 700 + count, count, rows=30)
        ta, tb, tab = (random_tensor(ctx, 701 + i + count, count, rows=15) for i in range(3))
        s = random_tensor(ctx, 704 + count, count, rows=10)
        carry = random_tensor(ctx, 706 + count, count, rows=2)
        inputs = [opened, ta, tb, tab, s, carry]
        copies = [t.clone() for t in inputs]
        for mode in (BOTH, COS, SIN):
            tp, comps = tc.triples_of(mode), tc.comps_of(mode)
            for products in (1, 2, 3, 4, 5) if count <= 257 else (1, 5):
                planes = random_tensor(ctx, 710 + products + count, count, rows=comps * products * nb)
                m = width // 2
                args = (opened[:2 * tp * products], ta[:tp * products], tb[:tp * products], tab[:tp * products], planes)
                masked, sv = ft.cproducts_trunc(ctx, products, mode, *args, width, m, kappa)
                want = tc.selftest_on_tensors(ctx, CPRODUCTS_TRUNC, list(args), [products, mode, width, m, kappa], [comps * products, comps * products], count)
                assert same(masked, want[0]) and same(sv, want[1]), (mode, products, count)
                if count in (1, 257):
                    for q in range(products):
                        pr = [sa.beaver_combine(ctx, opened[2 * r], opened[2 * r + 1], ta[r], tb[r], tab[r]) for r in range(tp * q, tp * q + tp)]
                        re = sa.sub(ctx, pr[0], pr[1])
                        vals = [re] if mode == COS else ([re] if mode == BOTH else []) + [sa.sub(ctx, sa.sub(ctx, pr[2], pr[0]), pr[1])]
                        for c, v in enumerate(vals):
                            row = comps * q + c
                            mk, r1 = fx.trunc_mask(ctx, v, planes[row * nb:(row + 1) * nb], width, m, kappa)
                            assert torch.equal(masked[row], mk) and torch.equal(sv[row], sa.add(ctx, v, r1)), (mode, products, q, c, count)
            for cvalues in (1, 2, 3, 4, 5) if count <= 257 else (1, 5):
                rows = 2 * cvalues
                for carried in (False, True):
                    for m in (1, 8, 61) + ((64, 127, 140) if p >> 64 else ()):
                        values = cvalues + carried
                        pairs = values // 2
                        trip = (ta[:tp * pairs] if pairs else None, tb[:tp * pairs] if pairs else None)
                        masked, kept = ft.tree_step(ctx, opened[:rows], s[:rows], m, mode=mode, ta=trip[0], tb=trip[1], carry=carry if carried else None)
                        want = tc.selftest_on_tensors(ctx, TREE_STEP, [opened[:rows], s[:rows], [pow(2, -m, p)], carry if carried else None, trip[0], trip[1]], [rows, 0, m, mode],
                                                      [2 * tp * pairs, 2 * (values & 1)], count)
                        assert (masked is None) == (pairs == 0) and (kept is None) == (values % 2 == 0)
                        assert (pairs == 0 or same(masked, want[0])) and (kept is None or same(kept, want[1])), (cvalues, carried, m, mode, count)
                        if count in (1, 257) and m in (8, 127):
                            zero = ctx.upload_ints([0] * count)
                            t = [fx.trunc_pr_finish(ctx, s[j], opened[j], zero, m) for j in range(rows)]
                            vals = [(t[2 * u], t[2 * u + 1]) for u in range(cvalues)] + ([(carry[0], carry[1])] if carried else [])
                            for u in range(2 * pairs):
                                for row, v in _masked_rows(ctx, sa, vals[u][0], vals[u][1], mode, u >> 1, u & 1, trip).items():
                                    assert torch.equal(masked[row], v), (cvalues, carried, m, mode, u, row)
                            if values & 1:
                                assert torch.equal(kept[0], vals[-1][0]) and torch.equal(kept[1], vals[-1][1])
        for rows in (1, 2):                                                     # final: the results
            for m in (8, 61) + ((127,) if p >> 64 else ()):
                none, res = ft.tree_step(ctx, opened[:rows], s[:rows], m, final=True)
                want = tc.selftest_on_tensors(ctx, TREE_STEP, [opened[:rows], s[:rows], [pow(2, -m, p)], None, None, None], [rows, 1, m, 0], [0, rows], count)
                assert none is None and same(res, want[1])
                if count in (1, 257):
                    zero = ctx.upload_ints([0] * count)
                    assert all(torch.equal(res[j], fx.trunc_pr_finish(ctx, s[j], opened[j], zero, m)) for j in range(rows))
        assert all(torch.equal(t, cp) for t, cp in zip(inputs, copies))


def test_out_honoured_overlap_refused_and_asynchronous():
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd._capi import HB_ERR_BAD_ARG, HbmpcBackendError
    from honeybadgermpc_amd.progs import fixedpoint_exp as fe
    from honeybadgermpc_amd.progs import fixedpoint_trig as ft

    p, count, width, kappa, m = BLS, 600, 134, 32, 66
    ctx = gpu_ctx(p)
    torch = ctx.torch
    groups, tables, tdev, ops = _lookup_case(ctx, fe, [(2, 2), (1, 0), (2, 1)], count, 800, 1)
    nxt = (random_tensor(ctx, 801, count, rows=3), random_tensor(ctx, 802, count, rows=3))
    opened = random_tensor(ctx, 803, count, rows=12)
    ta, tb, tab = (random_tensor(ctx, 804 + i, count, rows=6) for i in range(3))
    s = random_tensor(ctx, 808, count, rows=4)
    planes = random_tensor(ctx, 810, count, rows=4 * (width + kappa))
    carry = random_tensor(ctx, 811, count, rows=2)
    m0, k0 = random_tensor(ctx, 812, count, rows=6), random_tensor(ctx, 813, count, rows=10)

    def run():
        a = ft.finish_lookup_mask(ctx, groups, tdev, 1, 5, count, split=4, nxt=nxt, out=m0.clone(), kept_out=k0.clone(), **ops)
        b = ft.cproducts_trunc(ctx, 2, BOTH, opened, ta, tb, tab, planes, width, m, kappa)
        c = ft.tree_step(ctx, opened[:4], s, m, mode=BOTH, ta=ta[:3], tb=tb[:3], carry=carry)
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
    got = ft.cproducts_trunc(ctx, 2, BOTH, opened, ta, tb, tab, planes, width, m, kappa, out=(b0, b1))
    assert got[0].data_ptr() == b0.data_ptr() and got[1].data_ptr() == b1.data_ptr() and torch.equal(b0, first[2]) and torch.equal(b1, first[3])
    c0, c1 = torch.empty_like(first[4]), torch.empty_like(first[5])
    got = ft.tree_step(ctx, opened[:4], s, m, mode=BOTH, ta=ta[:3], tb=tb[:3], carry=carry, out=(c0, c1))
    assert got[0].data_ptr() == c0.data_ptr() and got[1].data_ptr() == c1.data_ptr() and torch.equal(c0, first[4]) and torch.equal(c1, first[5])
    a0, a1 = m0.clone(), k0.clone()
    got = ft.finish_lookup_mask(ctx, groups, tdev, 1, 5, count, nxt=nxt, out=a0, kept_out=a1, **ops)
    assert got[0].data_ptr() == a0.data_ptr() and got[1].data_ptr() == a1.data_ptr() and torch.equal(a0, first[0]) and torch.equal(a1, first[1])
    # ValueError before C for shapes
    c0.fill_(7)
    for i, call in enumerate([
            lambda: ft.cproducts_trunc(ctx, 2, BOTH, opened[:11], ta, tb, tab, planes, width, m, kappa),
            lambda: ft.cproducts_trunc(ctx, 2, BOTH, opened, ta, tb[:5], tab, planes, width, m, kappa),
            lambda: ft.cproducts_trunc(ctx, 2, BOTH, opened, ta, tb, tab, planes[:-1], width, m, kappa),
            lambda: ft.cproducts_trunc(ctx, 2, BOTH, opened, ta, tb, tab, planes, width, width, kappa),
            lambda: ft.cproducts_trunc(ctx, 2, BOTH, opened, ta, tb, tab, planes, 250, m, kappa),
            lambda: ft.cproducts_trunc(ctx, 2, 3, opened, ta, tb, tab, planes, width, m, kappa),
            lambda: ft.cproducts_trunc(ctx, 2, COS, opened, ta, tb, tab, planes, width, m, kappa),          # two triples a product in that mode
            lambda: ft.cproducts_trunc(ctx, 65, BOTH, opened, ta, tb, tab, planes, width, m, kappa),
            lambda: ft.tree_step(ctx, opened[:4], s, 0, ta=ta[:3], tb=tb[:3], carry=carry),
            lambda: ft.tree_step(ctx, opened[:4], s, 254, ta=ta[:3], tb=tb[:3], carry=carry),
            lambda: ft.tree_step(ctx, opened[:4], s, m, ta=ta[:4], tb=tb[:3], carry=carry),
            lambda: ft.tree_step(ctx, opened[:3], s, m, ta=ta[:3], tb=tb[:3]),
            lambda: ft.tree_step(ctx, opened[:3], s[:3], m, ta=ta[:3], tb=tb[:3]),                          # two rows a complex value
            lambda: ft.tree_step(ctx, opened[:4], s, m, ta=ta[:3], tb=tb[:3], carry=carry[:1]),
            lambda: ft.tree_step(ctx, opened[:4], s, m, carry=carry, final=True),
            lambda: ft.tree_step(ctx, opened[:4], s, m, mode=5, ta=ta[:3], tb=tb[:3], carry=carry),
            lambda: ft.tree_step(ctx, opened[:4], s, m, ta=ta[:3], tb=tb[:3], carry=carry, out=(c0[:-1], c1)),
            lambda: ft.finish_lookup_mask(ctx, [], tdev, 1, 5, count, nxt=nxt, **ops),
            lambda: ft.finish_lookup_mask(ctx, groups * 3, tdev, 1, 5, count, nxt=nxt, **ops),
            lambda: ft.finish_lookup_mask(ctx, [(7, 6, 0, 0, 0, 0)], tdev, 1, 5, count, nxt=nxt, **ops),
            lambda: ft.finish_lookup_mask(ctx, [(2, 0, 0, 0, 0, 0)], tdev, 1, 5, count, nxt=nxt, **ops),
            lambda: ft.finish_lookup_mask(ctx, groups, tdev, 1, 2, count, nxt=nxt, **ops),
            lambda: ft.finish_lookup_mask(ctx, groups[:1] * 2, tdev, 1, 5, count, nxt=nxt, **ops),
            lambda: ft.finish_lookup_mask(ctx, groups, tdev[:-1], 1, 5, count, nxt=nxt, **ops),
            lambda: ft.finish_lookup_mask(ctx, groups, tdev, 1, 5, count, nxt=nxt[:1], **ops),
            lambda: ft.finish_lookup_mask(ctx, groups, tdev, 1, 5, count, nxt=(nxt[0][:2], nxt[1]), **ops),
            lambda: ft.finish_lookup_mask(ctx, groups, tdev, 1, 5, count, split=3, nxt=nxt, **ops),
            lambda: ft.finish_lookup_mask(ctx, groups, tdev, 1, 5, count, split=32, nxt=nxt, **ops),
            lambda: ft.finish_lookup_mask(ctx, groups, tdev, 1, 5, count, mode=3, nxt=nxt, **ops),
            lambda: ft.finish_lookup_mask(ctx, groups, tdev, 1, 5, count, nxt=nxt, **dict(ops, tab=ops["tab"][:-1])),
            lambda: ft.finish_lookup_mask(ctx, groups, tdev, 1, 5, count - 1, nxt=nxt, **ops)]):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"bad call {i} was accepted")
    # an output laid over an input is refused by the C ABI, through Python too
    for call in (lambda: ft.cproducts_trunc(ctx, 2, BOTH, opened, ta, tb, tab, planes, width, m, kappa, out=(opened[:4], b1)),
                 lambda: ft.cproducts_trunc(ctx, 2, BOTH, opened, ta, tb, tab, planes, width, m, kappa, out=(b0, b0)),
                 lambda: ft.cproducts_trunc(ctx, 2, BOTH, opened, ta, tb, tab, planes, width, m, kappa, out=(b0, planes[3:7])),
                 lambda: ft.tree_step(ctx, opened[:4], s, m, ta=ta[:3], tb=tb[:3], carry=carry, out=(opened[2:8], c1)),
                 lambda: ft.tree_step(ctx, opened[:4], s, m, ta=ta[:3], tb=tb[:3], carry=carry, out=(c0, carry)),
                 lambda: ft.tree_step(ctx, opened[:4], s, m, final=True, out=(None, s)),
                 lambda: ft.finish_lookup_mask(ctx, groups, tdev, 1, 5, count, nxt=nxt, out=opened[:6], kept_out=ops["tab"][:10], **ops),
                 lambda: ft.finish_lookup_mask(ctx, groups, tdev, 1, 5, count, nxt=nxt, out=a0, kept_out=ops["opened"][:10], **ops),
                 lambda: ft.finish_lookup_mask(ctx, groups, tdev, 1, 5, count, nxt=nxt, out=a1[:6], kept_out=a1, **ops)):
        with pytest.raises(HbmpcBackendError):
            call()
    # count == 0: a successful call that launches nothing
    lib, st, P = ctx.lib, ctx.stream(), ctx.ptr
    one = ctx.host_elems([1])
    assert lib.hb_fxtrig_cproducts_trunc(ctx.h, 2, 0, P(opened), P(ta), P(tb), P(tab), P(planes), width, m, kappa, P(b0), P(b1), 0, st) == 0
    assert lib.hb_fxtrig_tree_step(ctx.h, 4, 0, P(opened), P(s), m, one.ctypes.data, P(carry), 0, P(ta), P(tb), P(c0), P(c1), 0, st) == 0
    assert lib.hb_fxtrig_cproducts_trunc(ctx.h, 0, 0, P(opened), P(ta), P(tb), P(tab), P(planes), width, m, kappa, P(b0), P(b1), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxtrig_tree_step(ctx.h, 4, 0, P(opened), P(s), m, None, P(carry), 0, P(ta), P(tb), P(c0), P(c1), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxtrig_tree_step(ctx.h, 4, 0, P(opened), P(s), m, one.ctypes.data, P(carry), 0, P(ta), P(tb), P(c0), P(c1), -1, st) == HB_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert bool((c0 == 7).all()) and torch.equal(b0, first[2]) and torch.equal(b1, first[3])


# ---- the protocol, end to end ---------------------------------------------------------------------------------------------------
async def _composed(co, x, bits, triples, demux_triples, f, k, kappa, g, radians, want):
    """the chain of fixedpoint_trig from what the package offered before: bit_decompose, demux, demux.lookup, share_arithmetic and
    fixedpoint.trunc_mask / trunc_pr_finish; the same preprocessing in the same order, the same opens -> the result shares in `want`'s order"""
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd.progs import bit_decomposition as bd
    from honeybadgermpc_amd.progs import demux as dx
    from honeybadgermpc_amd.progs import fixedpoint as fx
    from honeybadgermpc_amd.progs import fixedpoint_division as fd
    from honeybadgermpc_amd.progs import fixedpoint_trig as ft

    ctx = co.ctx
    torch, L, p = ctx.torch, ctx.n_limbs, ctx.modulus
    lay = ft.trig_layout(k, f, kappa, g, radians, want)
    fbits, width, nb, groups = lay["ft"], lay["width"], lay["width"] + kappa, lay["groups"]
    count = x.shape[0]
    rows = fd._Rows(bits, triples)
    G, widths = len(groups), [w for _, w in groups]

    async def truncate(vals, wd, m):
        masks = [fx.trunc_mask(ctx, v, rows.planes(wd + kappa), wd, m, kappa) for v in vals]
        opened = await co.open_share_array(torch.cat([mk for mk, _ in masks]))
        return [fx.trunc_pr_finish(ctx, v, opened[q * count:(q + 1) * count], masks[q][1], m) for q, v in enumerate(vals)]

    if radians:
        Lc, _, m = ft.turn_factor(k)
        x, = await truncate([sa.mul(ctx, x, Lc % p)], lay["turn_width"], m)
    planes = await bd.bit_decompose(co, x, rows.planes(lay["kv"] + kappa), rows.take(bd.bit_triples(fbits)), lay["kv"], fbits, kappa)
    group_bits = [planes[o:o + w].contiguous() for o, w in groups]
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
    vals = [tuple(dx.lookup(ctx, onehot[j], [[v % p] for v in t])[0] for t in tabs) for j, tabs in enumerate(ft.trig_tables(k, f, g, radians))]
    for products, mode, m in zip(lay["tree"], lay["modes"], lay["shifts"]):
        tp = tc.triples_of(mode)
        t = rows.take(products * tp)
        operands = [[a, b] + ([sa.add(ctx, a, b)] if tp == 3 else []) for a, b in vals[:2 * products]]
        opened = await co.open_share_array(torch.cat([sa.sub(ctx, operands[2 * q + side][i], t[side][tp * q + i]) for q in range(products) for i in range(tp) for side in (0, 1)]))
        prods = [sa.beaver_combine(ctx, opened[2 * r * count:(2 * r + 1) * count], opened[(2 * r + 1) * count:(2 * r + 2) * count], t[0][r], t[1][r], t[2][r]) for r in range(products * tp)]
        comps = []
        for q in range(products):
            pr = prods[tp * q:tp * q + tp]
            comps += ([sa.sub(ctx, pr[0], pr[1])] if mode != SIN else []) + ([sa.sub(ctx, sa.sub(ctx, pr[2], pr[0]), pr[1])] if mode != COS else [])
        done = await truncate(comps, width, m)
        if mode != BOTH:
            return (done[0],)
        vals = [(done[2 * q], done[2 * q + 1]) for q in range(products)] + ([vals[-1]] if len(vals) & 1 else [])
    return tuple(vals[0][0] if n == "cos" else vals[0][1] for n in want)


SMALL = [(8, 4, 8, 4), (8, 4, 8, 2), (16, 8, 8, 3)]                     # one group; two; an odd number of them
E2E = [(p, shape) for p in (BLS, bc.P64) for shape in SMALL] + [(BLS, (64, 32, 32, 8))]
E2E_IDS = [f"{bc.GPU_FIELD_IDS[bc.GPU_FIELDS.index(p)]}-k{k}-f{f}-g{g}" for p, (k, f, kappa, g) in E2E]


def _deal(ctx, ft, dx, rnd, p, n, t, lay, limits, kappa, count):
    """bit planes with an all-ones r1 planted under the first and the last truncation of element 1 (limits: trig_shifts), triples,
    demultiplexer triples, each with a canary row after its last -> (bits, trip, demux [party], r1s [element])"""
    n_planes, n_triples = lay["n_planes"], lay["n_triples"]
    bit_rows = [[rnd.getrandbits(1) for _ in range(count)] for _ in range(n_planes)]
    starts = [s for s, _ in tc.truncation_planes(lay, kappa)]
    assert len(starts) == len(limits)
    for which in {0, len(starts) - 1} if starts else ():
        for i in range(limits[which]):
            bit_rows[starts[which] + i][1] = 1
    r1s = [[sum(bit_rows[s + i][e] << i for i in range(m)) for s, m in zip(starts, limits)] for e in range(count)]
    ta, tb = ([[rnd.randrange(p) for _ in range(count)] for _ in range(n_triples)] for _ in range(2))
    tab = [[a * b % p for a, b in zip(ra, rb)] for ra, rb in zip(ta, tb)]
    canary = lambda: [rnd.randrange(p) for _ in range(count)]                  # a canary plane and canary rows: reading one would spoil the results
    widths = [w for _, w in lay["groups"]]
    return (bc.deal_planes(ctx, rnd, p, n, t, bit_rows + [canary()]), [bc.deal_planes(ctx, rnd, p, n, t, v + [canary()]) for v in (ta, tb, tab)],
            ec.deal_demux_triples(ctx, ft, dx, rnd, p, n, t, lay, widths, count), r1s)


@pytest.mark.parametrize("radians", [False, True], ids=["turns", "radians"])
@pytest.mark.parametrize("p, shape", E2E, ids=E2E_IDS)
def test_protocol_end_to_end(p, shape, radians):
    from honeybadgermpc_amd.progs import demux as dx
    from honeybadgermpc_amd.progs import fixedpoint_trig as ft

    k, f, kappa, g = shape
    n, t, count = 4, 1, 32 if k == 64 else 16
    ctx = gpu_ctx(p)
    torch = ctx.torch
    rnd = random.Random(100 * k + f + g + radians + p % 7)
    bad = set(rnd.sample(range(n), 1))
    honest = [i for i in range(n) if i not in bad]
    want = ("sin", "cos")
    lay = ft.trig_layout(k, f, kappa, g, radians, want)
    n_planes, n_triples, nb = lay["n_planes"], lay["n_triples"], lay["width"] + kappa
    pool = tc.operands(rnd, k, f, 8)
    xs = rnd.sample(pool, count)
    bits, trip, demux_prep, r1s = _deal(ctx, ft, dx, rnd, p, n, t, lay, ft.trig_shifts(k, f, g, radians, want), kappa, count)
    vals = bc.deal_planes(ctx, rnd, p, n, t, [[x % p for x in xs]])
    fn = ft.sincos if radians else ft.sincos_turns

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
                      lambda: fn(co, x, exact_bits, exact_triples, exact_demux, f, k, kappa, g, ("tan",)),
                      lambda: fn(co, x, exact_bits, exact_triples, exact_demux, f, k, kappa, g, want, 3),
                      lambda: fn(co, x, exact_bits, exact_triples, exact_demux, k, k, kappa, g),
                      lambda: fn(co, x, exact_bits, exact_triples, exact_demux, f, k, 200, g)):
            with pytest.raises(ValueError):
                await short()
        assert co.batches == 0                                             # refused before anything was opened
        fused = await fn(co, x, bits[i], triples, demux_prep[i], f, k, kappa, g)
        batches = co.batches
        exact = await fn(co, x, exact_bits, exact_triples, exact_demux, f, k, kappa, g, want, 4)         # another lane split: the same shares
        before = co.batches
        composed = await _composed(co, x, exact_bits, exact_triples, exact_demux, f, k, kappa, g, radians, want)
        assert co.batches - before == batches                               # the same opens, composed or fused
        assert all(torch.equal(a, b) for a, b in zip(fused, exact)), i
        assert all(torch.equal(a, c) for a, c in zip(fused, composed)), i      # share for share
        # want of one component: that component's same shares, from the rows the pair's run read for it
        if lay["tree"]:
            last = lay["planes"][f"tree{len(lay['tree']) - 1}"][0]
            sin_bits = torch.cat([exact_bits[:last], exact_bits[last + nb:last + 2 * nb]])
            cos_only = await fn(co, x, exact_bits[:n_planes - nb], tuple(v[:n_triples - 1] for v in triples), exact_demux, f, k, kappa, g, ("cos",))
            sin_only = await fn(co, x, sin_bits, exact_triples, exact_demux, f, k, kappa, g, ("sin",))
        else:
            cos_only = await fn(co, x, exact_bits, exact_triples, exact_demux, f, k, kappa, g, ("cos",))
            sin_only = await fn(co, x, exact_bits, exact_triples, exact_demux, f, k, kappa, g, ("sin",))
        assert len(cos_only) == len(sin_only) == 1 and torch.equal(sin_only[0], fused[0]) and torch.equal(cos_only[0], fused[1])
        swapped = await fn(co, x, exact_bits, exact_triples, exact_demux, f, k, kappa, g, ("cos", "sin"))
        assert torch.equal(swapped[0], fused[1]) and torch.equal(swapped[1], fused[0])
        opened = [ctx.download_ints(await co.open_share_array(v)) for v in fused]
        assert torch.equal(vals[i], keep[0]) and torch.equal(bits[i], keep[1]) and all(torch.equal(v, w) for v, w in zip(triples, keep[2]))
        assert all(torch.equal(a, c) and torch.equal(b, d) for (a, b), (c, d) in zip(demux_prep[i], keep[3]))
        return opened, batches

    results = bc.run_parties(p, n, t, bad, rnd, body)
    model = ft.sincos_model if radians else ft.sincos_turns_model
    expect = [model(xs[e], p, k, f, r1s[e], g) for e in range(count)]
    bound = ft.trig_error_bound(k, f, g, radians)
    for e, w in enumerate(expect):                                          # the model is within the bound
        enc = (tc.radians_enclosure if radians else tc.turns_enclosure)(xs[e], f)
        assert all(tc.error_ulps(tc.centered(v, p), enc[name]) <= bound * (1 << tc.EXTRA) for name, v in zip(want, w)), (e, xs[e])
    for i in honest:
        opened, batches = results[i]
        assert list(zip(*opened)) == expect, i
        assert batches == lay["opens"] == ft.trig_opens(k, f, g, radians)


def test_fixed_point_array_sincos():
    from honeybadgermpc_amd.progs import demux as dx
    from honeybadgermpc_amd.progs import fixedpoint as fx
    from honeybadgermpc_amd.progs import fixedpoint_trig as ft

    p, (k, f, kappa, g), n, t, count = BLS, (16, 8, 8, 3), 4, 1, 16
    ctx = gpu_ctx(p)
    rnd = random.Random(171)
    xs = tc.operands(rnd, k, f, 4)[:count]
    vals = bc.deal_planes(ctx, rnd, p, n, t, [[x % p for x in xs]])
    cases = [("sincos_turns", False, ("sin", "cos")), ("sincos", True, ("sin", "cos")), ("sin", True, ("sin",)), ("cos", True, ("cos",))]
    prep = [_deal(ctx, ft, dx, rnd, p, n, t, ft.trig_layout(k, f, kappa, g, radians, want), ft.trig_shifts(k, f, g, radians, want), kappa, count) for _, radians, want in cases]

    async def body(co, i):
        arr = fx.FixedPointArray(co, vals[i][0], f, k, kappa)
        out = []
        for (name, _, want), (bits, trip, demux_prep, _) in zip(cases, prep):
            res = await getattr(arr, name)(bits[i], tuple(tr[i] for tr in trip), demux_prep[i], g)
            res = res if isinstance(res, tuple) else (res,)
            assert len(res) == len(want) and all(isinstance(r, fx.FixedPointArray) and (r.f, r.k, r.kappa) == (f, k, kappa) for r in res)
            out.append([ctx.download_ints(await co.open_share_array(r.shares)) for r in res])
        return out

    for got in bc.run_parties(p, n, t, set(), rnd, body):
        for (name, radians, want), (_, _, _, r1s), res in zip(cases, prep, got):
            model = ft.sincos_model if radians else ft.sincos_turns_model
            assert list(zip(*res)) == [model(xs[e], p, k, f, r1s[e], g, want) for e in range(count)], name

"""GPU: honeybadgermpc_amd.progs.bit_decomposition -- the kernels of csrc/hb_bd.hip against Python ints and, bit for bit, against the
same steps composed from share_arithmetic (what the package offered before), the in-place level update, and the whole protocol over
OpenCoalescers in one process: bit_decompose, difference_bits and FixedPointArray.bits open to exactly bits_model -- no tolerance, the
result does not depend on the masks -- in bit_opens(m) batches from bit_triples(m) triple rows."""
import random

import pytest

import bitdec_cases as bc
from bitdec_cases import COUNTS, gpu_ctx, random_tensor, rows_of, sample
from conftest import BLS

pytestmark = pytest.mark.gpu


def _corners(ctx, c, m, count):
    if count >= 255:
        p = ctx.modulus
        c[:4] = ctx.upload_ints([0, (1 << m) - 1, (1 << m) % p, p - 1])


def _leaf_composed(ctx, sa, c, b, i):
    """the leaf of bit i from share_arithmetic: generate = a (1 - b), propagate = a + (1 - b) - 2 generate"""
    a, nb = bc.bit_elem(ctx, c, i), sa.add(ctx, sa.neg(ctx, b), 1)
    gen = sa.mul(ctx, a, nb)
    return gen, sa.sub(ctx, sa.add(ctx, a, nb), sa.mul(ctx, gen, 2))


# ---- the kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", bc.GPU_FIELDS, ids=bc.GPU_FIELD_IDS)
def test_leaf_and_sum_kernels(p):
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd.progs import bit_decomposition as bd

    ctx = gpu_ctx(p)
    torch = ctx.torch
    for k, m, kappa in bc.gpu_shapes(p):
        n = m - 1
        for count in COUNTS:
            checked = range(m) if m <= 9 or count <= 257 else (0, 1, 2, m - 2, m - 1)      # every plane is composed at the smaller counts
            c, bits = random_tensor(ctx, 5 + count, count), random_tensor(ctx, 6 + count, count, rows=m + 1)    # a plane more than needed is fine
            _corners(ctx, c, m, count)
            keep = (c.clone(), bits.clone())
            g, q = bd.sub_leaves(ctx, c, bits, m)
            assert tuple(g.shape) == tuple(q.shape) == (n, count, ctx.n_limbs)
            zero = ctx.upload_ints([0] * count)
            leaf_p = {}
            for i in checked:
                gen, prop = _leaf_composed(ctx, sa, c, bits[i], i)
                leaf_p[i] = prop
                if i == 0 and n:
                    assert torch.equal(g[0], sa.add(ctx, gen, prop)) and torch.equal(q[0], zero), (m, count)
                elif i < n:
                    assert torch.equal(g[i], gen) and torch.equal(q[i], prop), (m, count, i)
            idx = sample(count)[:16]
            if count:
                sel = torch.tensor(idx, device=ctx.tdev)
                cs, planes = ctx.download_ints(c.index_select(0, sel)), rows_of(ctx, bits.index_select(1, sel))
            if count and n:
                gs, qs = rows_of(ctx, g.index_select(1, sel)), rows_of(ctx, q.index_select(1, sel))
                for i in range(n):
                    for e, cv in enumerate(cs):
                        gg, qq = bc.leaf((cv >> i) & 1, planes[i][e], p)
                        assert (gs[i][e], qs[i][e]) == (((gg + qq) % p, 0) if i == 0 else (gg, qq)), (m, count, i, e)
            # the sum step over carries of any residues
            carries = random_tensor(ctx, 7 + count, count, rows=n)
            ta, tb, tab = (random_tensor(ctx, 8 + s + count, count, rows=n) for s in range(3))
            opened = random_tensor(ctx, 11 + count, count, rows=2 * n)
            keep2 = (carries.clone(), ta.clone(), tb.clone(), tab.clone(), opened.clone())
            masked = bd.sum_mask(ctx, c, bits, carries, m, ta, tb)
            out = bd.sum_combine(ctx, opened.view(2 * n * count, ctx.n_limbs), c, bits, carries, m, ta, tb, tab)     # flat, as an open returns it
            assert tuple(masked.shape) == (2 * n, count, ctx.n_limbs) and tuple(out.shape) == (m, count, ctx.n_limbs)
            a0 = bc.bit_elem(ctx, c, 0)
            assert torch.equal(out[0], sa.sub(ctx, sa.add(ctx, a0, bits[0]), sa.mul(ctx, sa.mul(ctx, a0, bits[0]), 2))), (m, count)
            for i in checked:
                if i == 0:
                    continue
                t = i - 1
                assert torch.equal(masked[2 * t], sa.sub(ctx, leaf_p[i], ta[t])) and torch.equal(masked[2 * t + 1], sa.sub(ctx, carries[t], tb[t])), (m, count, i)
                prod = sa.beaver_combine(ctx, opened[2 * t], opened[2 * t + 1], ta[t], tb[t], tab[t])
                assert torch.equal(out[i], sa.sub(ctx, sa.add(ctx, leaf_p[i], carries[t]), sa.mul(ctx, prod, 2))), (m, count, i)
            if count:
                outs = rows_of(ctx, out.index_select(1, sel))
                assert [outs[0][e] for e in range(len(idx))] == [(1 - planes[0][e]) % p if cv & 1 else planes[0][e] for e, cv in enumerate(cs)]
            if count and n:
                o, a, b, ab, cr, mk = (rows_of(ctx, v.index_select(1, sel)) for v in (opened, ta, tb, tab, carries, masked))
                for i in range(1, m):
                    t = i - 1
                    for e, cv in enumerate(cs):
                        lp = bc.leaf((cv >> i) & 1, planes[i][e], p)[1]
                        assert (mk[2 * t][e], mk[2 * t + 1][e]) == ((lp - a[t][e]) % p, (cr[t][e] - b[t][e]) % p), (m, count, i, e)
                        assert outs[i][e] == (lp + cr[t][e] - 2 * bc.beaver(o[2 * t][e], o[2 * t + 1][e], a[t][e], b[t][e], ab[t][e], p)) % p, (m, count, i, e)
            assert torch.equal(c, keep[0]) and torch.equal(bits, keep[1])
            assert all(torch.equal(v, w) for v, w in zip((carries, ta, tb, tab, opened), keep2))


@pytest.mark.parametrize("p", bc.GPU_FIELDS, ids=bc.GPU_FIELD_IDS)
def test_prefix_level_kernels_in_place(p):
    """every level of every shape over planes of any residues: the mask's rows, the nodes' new values, and every plane the level does
    not own exactly as it was"""
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd.progs import bit_decomposition as bd

    ctx = gpu_ctx(p)
    torch = ctx.torch
    for k, m, kappa in bc.gpu_shapes(p):
        n = m - 1
        for count in COUNTS:
            for level in range(bd.prefix_levels(m)):
                nodes, rows = bd.prefix_nodes(n, level), bc.triple_rows(bd, n, level)
                triples = bd.prefix_level_triples(m, level)
                g, q = random_tensor(ctx, 20 + count + level, count, rows=n), random_tensor(ctx, 21 + count + level, count, rows=n)
                ta, tb, tab = (random_tensor(ctx, 22 + s + count, count, rows=triples) for s in range(3))
                opened = random_tensor(ctx, 25 + count, count, rows=2 * triples)
                g0, q0 = g.clone(), q.clone()
                keep = (ta.clone(), tb.clone(), tab.clone(), opened.clone())
                masked = bd.prefix_mask(ctx, g, q, level, ta, tb)
                assert tuple(masked.shape) == (2 * triples, count, ctx.n_limbs)
                assert torch.equal(g, g0) and torch.equal(q, q0)
                res = bd.prefix_combine(ctx, opened.view(2 * triples * count, ctx.n_limbs), g, q, level, ta, tb, tab)
                assert res[0].data_ptr() == g.data_ptr() and res[1].data_ptr() == q.data_ptr()
                some = nodes if n <= 8 or count <= 257 else nodes[:2] + nodes[-2:]
                for j, part, g_only in some:
                    r0, r1 = rows[nodes.index((j, part, g_only))]
                    assert torch.equal(masked[2 * r0], sa.sub(ctx, q0[j], ta[r0])) and torch.equal(masked[2 * r0 + 1], sa.sub(ctx, g0[part], tb[r0])), (m, level, j)
                    assert torch.equal(g[j], sa.add(ctx, g0[j], sa.beaver_combine(ctx, opened[2 * r0], opened[2 * r0 + 1], ta[r0], tb[r0], tab[r0]))), (m, level, j)
                    if g_only:
                        assert torch.equal(q[j], q0[j]), (m, level, j)
                    else:
                        assert torch.equal(masked[2 * r1], sa.sub(ctx, q0[j], ta[r1])) and torch.equal(masked[2 * r1 + 1], sa.sub(ctx, q0[part], tb[r1])), (m, level, j)
                        assert torch.equal(q[j], sa.beaver_combine(ctx, opened[2 * r1], opened[2 * r1 + 1], ta[r1], tb[r1], tab[r1])), (m, level, j)
                owned = {j for j, _, _ in nodes}
                for i in range(n):
                    if i not in owned:
                        assert torch.equal(g[i], g0[i]) and torch.equal(q[i], q0[i]), (m, level, i)
                assert all(torch.equal(v, w) for v, w in zip((ta, tb, tab, opened), keep))
                if count:
                    sel = torch.tensor(sample(count)[:8], device=ctx.tdev)
                    o, a, b, ab, gi, qi, g1, q1, mk = (rows_of(ctx, v.index_select(1, sel)) for v in (opened, ta, tb, tab, g0, q0, g, q, masked))
                    for (j, part, g_only), (r0, r1) in zip(nodes, rows):
                        for e in range(len(sel)):
                            assert (mk[2 * r0][e], mk[2 * r0 + 1][e]) == ((qi[j][e] - a[r0][e]) % p, (gi[part][e] - b[r0][e]) % p)
                            assert g1[j][e] == (gi[j][e] + bc.beaver(o[2 * r0][e], o[2 * r0 + 1][e], a[r0][e], b[r0][e], ab[r0][e], p)) % p, (m, level, j, e)
                            if not g_only:
                                assert (mk[2 * r1][e], mk[2 * r1 + 1][e]) == ((qi[j][e] - a[r1][e]) % p, (qi[part][e] - b[r1][e]) % p)
                                assert q1[j][e] == bc.beaver(o[2 * r1][e], o[2 * r1 + 1][e], a[r1][e], b[r1][e], ab[r1][e], p), (m, level, j, e)


@pytest.mark.parametrize("count", (1, 257))
@pytest.mark.parametrize("p", bc.GPU_FIELDS, ids=bc.GPU_FIELD_IDS)
def test_every_step_equals_the_host_self_test(p, count):
    """One row body: for every step of csrc/hb_bd.hip the device's output equals, bit for bit, what hb_selftest_bd computes on the host
    from the same inputs -- the self test runs the rows the kernels run, addressing included.  m = 6: five planes and three levels, a
    g-only and a full node, two g-only nodes, then a single g-only node; m = 1: the sum step without a plane.  count 1 is one partial
    workgroup, 257 a second workgroup that holds one element."""
    from honeybadgermpc_amd.progs import bit_decomposition as bd

    ctx = gpu_ctx(p)
    torch, nl = ctx.torch, ctx.n_limbs
    seeds = iter(range(400, 500))

    def rnd(rows=None):
        return random_tensor(ctx, next(seeds), count, rows)

    def host(what, operands, params, outs):
        as_ints = [o if o is None or isinstance(o, (list, int)) else (ctx.download_ints(o.reshape(-1, nl)) if o.numel() else []) for o in operands + outs]
        rc, res = bc.run_bd(p, nl, what, as_ints[:len(operands)], params, as_ints[len(operands):], count)
        assert rc == 0
        return [ctx.upload_ints(o) for o in res]

    def same(dev, want):
        return torch.equal(dev.reshape(-1, nl), want)

    m, n = 6, 5
    c, bits = rnd(), rnd(m)
    g, q = bd.sub_leaves(ctx, c, bits, m)
    h = host(bc.LEAVES, [c, bits[:n]], [m], [n, n])
    assert same(g, h[0]) and same(q, h[1])
    assert [len(bd.prefix_nodes(n, level)) for level in range(bd.prefix_levels(m))] == [2, 2, 1]
    for level in range(3):
        triples = bd.prefix_level_triples(m, level)
        ta, tb, tab, opened = rnd(triples), rnd(triples), rnd(triples), rnd(2 * triples)
        masked = bd.prefix_mask(ctx, g, q, level, ta, tb)
        assert same(masked, host(bc.PREFIX_MASK, [g, q, ta, tb], [m, level], [2 * triples])[0]), level
        h = host(bc.PREFIX_COMBINE, [opened, ta, tb, tab], [m, level], [g, q])               # the planes before the level: updated in place
        bd.prefix_combine(ctx, opened.view(-1, nl), g, q, level, ta, tb, tab)
        assert same(g, h[0]) and same(q, h[1]), level
    for m in (6, 1):
        n = m - 1
        c, bits, carries = rnd(), rnd(m), g if n else rnd(0)
        ta, tb, tab, opened = rnd(n), rnd(n), rnd(n), rnd(2 * n)
        masked = bd.sum_mask(ctx, c, bits, carries, m, ta, tb)
        if n:
            assert same(masked, host(bc.SUM_MASK, [c, bits, carries, ta, tb], [m], [2 * n])[0])
        out = bd.sum_combine(ctx, opened.view(2 * n * count, nl), c, bits, carries, m, ta, tb, tab)
        assert tuple(out.shape) == (m, count, nl)
        assert same(out, host(bc.SUM_COMBINE, [opened, c, bits, carries, ta, tb, tab], [m], [m])[0]), m


@pytest.mark.parametrize("p, m", [(BLS, 33), (BLS, 9), (BLS, 2), (bc.P64, 17)], ids=["bls-33", "bls-9", "bls-2", "2^64-59-17"])
def test_chain_on_cleartext_values_gives_the_difference_bits(p, m):
    """the five calls chained on degree-0 shares (what a step opens is what its mask wrote): corners of c, and r all zeros, all ones
    and c2"""
    from honeybadgermpc_amd.progs import bit_decomposition as bd

    ctx = gpu_ctx(p)
    rnd = random.Random(m)
    top = (1 << m) - 1
    cs, rs = [], []
    for c in (0, top, (1 << m) % p, p - 1):
        for r in (0, top, c % (1 << m)):
            cs.append(c), rs.append(r)
    while len(cs) < 300:
        cs.append(rnd.randrange(p)), rs.append(rnd.getrandbits(m))
    count = len(cs)
    c = ctx.upload_ints(cs)
    bits = ctx.upload_ints([(r >> i) & 1 for i in range(m) for r in rs]).view(m, count, ctx.n_limbs)
    need = bd.bit_triples(m)
    ta, tb = ([rnd.randrange(p) for _ in range(need * count)] for _ in range(2))
    tab = [x * y % p for x, y in zip(ta, tb)]
    ta, tb, tab = (ctx.upload_ints(v).view(need, count, ctx.n_limbs) for v in (ta, tb, tab))
    g, q = bd.sub_leaves(ctx, c, bits, m)
    off = 0
    for level in range(bd.prefix_levels(m)):
        tr = bd.prefix_level_triples(m, level)
        sl = slice(off, off + tr)
        masked = bd.prefix_mask(ctx, g, q, level, ta[sl], tb[sl])
        bd.prefix_combine(ctx, masked, g, q, level, ta[sl], tb[sl], tab[sl])
        off += tr
    sl = slice(off, off + m - 1)
    masked = bd.sum_mask(ctx, c, bits, g, m, ta[sl], tb[sl])
    out = rows_of(ctx, bd.sum_combine(ctx, masked, c, bits, g, m, ta[sl], tb[sl], tab[sl]))
    assert off + m - 1 == need
    for e in range(count):
        assert [out[i][e] for i in range(m)] == bd.difference_bits_model(cs[e], rs[e], m), (m, cs[e], rs[e])


def test_inputs_untouched_out_honoured_overlap_refused_and_asynchronous():
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd._capi import HB_ERR_BAD_ARG, HbmpcBackendError
    from honeybadgermpc_amd.progs import bit_decomposition as bd

    p, count, m, level = BLS, 600, 9, 1
    ctx = gpu_ctx(p)
    torch = ctx.torch
    n, tr = m - 1, bd.prefix_level_triples(m, level)
    c, bits = random_tensor(ctx, 31, count), random_tensor(ctx, 32, count, rows=m)
    ta, tb, tab = (random_tensor(ctx, 33 + s, count, rows=n) for s in range(3))                    # n >= tr rows: sliced per call
    opened = random_tensor(ctx, 36, count, rows=2 * n)
    ops = [c, bits, ta, tb, tab, opened]
    copies = [t.clone() for t in ops]
    g, q = bd.sub_leaves(ctx, c, bits, m)
    lvl = bd.prefix_mask(ctx, g, q, level, ta[:tr], tb[:tr])
    g2, q2 = g.clone(), q.clone()
    bd.prefix_combine(ctx, opened[:2 * tr], g2, q2, level, ta[:tr], tb[:tr], tab[:tr])
    sm = bd.sum_mask(ctx, c, bits, g, m, ta, tb)
    out = bd.sum_combine(ctx, opened, c, bits, g, m, ta, tb, tab)
    # results consumed on the current stream without a synchronise, and on a side stream
    assert torch.equal(sa.sub(ctx, sa.add(ctx, out[3], out[3]), out[3]), out[3])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        gs, qs = bd.sub_leaves(ctx, c, bits, m)
        lvls = bd.prefix_mask(ctx, gs, qs, level, ta[:tr], tb[:tr])
        bd.prefix_combine(ctx, opened[:2 * tr], gs, qs, level, ta[:tr], tb[:tr], tab[:tr])
        outs = bd.sum_combine(ctx, opened, c, bits, g, m, ta, tb, tab)
    side.synchronize()
    assert torch.equal(lvls, lvl) and torch.equal(gs, g2) and torch.equal(qs, q2) and torch.equal(outs, out)
    # out given: written where asked, and handed back
    gb, qb = torch.empty_like(g), torch.empty_like(q)
    got = bd.sub_leaves(ctx, c, bits, m, out=(gb, qb))
    assert got[0].data_ptr() == gb.data_ptr() and got[1].data_ptr() == qb.data_ptr() and torch.equal(gb, g) and torch.equal(qb, q)
    lb, sb, ob = torch.empty_like(lvl), torch.empty_like(sm), torch.empty_like(out)
    assert bd.prefix_mask(ctx, g, q, level, ta[:tr], tb[:tr], out=lb).data_ptr() == lb.data_ptr() and torch.equal(lb, lvl)
    assert bd.sum_mask(ctx, c, bits, g, m, ta, tb, out=sb).data_ptr() == sb.data_ptr() and torch.equal(sb, sm)
    assert bd.sum_combine(ctx, opened, c, bits, g, m, ta, tb, tab, out=ob).data_ptr() == ob.data_ptr() and torch.equal(ob, out)
    assert all(torch.equal(t, cp) for t, cp in zip(ops, copies))
    # argument checks raise before C and nothing is launched: the buffers keep their contents
    ob.fill_(7)
    g3, q3 = g.clone(), q.clone()
    wide = torch.zeros((n, count, 2, ctx.n_limbs), dtype=torch.int64, device=ctx.tdev)
    bad_calls = [
        lambda: bd.sub_leaves(ctx, c, bits[:n - 1], m),                                            # too few planes
        lambda: bd.sub_leaves(ctx, c[:-1], bits, m),
        lambda: bd.sub_leaves(ctx, c, bits, 0),
        lambda: bd.sub_leaves(ctx, c, bits, 254),
        lambda: bd.sub_leaves(ctx, c, bits, m, out=gb),
        lambda: bd.sub_leaves(ctx, c, bits, m, out=(gb[:-1], qb)),
        lambda: bd.sub_leaves(ctx, c, bits.cpu(), m),
        lambda: bd.prefix_mask(ctx, g, q[:-1], level, ta[:tr], tb[:tr]),
        lambda: bd.prefix_mask(ctx, g, q, level, ta[:tr - 1], tb[:tr]),
        lambda: bd.prefix_mask(ctx, g, q, level, ta[:tr + 1], tb[:tr + 1]),
        lambda: bd.prefix_mask(ctx, g, q, 3, ta[:tr], tb[:tr]),                                    # level >= the number of levels
        lambda: bd.prefix_mask(ctx, g, q, -1, ta[:tr], tb[:tr]),
        lambda: bd.prefix_mask(ctx, g[:1], q[:1], 0, ta[:1], tb[:1]),                              # one plane has no level
        lambda: bd.prefix_mask(ctx, g, q, level, ta[:tr], tb[:tr], out=lb[:-1]),
        lambda: bd.prefix_combine(ctx, opened[:2 * tr - 1], g3, q3, level, ta[:tr], tb[:tr], tab[:tr]),
        lambda: bd.prefix_combine(ctx, opened[:2 * tr], g3, q3, level, ta[:tr], tb[:tr], tab[:tr, :-1]),
        lambda: bd.prefix_combine(ctx, opened[:2 * tr], wide[:, :, 0], q3, level, ta[:tr], tb[:tr], tab[:tr]),     # in place needs the array itself
        lambda: bd.prefix_combine(ctx, opened[:2 * tr], g3, wide[:, :, 0], level, ta[:tr], tb[:tr], tab[:tr]),
        lambda: bd.sum_mask(ctx, c, bits[:n], g, m, ta, tb),
        lambda: bd.sum_mask(ctx, c, bits, g[:-1], m, ta, tb),
        lambda: bd.sum_mask(ctx, c, bits, g, m, ta[:-1], tb),
        lambda: bd.sum_combine(ctx, opened[:-1], c, bits, g, m, ta, tb, tab, out=ob),
        lambda: bd.sum_combine(ctx, opened, c, bits, g, m, ta, tb, tab[:-1], out=ob),
        lambda: bd.sum_combine(ctx, opened, c, bits, g, m, ta, tb, tab, out=ob[:-1]),
        lambda: bd.sum_combine(ctx, opened, c, bits, g, m + 1, ta, tb, tab, out=ob),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"bad call {i} was accepted")
    for call in (lambda: bd.sub_leaves(ctx, c.to(torch.int32), bits, m), lambda: bd.sum_mask(ctx, c, bits, None, m, ta, tb),
                 lambda: bd.prefix_mask(ctx, [1], q, level, ta[:tr], tb[:tr])):
        with pytest.raises(TypeError):
            call()
    # an output laid over an input is refused by the C ABI, through Python too
    tr2 = bd.prefix_level_triples(m, 2)
    assert 2 * tr2 == n                                                                            # level 2's array to open is as long as g
    buf = random_tensor(ctx, 37, count, rows=3 * n)
    for call in (lambda: bd.sub_leaves(ctx, c, bits, m, out=(bits[:n], qb)), lambda: bd.sub_leaves(ctx, c, bits, m, out=(gb, gb)),
                 lambda: bd.prefix_mask(ctx, g3, q3, 2, ta[:tr2], tb[:tr2], out=g3),
                 lambda: bd.prefix_combine(ctx, opened[:2 * tr], g3, g3, level, ta[:tr], tb[:tr], tab[:tr]),
                 lambda: bd.prefix_combine(ctx, g3, g3, q3, 2, ta[:tr2], tb[:tr2], tab[:tr2]),
                 lambda: bd.sum_mask(ctx, c, bits, g, m, buf[n:2 * n], tb, out=buf[:2 * n]),
                 lambda: bd.sum_combine(ctx, opened, c, bits, g, m, ta, tb, tab, out=bits),
                 lambda: bd.sum_combine(ctx, opened, c, bits, g, m, ta, tb, tab, out=opened[:m])):
        with pytest.raises(HbmpcBackendError):
            call()
    # ... and the C ABI itself
    lib, st, P = ctx.lib, ctx.stream(), ctx.ptr
    assert lib.hb_bd_leaves(ctx.h, P(c), P(bits), m, P(gb), None, count, st) == HB_ERR_BAD_ARG
    assert lib.hb_bd_leaves(ctx.h, P(c), P(bits), 0, P(gb), P(qb), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_bd_leaves(ctx.h, P(c), P(bits), 254, P(gb), P(qb), count, st) == HB_ERR_BAD_ARG                  # m out of range for the modulus
    assert lib.hb_bd_leaves(ctx.h, P(c), P(bits), m, P(gb), P(qb), -1, st) == HB_ERR_BAD_ARG
    assert lib.hb_bd_prefix_mask(ctx.h, P(g), P(q), m, 3, P(ta), P(tb), P(lb), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_bd_prefix_mask(ctx.h, P(g), P(q), 2, 0, P(ta), P(tb), P(lb), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_bd_prefix_mask(ctx.h, P(g), None, m, level, P(ta), P(tb), P(lb), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_bd_prefix_mask(ctx.h, P(g), P(q), m, level, P(ta), P(tb), P(q), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_bd_prefix_combine(ctx.h, P(opened), P(g3), P(q3), m, 3, P(ta), P(tb), P(tab), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_bd_prefix_combine(ctx.h, P(opened), P(g3), P(q3), m, -1, P(ta), P(tb), P(tab), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_bd_prefix_combine(ctx.h, P(opened), P(g3), P(q3), m, level, P(ta), P(tb), None, count, st) == HB_ERR_BAD_ARG
    assert lib.hb_bd_prefix_combine(ctx.h, P(opened), P(g3), P(q3), m, level, P(g3), P(tb), P(tab), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_bd_sum_mask(ctx.h, P(c), P(bits), P(g), m, P(ta), P(tb), None, count, st) == HB_ERR_BAD_ARG
    assert lib.hb_bd_sum_mask(ctx.h, P(c), P(bits), P(g), m, P(ta), P(tb), P(g), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_bd_sum_combine(ctx.h, P(opened), P(c), P(bits), P(g), m, P(ta), P(tb), P(tab), None, count, st) == HB_ERR_BAD_ARG
    assert lib.hb_bd_sum_combine(ctx.h, P(opened), P(c), P(bits), P(g), m, P(ta), P(tb), P(tab), P(c), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_bd_sum_combine(ctx.h, P(opened), P(c), P(bits), P(g), 0, P(ta), P(tb), P(tab), P(ob), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_bd_sum_combine(ctx.h, P(opened), P(c), P(bits), P(g), m, P(ta), P(tb), P(tab), P(ob), -2, st) == HB_ERR_BAD_ARG
    # count == 0: a successful call that launches nothing
    assert lib.hb_bd_leaves(ctx.h, P(c), P(bits), m, P(gb), P(qb), 0, st) == 0
    assert lib.hb_bd_prefix_combine(ctx.h, P(opened), P(g3), P(q3), m, level, P(ta), P(tb), P(tab), 0, st) == 0
    assert lib.hb_bd_sum_combine(ctx.h, P(opened), P(c), P(bits), P(g), m, P(ta), P(tb), P(tab), P(ob), 0, st) == 0
    torch.cuda.synchronize()
    assert bool((ob == 7).all()) and torch.equal(g3, g) and torch.equal(q3, q) and torch.equal(gb, g) and torch.equal(qb, q)
    assert all(torch.equal(t, cp) for t, cp in zip(ops, copies))


# ---- the protocol, end to end ---------------------------------------------------------------------------------------------------
E2E = [(p, shape) for p in bc.GPU_FIELDS for shape in bc.gpu_shapes(p)]
E2E_IDS = [f"{bc.GPU_FIELD_IDS[bc.GPU_FIELDS.index(p)]}-k{k}-m{m}" for p, (k, m, kappa) in E2E]


@pytest.mark.parametrize("n, t, liars", [(4, 1, 1), (7, 2, 0)], ids=["n4-t1-one-garbling", "n7-t2"])
@pytest.mark.parametrize("p, shape", E2E, ids=E2E_IDS)
def test_protocol_end_to_end(p, shape, n, t, liars):
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd.progs import bit_decomposition as bd
    from honeybadgermpc_amd.progs import fixedpoint as fx

    k, m, kappa = shape
    count = 33
    ctx = gpu_ctx(p)
    torch = ctx.torch
    rnd = random.Random(1000 * n + 10 * m + k)
    bad = set(rnd.sample(range(n), liars))
    honest = [i for i in range(n) if i not in bad]
    top = 1 << (k - 1)
    xs = [x for x in (0, 1, -1, top - 1, -top, (1 << m) - 1, 1 << m) if -top <= x < top]
    xs += [rnd.randrange(-top, top) for _ in range(count - len(xs))]
    need = bd.bit_triples(m)
    bit_rows = [[rnd.getrandbits(1) for _ in range(count)] for _ in range(k + kappa)]
    for i in range(m):
        bit_rows[i][0] = bit_rows[i][2] = 1                                # an all-ones r1 under x = 0 and x = -1
    cs = [rnd.randrange(p) for _ in range(count)]                        # difference_bits: a PUBLIC value against shared bits
    r1 = [sum(bit_rows[i][e] << i for i in range(m)) for e in range(count)]

    def triples_rows(rows, canary):
        ta, tb = ([[rnd.randrange(p) for _ in range(count)] for _ in range(rows)] for _ in range(2))
        tab = [[a * b % p for a, b in zip(ra, rb)] for ra, rb in zip(ta, tb)]
        if canary:                                                       # a row that is no triple: reading it would spoil the result
            ta.append([rnd.randrange(p) for _ in range(count)]), tb.append([rnd.randrange(p) for _ in range(count)]), tab.append([rnd.randrange(p) for _ in range(count)])
        return [bc.deal_planes(ctx, rnd, p, n, t, v) for v in (ta, tb, tab)]

    bits = bc.deal_planes(ctx, rnd, p, n, t, bit_rows)
    trip = triples_rows(need, True) if need else [[torch.zeros((1, count, ctx.n_limbs), dtype=torch.int64, device=ctx.tdev)] * n] * 3
    trip_div = triples_rows(fx.carry_triples(m), False)
    vals = bc.deal_planes(ctx, rnd, p, n, t, [[v % p for v in xs]])
    c_public = ctx.upload_ints(cs)

    async def body(co, i):
        x = vals[i][0]
        triples = tuple(tr[i] for tr in trip)
        got, batches = {}, {}
        keep = (x.clone(), bits[i].clone(), [v.clone() for v in triples])

        async def step(name, coro):
            before = co.batches
            planes = await coro
            batches[name] = co.batches - before
            assert tuple(planes.shape) == (m, count, ctx.n_limbs)
            got[name] = ctx.download_ints(await co.open_share_array(planes.reshape(m * count, ctx.n_limbs)))
            return planes

        planes = await step("bit_decompose", bd.bit_decompose(co, x, bits[i], triples, k, m, kappa))
        await step("difference_bits", bd.difference_bits(co, c_public, bits[i][:m], triples))
        await step("FixedPointArray.bits", fx.FixedPointArray(co, x, 4, k, kappa).bits(m, bits[i], triples))
        await step("exact rows", bd.bit_decompose(co, x, bits[i], tuple(v[:need] for v in triples), k, m, kappa))
        if need:
            with pytest.raises(ValueError):
                await bd.bit_decompose(co, x, bits[i], tuple(v[:need - 1] for v in triples), k, m, kappa)
        horner = planes[m - 1]
        for j in range(m - 2, -1, -1):
            horner = sa.add(ctx, sa.add(ctx, horner, horner), planes[j])
        got["horner"] = ctx.download_ints(await co.open_share_array(horner))
        got["div2m"] = ctx.download_ints(await co.open_share_array(await fx.div2m(co, x, bits[i], tuple(tr[i] for tr in trip_div), k, m, kappa)))
        assert torch.equal(x, keep[0]) and torch.equal(bits[i], keep[1]) and all(torch.equal(v, w) for v, w in zip(triples, keep[2]))
        return got, batches

    results = bc.run_parties(p, n, t, bad, rnd, body)
    want = [b for i in range(m) for b in (bd.bits_model(x % p, p, k, m)[i] for x in xs)]
    want_diff = [b for i in range(m) for b in (bd.difference_bits_model(c, r, m)[i] for c, r in zip(cs, r1))]
    assert set(want) <= {0, 1} and [sum(want[i * count + e] << i for i in range(m)) for e in range(count)] == [x % (1 << m) for x in xs]
    for i in honest:
        got, batches = results[i]
        assert got["bit_decompose"] == want and got["FixedPointArray.bits"] == want and got["exact rows"] == want, i
        assert got["difference_bits"] == want_diff, i
        assert got["horner"] == got["div2m"] == [x % (1 << m) for x in xs], i
        assert batches == {"bit_decompose": bd.bit_opens(m), "difference_bits": bd.bit_opens(m) - 1, "FixedPointArray.bits": bd.bit_opens(m),
                           "exact rows": bd.bit_opens(m)}, i


def test_coroutines_refuse_short_preprocessing_before_anything_is_opened():
    from honeybadgermpc_amd.progs import bit_decomposition as bd
    from honeybadgermpc_amd.progs import fixedpoint as fx

    p, n, t, count, k, m, kappa = BLS, 4, 1, 9, 64, 33, 32
    ctx = gpu_ctx(p)
    x = random_tensor(ctx, 40, count)
    bits = random_tensor(ctx, 41, count, rows=k + kappa)
    need = bd.bit_triples(m)
    tr = tuple(random_tensor(ctx, 42 + s, count, rows=need) for s in range(3))

    async def refused(co, i):
        if i:
            return None
        short_bits, short_tr = bits[:k + kappa - 1], tuple(v[:need - 1] for v in tr)
        for coro in (lambda: bd.bit_decompose(co, x, short_bits, tr, k, m, kappa), lambda: bd.bit_decompose(co, x, bits, short_tr, k, m, kappa),
                     lambda: bd.bit_decompose(co, x, bits, tr, k, k, kappa), lambda: bd.bit_decompose(co, x, bits, tr, 222, m, kappa),
                     lambda: bd.bit_decompose(co, x[:4], bits, tr, k, m, kappa), lambda: bd.bit_decompose(co, x, bits, (tr[0], tr[1]), k, m, kappa),
                     lambda: bd.difference_bits(co, x, bits[:m], short_tr), lambda: bd.difference_bits(co, x, bits[:m, :4], tr),
                     lambda: fx.FixedPointArray(co, x, 32, k, kappa).bits(m, short_bits, tr), lambda: fx.FixedPointArray(co, x, 32, k, kappa).bits(m, bits, short_tr)):
            with pytest.raises(ValueError):
                await coro()
        return co.batches

    results = bc.run_parties(p, n, t, set(), random.Random(3), refused)
    assert results[0] == 0                                               # nothing was opened

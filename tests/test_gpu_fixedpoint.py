"""GPU: honeybadgermpc_amd.progs.fixedpoint -- the kernels of csrc/hb_fxp.hip against Python ints and, bit for bit, against the same
steps composed from share_arithmetic (what the package offered before), and the whole protocol over an OpenCoalescer: trunc_pr, div2m,
trunc, ltz, lt, mul and FixedPointArray open to the host models' values in the stated number of batches.  Exact equality everywhere
but for the decoded floats, which are held to the reference's own epsilon."""
import asyncio
import random

import numpy as np
import pytest

from conftest import BLS

pytestmark = pytest.mark.gpu

GOLDILOCKS = 0xFFFFFFFF00000001
P64 = (1 << 64) - 59
P256 = (1 << 256) - 189
FIELDS = [BLS, P256, P64, GOLDILOCKS]
FIELD_IDS = ["bls", "2^256-189", "2^64-59", "goldilocks"]
COUNTS = (0, 1, 255, 256, 257, 5000)
EPSILON = 1e-4                      # the reference's, tests/progs/test_fixedpoint.py:28


def _ctx(p):
    from honeybadgermpc_amd._capi import Context

    return Context.get(p)


def _shapes(p):
    return [(128, 32, 32), (64, 63, 32)] if p >> 64 else [(32, 8, 16), (16, 15, 16)]


def _random_tensor(ctx, seed, count, rows=None):
    """uniform canonical residues made on the device side (numpy limbs, reduced by hb_reduce)"""
    g = np.random.default_rng(seed)
    n = count if rows is None else rows * count
    limbs = g.integers(-(1 << 63), (1 << 63) - 1, size=(n, ctx.n_limbs), dtype=np.int64, endpoint=True)
    t = ctx.reduce_(ctx.to_device(limbs))
    return t if rows is None else t.view(rows, count, ctx.n_limbs)


def _ints(ctx, t):
    return ctx.download_ints(t.reshape(-1, ctx.n_limbs))


def _rows(ctx, t):
    """(rows, count, limbs) -> [row][element] ints"""
    flat, count = _ints(ctx, t), t.shape[1]
    return [flat[r * count:(r + 1) * count] for r in range(t.shape[0])]


def _sample(count):
    return list(range(count)) if count <= 257 else sorted({0, 1, 255, 256, 257, count - 1} | set(random.Random(count).sample(range(count), 40)))


def _low_bits(ctx, c, m):
    """c mod 2^m on the limbs, with torch alone"""
    out = c.clone()
    for j in range(ctx.n_limbs):
        rem = m - 64 * j
        if rem <= 0:
            out[:, j] = 0
        elif rem < 64:
            out[:, j] &= (1 << rem) - 1
    return out


def _bit_elem(ctx, c, i):
    """bit i of c as a field element array"""
    out = ctx.torch.zeros_like(c)
    out[:, 0] = (c[:, i // 64] >> (i % 64)) & 1
    return out


# ---- the kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", FIELDS, ids=FIELD_IDS)
def test_mask_and_trunc_pr_kernels(p):
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd.progs import fixedpoint as fx

    ctx = _ctx(p)
    torch = ctx.torch
    for k, m, kappa in _shapes(p):
        n = k + kappa
        inv = pow(2, -m, p)
        for count in COUNTS:
            x, bits = _random_tensor(ctx, 1 + count, count), _random_tensor(ctx, 2 + count, count, rows=n + 1)        # a plane more than needed is fine
            keep = (x.clone(), bits.clone())
            masked, r1 = fx.trunc_mask(ctx, x, bits, k, m, kappa)
            q1, q2 = fx.random2m(ctx, bits, k, m, kappa)
            assert tuple(masked.shape) == tuple(r1.shape) == tuple(q2.shape) == (count, ctx.n_limbs) and torch.equal(q1, r1)
            # composed: Horner over the planes from share_arithmetic
            hi, lo = ctx.upload_ints([0] * count), ctx.upload_ints([0] * count)
            for i in range(n - 1, -1, -1):
                if i >= m:
                    hi = sa.add(ctx, sa.add(ctx, hi, hi), bits[i])
                else:
                    lo = sa.add(ctx, sa.add(ctx, lo, lo), bits[i])
            whole = sa.add(ctx, sa.mul(ctx, hi, pow(2, m, p)), lo)
            assert torch.equal(r1, lo) and torch.equal(q2, hi) and torch.equal(masked, sa.add(ctx, sa.add(ctx, x, pow(2, k - 1, p)), whole)), (k, m, count)
            idx = _sample(count)
            if count:
                sel = torch.tensor(idx, device=ctx.tdev)
                planes = _rows(ctx, bits[:n].index_select(1, sel))
                xs = ctx.download_ints(x.index_select(0, sel))
                want_r1 = [sum(planes[i][e] << i for i in range(m)) % p for e in range(len(idx))]
                want_all = [sum(planes[i][e] << i for i in range(n)) % p for e in range(len(idx))]
                assert ctx.download_ints(r1.index_select(0, sel)) == want_r1
                assert ctx.download_ints(masked.index_select(0, sel)) == [(a + (1 << (k - 1)) + b) % p for a, b in zip(xs, want_all)], (k, m, count)
            # after the open: c any residue (corners in front)
            c = _random_tensor(ctx, 3 + count, count)
            if count >= 255:
                c[:4] = ctx.upload_ints([0, (1 << m) - 1, 1 << m, p - 1])
            got = fx.trunc_pr_finish(ctx, x, c, r1, m)
            assert torch.equal(got, sa.mul(ctx, sa.add(ctx, sa.sub(ctx, x, _low_bits(ctx, c, m)), r1), inv)), (k, m, count)
            if count:
                cs, rs = ctx.download_ints(c.index_select(0, sel)), ctx.download_ints(r1.index_select(0, sel))
                assert ctx.download_ints(got.index_select(0, sel)) == [(a - b % (1 << m) + d) * inv % p for a, b, d in zip(xs, cs, rs)], (k, m, count)
            assert torch.equal(x, keep[0]) and torch.equal(bits, keep[1])


@pytest.mark.parametrize("p", FIELDS, ids=FIELD_IDS)
def test_leaf_carry_and_finish_kernels(p):
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd.progs import fixedpoint as fx

    ctx = _ctx(p)
    torch = ctx.torch
    for k, m, kappa in _shapes(p):
        inv = pow(2, -m, p)
        for count in COUNTS:
            if m > 16 and count == 5000:
                rows_checked = (0, 1, m - 1, m)           # the composition of every plane is checked at the smaller counts
            else:
                rows_checked = range(m + 1)
            x, c, bits = _random_tensor(ctx, 4 + count, count), _random_tensor(ctx, 5 + count, count), _random_tensor(ctx, 6 + count, count, rows=m)
            if count >= 255:
                c[:4] = ctx.upload_ints([0, (1 << m) - 1, 1 << m, p - 1])
            keep = (c.clone(), bits.clone())
            g, q = fx.ltl_leaves(ctx, c, bits, m)
            assert tuple(g.shape) == tuple(q.shape) == (m + 1, count, ctx.n_limbs)
            one, zero = ctx.upload_ints([1] * count), ctx.upload_ints([0] * count)
            for j in rows_checked:
                if j == m:
                    assert torch.equal(g[j], one) and torch.equal(q[j], zero)
                    continue
                # the reference's formulas (fixedpoint.py:143-147, :168): carry = a (1 - b), all_one = a + (1 - b) - 2 carry
                a, nb = _bit_elem(ctx, c, m - 1 - j), sa.add(ctx, sa.neg(ctx, bits[m - 1 - j]), 1)
                carry = sa.mul(ctx, a, nb)
                assert torch.equal(g[j], carry) and torch.equal(q[j], sa.sub(ctx, sa.add(ctx, a, nb), sa.mul(ctx, carry, 2))), (m, count, j)
            if count:
                sel = torch.tensor(_sample(count)[:16], device=ctx.tdev)
                cs, planes = ctx.download_ints(c.index_select(0, sel)), _rows(ctx, bits.index_select(1, sel))
                gs, qs = _rows(ctx, g.index_select(1, sel)), _rows(ctx, q.index_select(1, sel))
                for j in range(m):
                    for e, cv in enumerate(cs):
                        b = planes[m - 1 - j][e]
                        assert (gs[j][e], qs[j][e]) == (((1 - b) % p, b) if (cv >> (m - 1 - j)) & 1 else (0, (1 - b) % p)), (m, count, j, e)
            assert torch.equal(c, keep[0]) and torch.equal(bits, keep[1])
            # levels of the tree over random planes: even, odd and root
            for nodes, root in ((2, True), (2, False), (5, False), (m + 1, False)):
                triples = 1 if root else 2 * (nodes // 2)
                gg, qq = _random_tensor(ctx, 7 + count, count, rows=nodes), _random_tensor(ctx, 8 + count, count, rows=nodes)
                ta, tb, tab = (_random_tensor(ctx, 9 + s + count, count, rows=triples) for s in range(3))
                opened = _random_tensor(ctx, 12 + count, count, rows=2 * triples)
                masked = fx.carry_mask(ctx, gg, qq, ta, tb, root=root)
                res = fx.carry_combine(ctx, opened.view(-1, ctx.n_limbs), gg, qq, ta, tb, tab, root=root)
                assert tuple(masked.shape) == (2 * triples, count, ctx.n_limbs)
                g2, q2 = (res, None) if root else res
                for t in range(triples if nodes <= 5 or count <= 257 else 4):
                    node = t // 2
                    assert torch.equal(masked[2 * t], sa.sub(ctx, qq[2 * node], ta[t])), (nodes, t)
                    assert torch.equal(masked[2 * t + 1], sa.sub(ctx, (qq if t & 1 else gg)[2 * node + 1], tb[t])), (nodes, t)
                    prod = sa.beaver_combine(ctx, opened[2 * t], opened[2 * t + 1], ta[t], tb[t], tab[t])
                    if t & 1:
                        assert torch.equal(q2[node], prod), (nodes, t)
                    else:
                        assert torch.equal(g2 if root else g2[node], sa.add(ctx, gg[2 * node], prod)), (nodes, t)
                if nodes & 1:
                    assert torch.equal(g2[-1], gg[-1]) and torch.equal(q2[-1], qq[-1])
                if count and nodes == 5:
                    sel = torch.tensor(_sample(count)[:8], device=ctx.tdev)
                    o, a, b, ab = (_rows(ctx, v.index_select(1, sel)) for v in (opened, ta, tb, tab))
                    g0, g1, q1 = _rows(ctx, gg.index_select(1, sel)), _rows(ctx, g2.index_select(1, sel)), _rows(ctx, q2.index_select(1, sel))
                    for e in range(len(sel)):
                        bv = [(o[2 * t][e] * o[2 * t + 1][e] + o[2 * t][e] * b[t][e] + o[2 * t + 1][e] * a[t][e] + ab[t][e]) % p for t in range(4)]
                        assert [g1[0][e], q1[0][e], g1[1][e], q1[1][e]] == [(g0[0][e] + bv[0]) % p, bv[1], (g0[2][e] + bv[2]) % p, bv[3]]
            # the finish
            r1, carry = _random_tensor(ctx, 13 + count, count), _random_tensor(ctx, 14 + count, count)
            c2 = _low_bits(ctx, c, m)
            a2 = sa.add(ctx, sa.sub(ctx, c2, r1), sa.mul(ctx, sa.add(ctx, sa.neg(ctx, carry), 1), pow(2, m, p)))
            tr = sa.mul(ctx, sa.sub(ctx, x, a2), inv)
            assert torch.equal(fx.div2m_finish(ctx, None, c, r1, carry, m), a2) and torch.equal(fx.div2m_finish(ctx, x, c, r1, carry, m, fx.MOD), a2)
            assert torch.equal(fx.div2m_finish(ctx, x, c, r1, carry, m, fx.TRUNC), tr)
            assert torch.equal(fx.div2m_finish(ctx, x, c, r1, carry, m, fx.NEG_TRUNC), sa.neg(ctx, tr))
            if count:
                sel = torch.tensor(_sample(count)[:32], device=ctx.tdev)
                xs, cs, rs, ks = (ctx.download_ints(v.index_select(0, sel)) for v in (x, c, r1, carry))
                want = [(a - (b % (1 << m) - d + (1 << m) * (1 - e))) * inv % p for a, b, d, e in zip(xs, cs, rs, ks)]
                assert ctx.download_ints(fx.div2m_finish(ctx, x, c, r1, carry, m, fx.TRUNC).index_select(0, sel)) == want


@pytest.mark.parametrize("count", (1, 257))
@pytest.mark.parametrize("p", FIELDS, ids=FIELD_IDS)
def test_every_step_equals_the_host_self_test(p, count):
    """One row body: for every step of csrc/hb_fxp.hip the device's output equals, bit for bit, what hb_selftest_fxp computes on the host
    from the same inputs -- the self test runs the rows the kernels run, addressing included.  m = 4: the tree's levels have 5, 3 and 2
    nodes, so the odd plane is copied at 5 and at 3 and the root, where p is not written, has 2.  count 1 is one partial workgroup, 257
    a second workgroup that holds one element."""
    import bitdec_cases as bc
    from honeybadgermpc_amd.progs import fixedpoint as fx

    ctx = _ctx(p)
    torch, nl = ctx.torch, ctx.n_limbs
    k, m, kappa = 8, 4, 8
    MASK, TRUNC_PR, LEAVES, CARRY_MASK, CARRY_COMBINE, FINISH = range(6)
    seeds = iter(range(300, 400))

    def rnd(rows=None):
        return _random_tensor(ctx, next(seeds), count, rows)

    def host(what, operands, params, out_rows):
        rc, outs = bc.run_fxp(p, nl, what, [o if o is None or isinstance(o, list) else _ints(ctx, o) for o in operands], params, out_rows, count)
        assert rc == 0
        return [None if o is None else ctx.upload_ints(o) for o in outs]

    def same(dev, want):
        return torch.equal(dev.reshape(-1, nl), want)

    x, c, bits, inv = rnd(), rnd(), rnd(k + kappa), [pow(2, -m, p)]
    masked, r1 = fx.trunc_mask(ctx, x, bits, k, m, kappa)
    h = host(MASK, [x, bits], [k, m, kappa], [1, 1])
    assert same(masked, h[0]) and same(r1, h[1])
    q1, q2 = fx.random2m(ctx, bits, k, m, kappa)
    h = host(MASK, [None, bits], [k, m, kappa], [1, 1])
    assert same(q2, h[0]) and same(q1, h[1])
    assert same(fx.trunc_pr_finish(ctx, x, c, r1, m), host(TRUNC_PR, [x, c, r1, inv], [k, m, kappa], [1])[0])
    g, q = fx.ltl_leaves(ctx, c, bits[:m], m)
    h = host(LEAVES, [c, bits[:m]], [k, m, kappa], [m + 1, m + 1])
    assert same(g, h[0]) and same(q, h[1])
    for nodes, root in ((5, False), (3, False), (2, True)):
        assert g.shape[0] == q.shape[0] == nodes
        triples, out_nodes = 1 if root else 2 * (nodes // 2), (nodes + 1) // 2
        ta, tb, tab = rnd(triples), rnd(triples), rnd(triples)
        masked = fx.carry_mask(ctx, g, q, ta, tb, root=root)
        assert same(masked, host(CARRY_MASK, [g, q, ta, tb], [k, m, kappa, nodes, int(root)], [2 * triples])[0]), nodes
        opened = rnd(2 * triples)
        res = fx.carry_combine(ctx, opened.view(-1, nl), g, q, ta, tb, tab, root=root)
        h = host(CARRY_COMBINE, [opened, g, q, ta, tb, tab], [k, m, kappa, nodes, int(root)], [out_nodes, None if root else out_nodes])
        if root:
            assert same(res, h[0])
        else:
            assert same(res[0], h[0]) and same(res[1], h[1]), nodes
            g, q = res
    carry = res
    for mode in (fx.MOD, fx.TRUNC, fx.NEG_TRUNC):
        xin = None if mode == fx.MOD else x
        assert same(fx.div2m_finish(ctx, xin, c, r1, carry, m, mode), host(FINISH, [xin, c, r1, carry, inv], [k, m, kappa, mode], [1])[0]), mode


def test_inputs_untouched_out_given_arguments_checked_and_asynchronous():
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd._capi import HB_ERR_BAD_ARG
    from honeybadgermpc_amd.progs import fixedpoint as fx

    p, count, k, m, kappa = BLS, 600, 64, 33, 32
    ctx = _ctx(p)
    torch = ctx.torch
    n, inv = k + kappa, pow(2, -m, p)
    x, c, carry = (_random_tensor(ctx, s, count) for s in (21, 22, 23))
    bits = _random_tensor(ctx, 24, count, rows=n)
    ops = [x, c, carry, bits]
    copies = [t.clone() for t in ops]
    masked, r1 = fx.trunc_mask(ctx, x, bits, k, m, kappa)
    want_pr = fx.trunc_pr_finish(ctx, x, c, r1, m)
    want_fin = fx.div2m_finish(ctx, x, c, r1, carry, m, fx.TRUNC)
    g, q = fx.ltl_leaves(ctx, c, bits, m)
    xs, cs, rs = (ctx.download_ints(v) for v in (x, c, r1))
    assert ctx.download_ints(want_pr) == [(a - b % (1 << m) + d) * inv % p for a, b, d in zip(xs, cs, rs)]
    # results consumed on the current stream without a synchronise, and on a side stream
    assert torch.equal(sa.sub(ctx, sa.add(ctx, want_pr, want_pr), want_pr), want_pr)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m2, r2 = fx.trunc_mask(ctx, x, bits, k, m, kappa)
        pr2 = sa.add(ctx, fx.trunc_pr_finish(ctx, x, c, r2, m), 1)
        g2, q2 = fx.ltl_leaves(ctx, c, bits, m)
    side.synchronize()
    assert torch.equal(m2, masked) and torch.equal(pr2, sa.add(ctx, want_pr, 1)) and torch.equal(g2, g) and torch.equal(q2, q)
    # out given: written where asked, and handed back
    buf, buf2 = ctx.empty(count), ctx.empty(count)
    got = fx.trunc_mask(ctx, x, bits, k, m, kappa, out=buf, r1_out=buf2)
    assert got[0] is buf and got[1] is buf2 and torch.equal(buf, masked) and torch.equal(buf2, r1)
    assert fx.trunc_pr_finish(ctx, x, c, r1, m, out=buf) is buf and torch.equal(buf, want_pr)
    assert fx.div2m_finish(ctx, x, c, r1, carry, m, fx.TRUNC, out=buf) is buf and torch.equal(buf, want_fin)
    gb, qb = torch.empty_like(g), torch.empty_like(q)
    got = fx.ltl_leaves(ctx, c, bits, m, out=(gb, qb))
    assert got[0].data_ptr() == gb.data_ptr() and torch.equal(gb, g) and torch.equal(qb, q)
    ta, tb, tab = (_random_tensor(ctx, 30 + s, count, rows=2 * ((m + 1) // 2)) for s in range(3))
    lvl = fx.carry_mask(ctx, g, q, ta, tb)
    lb = torch.empty_like(lvl)
    assert fx.carry_mask(ctx, g, q, ta, tb, out=lb).data_ptr() == lb.data_ptr() and torch.equal(lb, lvl)
    ng, nq = fx.carry_combine(ctx, lvl, g, q, ta, tb, tab)
    ob = (torch.empty_like(ng), torch.empty_like(nq))
    got = fx.carry_combine(ctx, lvl, g, q, ta, tb, tab, out=ob)
    assert got[0].data_ptr() == ob[0].data_ptr() and torch.equal(ob[0], ng) and torch.equal(ob[1], nq)
    assert all(torch.equal(t, cp) for t, cp in zip(ops, copies))
    # in place over a same-index input
    xx = x.clone()
    assert fx.trunc_mask(ctx, xx, bits, k, m, kappa, out=xx)[0] is xx and torch.equal(xx, masked)
    for which in range(3):
        arrs = [x.clone(), c.clone(), r1.clone()]
        assert fx.trunc_pr_finish(ctx, *arrs, m, out=arrs[which]) is arrs[which] and torch.equal(arrs[which], want_pr)
    kk = carry.clone()
    assert fx.div2m_finish(ctx, x, c, r1, kk, m, fx.TRUNC, out=kk) is kk and torch.equal(kk, want_fin)
    # a strided view of an input is taken as its values
    wide = torch.zeros((count, 2, ctx.n_limbs), dtype=torch.int64, device=ctx.tdev)
    wide[:, 0] = x
    assert torch.equal(fx.trunc_mask(ctx, wide[:, 0], bits, k, m, kappa)[0], masked)
    assert torch.equal(fx.trunc_pr_finish(ctx, wide[:, 0], c, r1, m), want_pr)
    # argument checks raise before C and nothing is launched: the output buffer keeps its contents
    buf.fill_(7)
    seven = buf.clone()
    strided = torch.zeros((2 * count, ctx.n_limbs), dtype=torch.int64, device=ctx.tdev)[::2]
    bad_calls = [
        lambda: fx.trunc_mask(ctx, x[:-1], bits, k, m, kappa, out=buf),                        # a short operand
        lambda: fx.trunc_mask(ctx, x, bits[:n - 1], k, m, kappa, out=buf),                     # too few planes
        lambda: fx.trunc_mask(ctx, x, bits[:, :-1], k, m, kappa, out=buf),
        lambda: fx.trunc_mask(ctx, x, bits.reshape(-1, ctx.n_limbs), k, m, kappa, out=buf),
        lambda: fx.trunc_mask(ctx, torch.cat([x, x]), bits, k, m, kappa, out=buf),             # a long one
        lambda: fx.trunc_mask(ctx, x, bits, k, m, kappa, out=buf[:-1]),
        lambda: fx.trunc_mask(ctx, x, bits, k, m, kappa, out=strided),
        lambda: fx.trunc_mask(ctx, x, bits, k, m, kappa, out=buf, r1_out=buf),
        lambda: fx.trunc_mask(ctx, x, bits, k, k, kappa, out=buf),                             # m >= k
        lambda: fx.trunc_mask(ctx, x, bits, 222, m, kappa, out=buf),                           # would wrap
        lambda: fx.trunc_mask(ctx, x.cpu(), bits, k, m, kappa, out=buf),                       # another device
        lambda: fx.trunc_mask(ctx, x, bits.cpu(), k, m, kappa, out=buf),
        lambda: fx.trunc_mask(ctx, x[:, :2], bits, k, m, kappa, out=buf),                      # not `limbs` wide
        lambda: fx.random2m(ctx, bits[:n - 1], k, m, kappa, out=(buf, buf2)),
        lambda: fx.trunc_pr_finish(ctx, x, c[:-1], r1, m, out=buf),
        lambda: fx.trunc_pr_finish(ctx, x, c, torch.cat([r1, r1]), m, out=buf),
        lambda: fx.trunc_pr_finish(ctx, x, c, r1, 0, out=buf),
        lambda: fx.trunc_pr_finish(ctx, x, c, r1, m, out=strided),
        lambda: fx.trunc_pr_finish(ctx, x, c.cpu(), r1, m, out=buf),
        lambda: fx.div2m_finish(ctx, x, c, r1, carry[:-1], m, fx.TRUNC, out=buf),
        lambda: fx.div2m_finish(ctx, x, c, r1, carry, m, 5, out=buf),
        lambda: fx.div2m_finish(ctx, x[:3], c, r1, carry, m, fx.MOD, out=buf),
        lambda: fx.div2m_finish(ctx, x, c, r1, carry, m, fx.TRUNC, out=buf[:5]),
        lambda: fx.ltl_leaves(ctx, c, bits[:m - 1], m),
        lambda: fx.ltl_leaves(ctx, c, bits, m, out=(gb[:-1], qb)),
        lambda: fx.ltl_leaves(ctx, c, bits, m, out=gb),
        lambda: fx.carry_mask(ctx, g, q[:-1], ta, tb),
        lambda: fx.carry_mask(ctx, g, q, ta[:-1], tb),
        lambda: fx.carry_mask(ctx, g, q, ta, tb, root=True),                                   # a root of more than two planes
        lambda: fx.carry_mask(ctx, g[:1], q[:1], ta[:1], tb[:1]),
        lambda: fx.carry_combine(ctx, lvl[:-1], g, q, ta, tb, tab),
        lambda: fx.carry_combine(ctx, lvl, g, q, ta, tb, tab[:, :-1]),
        lambda: fx.carry_combine(ctx, lvl, g, q, ta, tb, tab, out=(ob[0][:-1], ob[1])),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"bad call {i} was accepted")
    for call in (
        lambda: fx.trunc_mask(ctx, x.to(torch.int32), bits, k, m, kappa, out=buf),
        lambda: fx.trunc_mask(ctx, xs, bits, k, m, kappa, out=buf),
        lambda: fx.trunc_pr_finish(ctx, x, c, r1.to(torch.float64), m, out=buf),
        lambda: fx.div2m_finish(ctx, x, c, r1, None, m, fx.TRUNC, out=buf),
        lambda: fx.ltl_leaves(ctx, cs, bits, m),
    ):
        with pytest.raises(TypeError):
            call()
    assert torch.equal(buf, seven)
    # ... and the C ABI refuses what gets past Python
    lib, st, P = ctx.lib, ctx.stream(), ctx.ptr
    inv_h = ctx.host_elems([inv])
    too_big = ctx.host_elems([0])
    too_big[:] = np.frombuffer(int(p).to_bytes(32, "little"), dtype=np.uint64)
    assert lib.hb_fxp_mask(ctx.h, P(x), P(bits), k, m, kappa, P(buf), P(buf2), -1, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxp_mask(ctx.h, P(x), None, k, m, kappa, P(buf), P(buf2), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxp_mask(ctx.h, P(x), P(bits), k, m, kappa, None, P(buf2), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxp_mask(ctx.h, P(x), P(bits), k, m, kappa, P(buf), None, count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxp_mask(ctx.h, P(x), P(bits), k, m, kappa, P(buf), P(buf), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxp_mask(ctx.h, P(x), P(bits), k, k, kappa, P(buf), P(buf2), count, st) == HB_ERR_BAD_ARG          # m >= k
    assert lib.hb_fxp_mask(ctx.h, P(x), P(bits), k, 0, kappa, P(buf), P(buf2), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxp_mask(ctx.h, P(x), P(bits), k, m, 190, P(buf), P(buf2), count, st) == HB_ERR_BAD_ARG            # k + kappa + 1 = 255 bits: would wrap
    assert lib.hb_fxp_mask(ctx.h, P(x), P(bits), k, m, -1, P(buf), P(buf2), count, st) == HB_ERR_BAD_ARG
    good = [P(x), P(c), P(r1)]
    for i in range(3):
        args = list(good)
        args[i] = None
        assert lib.hb_fxp_trunc_pr(ctx.h, *args, m, inv_h.ctypes.data, P(buf), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxp_trunc_pr(ctx.h, *good, m, None, P(buf), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxp_trunc_pr(ctx.h, *good, m, too_big.ctypes.data, P(buf), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxp_trunc_pr(ctx.h, *good, m, inv_h.ctypes.data, None, count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxp_trunc_pr(ctx.h, *good, m, inv_h.ctypes.data, P(buf), -1, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxp_trunc_pr(ctx.h, *good, 0, inv_h.ctypes.data, P(buf), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxp_trunc_pr(ctx.h, *good, 254, inv_h.ctypes.data, P(buf), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxp_ltl_leaves(ctx.h, P(c), P(bits), m, P(gb), None, count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxp_ltl_leaves(ctx.h, P(c), P(bits), m, P(gb), P(gb), count, st) == HB_ERR_BAD_ARG                 # g and p one array
    assert lib.hb_fxp_ltl_leaves(ctx.h, P(c), P(bits), 0, P(gb), P(qb), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxp_ltl_leaves(ctx.h, P(c), P(bits), m, P(gb), P(qb), -3, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxp_carry_mask(ctx.h, P(g), P(q), 1, 0, P(ta), P(tb), P(lb), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxp_carry_mask(ctx.h, P(g), P(q), 4, 1, P(ta), P(tb), P(lb), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxp_carry_mask(ctx.h, P(g), None, 4, 0, P(ta), P(tb), P(lb), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxp_carry_mask(ctx.h, P(g), P(q), 4, 0, P(ta), P(tb), P(g), count, st) == HB_ERR_BAD_ARG            # masked over an input
    assert lib.hb_fxp_carry_combine(ctx.h, P(lvl), P(g), P(q), 4, 0, P(ta), P(tb), P(tab), P(ob[0]), None, count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxp_carry_combine(ctx.h, P(lvl), P(g), P(q), 4, 0, P(ta), P(tb), P(tab), P(g), P(ob[1]), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxp_carry_combine(ctx.h, P(lvl), P(g), P(q), 4, 0, P(ta), P(tb), None, P(ob[0]), P(ob[1]), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxp_carry_combine(ctx.h, P(lvl), P(g), P(q), 4, 0, P(ta), P(tb), P(tab), P(ob[0]), P(ob[1]), -1, st) == HB_ERR_BAD_ARG
    fin = [P(x), P(c), P(r1), P(carry)]
    assert lib.hb_fxp_div2m_finish(ctx.h, *fin, m, inv_h.ctypes.data, 3, P(buf), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxp_div2m_finish(ctx.h, None, *fin[1:], m, inv_h.ctypes.data, fx.TRUNC, P(buf), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxp_div2m_finish(ctx.h, *fin, m, None, fx.TRUNC, P(buf), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxp_div2m_finish(ctx.h, *fin, m, too_big.ctypes.data, fx.TRUNC, P(buf), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxp_div2m_finish(ctx.h, *fin, m, inv_h.ctypes.data, fx.TRUNC, None, count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxp_div2m_finish(ctx.h, *fin, m, inv_h.ctypes.data, fx.TRUNC, P(buf), -1, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxp_div2m_finish(ctx.h, *fin, 0, inv_h.ctypes.data, fx.TRUNC, P(buf), count, st) == HB_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert torch.equal(buf, seven) and all(torch.equal(t, cp) for t, cp in zip(ops, copies))
    assert lib.hb_fxp_mask(ctx.h, P(x), P(bits), k, m, kappa, P(buf), P(buf2), 0, st) == 0 and torch.equal(buf, seven)     # count == 0: nothing launched
    assert lib.hb_fxp_trunc_pr(ctx.h, *good, m, inv_h.ctypes.data, P(buf), 0, st) == 0 and torch.equal(buf, seven)
    assert lib.hb_fxp_div2m_finish(ctx.h, *fin, m, inv_h.ctypes.data, fx.TRUNC, P(buf), 0, st) == 0 and torch.equal(buf, seven)
    assert lib.hb_fxp_trunc_pr(ctx.h, *good, m, inv_h.ctypes.data, P(buf), count, st) == 0
    assert torch.equal(buf, want_pr)


# ---- the protocol, end to end over the in-process tagged network of tests/test_gpu_mimc.py (restated) ----------------------
class _TaggedNet:
    """get_send_recv(tag) -> (send, recv) for party i, as the runtime hands out per-share-id channels (mpc.py:196-205)"""

    def __init__(self, n):
        self.n, self.q = n, [dict() for _ in range(n)]

    def _queue(self, party, tag):
        return self.q[party].setdefault(tag, asyncio.Queue())

    def get_send_recv(self, i, tamper=None):
        def factory(tag):
            def send(dest, msg):
                self._queue(dest, tag).put_nowait((i, tamper(msg) if tamper else msg))

            return send, self._queue(i, tag).get

        return factory


def _deal(rnd, p, n, degree, values):
    """-> [party][k]: Shamir shares of values[k] at the points 1..n"""
    out = [[0] * len(values) for _ in range(n)]
    for k, v in enumerate(values):
        coeffs = [rnd.randrange(p) for _ in range(degree)]
        for i in range(n):
            acc = 0
            for co in reversed(coeffs):
                acc = (acc + co) * (i + 1) % p
            out[i][k] = (acc + v) % p
    return out


def _deal_planes(ctx, rnd, p, n, t, rows):
    """rows: [row][element] values -> [party] tensors (rows, count, limbs)"""
    count = len(rows[0])
    dealt = _deal(rnd, p, n, t, [v for row in rows for v in row])
    return [ctx.upload_ints(d).view(len(rows), count, ctx.n_limbs) for d in dealt]


def _run_parties(p, n, t, bad, rnd, body):
    """every party runs `body(co, i)` over its own OpenCoalescer -> [result per party]"""
    from honeybadgermpc_amd import wire
    from honeybadgermpc_amd.open_coalescer import OpenCoalescer

    def garble(msg):
        tag, blob = msg
        count = wire.unpack_limbs(blob).shape[0]
        return (tag, wire.pack_ints([rnd.randrange(p) for _ in range(count)], p))

    async def party(i, net):
        co = OpenCoalescer(p, n, t, i, net.get_send_recv(i, garble if i in bad else None))
        return await body(co, i)

    async def main():
        net = _TaggedNet(n)
        return await asyncio.gather(*[party(i, net) for i in range(n)])

    results = asyncio.run(main())
    _ctx(p).torch.cuda.synchronize()
    return results


def _masks(bit_rows, e, n_bits, m):
    return sum(bit_rows[i][e] << i for i in range(m)), sum(bit_rows[m + i][e] << i for i in range(n_bits - m))


def _protocol_case(p, n, t, liars, count, f, k, kappa, seed):
    from honeybadgermpc_amd.progs import fixedpoint as fx

    ctx = _ctx(p)
    rnd = random.Random(seed)
    bad = set(rnd.sample(range(n), liars))
    honest = [i for i in range(n) if i not in bad]
    m, top = k // 2, 1 << (k - 1)
    # signed k-bit inputs for the integer protocols; reals in (0, 100) and (-100, 0) for the wrapper (the reference's own test)
    xs = ([0, 1, -1, top - 1, -(top - 1), -top] + [rnd.randrange(-top, top) for _ in range(count)])[-count:]
    ys = [rnd.randrange(-top // 2, top // 2) for _ in range(count)]
    xh = [v // 2 for v in xs]                                            # x - y must stay a k-bit value
    scale = 100.0 if f >= 32 else 7.0                                    # (f, k) = (8, 16): |a b| must stay below 2^(k - 1 - f)
    fa, fb = [rnd.uniform(0, scale) for _ in range(count)], [-rnd.uniform(0, scale) for _ in range(count)]
    ia, ib = [fx.to_fixed_point_repr(v, f) for v in fa], [fx.to_fixed_point_repr(v, f) for v in fb]
    n_planes, n_triples = 2 * k + kappa, fx.carry_triples(k - 1)
    bit_rows = [[rnd.getrandbits(1) for _ in range(count)] for _ in range(n_planes)]
    bit_rows[0] = [1] * count
    ta = [[rnd.randrange(p) for _ in range(count)] for _ in range(n_triples)]
    tb = [[rnd.randrange(p) for _ in range(count)] for _ in range(n_triples)]
    tab = [[a * b % p for a, b in zip(ra, rb)] for ra, rb in zip(ta, tb)]
    bits = _deal_planes(ctx, rnd, p, n, t, bit_rows)
    trip = [_deal_planes(ctx, rnd, p, n, t, rows) for rows in (ta, tb, tab)]
    vals = _deal_planes(ctx, rnd, p, n, t, [[v % p for v in row] for row in (xs, ys, xh, ia, ib)])
    lv_m, lv_k = fx.carry_levels(m), fx.carry_levels(k - 1)
    c_public = ctx.upload_ints([v % p for v in ys])                      # bit_ltl compares a PUBLIC value with shared bits

    async def body(co, i):
        x, y, xhalf, a, b = (vals[i][r] for r in range(5))
        triples = tuple(tr[i] for tr in trip)
        one = tuple(tr[i][0] for tr in trip)
        got, batches = {}, {}

        async def step(name, coro):
            before = co.batches
            shares = await coro
            batches[name] = co.batches - before
            got[name] = ctx.download_ints(await co.open_share_array(shares))

        keep = (x.clone(), bits[i].clone(), triples[0].clone())
        await step("trunc_pr", fx.trunc_pr(co, x, bits[i], k, m, kappa))
        await step("div2m", fx.div2m(co, x, bits[i], triples, k, m, kappa))
        await step("trunc", fx.trunc(co, x, bits[i], triples, k, m, kappa))
        await step("ltz", fx.ltz(co, x, bits[i], triples, k, kappa))
        await step("lt", fx.lt(co, xhalf, y, bits[i], triples, k, kappa))
        await step("mul", fx.mul(co, a, b, one, bits[i], f, k, kappa))
        await step("bit_ltl", fx.bit_ltl(co, c_public, bits[i][:m], triples))
        assert ctx.torch.equal(x, keep[0]) and ctx.torch.equal(bits[i], keep[1]) and ctx.torch.equal(triples[0], keep[2])
        A, B = fx.FixedPointArray(co, a, f, k, kappa), fx.FixedPointArray(co, b, f, k, kappa)
        got["A"], got["B"] = await A.open(), await B.open()
        got["A+B"], got["A-B"] = await (A + B).open(), await (A - B).open()
        got["-A"] = await A.neg().open()
        got["A*B"] = await (await A.mul(B, one, bits[i])).open()
        got["A/4"] = await (await A.div(4, bits[i])).open()
        for name, coro in (("A<0", A.ltz(bits[i], triples)), ("B<0", B.ltz(bits[i], triples)), ("A<B", A.lt(B, bits[i], triples)), ("B<A", B.lt(A, bits[i], triples))):
            got[name] = ctx.download_ints(await co.open_share_array(await coro))
        return got, batches

    results = _run_parties(p, n, t, bad, rnd, body)
    nb = k + kappa
    mk = [_masks(bit_rows, e, nb, m) for e in range(count)]
    mk1 = [_masks(bit_rows, e, nb, k - 1) for e in range(count)]
    mmul = [_masks(bit_rows, e, 2 * k + kappa, f) for e in range(count)]
    want = {
        "trunc_pr": [fx.trunc_pr_model(x % p, *mk[e], p, k, m, kappa) for e, x in enumerate(xs)],
        "div2m": [x % (1 << m) for x in xs],
        "trunc": [(x >> m) % p for x in xs],
        "ltz": [int(x < 0) for x in xs],
        "lt": [int(a < b) for a, b in zip(xh, ys)],
        "mul": [fx.trunc_pr_model(a * b % p, *mmul[e], p, 2 * k, f, kappa) for e, (a, b) in enumerate(zip(ia, ib))],
        "bit_ltl": [int((y % p) % (1 << m) < mk[e][0]) for e, y in enumerate(ys)],
        "A<0": [0] * count, "B<0": [1] * count, "A<B": [0] * count, "B<A": [1] * count,
    }
    assert want["div2m"] == [fx.div2m_model(x % p, *mk[e], p, k, m, kappa) for e, x in enumerate(xs)]
    assert want["ltz"] == [fx.ltz_model(x % p, *mk1[e], p, k, kappa) for e, x in enumerate(xs)]
    eps = EPSILON if f >= 32 else 2.0 ** -(f - 4)                        # (f = 8: the representation itself resolves 2^-8)
    for i in honest:
        got, batches = results[i]
        for name, w in want.items():
            assert got[name] == w, (i, name)
        assert batches == {"trunc_pr": 1, "div2m": 1 + lv_m, "trunc": 1 + lv_m, "ltz": 1 + lv_k, "lt": 1 + lv_k, "mul": 2, "bit_ltl": lv_m}, i
        for e in range(count):
            assert abs(got["A"][e] - fa[e]) < eps and abs(got["B"][e] - fb[e]) < eps
            assert abs(got["A+B"][e] - (fa[e] + fb[e])) < eps and abs(got["A-B"][e] - (fa[e] - fb[e])) < eps and abs(got["-A"][e] + fa[e]) < eps
            assert abs(got["A*B"][e] - fa[e] * fb[e]) < (eps if f >= 32 else 1.0), (i, e)
            assert abs(got["A/4"][e] - fa[e] / 4) < eps


@pytest.mark.parametrize("n, t, liars, count", [(4, 1, 0, 1), (4, 1, 0, 20), (4, 1, 0, 256), (7, 2, 0, 1), (7, 2, 0, 20), (4, 1, 1, 1), (4, 1, 1, 20), (7, 2, 2, 1), (7, 2, 2, 20)])
def test_protocol_end_to_end(n, t, liars, count):
    from honeybadgermpc_amd.progs import fixedpoint as fx

    _protocol_case(BLS, n, t, liars, count, fx.F, fx.K, fx.KAPPA, 1000 * n + 10 * count + liars)


def test_protocol_narrow_field():
    """the 8-byte width: 2^64 - 59 with (f, k, kappa) = (8, 16, 16)"""
    _protocol_case(P64, 4, 1, 0, 20, 8, 16, 16, 64)


def test_coroutines_refuse_short_preprocessing_before_anything_is_opened():
    from honeybadgermpc_amd.progs import fixedpoint as fx

    p, n, t, count, k, kappa = BLS, 4, 1, 9, 64, 32
    ctx = _ctx(p)
    rnd = random.Random(3)
    x = _random_tensor(ctx, 40, count)
    bits = _random_tensor(ctx, 41, count, rows=2 * k + kappa)
    need = fx.carry_triples(k - 1)
    tr = tuple(_random_tensor(ctx, 42 + s, count, rows=need) for s in range(3))
    one = tuple(v[0] for v in tr)

    async def refused(co, i):
        if i:
            return None
        short_bits, short_tr = bits[:k + kappa - 1], tuple(v[:need - 1] for v in tr)
        for coro in (lambda: fx.trunc_pr(co, x, short_bits, k, 32, kappa), lambda: fx.trunc_pr(co, x, bits[:, :5], k, 32, kappa), lambda: fx.trunc_pr(co, x, bits, k, k, kappa),
                     lambda: fx.div2m(co, x, short_bits, tr, k, 32, kappa), lambda: fx.div2m(co, x, bits, tuple(v[:61] for v in tr), k, 32, kappa),
                     lambda: fx.trunc(co, x, bits, (tr[0], tr[1]), k, 32, kappa), lambda: fx.trunc(co, x, bits, (tr[0], tr[1], tr[2][:, :4]), k, 32, kappa),
                     lambda: fx.ltz(co, x, bits, short_tr), lambda: fx.ltz(co, x, short_bits, tr), lambda: fx.ltz(co, x[:5], bits, tr),
                     lambda: fx.lt(co, x, x[:3], bits, tr), lambda: fx.lt(co, x, x, bits, short_tr),
                     lambda: fx.mul(co, x, x, one, bits[:2 * k + kappa - 1]), lambda: fx.mul(co, x, x, (one[0], one[1][:4], one[2]), bits), lambda: fx.mul(co, x, x[:2], one, bits),
                     lambda: fx.get_carry_bit(co, x, bits[:32], tuple(v[:62] for v in tr)), lambda: fx.bit_ltl(co, x, bits[:32, :4], tr),
                     lambda: fx.FixedPointArray(co, x).ltz(short_bits, tr)):
            with pytest.raises(ValueError):
                await coro()
        return co.batches

    results = _run_parties(p, n, t, set(), rnd, refused)
    assert results[0] == 0                                               # nothing was opened

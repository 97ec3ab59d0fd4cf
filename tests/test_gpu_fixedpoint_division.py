"""GPU: honeybadgermpc_amd.progs.fixedpoint_division -- the kernels of csrc/hb_div.hip against the same steps composed from
share_arithmetic and fixedpoint.trunc_mask / trunc_pr_finish (what the package offered before) and against Python ints on sampled
elements, the in-place OR level, and the whole protocol over OpenCoalescers in one process: div, reciprocal, FixedPointArray.divide and
normalize open to exactly div_model / norm_model -- no tolerance -- in div_opens batches from div_triples triple rows and div_planes bit
planes."""
import random

import pytest

import bitdec_cases as bc
import division_cases as dc
from bitdec_cases import COUNTS, gpu_ctx, random_tensor, rows_of, sample
from conftest import BLS

pytestmark = pytest.mark.gpu


# ---- the kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", bc.GPU_FIELDS, ids=bc.GPU_FIELD_IDS)
def test_or_level_kernels_in_place(p):
    """every level over planes of any residues, both directions: the mask's rows, the nodes' new values, and every plane the level does
    not own exactly as it was"""
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd.progs import fixedpoint_division as fd

    ctx = gpu_ctx(p)
    torch = ctx.torch
    for n in dc.OR_PLANES:
        assert fd.preor_levels(n) == (n - 1).bit_length()
        for count in COUNTS:
            for level in range(fd.preor_levels(n)):
                for from_top in ((True, False) if n in (5, 9) or count == 257 else (True,)):
                    at = (lambda r: n - 1 - r) if from_top else (lambda r: r)
                    nodes = fd.preor_nodes(n, level)
                    tr = len(nodes)
                    y = random_tensor(ctx, 50 + count + level, count, rows=n)
                    ta, tb, tab = (random_tensor(ctx, 51 + s + count, count, rows=tr) for s in range(3))
                    opened = random_tensor(ctx, 54 + count, count, rows=2 * tr)
                    y0, keep = y.clone(), (ta.clone(), tb.clone(), tab.clone(), opened.clone())
                    masked = fd.or_mask(ctx, y, level, ta, tb, from_top)
                    assert tuple(masked.shape) == (2 * tr, count, ctx.n_limbs) and torch.equal(y, y0)
                    res = fd.or_combine(ctx, opened.view(2 * tr * count, ctx.n_limbs), y, level, ta, tb, tab, from_top)        # flat, as an open returns it
                    assert res.data_ptr() == y.data_ptr()
                    some = list(enumerate(nodes)) if n <= 9 or count <= 257 else list(enumerate(nodes))[:2] + list(enumerate(nodes))[-2:]
                    for i, (j, q) in some:
                        assert torch.equal(masked[2 * i], sa.sub(ctx, y0[at(j)], ta[i])) and torch.equal(masked[2 * i + 1], sa.sub(ctx, y0[at(q)], tb[i])), (n, level, j)
                        prod = sa.beaver_combine(ctx, opened[2 * i], opened[2 * i + 1], ta[i], tb[i], tab[i])
                        assert torch.equal(y[at(j)], sa.sub(ctx, sa.add(ctx, y0[at(j)], y0[at(q)]), prod)), (n, level, j, count)
                    owned = {at(j) for j, _ in nodes}
                    for i in range(n):
                        if i not in owned:
                            assert torch.equal(y[i], y0[i]), (n, level, i)
                    assert all(torch.equal(v, w) for v, w in zip((ta, tb, tab, opened), keep))
                    if count:
                        sel = torch.tensor(sample(count)[:8], device=ctx.tdev)
                        o, a, b, ab, yi, y1, mk = (rows_of(ctx, v.index_select(1, sel)) for v in (opened, ta, tb, tab, y0, y, masked))
                        for i, (j, q) in enumerate(nodes):
                            for e in range(len(sel)):
                                assert (mk[2 * i][e], mk[2 * i + 1][e]) == ((yi[at(j)][e] - a[i][e]) % p, (yi[at(q)][e] - b[i][e]) % p)
                                assert y1[at(j)][e] == (yi[at(j)][e] + yi[at(q)][e] - bc.beaver(o[2 * i][e], o[2 * i + 1][e], a[i][e], b[i][e], ab[i][e], p)) % p


def _trunc_shapes(p):
    """(width, m, kappa): the widths div uses at (8, 4), (12, 8) and (64, 32), and m at both ends"""
    return [(16, 6, 8), (16, 8, 8), (28, 16, 8), (128, 64, 32), (128, 127, 32)] if p >> 64 else [(16, 8, 8), (32, 16, 8), (40, 1, 8)]


@pytest.mark.parametrize("p", bc.GPU_FIELDS, ids=bc.GPU_FIELD_IDS)
def test_pair_norm_and_step_kernels(p):
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd.progs import fixedpoint as fx
    from honeybadgermpc_amd.progs import fixedpoint_division as fd

    ctx = gpu_ctx(p)
    torch = ctx.torch
    L = ctx.n_limbs
    rnd = random.Random(p % 997)
    for count in COUNTS:
        sel = torch.tensor(sample(count)[:8], device=ctx.tdev) if count else None
        x, u, aux, e0, e1 = (random_tensor(ctx, 60 + s + count, count) for s in range(5))
        ta, tb, tab = (random_tensor(ctx, 65 + s + count, count, rows=2) for s in range(3))
        opened = random_tensor(ctx, 70 + count, count, rows=4)
        na, nb = random_tensor(ctx, 71 + count, count), random_tensor(ctx, 72 + count, count)
        inputs = [x, u, aux, e0, e1, ta, tb, tab, opened, na, nb]
        copies = [t.clone() for t in inputs]
        prod = [sa.beaver_combine(ctx, opened[2 * r], opened[2 * r + 1], ta[r], tb[r], tab[r]) for r in range(2)]
        # the masked pair of one product
        got = fd.pair_mask(ctx, u, x, ta[0], tb[0])
        assert tuple(got.shape) == (2, count, L) and torch.equal(got[0], sa.sub(ctx, u, ta[0])) and torch.equal(got[1], sa.sub(ctx, x, tb[0]))
        # the scale step: v by Horner over z_i = y_i - y_{i+1}, then the masked pairs
        for n in dc.OR_PLANES:
            y = random_tensor(ctx, 73 + n + count, count, rows=n)
            yk = y.clone()
            acc = ctx.upload_ints([0] * count)
            for i in range(n):
                z = sa.sub(ctx, y[i], y[i + 1]) if i + 1 < n else y[i]
                acc = sa.add(ctx, sa.add(ctx, acc, acc), z)
            for signed in (True, False):
                products = 2 if signed else 1
                masked, v = fd.norm_mask(ctx, x, y, u if signed else None, ta[:products], tb[:products])
                assert tuple(masked.shape) == (2 * products, count, L) and torch.equal(v, acc), (n, count)
                want = [sa.sub(ctx, x, ta[0]), sa.sub(ctx, acc, tb[0])] + ([sa.sub(ctx, u, ta[1]), sa.sub(ctx, acc, tb[1])] if signed else [])
                assert all(torch.equal(masked[r], w) for r, w in enumerate(want)), (n, count, signed)
            assert torch.equal(y, yk)
            if count:
                ys, vs = rows_of(ctx, y.index_select(1, sel)), ctx.download_ints(v.index_select(0, sel))
                for e in range(len(sel)):
                    col = [ys[i][e] for i in range(n)] + [0]
                    assert vs[e] == sum((col[i] - col[i + 1]) << (n - 1 - i) for i in range(n)) % p, (n, count, e)
        # products to what the next open needs
        cst = rnd.randrange(p)
        cst_t = ctx.upload_ints([cst] * count)
        assert torch.equal(fd.product_step(ctx, fd.SIGN, opened[:2], ta[:1], tb[:1], tab[:1], aux=aux), sa.sub(ctx, aux, sa.mul(ctx, prod[0], 2)))
        for products in (2, 1):
            vp = sa.sub(ctx, aux, sa.mul(ctx, prod[1], 2)) if products == 2 else aux
            out = fd.product_step(ctx, fd.NORM, opened[:2 * products].reshape(2 * products * count, L), ta[:products], tb[:products], tab[:products], aux=aux)
            assert tuple(out.shape) == (2, count, L) and torch.equal(out[0], prod[0]) and torch.equal(out[1], vp), (count, products)
            out = fd.product_step(ctx, fd.NORM, opened[:2 * products], ta[:products], tb[:products], tab[:products], aux=aux, cst=cst, nxt=(na, nb))
            d = sa.sub(ctx, cst_t, sa.mul(ctx, prod[0], 2))
            assert torch.equal(out[0], sa.sub(ctx, d, na)) and torch.equal(out[1], sa.sub(ctx, vp, nb)), (count, products)
        for width, m, kappa in _trunc_shapes(p):
            nbits = width + kappa
            bits = random_tensor(ctx, 80 + width + count, count, rows=2 * nbits + 1)     # planes of any residues, and one more than needed
            bk = bits.clone()
            composed = []
            for r in range(2):
                mk, r1 = fx.trunc_mask(ctx, prod[r], bits[r * nbits:(r + 1) * nbits], width, m, kappa)
                composed.append((mk, sa.add(ctx, prod[r], r1)))
            masked, kept = fd.product_step(ctx, fd.FIRST, opened, ta, tb, tab, cst=cst, bits=bits, width=width, m=m, kappa=kappa)
            mk1, r1 = fx.trunc_mask(ctx, prod[1], bits[:nbits], width, m, kappa)
            assert tuple(masked.shape) == (1, count, L) and tuple(kept.shape) == (2, count, L)
            assert torch.equal(masked[0], mk1) and torch.equal(kept[0], sa.add(ctx, prod[1], r1)) and torch.equal(kept[1], sa.sub(ctx, cst_t, prod[0])), (count, width, m)
            for products in (1, 2):
                masked, s = fd.product_step(ctx, fd.TRUNC, opened[:2 * products], ta[:products], tb[:products], tab[:products], bits=bits, width=width, m=m, kappa=kappa)
                assert tuple(masked.shape) == tuple(s.shape) == (products, count, L)
                for r in range(products):
                    assert torch.equal(masked[r], composed[r][0]) and torch.equal(s[r], composed[r][1]), (count, width, m, products, r)
            assert torch.equal(bits, bk)
            if count and width in (16, 128, 32):
                o, a, b, ab, bt, mk, ss = (rows_of(ctx, t.index_select(1, sel)) for t in (opened, ta, tb, tab, bits, masked, s))
                for r in range(2):
                    for e in range(len(sel)):
                        pr = bc.beaver(o[2 * r][e], o[2 * r + 1][e], a[r][e], b[r][e], ab[r][e], p)
                        rr = sum(bt[r * nbits + i][e] << i for i in range(nbits))
                        r1v = sum(bt[r * nbits + i][e] << i for i in range(m))
                        assert (mk[r][e], ss[r][e]) == ((pr + (1 << (width - 1)) + rr) % p, (pr + r1v) % p), (count, width, m, r, e)
        # truncation to what the next open needs
        vals, r1s, c = (random_tensor(ctx, 90 + s + count, count, rows=2) for s in range(3))
        s2 = torch.stack([sa.add(ctx, vals[r], r1s[r]) for r in range(2)]) if count else vals.clone()
        kc = (s2.clone(), c.clone())
        for m in (1, 8) + ((64, 127, 130) if p >> 64 else (61,)):
            t = [fx.trunc_pr_finish(ctx, vals[r], c[r], r1s[r], m) for r in range(2)]
            assert torch.equal(fd.trunc_step(ctx, fd.T_RESULT, c[:1], s2[:1], m), t[0]), (count, m)
            out = fd.trunc_step(ctx, fd.T_RECIP, c[0], s2[:1], m, ta, tb, ext=(e0, e1))
            want = [sa.sub(ctx, e0, ta[0]), sa.sub(ctx, t[0], tb[0]), sa.sub(ctx, e1, ta[1]), sa.sub(ctx, t[0], tb[1])]
            assert tuple(out.shape) == (4, count, L) and all(torch.equal(out[r], w) for r, w in enumerate(want)), (count, m)
            for rows in (1, 2):
                xs = t[1] if rows == 2 else x
                for products in (1, 2):
                    out = fd.trunc_step(ctx, fd.T_GOLD, c[:rows].reshape(rows * count, L), s2[:rows], m, ta[:products], tb[:products], x=x if rows == 1 else None, alpha=cst)
                    want = [sa.sub(ctx, t[0], ta[0]), sa.sub(ctx, sa.add(ctx, xs, cst_t), tb[0])] + ([sa.sub(ctx, xs, ta[1]), sa.sub(ctx, xs, tb[1])] if products == 2 else [])
                    assert tuple(out.shape) == (2 * products, count, L) and all(torch.equal(out[r], w) for r, w in enumerate(want)), (count, m, rows, products)
            if count:
                cs, ss, a, b, got = (rows_of(ctx, v.index_select(1, sel)) for v in (c, s2, ta, tb, out))
                inv = pow(2, -m, p)
                for e in range(len(sel)):
                    t0, t1 = ((ss[r][e] - cs[r][e] % (1 << m)) * inv % p for r in range(2))
                    assert [got[r][e] for r in range(4)] == [(t0 - a[0][e]) % p, (cst + t1 - b[0][e]) % p, (t1 - a[1][e]) % p, (t1 - b[1][e]) % p], (count, m, e)
        assert torch.equal(s2, kc[0]) and torch.equal(c, kc[1]) and all(torch.equal(t, cp) for t, cp in zip(inputs, copies))


def test_inputs_untouched_out_honoured_overlap_refused_and_asynchronous():
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd._capi import HB_ERR_BAD_ARG, HbmpcBackendError
    from honeybadgermpc_amd.progs import fixedpoint_division as fd

    p, count, n, level, width, m, kappa = BLS, 600, 9, 1, 16, 8, 8
    ctx = gpu_ctx(p)
    torch = ctx.torch
    L, nbits = ctx.n_limbs, width + kappa
    tr = fd.preor_level_triples(n, level)
    x, u, v0, e0, e1 = (random_tensor(ctx, 131 + s, count) for s in range(5))
    y = random_tensor(ctx, 136, count, rows=n)
    ta, tb, tab = (random_tensor(ctx, 137 + s, count, rows=n) for s in range(3))                  # n >= tr rows: sliced per call
    opened = random_tensor(ctx, 140, count, rows=2 * n)
    bits = random_tensor(ctx, 141, count, rows=2 * nbits)
    ops = [x, u, v0, e0, e1, y, ta, tb, tab, opened, bits]
    copies = [t.clone() for t in ops]
    alpha = 1 << 8

    def run():
        y2 = y.clone()
        lvl = fd.or_mask(ctx, y2, level, ta[:tr], tb[:tr])
        fd.or_combine(ctx, opened[:2 * tr], y2, level, ta[:tr], tb[:tr], tab[:tr])
        pm = fd.pair_mask(ctx, u, x, ta[0], tb[0])
        nm, v = fd.norm_mask(ctx, x, y, u, ta[:2], tb[:2])
        sg = fd.product_step(ctx, fd.SIGN, opened[:2], ta[:1], tb[:1], tab[:1], aux=x)
        nr = fd.product_step(ctx, fd.NORM, opened[:4], ta[:2], tb[:2], tab[:2], aux=v0, cst=5, nxt=(ta[2], tb[2]))
        fm, fk = fd.product_step(ctx, fd.FIRST, opened[:4], ta[:2], tb[:2], tab[:2], cst=alpha, bits=bits, width=width, m=m, kappa=kappa)
        tm, ts = fd.product_step(ctx, fd.TRUNC, opened[:4], ta[:2], tb[:2], tab[:2], bits=bits, width=width, m=m, kappa=kappa)
        rc = fd.trunc_step(ctx, fd.T_RECIP, opened[:1], ts[:1], m, ta[:2], tb[:2], ext=(e0, e1))
        gd = fd.trunc_step(ctx, fd.T_GOLD, opened[:2], ts, m, ta[:2], tb[:2], alpha=alpha)
        rs = fd.trunc_step(ctx, fd.T_RESULT, opened[:1], ts[:1], m)
        return [y2, lvl, pm, nm, v, sg, nr, fm, fk, tm, ts, rc, gd, rs]

    first = run()
    # results consumed on the current stream without a synchronise, and on a side stream
    rs = first[-1]
    assert torch.equal(sa.sub(ctx, sa.add(ctx, rs, rs), rs), rs)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        second = run()
    side.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    y2, lvl, pm, nm, v, sg, nr, fm, fk, tm, ts, rc, gd, rs = first
    # out given: written where asked, and handed back
    ob = torch.empty_like(lvl)
    assert fd.or_mask(ctx, y, level, ta[:tr], tb[:tr], out=ob).data_ptr() == ob.data_ptr()
    ob2, vb = torch.empty_like(nm), torch.empty_like(v)
    got = fd.norm_mask(ctx, x, y, u, ta[:2], tb[:2], out=ob2, v_out=vb)
    assert got[0].data_ptr() == ob2.data_ptr() and got[1].data_ptr() == vb.data_ptr() and torch.equal(ob2, nm) and torch.equal(vb, v)
    pb = torch.empty_like(pm)
    assert fd.pair_mask(ctx, u, x, ta[0], tb[0], out=pb).data_ptr() == pb.data_ptr() and torch.equal(pb, pm)
    sb = torch.empty_like(sg)
    assert fd.product_step(ctx, fd.SIGN, opened[:2], ta[:1], tb[:1], tab[:1], aux=x, out=sb).data_ptr() == sb.data_ptr() and torch.equal(sb, sg)
    mb, kb = torch.empty_like(tm), torch.empty_like(ts)
    got = fd.product_step(ctx, fd.TRUNC, opened[:4], ta[:2], tb[:2], tab[:2], bits=bits, width=width, m=m, kappa=kappa, out=(mb, kb))
    assert got[0].data_ptr() == mb.data_ptr() and got[1].data_ptr() == kb.data_ptr() and torch.equal(mb, tm) and torch.equal(kb, ts)
    gb = torch.empty_like(gd)
    assert fd.trunc_step(ctx, fd.T_GOLD, opened[:2], ts, m, ta[:2], tb[:2], alpha=alpha, out=gb).data_ptr() == gb.data_ptr() and torch.equal(gb, gd)
    assert all(torch.equal(t, cp) for t, cp in zip(ops, copies))
    # argument checks raise before C and nothing is launched: the buffers keep their contents
    gb.fill_(7)
    y3 = y.clone()
    wide = torch.zeros((n, count, 2, L), dtype=torch.int64, device=ctx.tdev)
    bad_calls = [
        lambda: fd.or_mask(ctx, y, level, ta[:tr - 1], tb[:tr]),
        lambda: fd.or_mask(ctx, y, level, ta[:tr + 1], tb[:tr + 1]),
        lambda: fd.or_mask(ctx, y, 4, ta[:tr], tb[:tr]),                                          # level >= the number of levels
        lambda: fd.or_mask(ctx, y, -1, ta[:tr], tb[:tr]),
        lambda: fd.or_mask(ctx, y[:1], 0, ta[:1], tb[:1]),                                        # one plane has no level
        lambda: fd.or_mask(ctx, y, level, ta[:tr], tb[:tr], out=ob[:-1]),
        lambda: fd.or_combine(ctx, opened[:2 * tr - 1], y3, level, ta[:tr], tb[:tr], tab[:tr]),
        lambda: fd.or_combine(ctx, opened[:2 * tr], wide[:, :, 0], level, ta[:tr], tb[:tr], tab[:tr]),   # in place needs the array itself
        lambda: fd.or_combine(ctx, opened[:2 * tr], y3, level, ta[:tr], tb[:tr], tab[:tr, :-1]),
        lambda: fd.norm_mask(ctx, x, y, u, ta[:1], tb[:1]),                                       # signed takes two triples
        lambda: fd.norm_mask(ctx, x, y, None, ta[:2], tb[:2]),
        lambda: fd.norm_mask(ctx, x[:-1], y, u, ta[:2], tb[:2]),
        lambda: fd.pair_mask(ctx, u, x[:-1], ta[0], tb[0]),
        lambda: fd.product_step(ctx, 9, opened[:2], ta[:1], tb[:1], tab[:1], aux=x),
        lambda: fd.product_step(ctx, fd.SIGN, opened[:4], ta[:2], tb[:2], tab[:2], aux=x),
        lambda: fd.product_step(ctx, fd.SIGN, opened[:3], ta[:1], tb[:1], tab[:1], aux=x),
        lambda: fd.product_step(ctx, fd.FIRST, opened[:2], ta[:1], tb[:1], tab[:1], cst=alpha, bits=bits, width=width, m=m, kappa=kappa),
        lambda: fd.product_step(ctx, fd.TRUNC, opened[:4], ta[:2], tb[:2], tab[:2], bits=bits[:-1], width=width, m=m, kappa=kappa),
        lambda: fd.product_step(ctx, fd.TRUNC, opened[:4], ta[:2], tb[:2], tab[:2], bits=bits, width=width, m=width, kappa=kappa),
        lambda: fd.product_step(ctx, fd.TRUNC, opened[:4], ta[:2], tb[:2], tab[:2], bits=bits, width=250, m=m, kappa=kappa),
        lambda: fd.product_step(ctx, fd.TRUNC, opened[:4], ta[:2], tb[:2], tab[:2], bits=bits, width=width, m=m, kappa=kappa, out=(mb, kb[:-1])),
        lambda: fd.product_step(ctx, fd.NORM, opened[:4], ta[:2], tb[:2], tab[:2], aux=v0, cst=5, nxt=(ta[2],)),
        lambda: fd.trunc_step(ctx, 5, opened[:1], ts[:1], m),
        lambda: fd.trunc_step(ctx, fd.T_RESULT, opened[:1], ts[:1], 0),
        lambda: fd.trunc_step(ctx, fd.T_RESULT, opened[:1], ts[:1], 254),
        lambda: fd.trunc_step(ctx, fd.T_RESULT, opened[:2], ts, m),
        lambda: fd.trunc_step(ctx, fd.T_RECIP, opened[:1], ts[:1], m, ta[:1], tb[:1], ext=(e0, e1)),
        lambda: fd.trunc_step(ctx, fd.T_GOLD, opened[:2], ts, m, ta[:2], tb[:1], alpha=alpha),
        lambda: fd.trunc_step(ctx, fd.T_GOLD, opened[:2], ts, m, ta[:2], tb[:2], alpha=alpha, out=gb[:-1]),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"bad call {i} was accepted")
    for call in (lambda: fd.or_mask(ctx, y.to(torch.int32), level, ta[:tr], tb[:tr]), lambda: fd.norm_mask(ctx, x, [1], u, ta[:2], tb[:2]),
                 lambda: fd.trunc_step(ctx, fd.T_GOLD, opened[:1], ts[:1], m, ta[:2], tb[:2], alpha=alpha)):      # one row needs the kept x
        with pytest.raises(TypeError):
            call()
    # an output laid over an input is refused by the C ABI, through Python too
    buf = random_tensor(ctx, 142, count, rows=6)
    for call in (lambda: fd.or_mask(ctx, y3, level, ta[:tr], tb[:tr], out=y3[:2 * tr]),
                 lambda: fd.or_combine(ctx, y3[:2 * tr], y3, level, ta[:tr], tb[:tr], tab[:tr]),
                 lambda: fd.or_combine(ctx, opened[:2 * tr], y3, level, y3[:tr], tb[:tr], tab[:tr]),
                 lambda: fd.norm_mask(ctx, x, y, u, buf[:2], tb[:2], out=buf[:4]),
                 lambda: fd.norm_mask(ctx, x, y, u, ta[:2], tb[:2], v_out=x),
                 lambda: fd.pair_mask(ctx, u, x, buf[0], tb[0], out=buf[:2]),
                 lambda: fd.product_step(ctx, fd.SIGN, opened[:2], ta[:1], tb[:1], tab[:1], aux=x, out=x),
                 lambda: fd.product_step(ctx, fd.TRUNC, opened[:4], ta[:2], tb[:2], tab[:2], bits=bits, width=width, m=m, kappa=kappa, out=(mb, mb)),
                 lambda: fd.product_step(ctx, fd.TRUNC, opened[:4], ta[:2], tb[:2], tab[:2], bits=bits, width=width, m=m, kappa=kappa, out=(bits[:2], kb)),
                 lambda: fd.trunc_step(ctx, fd.T_RESULT, opened[:1], ts[:1], m, out=ts[0]),
                 lambda: fd.trunc_step(ctx, fd.T_GOLD, buf[:2], ts, m, ta[:2], tb[:2], alpha=alpha, out=buf[:4])):
        with pytest.raises(HbmpcBackendError):
            call()
    # ... and the C ABI itself
    lib, st, P = ctx.lib, ctx.stream(), ctx.ptr
    one_elem = ctx.host_elems([1])
    one = one_elem.ctypes.data
    assert lib.hb_div_pair_mask(ctx.h, P(u), P(x), P(ta), P(tb), None, count, st) == HB_ERR_BAD_ARG
    assert lib.hb_div_pair_mask(ctx.h, P(u), P(x), P(ta), P(tb), P(u), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_div_or_mask(ctx.h, P(y), n, 4, 1, P(ta), P(tb), P(ob), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_div_or_mask(ctx.h, P(y), 257, 0, 1, P(ta), P(tb), P(ob), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_div_or_mask(ctx.h, P(y), n, level, 1, P(ta), P(tb), P(y), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_div_or_mask(ctx.h, P(y), n, level, 1, P(ta), P(tb), P(ob), -1, st) == HB_ERR_BAD_ARG
    assert lib.hb_div_or_combine(ctx.h, P(opened), P(y3), n, -1, 1, P(ta), P(tb), P(tab), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_div_or_combine(ctx.h, P(opened), P(y3), n, level, 1, P(ta), P(tb), None, count, st) == HB_ERR_BAD_ARG
    assert lib.hb_div_or_combine(ctx.h, P(opened), P(y3), n, level, 1, P(y3), P(tb), P(tab), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_div_norm_mask(ctx.h, P(x), P(y), 0, P(u), P(ta), P(tb), P(ob2), P(vb), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_div_norm_mask(ctx.h, P(x), P(y), n, P(u), P(ta), P(tb), P(ob2), None, count, st) == HB_ERR_BAD_ARG
    assert lib.hb_div_norm_mask(ctx.h, P(x), P(y), n, P(u), P(ta), P(tb), P(y), P(vb), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_div_product_step(ctx.h, 9, 1, P(opened), P(ta), P(tb), P(tab), P(x), None, None, None, None, 0, 0, 0, P(sb), None, count, st) == HB_ERR_BAD_ARG
    assert lib.hb_div_product_step(ctx.h, fd.SIGN, 2, P(opened), P(ta), P(tb), P(tab), P(x), None, None, None, None, 0, 0, 0, P(sb), None, count, st) == HB_ERR_BAD_ARG
    assert lib.hb_div_product_step(ctx.h, fd.SIGN, 1, P(opened), P(ta), P(tb), P(tab), None, None, None, None, None, 0, 0, 0, P(sb), None, count, st) == HB_ERR_BAD_ARG
    assert lib.hb_div_product_step(ctx.h, fd.NORM, 2, P(opened), P(ta), P(tb), P(tab), P(v0), one, P(ta), None, None, 0, 0, 0, P(ob2), None, count, st) == HB_ERR_BAD_ARG
    assert lib.hb_div_product_step(ctx.h, fd.NORM, 2, P(opened), P(ta), P(tb), P(tab), P(v0), None, P(ta), P(tb), None, 0, 0, 0, P(ob2), None, count, st) == HB_ERR_BAD_ARG
    assert lib.hb_div_product_step(ctx.h, fd.TRUNC, 2, P(opened), P(ta), P(tb), P(tab), None, None, None, None, P(bits), width, width, kappa, P(mb), P(kb), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_div_product_step(ctx.h, fd.TRUNC, 2, P(opened), P(ta), P(tb), P(tab), None, None, None, None, P(bits), width, m, kappa, P(mb), None, count, st) == HB_ERR_BAD_ARG
    assert lib.hb_div_product_step(ctx.h, fd.TRUNC, 2, P(opened), P(ta), P(tb), P(tab), None, None, None, None, P(bits), width, m, kappa, P(mb), P(opened), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_div_trunc_step(ctx.h, 5, 1, 0, P(opened), P(ts), m, one, None, None, None, None, None, None, P(gb), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_div_trunc_step(ctx.h, fd.T_RESULT, 1, 0, P(opened), P(ts), m, None, None, None, None, None, None, None, P(gb), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_div_trunc_step(ctx.h, fd.T_RESULT, 1, 1, P(opened), P(ts), m, one, None, None, None, None, None, None, P(gb), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_div_trunc_step(ctx.h, fd.T_RESULT, 1, 0, P(opened), P(ts), m, one, None, None, None, None, None, None, P(ts), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_div_trunc_step(ctx.h, fd.T_GOLD, 1, 2, P(opened), P(ts), m, one, one, None, None, None, P(ta), P(tb), P(gb), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_div_trunc_step(ctx.h, fd.T_GOLD, 2, 2, P(opened), P(ts), m, one, None, None, None, None, P(ta), P(tb), P(gb), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_div_trunc_step(ctx.h, fd.T_RECIP, 1, 2, P(opened), P(ts), m, one, None, None, P(e0), None, P(ta), P(tb), P(gb), count, st) == HB_ERR_BAD_ARG
    # count == 0: a successful call that launches nothing
    assert lib.hb_div_or_combine(ctx.h, P(opened), P(y3), n, level, 1, P(ta), P(tb), P(tab), 0, st) == 0
    assert lib.hb_div_norm_mask(ctx.h, P(x), P(y), n, P(u), P(ta), P(tb), P(ob2), P(vb), 0, st) == 0
    assert lib.hb_div_product_step(ctx.h, fd.TRUNC, 2, P(opened), P(ta), P(tb), P(tab), None, None, None, None, P(bits), width, m, kappa, P(mb), P(kb), 0, st) == 0
    assert lib.hb_div_trunc_step(ctx.h, fd.T_GOLD, 2, 2, P(opened), P(ts), m, one, one, None, None, None, P(ta), P(tb), P(gb), 0, st) == 0
    torch.cuda.synchronize()
    assert bool((gb == 7).all()) and torch.equal(y3, y) and torch.equal(ob2, nm) and torch.equal(vb, v) and torch.equal(mb, tm) and torch.equal(kb, ts) and torch.equal(sb, sg)
    assert all(torch.equal(t, cp) for t, cp in zip(ops, copies))


# ---- the protocol, end to end ---------------------------------------------------------------------------------------------------
WIDE_SHAPES, NARROW_SHAPES = [(8, 4, 8), (12, 8, 8), (16, 8, 8)], [(8, 4, 8), (16, 8, 8)]
E2E = [(p, shape, n) for n in (4, 7) for p in bc.GPU_FIELDS for shape in (WIDE_SHAPES if p >> 64 else NARROW_SHAPES)] + [(BLS, (64, 32, 32), 4)]
E2E_IDS = [f"n{n}-{bc.GPU_FIELD_IDS[bc.GPU_FIELDS.index(p)]}-k{k}-f{f}" for p, (k, f, kappa), n in E2E]


@pytest.mark.parametrize("signed", [True, False], ids=["signed", "unsigned"])
@pytest.mark.parametrize("p, shape, n", E2E, ids=E2E_IDS)
def test_protocol_end_to_end(p, shape, n, signed):
    from honeybadgermpc_amd.progs import fixedpoint as fx
    from honeybadgermpc_amd.progs import fixedpoint_division as fd

    k, f, kappa = shape
    t, liars = (1, 1) if n == 4 else (2, 0)
    count = 33
    ctx = gpu_ctx(p)
    torch = ctx.torch
    rnd = random.Random(1000 * n + 10 * k + f + signed)
    bad = set(rnd.sample(range(n), liars))
    honest = [i for i in range(n) if i not in bad]
    lay = fd.div_layout(k, f, kappa, None, signed)
    theta, n_planes, n_triples = lay["theta"], lay["n_planes"], lay["n_triples"]
    assert theta == fd.goldschmidt_iterations(k, f)
    avals, bvals = dc.e2e_inputs(rnd, k, f, count, signed)
    low = 1 << (2 * f - k + 2)                                            # reciprocal: 2^f 2^f / |b| < 2^(k-2)
    rvals = [b if abs(b) > low else (low + 1 + e) * (-1 if b < 0 else 1) for e, b in enumerate(bvals)]
    bit_rows = [[rnd.getrandbits(1) for _ in range(count)] for _ in range(n_planes)]
    start, _ = lay["planes"]["y0"]
    for i in range(f):
        bit_rows[start + i][0] = 1                                       # an all-ones r1 under the truncation of Y = [a w]
    names = ["w", "y0"] + [f"iter{i}.{v}" for i in range(1, theta) for v in "yx"] + ["last"]
    limits = dc.r1_limits(fd, k, f, theta)
    r1s = [[sum(bit_rows[lay["planes"][name][0] + i][e] << i for i in range(m)) for name, m in zip(names, limits)] for e in range(count)]
    bit_rows.append([rnd.randrange(p) for _ in range(count)])            # a canary plane and a canary row: reading either would spoil the results
    ta, tb = ([[rnd.randrange(p) for _ in range(count)] for _ in range(n_triples)] for _ in range(2))
    tab = [[x * y % p for x, y in zip(ra, rb)] for ra, rb in zip(ta, tb)]
    for v in (ta, tb, tab):
        v.append([rnd.randrange(p) for _ in range(count)])
    bits = bc.deal_planes(ctx, rnd, p, n, t, bit_rows)
    trip = [bc.deal_planes(ctx, rnd, p, n, t, v) for v in (ta, tb, tab)]
    vals = bc.deal_planes(ctx, rnd, p, n, t, [[v % p for v in avals], [v % p for v in bvals], [v % p for v in rvals]])
    n_or = 9
    or_bits = [[rnd.getrandbits(1) for _ in range(count)] for _ in range(n_or)]
    or_planes = bc.deal_planes(ctx, rnd, p, n, t, or_bits)

    async def body(co, i):
        a, b, r = vals[i][0], vals[i][1], vals[i][2]
        triples = tuple(tr[i] for tr in trip)
        exact_bits, exact_triples = bits[i][:n_planes], tuple(v[:n_triples] for v in triples)
        keep = (vals[i].clone(), bits[i].clone(), [v.clone() for v in triples], or_planes[i].clone())
        for short in (lambda: fd.div(co, a, b, exact_bits, tuple(v[:n_triples - 1] for v in triples), f, k, kappa, signed=signed),
                      lambda: fd.div(co, a, b, exact_bits[:n_planes - 1], exact_triples, f, k, kappa, signed=signed),
                      lambda: fd.reciprocal(co, r, exact_bits[:n_planes - 1], exact_triples, f, k, kappa, signed=signed),
                      lambda: fd.normalize(co, b, exact_bits, tuple(v[:fd.norm_triples(k, signed) - 1] for v in triples), k, kappa, signed),
                      lambda: fx.FixedPointArray(co, a, f, k, kappa).divide(fx.FixedPointArray(co, b, f, k, kappa), exact_bits, tuple(v[:n_triples - 1] for v in triples), signed),
                      lambda: fd.prefix_or(co, or_planes[i], tuple(v[:fd.preor_triples(n_or) - 1] for v in triples))):
            with pytest.raises(ValueError):
                await short()
        assert co.batches == 0                                            # one row fewer: refused before anything was opened
        got, batches = {}, {}

        async def step(name, coro):
            before = co.batches
            res = await coro
            batches[name] = co.batches - before
            if isinstance(res, fx.FixedPointArray):
                assert (res.f, res.k, res.kappa) == (f, k, kappa)
                res = res.shares
            res = res if isinstance(res, tuple) else (res,)
            got[name] = [ctx.download_ints(await co.open_share_array(v.reshape(-1, ctx.n_limbs))) for v in res]

        await step("div", fd.div(co, a, b, bits[i], triples, f, k, kappa, signed=signed))
        await step("exact rows", fd.div(co, a, b, exact_bits, exact_triples, f, k, kappa, theta, signed))
        await step("reciprocal", fd.reciprocal(co, r, exact_bits, exact_triples, f, k, kappa, signed=signed))
        await step("divide", fx.FixedPointArray(co, a, f, k, kappa).divide(fx.FixedPointArray(co, b, f, k, kappa), bits[i], triples, signed))
        await step("FixedPointArray.reciprocal", fx.FixedPointArray(co, r, f, k, kappa).reciprocal(exact_bits, exact_triples, signed))
        await step("normalize", fd.normalize(co, b, bits[i], triples, k, kappa, signed))
        await step("prefix_or top", fd.prefix_or(co, or_planes[i], triples))
        await step("prefix_or bottom", fd.prefix_or(co, or_planes[i], tuple(v[:fd.preor_triples(n_or)] for v in triples), from_top=False))
        assert torch.equal(vals[i], keep[0]) and torch.equal(bits[i], keep[1]) and all(torch.equal(v, w) for v, w in zip(triples, keep[2])) and torch.equal(or_planes[i], keep[3])
        return got, batches

    results = bc.run_parties(p, n, t, bad, rnd, body)
    want_div = [fd.div_model(avals[e], bvals[e], p, k, f, r1s[e], theta, signed) for e in range(count)]
    want_rec = [fd.div_model(1 << f, rvals[e], p, k, f, r1s[e], theta, signed) for e in range(count)]
    norm = [fd.norm_model(b, k, signed) for b in bvals]
    bound = fd.div_error_bound(k, f, theta)
    assert all(abs(fd._centered(w, p) - avals[e] * 2 ** f / bvals[e]) <= bound for e, w in enumerate(want_div))     # the fixed inputs are in range
    for i in honest:
        got, batches = results[i]
        assert got["div"] == [want_div] and got["exact rows"] == [want_div] and got["divide"] == [want_div], i
        assert got["reciprocal"] == [want_rec] and got["FixedPointArray.reciprocal"] == [want_rec], i
        assert got["normalize"] == [[c % p for c, _ in norm], [v % p for _, v in norm]], i
        assert got["prefix_or top"] == [[int(any(or_bits[j][e] for j in range(r, n_or))) for r in range(n_or) for e in range(count)]], i
        assert got["prefix_or bottom"] == [[int(any(or_bits[j][e] for j in range(r + 1))) for r in range(n_or) for e in range(count)]], i
        assert batches == {"div": lay["opens"], "exact rows": lay["opens"], "reciprocal": lay["opens"], "divide": lay["opens"], "FixedPointArray.reciprocal": lay["opens"],
                           "normalize": fd.norm_opens(k, signed),
                           "prefix_or top": fd.preor_levels(n_or), "prefix_or bottom": fd.preor_levels(n_or)}, i
        assert lay["opens"] == fd.div_opens(k, f, theta, signed)


"""GPU: honeybadgermpc_amd.progs.fixedpoint_sqrt -- every step of csrc/hb_fxsqrt.hip bit-equal to its host self-test row (the same row,
the same step function) and to the step composed from share_arithmetic; inputs untouched, out= honoured, overlaps refused, nothing
synchronises; and the whole protocol among n = 4 parties in one process: sqrt, rsqrt and sqrt_rsqrt open to exactly sqrt_model for the
dealt r1 -- no tolerance -- and their shares are bit-equal to the same steps composed from share_arithmetic, fixedpoint.trunc_mask /
trunc_pr_finish and index_select, in sqrt_opens batches from sqrt_triples triple rows and sqrt_planes bit planes."""
import random

import pytest

import bitdec_cases as bc
import sqrt_cases as sc
from bitdec_cases import COUNTS, gpu_ctx, random_tensor
from conftest import BLS
from sqrt_cases import BOTH, FIRST, GH, NORM_MASK, OUT, R, RSQRT, SQRT, TRUNC_STEP

pytestmark = pytest.mark.gpu
PLANES = (1, 2, 3, 7, 15, 63)


# ---- the kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", bc.GPU_FIELDS, ids=bc.GPU_FIELD_IDS)
def test_every_step_equals_its_selftest_row(p):
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd.progs import fixedpoint as fx
    from honeybadgermpc_amd.progs import fixedpoint_sqrt as fs

    ctx = gpu_ctx(p)
    torch = ctx.torch
    L = ctx.n_limbs
    rnd = random.Random(p % 991)
    same = lambda got, want: torch.equal(got.cpu(), want)
    for count in COUNTS:
        x, na, nb = (random_tensor(ctx, 300 + s + count, count) for s in range(3))
        ta, tb, tab, kept = (random_tensor(ctx, 303 + s + count, count, rows=2) for s in range(4))
        opened, s2 = random_tensor(ctx, 307 + count, count, rows=2), random_tensor(ctx, 308 + count, count, rows=2)
        inputs = [x, na, nb, ta, tb, tab, kept, opened, s2]
        copies = [t.clone() for t in inputs]
        # the scale step: 1 and 2 sets of weights, any residues for weights
        for n in PLANES:
            y = random_tensor(ctx, 310 + n + count, count, rows=n)
            yk = y.clone()
            for sets in (1, 2):
                w = random_tensor(ctx, 311 + n + sets, sets * n).view(sets, n, L)
                masked, kp = fs.sqrt_norm_mask(ctx, x, y, w, ta[:1], tb[:1])
                assert tuple(masked.shape) == (2, count, L) and tuple(kp.shape) == (1 + sets, count, L)
                want = sc.selftest_on_tensors(ctx, NORM_MASK, [x, y, w, ta[:1], tb[:1]], [n, sets], [2, 1 + sets], count)
                assert same(masked, want[0]) and same(kp, want[1]), (n, sets, count)
                if count in (1, 257) and n in (3, 15):                          # ... and the composed step
                    wi = ctx.download_ints(w.reshape(-1, L))
                    acc, ts = ctx.upload_ints([0] * count), [ctx.upload_ints([0] * count) for _ in range(sets)]
                    for i in range(n):
                        acc = sa.sub(ctx, sa.add(ctx, acc, acc), y[i]) if i else y[i].clone()
                        ts = [sa.add(ctx, t, sa.mul(ctx, y[i], wi[s * n + i])) for s, t in enumerate(ts)]
                    assert torch.equal(kp[0], acc) and all(torch.equal(kp[1 + s], t) for s, t in enumerate(ts)), (n, sets, count)
                    assert torch.equal(masked[0], sa.sub(ctx, x, ta[0])) and torch.equal(masked[1], sa.sub(ctx, acc, tb[0]))
            assert torch.equal(y, yk)
        # the first approximation
        for k in (8, 16, 64):
            if fs.a_prime(k) >= p:
                continue
            masked, h = fs.sqrt_first(ctx, opened.view(2 * count, L), ta[:1], tb[:1], tab[:1], (na, nb), k)
            assert tuple(masked.shape) == (2, count, L) and tuple(h.shape) == (count, L)
            want = sc.selftest_on_tensors(ctx, FIRST, [opened, ta[:1], tb[:1], tab[:1], [fs.a_prime(k)], [fs.Y0_SLOPE], na, nb], [], [2, 1], count)
            assert same(masked, want[0]) and same(h.view(1, count, L), want[1]), (k, count)
            c = sa.beaver_combine(ctx, opened[0], opened[1], ta[0], tb[0], tab[0])
            y0 = sa.add(ctx, sa.neg(ctx, sa.mul(ctx, c, fs.Y0_SLOPE)), fs.a_prime(k))
            assert torch.equal(h, y0) and torch.equal(masked[0], sa.sub(ctx, c, na)) and torch.equal(masked[1], sa.sub(ctx, y0, nb)), (k, count)
        # truncation to what the next open needs: every mode, one and two products
        vals, r1s = random_tensor(ctx, 320 + count, count, rows=2), random_tensor(ctx, 321 + count, count, rows=2)
        for m in (1, 8) + ((64, 127, 140) if p >> 64 else (61,)):
            inv, cst = [pow(2, -m, p)], rnd.randrange(p)
            ss = torch.stack([sa.add(ctx, vals[r], r1s[r]) for r in range(2)]) if count else vals.clone()
            t = [fx.trunc_pr_finish(ctx, vals[r], opened[r], r1s[r], m) for r in range(2)]
            for rows in (1, 2):
                masked, gh = fs.sqrt_trunc_step(ctx, GH, opened[:rows], ss[:rows], m, ta[:1], tb[:1], kept=kept[0] if rows == 1 else None)
                want = sc.selftest_on_tensors(ctx, TRUNC_STEP, [opened[:rows], ss[:rows], inv, None, kept[:1] if rows == 1 else None, ta[:1], tb[:1]], [GH, rows, BOTH, m],
                                              [2, 2], count)
                assert same(masked, want[0]) and same(gh, want[1]), (m, rows, count)
                h = t[1] if rows == 2 else kept[0]
                assert torch.equal(gh[0], t[0]) and torch.equal(gh[1], h) and torch.equal(masked[0], sa.sub(ctx, t[0], ta[0])) and torch.equal(masked[1], sa.sub(ctx, h, tb[0]))
            r = sa.add(ctx, sa.neg(ctx, t[0]), cst)
            for which in (SQRT, RSQRT, BOTH):
                products = 2 if which == BOTH else 1
                masked = fs.sqrt_trunc_step(ctx, R, opened[0], ss[:1], m, ta[:products], tb[:products], kept=kept, which=which, cst=cst)
                want = sc.selftest_on_tensors(ctx, TRUNC_STEP, [opened[:1], ss[:1], inv, [cst], kept, ta[:products], tb[:products]], [R, 1, which, m], [2 * products, 0], count)
                assert tuple(masked.shape) == (2 * products, count, L) and same(masked, want[0]), (m, which, count)
                firsts = [kept[0], kept[1]] if which == BOTH else [kept[0 if which == SQRT else 1]]
                for q, first in enumerate(firsts):
                    assert torch.equal(masked[2 * q], sa.sub(ctx, first, ta[q])) and torch.equal(masked[2 * q + 1], sa.sub(ctx, r, tb[q])), (m, which, q)
                masked = fs.sqrt_trunc_step(ctx, OUT, opened[:products], ss[:products], m, ta[:products], tb[:products], kept=kept[:products], which=which)
                want = sc.selftest_on_tensors(ctx, TRUNC_STEP, [opened[:products], ss[:products], inv, None, kept[:products], ta[:products], tb[:products]],
                                              [OUT, products, which, m], [2 * products, 0], count)
                assert tuple(masked.shape) == (2 * products, count, L) and same(masked, want[0]), (m, which, count)
                for q in range(products):
                    assert torch.equal(masked[2 * q], sa.sub(ctx, t[q], ta[q])) and torch.equal(masked[2 * q + 1], sa.sub(ctx, kept[q], tb[q])), (m, which, q)
        assert all(torch.equal(t, cp) for t, cp in zip(inputs, copies))


def test_inputs_untouched_out_honoured_overlap_refused_and_asynchronous():
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd._capi import HB_ERR_BAD_ARG, HbmpcBackendError
    from honeybadgermpc_amd.progs import fixedpoint_sqrt as fs

    p, count, n, m, k = BLS, 600, 9, 8, 16
    ctx = gpu_ctx(p)
    torch = ctx.torch
    L = ctx.n_limbs
    x, na, nb = (random_tensor(ctx, 400 + s, count) for s in range(3))
    y = random_tensor(ctx, 403, count, rows=n)
    w = random_tensor(ctx, 404, 2 * n).view(2, n, L)
    ta, tb, tab, kept, opened, ss = (random_tensor(ctx, 405 + s, count, rows=2) for s in range(6))
    ops = [x, na, nb, y, w, ta, tb, tab, kept, opened, ss]
    copies = [t.clone() for t in ops]
    cst = 3 << 15

    def run():
        nm, kp = fs.sqrt_norm_mask(ctx, x, y, w, ta[:1], tb[:1])
        fm, h = fs.sqrt_first(ctx, opened, ta[:1], tb[:1], tab[:1], (na, nb), k)
        gm, gh = fs.sqrt_trunc_step(ctx, GH, opened, ss, m, ta[:1], tb[:1])
        g1, gh1 = fs.sqrt_trunc_step(ctx, GH, opened[:1], ss[:1], m, ta[:1], tb[:1], kept=h)
        rm = fs.sqrt_trunc_step(ctx, R, opened[:1], ss[:1], m, ta, tb, kept=gh, which=BOTH, cst=cst)
        om = fs.sqrt_trunc_step(ctx, OUT, opened, ss, m, ta, tb, kept=kp[1:], which=BOTH)
        return [nm, kp, fm, h, gm, gh, g1, gh1, rm, om]

    first = run()
    om = first[-1]
    assert torch.equal(sa.sub(ctx, sa.add(ctx, om[0], om[0]), om[0]), om[0])      # consumed on the current stream without a synchronise
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        second = run()
    side.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    nm, kp, fm, h, gm, gh, g1, gh1, rm, om = first
    # out given: written where asked, and handed back
    b0, b1 = torch.empty_like(nm), torch.empty_like(kp)
    got = fs.sqrt_norm_mask(ctx, x, y, w, ta[:1], tb[:1], out=b0, kept_out=b1)
    assert got[0].data_ptr() == b0.data_ptr() and got[1].data_ptr() == b1.data_ptr() and torch.equal(b0, nm) and torch.equal(b1, kp)
    f0, f1 = torch.empty_like(fm), torch.empty_like(h)
    got = fs.sqrt_first(ctx, opened, ta[:1], tb[:1], tab[:1], (na, nb), k, out=(f0, f1))
    assert got[0].data_ptr() == f0.data_ptr() and got[1].data_ptr() == f1.data_ptr() and torch.equal(f0, fm) and torch.equal(f1, h)
    g0b, g1b = torch.empty_like(gm), torch.empty_like(gh)
    got = fs.sqrt_trunc_step(ctx, GH, opened, ss, m, ta[:1], tb[:1], out=(g0b, g1b))
    assert got[0].data_ptr() == g0b.data_ptr() and got[1].data_ptr() == g1b.data_ptr() and torch.equal(g0b, gm) and torch.equal(g1b, gh)
    rb = torch.empty_like(rm)
    assert fs.sqrt_trunc_step(ctx, R, opened[:1], ss[:1], m, ta, tb, kept=gh, which=BOTH, cst=cst, out=rb).data_ptr() == rb.data_ptr() and torch.equal(rb, rm)
    assert all(torch.equal(t, cp) for t, cp in zip(ops, copies))
    # argument checks raise before C and nothing is launched: the buffers keep their contents
    rb.fill_(7)
    bad_calls = [
        lambda: fs.sqrt_norm_mask(ctx, x, y, w[:, :-1], ta[:1], tb[:1]),
        lambda: fs.sqrt_norm_mask(ctx, x, y, w, ta, tb),
        lambda: fs.sqrt_norm_mask(ctx, x[:-1], y, w, ta[:1], tb[:1]),
        lambda: fs.sqrt_norm_mask(ctx, x, y, w, ta[:1], tb[:1], out=b0[:-1]),
        lambda: fs.sqrt_first(ctx, opened[:1], ta[:1], tb[:1], tab[:1], (na, nb), k),
        lambda: fs.sqrt_first(ctx, opened, ta, tb, tab, (na, nb), k),
        lambda: fs.sqrt_first(ctx, opened, ta[:1], tb[:1], tab[:1], (na,), k),
        lambda: fs.sqrt_first(ctx, opened, ta[:1], tb[:1], tab[:1], (na, nb), 300),
        lambda: fs.sqrt_trunc_step(ctx, 3, opened, ss, m, ta[:1], tb[:1]),
        lambda: fs.sqrt_trunc_step(ctx, GH, opened, ss, 0, ta[:1], tb[:1]),
        lambda: fs.sqrt_trunc_step(ctx, GH, opened, ss, 254, ta[:1], tb[:1]),
        lambda: fs.sqrt_trunc_step(ctx, GH, opened, ss, m, ta, tb),
        lambda: fs.sqrt_trunc_step(ctx, R, opened, ss, m, ta, tb, kept=gh, which=BOTH, cst=cst),
        lambda: fs.sqrt_trunc_step(ctx, R, opened[:1], ss[:1], m, ta, tb, kept=gh, which=SQRT, cst=cst),
        lambda: fs.sqrt_trunc_step(ctx, R, opened[:1], ss[:1], m, ta, tb, kept=gh, which=7, cst=cst),
        lambda: fs.sqrt_trunc_step(ctx, R, opened[:1], ss[:1], m, ta, tb, kept=gh[:1], which=BOTH, cst=cst),
        lambda: fs.sqrt_trunc_step(ctx, R, opened[:1], ss[:1], m, ta, tb, kept=gh, which=BOTH, cst=cst, out=rb[:-1]),
        lambda: fs.sqrt_trunc_step(ctx, OUT, opened, ss, m, ta, tb, kept=kp[1:], which=SQRT),
        lambda: fs.sqrt_trunc_step(ctx, OUT, opened[:1], ss[:1], m, ta[:1], tb[:1], kept=kp[1:2], which=BOTH),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"bad call {i} was accepted")
    with pytest.raises(TypeError):
        fs.sqrt_trunc_step(ctx, GH, opened[:1], ss[:1], m, ta[:1], tb[:1])          # one row needs the kept h
    # an output laid over an input is refused by the C ABI, through Python too
    buf = random_tensor(ctx, 420, count, rows=8)
    for call in (lambda: fs.sqrt_norm_mask(ctx, x, y, w, buf[:1], tb[:1], out=buf[:2]),
                 lambda: fs.sqrt_norm_mask(ctx, x, y, w, ta[:1], tb[:1], kept_out=y[:3]),
                 lambda: fs.sqrt_norm_mask(ctx, x, y, w, ta[:1], tb[:1], out=buf[:2], kept_out=buf[1:4]),
                 lambda: fs.sqrt_first(ctx, opened, ta[:1], tb[:1], tab[:1], (na, nb), k, out=(opened, f1)),
                 lambda: fs.sqrt_first(ctx, opened, ta[:1], tb[:1], tab[:1], (na, nb), k, out=(f0, na)),
                 lambda: fs.sqrt_trunc_step(ctx, GH, opened, ss, m, ta[:1], tb[:1], out=(ss, g1b)),
                 lambda: fs.sqrt_trunc_step(ctx, GH, opened, ss, m, ta[:1], tb[:1], out=(g0b, g0b)),
                 lambda: fs.sqrt_trunc_step(ctx, R, opened[:1], ss[:1], m, ta, tb, kept=buf[:2], which=BOTH, cst=cst, out=buf[:4]),
                 lambda: fs.sqrt_trunc_step(ctx, OUT, buf[:2], ss, m, ta, tb, kept=kp[1:], which=BOTH, out=buf[:4])):
        with pytest.raises(HbmpcBackendError):
            call()
    # ... and the C ABI itself
    lib, st, P = ctx.lib, ctx.stream(), ctx.ptr
    one_elem = ctx.host_elems([1])
    one = one_elem.ctypes.data
    assert lib.hb_fxsqrt_norm_mask(ctx.h, P(x), P(y), 0, P(w), 1, P(ta), P(tb), P(b0), P(b1), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxsqrt_norm_mask(ctx.h, P(x), P(y), n, P(w), 3, P(ta), P(tb), P(b0), P(b1), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxsqrt_norm_mask(ctx.h, P(x), P(y), n, None, 2, P(ta), P(tb), P(b0), P(b1), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxsqrt_norm_mask(ctx.h, P(x), P(y), n, P(w), 2, P(ta), P(tb), P(y), P(b1), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxsqrt_norm_mask(ctx.h, P(x), P(y), n, P(w), 2, P(ta), P(tb), P(b0), P(b1), -1, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxsqrt_first(ctx.h, P(opened), P(ta), P(tb), P(tab), None, one, P(na), P(nb), P(f0), P(f1), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxsqrt_first(ctx.h, P(opened), P(ta), P(tb), P(tab), one, one, P(na), None, P(f0), P(f1), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxsqrt_first(ctx.h, P(opened), P(ta), P(tb), P(tab), one, one, P(na), P(nb), P(f0), P(tab), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxsqrt_trunc_step(ctx.h, 3, 1, 3, P(opened), P(ss), m, one, None, P(kept), P(ta), P(tb), P(g0b), P(g1b), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxsqrt_trunc_step(ctx.h, GH, 2, 3, P(opened), P(ss), m, None, None, None, P(ta), P(tb), P(g0b), P(g1b), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxsqrt_trunc_step(ctx.h, GH, 2, 3, P(opened), P(ss), m, one, None, None, P(ta), P(tb), P(g0b), None, count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxsqrt_trunc_step(ctx.h, GH, 2, 3, P(opened), P(ss), m, one, None, None, P(ta), P(tb), P(g0b), P(ss), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxsqrt_trunc_step(ctx.h, R, 1, 3, P(opened), P(ss), m, one, None, P(kept), P(ta), P(tb), P(rb), None, count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxsqrt_trunc_step(ctx.h, R, 1, 3, P(opened), P(ss), m, one, one, None, P(ta), P(tb), P(rb), None, count, st) == HB_ERR_BAD_ARG
    assert lib.hb_fxsqrt_trunc_step(ctx.h, OUT, 2, 1, P(opened), P(ss), m, one, None, P(kept), P(ta), P(tb), P(rb), None, count, st) == HB_ERR_BAD_ARG
    # count == 0: a successful call that launches nothing
    assert lib.hb_fxsqrt_norm_mask(ctx.h, P(x), P(y), n, P(w), 2, P(ta), P(tb), P(b0), P(b1), 0, st) == 0
    assert lib.hb_fxsqrt_first(ctx.h, P(opened), P(ta), P(tb), P(tab), one, one, P(na), P(nb), P(f0), P(f1), 0, st) == 0
    assert lib.hb_fxsqrt_trunc_step(ctx.h, R, 1, 3, P(opened), P(ss), m, one, one, P(kept), P(ta), P(tb), P(rb), None, 0, st) == 0
    torch.cuda.synchronize()
    assert bool((rb == 7).all()) and torch.equal(b0, nm) and torch.equal(b1, kp) and torch.equal(f0, fm) and torch.equal(f1, h) and torch.equal(g0b, gm) and torch.equal(g1b, gh)
    assert all(torch.equal(t, cp) for t, cp in zip(ops, copies))


# ---- the protocol, end to end ---------------------------------------------------------------------------------------------------
async def _composed(co, x, bits, triples, f, k, kappa, theta, what):
    """the chain of fixedpoint_sqrt from what the package offered before: share_arithmetic, fixedpoint.trunc_mask / trunc_pr_finish,
    index_select; the same preprocessing in the same order -> the result shares"""
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd.progs import bit_decomposition as bd
    from honeybadgermpc_amd.progs import fixedpoint as fx
    from honeybadgermpc_amd.progs import fixedpoint_division as fd
    from honeybadgermpc_amd.progs import fixedpoint_sqrt as fs

    ctx = co.ctx
    torch = ctx.torch
    lay = fs.sqrt_layout(k, f, kappa, theta, what)
    theta, width = lay["theta"], lay["width"]
    n, nb, res, beta = k - 1, width + kappa, 2 if what == BOTH else 1, 1 << (k - 1)
    count = x.shape[0]
    rows = fd._Rows(bits, triples)
    shifts = iter(fs.sqrt_shifts(k, theta, what))
    row = lambda t, r: t.index_select(0, torch.tensor([r], device=ctx.tdev))[0]

    async def product(u, v):
        a, b, ab = (t[0] for t in rows.take(1))
        opened = await co.open_share_array(torch.cat([sa.sub(ctx, u, a), sa.sub(ctx, v, b)]))
        return sa.beaver_combine(ctx, opened[:count], opened[count:], a, b, ab)

    async def products(pairs):
        """several products in ONE open, as the fused steps have them"""
        t = rows.take(len(pairs))
        opened = await co.open_share_array(torch.cat([m for q, (u, v) in enumerate(pairs) for m in (sa.sub(ctx, u, t[0][q]), sa.sub(ctx, v, t[1][q]))]))
        return [sa.beaver_combine(ctx, opened[2 * q * count:(2 * q + 1) * count], opened[(2 * q + 1) * count:(2 * q + 2) * count], t[0][q], t[1][q], t[2][q]) for q in range(len(pairs))]

    async def truncate(vals):
        ms = [next(shifts) for _ in vals]
        masks = [fx.trunc_mask(ctx, v, rows.planes(nb), width, m, kappa) for v, m in zip(vals, ms)]
        opened = await co.open_share_array(torch.cat([mk for mk, _ in masks]))
        return [fx.trunc_pr_finish(ctx, v, opened[q * count:(q + 1) * count], masks[q][1], m) for q, (v, m) in enumerate(zip(vals, ms))]

    y = await bd.bit_decompose(co, x, rows.planes(k + kappa), rows.take(bd.bit_triples(n)), k, n, kappa)
    await fd._prefix_or_in_place(co, y, rows)
    weights = fs.sqrt_weights(k, f, what)
    weights = weights if what == BOTH else (weights,)
    v, tw = ctx.upload_ints([0] * count), [ctx.upload_ints([0] * count) for _ in weights]
    for i in range(n):
        z = sa.sub(ctx, row(y, i), row(y, i + 1)) if i + 1 < n else row(y, i)
        v = sa.add(ctx, v, sa.mul(ctx, z, 1 << (n - 1 - i)))
        tw = [sa.add(ctx, t, sa.mul(ctx, z, ws[i])) for t, ws in zip(tw, weights)]
    c = await product(x, v)
    h = sa.add(ctx, sa.neg(ctx, sa.mul(ctx, c, fs.Y0_SLOPE)), fs.a_prime(k))
    g, = await truncate([await product(c, h)])
    for i in range(theta):
        t, = await truncate([await product(g, h)])
        r = sa.add(ctx, sa.neg(ctx, t), 3 * beta)
        which = BOTH if i < theta - 1 else what
        new = await truncate(await products(([(g, r)] if which & SQRT else []) + ([(h, r)] if which & RSQRT else [])))
        if which & SQRT:
            g = new[0]
        if which & RSQRT:
            h = new[-1]
    return tuple(await truncate(await products([(u, t) for u, t in zip(([g] if what & SQRT else []) + ([h] if what & RSQRT else []), tw)])))


SMALL = [(8, 4, 8), (16, 8, 8)]
E2E = [(p, shape) for p in bc.GPU_FIELDS for shape in SMALL] + [(BLS, (64, 32, 32))]
E2E_IDS = [f"{bc.GPU_FIELD_IDS[bc.GPU_FIELDS.index(p)]}-k{k}-f{f}" for p, (k, f, kappa) in E2E]


@pytest.mark.parametrize("what", [SQRT, RSQRT, BOTH], ids=["sqrt", "rsqrt", "both"])
@pytest.mark.parametrize("p, shape", E2E, ids=E2E_IDS)
def test_protocol_end_to_end(p, shape, what):
    from honeybadgermpc_amd.progs import fixedpoint as fx
    from honeybadgermpc_amd.progs import fixedpoint_sqrt as fs

    k, f, kappa = shape
    n, t, count = 4, 1, 16
    ctx = gpu_ctx(p)
    torch = ctx.torch
    rnd = random.Random(100 * k + f + what + p % 7)
    bad = set(rnd.sample(range(n), 1))
    honest = [i for i in range(n) if i not in bad]
    lay = fs.sqrt_layout(k, f, kappa, None, what)
    theta, n_planes, n_triples, width = lay["theta"], lay["n_planes"], lay["n_triples"], lay["width"]
    assert theta == fs.sqrt_iterations(k, f) and width + kappa + 1 <= p.bit_length() - 1          # the width fits both field classes at the small shapes
    xs = sc.e2e_inputs(rnd, k, f, count)
    bit_rows = [[rnd.getrandbits(1) for _ in range(count)] for _ in range(n_planes)]
    starts, limits = sc.truncation_planes(lay, kappa), fs.sqrt_shifts(k, theta, what)
    assert len(starts) == len(limits)
    for which in (0, 1, len(starts) - 1):                                  # an all-ones r1 under g0, the first t and the last result, element 1
        for i in range(limits[which]):
            bit_rows[starts[which] + i][1] = 1
    r1s = [[sum(bit_rows[s + i][e] << i for i in range(m)) for s, m in zip(starts, limits)] for e in range(count)]
    bit_rows.append([rnd.randrange(p) for _ in range(count)])              # a canary plane and a canary row: reading either would spoil the results
    ta, tb = ([[rnd.randrange(p) for _ in range(count)] for _ in range(n_triples)] for _ in range(2))
    tab = [[a * b % p for a, b in zip(ra, rb)] for ra, rb in zip(ta, tb)]
    for v in (ta, tb, tab):
        v.append([rnd.randrange(p) for _ in range(count)])
    bits = bc.deal_planes(ctx, rnd, p, n, t, bit_rows)
    trip = [bc.deal_planes(ctx, rnd, p, n, t, v) for v in (ta, tb, tab)]
    vals = bc.deal_planes(ctx, rnd, p, n, t, [xs])
    fn = {SQRT: fs.sqrt, RSQRT: fs.rsqrt, BOTH: fs.sqrt_rsqrt}[what]

    async def body(co, i):
        x = vals[i][0]
        triples = tuple(tr[i] for tr in trip)
        exact_bits, exact_triples = bits[i][:n_planes], tuple(v[:n_triples] for v in triples)
        keep = (vals[i].clone(), bits[i].clone(), [v.clone() for v in triples])
        for short in (lambda: fn(co, x, exact_bits, tuple(v[:n_triples - 1] for v in triples), f, k, kappa),
                      lambda: fn(co, x, exact_bits[:n_planes - 1], exact_triples, f, k, kappa),
                      lambda: fn(co, x, exact_bits, exact_triples, f, k, kappa, theta=0),
                      lambda: fn(co, x, exact_bits, exact_triples, k - 1, k, kappa)):
            with pytest.raises(ValueError):
                await short()
        assert co.batches == 0                                             # refused before anything was opened
        before = co.batches
        fused = await fn(co, x, bits[i], triples, f, k, kappa)
        batches = co.batches - before
        fused = fused if isinstance(fused, tuple) else (fused,)
        exact = await fn(co, x, exact_bits, exact_triples, f, k, kappa, theta)
        exact = exact if isinstance(exact, tuple) else (exact,)
        before = co.batches
        composed = await _composed(co, x, exact_bits, exact_triples, f, k, kappa, theta, what)
        assert co.batches - before == batches                               # the same opens, composed or fused
        assert len(fused) == len(exact) == len(composed) == (2 if what == BOTH else 1)
        assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(fused, exact, composed)), i          # share for share
        opened = [ctx.download_ints(await co.open_share_array(v)) for v in fused]
        assert torch.equal(vals[i], keep[0]) and torch.equal(bits[i], keep[1]) and all(torch.equal(v, w) for v, w in zip(triples, keep[2]))
        return opened, batches

    results = bc.run_parties(p, n, t, bad, rnd, body)
    want = [fs.sqrt_model(xs[e], p, k, f, r1s[e], theta, what) for e in range(count)]
    want = [list(col) for col in zip(*want)] if what == BOTH else [want]
    root, inverse = fs.sqrt_error_bound(k, f, theta, BOTH)
    from math import isqrt
    for q, col in enumerate(want):                                          # the fixed inputs are in range: the model is within the bound
        for e, w in enumerate(col):
            if (what == BOTH and q == 0) or what == SQRT:
                assert abs(w - isqrt(xs[e] << f)) <= root
            elif xs[e]:
                assert abs(w - sc.exact_rsqrt(xs[e], f)) <= inverse
    for i in honest:
        opened, batches = results[i]
        assert opened == want, i
        assert batches == lay["opens"] == fs.sqrt_opens(k, f, theta, what)


def test_fixed_point_array_sqrt_and_rsqrt():
    from honeybadgermpc_amd.progs import fixedpoint as fx
    from honeybadgermpc_amd.progs import fixedpoint_sqrt as fs

    p, (k, f, kappa), n, t, count = BLS, (16, 8, 8), 4, 1, 16
    ctx = gpu_ctx(p)
    rnd = random.Random(168)
    xs = sc.e2e_inputs(rnd, k, f, count)
    lay = fs.sqrt_layout(k, f, kappa, None, SQRT)
    assert (lay["n_planes"], lay["n_triples"]) == (fs.sqrt_planes(k, f, kappa, None, RSQRT), fs.sqrt_triples(k, f, None, RSQRT))
    bit_rows = [[rnd.getrandbits(1) for _ in range(count)] for _ in range(lay["n_planes"])]
    starts, limits = sc.truncation_planes(lay, kappa), fs.sqrt_shifts(k, lay["theta"], SQRT)
    r1s = [[sum(bit_rows[s + i][e] << i for i in range(m)) for s, m in zip(starts, limits)] for e in range(count)]
    ta, tb = ([[rnd.randrange(p) for _ in range(count)] for _ in range(lay["n_triples"])] for _ in range(2))
    tab = [[a * b % p for a, b in zip(ra, rb)] for ra, rb in zip(ta, tb)]
    bits = bc.deal_planes(ctx, rnd, p, n, t, bit_rows)
    trip = [bc.deal_planes(ctx, rnd, p, n, t, v) for v in (ta, tb, tab)]
    vals = bc.deal_planes(ctx, rnd, p, n, t, [xs])

    async def body(co, i):
        arr = fx.FixedPointArray(co, vals[i][0], f, k, kappa)
        triples = tuple(tr[i] for tr in trip)
        out = []
        for res in (await arr.sqrt(bits[i], triples), await arr.rsqrt(bits[i], triples)):
            assert isinstance(res, fx.FixedPointArray) and (res.f, res.k, res.kappa) == (f, k, kappa)
            out.append(ctx.download_ints(await co.open_share_array(res.shares)))
        return out

    for got in bc.run_parties(p, n, t, set(), rnd, body):
        assert got[0] == [fs.sqrt_model(xs[e], p, k, f, r1s[e], None, SQRT) for e in range(count)]
        assert got[1] == [fs.sqrt_model(xs[e], p, k, f, r1s[e], None, RSQRT) for e in range(count)]

"""GPU: honeybadgermpc_amd.progs.fixedpoint_log -- every step of csrc/hb_fxlog.hip bit-equal to its host self-test row (the same row, the
same step function) and to the step composed from share_arithmetic; inputs untouched, out= honoured, overlaps refused, nothing
synchronises; and the whole protocol among n = 4 parties in one process: log2 and log open to exactly log_model for the dealt r1 -- no
tolerance -- and their shares are bit-equal to the same steps composed from share_arithmetic and fixedpoint.trunc_mask /
trunc_pr_finish, in log_opens batches from log_triples triple rows and log_planes bit planes."""
import random

import pytest

import bitdec_cases as bc
import log_cases as lc
from bitdec_cases import COUNTS, gpu_ctx, random_tensor
from conftest import BLS
from log_cases import DEGREES, E, FINISH, FIRST, LEVEL, POLY_MASK

pytestmark = pytest.mark.gpu


# ---- the kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", bc.GPU_FIELDS, ids=bc.GPU_FIELD_IDS)
def test_every_step_equals_its_selftest_row(p):
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd.progs import fixedpoint as fx
    from honeybadgermpc_amd.progs import fixedpoint_log as fl

    ctx = gpu_ctx(p)
    torch = ctx.torch
    L = ctx.n_limbs
    kappa = 8
    same = lambda got, want: torch.equal(got.cpu(), want)
    shifts = (1, 8) + ((64, 127, 140) if p >> 64 else (61,))
    for count in COUNTS:
        compose = count in (1, 257)
        opened, s, ta, tb, powers0 = (random_tensor(ctx, 500 + q + count, count, rows=13) for q in range(5))
        tab, ybig, na, nb, ipart = (random_tensor(ctx, 505 + q + count, count) for q in range(5))
        inputs = [opened, s, ta, tb, powers0, tab, ybig, na, nb, ipart]
        copies = [t.clone() for t in inputs]
        # the first step
        masked, powers = fl.log_first(ctx, opened[:2], ta[:1], tb[:1], tab.view(1, count, L), ybig, (na, nb), 5)
        assert tuple(masked.shape) == (2, count, L) and tuple(powers.shape) == (5, count, L)
        want = lc.selftest_on_tensors(ctx, FIRST, [opened[:2], ta[:1], tb[:1], tab, ybig, na, nb], [], [2, 1], count)
        assert same(masked, want[0]) and same(powers[:1], want[1]), count
        if compose:
            c = sa.beaver_combine(ctx, opened[0], opened[1], ta[0], tb[0], tab)
            t = sa.sub(ctx, sa.mul(ctx, c, 4), sa.mul(ctx, ybig, 3))
            assert torch.equal(powers[0], t) and torch.equal(masked[0], sa.sub(ctx, t, na)) and torch.equal(masked[1], sa.sub(ctx, t, nb))
        # the last step
        for m in shifts:
            out = fl.log_finish(ctx, opened[0], s[:1], m, ipart)
            want = lc.selftest_on_tensors(ctx, FINISH, [opened[:1], s[:1], [pow(2, -m, p)], ipart], [m], [1], count)
            assert tuple(out.shape) == (count, L) and same(out.view(1, count, L), want[0]), (m, count)
            if compose:
                zero = ctx.upload_ints([0] * count)
                assert torch.equal(out, sa.add(ctx, fx.trunc_pr_finish(ctx, s[0], opened[0], zero, m), ipart))
        # a level and the polynomial, at every degree where the closed-form operand rows differ, at every level
        for d in DEGREES:
            coef = random_tensor(ctx, 520 + d, d + 1)
            coef_ints = ctx.download_ints(coef)
            for level in range(1, lc.levels(d) + 1):
                done = len(lc.level_powers(level, d))
                half = 1 << (level - 1)
                for m in shifts if (d, level) in ((13, 3), (5, 1), (13, 4), (3, 2)) else (8,):
                    new = [fx.trunc_pr_finish(ctx, s[q], opened[q], ctx.upload_ints([0] * count), m) for q in range(done)] if compose else None
                    if level < lc.levels(d):
                        nxt = len(lc.level_powers(level + 1, d))
                        pw = powers0[:d].clone()
                        masked = fl.log_level(ctx, level, d, opened[:done], s[:done], m, ta[:nxt], tb[:nxt], pw)
                        assert tuple(masked.shape) == (2 * nxt, count, L)
                        want = lc.selftest_on_tensors(ctx, LEVEL, [opened[:done], s[:done], [pow(2, -m, p)], ta[:nxt], tb[:nxt]], [level, d, m], [2 * nxt, d], count,
                                                      preset={1: powers0[:d]})
                        assert same(masked, want[0]) and same(pw, want[1]), (d, level, m, count)
                        if compose:
                            allp = [powers0[j] for j in range(half)] + new
                            assert all(torch.equal(pw[half + q], new[q]) for q in range(done)) and torch.equal(pw[:half], powers0[:half])
                            assert torch.equal(pw[half + done:], powers0[half + done:d])
                            for q in range(nxt):
                                assert torch.equal(masked[2 * q], sa.sub(ctx, allp[2 * half - 1], ta[q])) and torch.equal(masked[2 * q + 1], sa.sub(ctx, allp[q], tb[q]))
                    else:
                        m_out = m if m + 5 + kappa + 1 <= p.bit_length() - 1 else 8
                        width = m_out + 5
                        planes = ctx.upload_ints([(i * 7 + r * 3 + (i * r) % 5) & 1 for r in range(width + kappa) for i in range(count)]).view(width + kappa, count, L)
                        masked, kept = fl.log_poly_mask(ctx, d, opened[:done], s[:done], m, powers0[:d], ybig, coef, planes, width, m_out, kappa)
                        assert tuple(masked.shape) == (1, count, L) and tuple(kept.shape) == (1, count, L)
                        want = lc.selftest_on_tensors(ctx, POLY_MASK, [opened[:done], s[:done], [pow(2, -m, p)], powers0[:d], ybig, coef, planes],
                                                      [d, m, width, m_out, kappa], [1, 1], count)
                        assert same(masked, want[0]) and same(kept, want[1]), (d, m, count)
                        if compose:
                            allp = [powers0[j] for j in range(half)] + new
                            poly = sa.mul(ctx, ybig, coef_ints[0])
                            for j in range(1, d + 1):
                                poly = sa.add(ctx, poly, sa.mul(ctx, allp[j - 1], coef_ints[j]))
                            mk, r1 = fx.trunc_mask(ctx, poly, planes, width, m_out, kappa)
                            assert torch.equal(masked[0], mk) and torch.equal(kept[0], sa.add(ctx, poly, r1)), (d, m, count)
        assert all(torch.equal(t, cp) for t, cp in zip(inputs, copies))


def test_inputs_untouched_out_honoured_overlap_refused_and_asynchronous():
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd._capi import HB_ERR_BAD_ARG, HbmpcBackendError
    from honeybadgermpc_amd.progs import fixedpoint_log as fl

    p, count, d, m, kappa, width = BLS, 600, 5, 8, 8, 24
    ctx = gpu_ctx(p)
    torch = ctx.torch
    L = ctx.n_limbs
    opened, s, ta, tb, tab, pw0 = (random_tensor(ctx, 600 + q, count, rows=5) for q in range(6))
    ybig, na, nb, ipart = (random_tensor(ctx, 610 + q, count) for q in range(4))
    coef = random_tensor(ctx, 620, d + 1)
    planes = ctx.upload_ints([(i + r) & 1 for r in range(width + kappa) for i in range(count)]).view(width + kappa, count, L)
    ops = [opened, s, ta, tb, tab, pw0, ybig, na, nb, ipart, coef, planes]
    copies = [t.clone() for t in ops]

    def run():
        fm, pw = fl.log_first(ctx, opened[:2], ta[:1], tb[:1], tab[:1], ybig, (na, nb), d)
        pw1 = pw0.clone()
        lm = fl.log_level(ctx, 1, d, opened[:1], s[:1], m, ta[:2], tb[:2], pw1)
        pw2 = pw0.clone()
        l2 = fl.log_level(ctx, 2, d, opened[:2], s[:2], m, ta[:1], tb[:1], pw2)
        pm, ks = fl.log_poly_mask(ctx, d, opened[:1], s[:1], m, pw0, ybig, coef, planes, width, m, kappa)
        out = fl.log_finish(ctx, opened[0], s[:1], m, ipart)
        return [fm, pw[:1], lm, pw1, l2, pw2, pm, ks, out]

    first = run()
    out = first[-1]
    assert torch.equal(sa.sub(ctx, sa.add(ctx, out, out), out), out)               # consumed on the current stream without a synchronise
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        second = run()
    side.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    fm, pwr, lm, pw1, l2, pw2, pm, ks, out = first
    # out given: written where asked, and handed back
    b0, b1 = torch.empty_like(fm), torch.empty((d, count, L), dtype=torch.int64, device=fm.device)
    got = fl.log_first(ctx, opened[:2], ta[:1], tb[:1], tab[:1], ybig, (na, nb), d, out=(b0, b1))
    assert got[0].data_ptr() == b0.data_ptr() and got[1].data_ptr() == b1.data_ptr() and torch.equal(b0, fm) and torch.equal(b1[:1], pwr)
    lb, pwb = torch.empty_like(lm), pw0.clone()
    assert fl.log_level(ctx, 1, d, opened[:1], s[:1], m, ta[:2], tb[:2], pwb, out=lb).data_ptr() == lb.data_ptr() and torch.equal(lb, lm) and torch.equal(pwb, pw1)
    p0, p1 = torch.empty_like(pm), torch.empty_like(ks)
    got = fl.log_poly_mask(ctx, d, opened[:1], s[:1], m, pw0, ybig, coef, planes, width, m, kappa, out=(p0, p1))
    assert got[0].data_ptr() == p0.data_ptr() and got[1].data_ptr() == p1.data_ptr() and torch.equal(p0, pm) and torch.equal(p1, ks)
    ob = torch.empty_like(out)
    assert fl.log_finish(ctx, opened[0], s[:1], m, ipart, out=ob).data_ptr() == ob.data_ptr() and torch.equal(ob, out)
    assert all(torch.equal(t, cp) for t, cp in zip(ops, copies))
    # argument checks raise before C and nothing is launched: the buffers keep their contents
    ob.fill_(7)
    bad_calls = [
        lambda: fl.log_first(ctx, opened[:1], ta[:1], tb[:1], tab[:1], ybig, (na, nb), d),
        lambda: fl.log_first(ctx, opened[:2], ta[:2], tb[:2], tab[:2], ybig, (na, nb), d),
        lambda: fl.log_first(ctx, opened[:2], ta[:1], tb[:1], tab[:1], ybig, (na,), d),
        lambda: fl.log_first(ctx, opened[:2], ta[:1], tb[:1], tab[:1], ybig, (na, nb), 1),
        lambda: fl.log_first(ctx, opened[:2], ta[:1], tb[:1], tab[:1], ybig[:-1], (na, nb), d),
        lambda: fl.log_level(ctx, 0, d, opened[:1], s[:1], m, ta[:2], tb[:2], pwb),
        lambda: fl.log_level(ctx, 3, d, opened[:1], s[:1], m, ta[:1], tb[:1], pwb),
        lambda: fl.log_level(ctx, 1, 2, opened[:1], s[:1], m, ta[:1], tb[:1], pwb),
        lambda: fl.log_level(ctx, 1, d, opened[:1], s[:1], 0, ta[:2], tb[:2], pwb),
        lambda: fl.log_level(ctx, 1, d, opened[:1], s[:1], 254, ta[:2], tb[:2], pwb),
        lambda: fl.log_level(ctx, 1, d, opened[:2], s[:2], m, ta[:2], tb[:2], pwb),
        lambda: fl.log_level(ctx, 1, d, opened[:1], s[:1], m, ta[:1], tb[:1], pwb),
        lambda: fl.log_level(ctx, 1, d, opened[:1], s[:1], m, ta[:2], tb[:2], pwb[:4]),
        lambda: fl.log_poly_mask(ctx, 1, opened[:1], s[:1], m, pw0, ybig, coef, planes, width, m, kappa),
        lambda: fl.log_poly_mask(ctx, d, opened[:2], s[:2], m, pw0, ybig, coef, planes, width, m, kappa),
        lambda: fl.log_poly_mask(ctx, d, opened[:1], s[:1], m, pw0[:4], ybig, coef, planes, width, m, kappa),
        lambda: fl.log_poly_mask(ctx, d, opened[:1], s[:1], m, pw0, ybig, coef[:d], planes, width, m, kappa),
        lambda: fl.log_poly_mask(ctx, d, opened[:1], s[:1], m, pw0, ybig, coef, planes[:-1], width, m, kappa),
        lambda: fl.log_poly_mask(ctx, d, opened[:1], s[:1], m, pw0, ybig, coef, planes, width, width, kappa),
        lambda: fl.log_poly_mask(ctx, d, opened[:1], s[:1], m, pw0, ybig, coef, planes, 250, m, kappa),
        lambda: fl.log_finish(ctx, opened[0], s[:1], 0, ipart),
        lambda: fl.log_finish(ctx, opened[0], s[:2], m, ipart),
        lambda: fl.log_finish(ctx, opened[0], s[:1], m, ipart, out=ob[:-1]),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"bad call {i} was accepted")
    # an output laid over an input is refused by the C ABI, through Python too
    buf = random_tensor(ctx, 630, count, rows=8)
    for call in (lambda: fl.log_first(ctx, opened[:2], ta[:1], tb[:1], tab[:1], ybig, (na, nb), d, out=(opened[:2], b1)),
                 lambda: fl.log_first(ctx, opened[:2], ta[:1], tb[:1], tab[:1], buf[0], (na, nb), d, out=(b0, buf[:5])),
                 lambda: fl.log_first(ctx, opened[:2], ta[:1], tb[:1], tab[:1], ybig, (na, nb), d, out=(buf[:2], buf[1:6])),
                 lambda: fl.log_level(ctx, 1, d, opened[:1], s[:1], m, ta[:2], tb[:2], pwb, out=pwb[:4]),
                 lambda: fl.log_level(ctx, 1, d, buf[:1], s[:1], m, ta[:2], tb[:2], pwb, out=buf[:4]),
                 lambda: fl.log_level(ctx, 1, d, opened[:1], s[:1], m, buf[:2], tb[:2], buf[1:6]),
                 lambda: fl.log_poly_mask(ctx, d, opened[:1], s[:1], m, pw0, ybig, coef, planes, width, m, kappa, out=(pw0[:1], p1)),
                 lambda: fl.log_poly_mask(ctx, d, opened[:1], s[:1], m, pw0, ybig, coef, planes, width, m, kappa, out=(p0, planes[3:4])),
                 lambda: fl.log_poly_mask(ctx, d, opened[:1], s[:1], m, pw0, ybig, coef, planes, width, m, kappa, out=(p0, p0)),
                 lambda: fl.log_finish(ctx, opened[0], s[:1], m, ipart, out=ipart),
                 lambda: fl.log_finish(ctx, opened[0], s[:1], m, ipart, out=s[0])):
        with pytest.raises(HbmpcBackendError):
            call()
    # ... and the C ABI itself
    lib, st, P = ctx.lib, ctx.stream(), ctx.ptr
    one_elem = ctx.host_elems([1])
    one = one_elem.ctypes.data
    A = HB_ERR_BAD_ARG
    assert lib.hb_fxlog_first(ctx.h, P(opened), P(ta), P(tb), P(tab), None, P(na), P(nb), P(b0), P(b1), count, st) == A
    assert lib.hb_fxlog_first(ctx.h, P(opened), P(ta), P(tb), P(tab), P(ybig), P(na), P(nb), P(b0), P(ybig), count, st) == A
    assert lib.hb_fxlog_first(ctx.h, P(opened), P(ta), P(tb), P(tab), P(ybig), P(na), P(nb), P(b0), P(b1), -1, st) == A
    assert lib.hb_fxlog_level(ctx.h, 1, 1, P(opened), P(s), m, one, P(ta), P(tb), P(lb), P(pwb), count, st) == A
    assert lib.hb_fxlog_level(ctx.h, 1, 65, P(opened), P(s), m, one, P(ta), P(tb), P(lb), P(pwb), count, st) == A
    assert lib.hb_fxlog_level(ctx.h, 3, d, P(opened), P(s), m, one, P(ta), P(tb), P(lb), P(pwb), count, st) == A
    assert lib.hb_fxlog_level(ctx.h, 0, d, P(opened), P(s), m, one, P(ta), P(tb), P(lb), P(pwb), count, st) == A
    assert lib.hb_fxlog_level(ctx.h, 1, d, P(opened), P(s), m, None, P(ta), P(tb), P(lb), P(pwb), count, st) == A
    assert lib.hb_fxlog_level(ctx.h, 1, d, P(opened), P(s), 254, one, P(ta), P(tb), P(lb), P(pwb), count, st) == A
    assert lib.hb_fxlog_level(ctx.h, 1, d, P(opened), P(s), m, one, P(ta), P(tb), P(lb), None, count, st) == A
    assert lib.hb_fxlog_level(ctx.h, 1, d, P(opened), P(s), m, one, P(ta), P(tb), P(ta), P(pwb), count, st) == A
    assert lib.hb_fxlog_poly_mask(ctx.h, 1, P(opened), P(s), m, one, P(pw0), P(ybig), P(coef), P(planes), width, m, kappa, P(p0), P(p1), count, st) == A
    assert lib.hb_fxlog_poly_mask(ctx.h, d, P(opened), P(s), m, one, P(pw0), P(ybig), None, P(planes), width, m, kappa, P(p0), P(p1), count, st) == A
    assert lib.hb_fxlog_poly_mask(ctx.h, d, P(opened), P(s), m, one, P(pw0), P(ybig), P(coef), P(planes), 250, m, kappa, P(p0), P(p1), count, st) == A
    assert lib.hb_fxlog_poly_mask(ctx.h, d, P(opened), P(s), m, one, P(pw0), P(ybig), P(coef), P(planes), width, m, kappa, P(p0), P(coef), count, st) == A
    assert lib.hb_fxlog_finish(ctx.h, P(opened), P(s), 0, one, P(ipart), P(ob), count, st) == A
    assert lib.hb_fxlog_finish(ctx.h, P(opened), P(s), m, None, P(ipart), P(ob), count, st) == A
    assert lib.hb_fxlog_finish(ctx.h, P(opened), P(s), m, one, P(ipart), P(s), count, st) == A
    # count == 0: a successful call that launches nothing
    assert lib.hb_fxlog_first(ctx.h, P(opened), P(ta), P(tb), P(tab), P(ybig), P(na), P(nb), P(b0), P(b1), 0, st) == 0
    assert lib.hb_fxlog_level(ctx.h, 1, d, P(opened), P(s), m, one, P(ta), P(tb), P(lb), P(pwb), 0, st) == 0
    assert lib.hb_fxlog_poly_mask(ctx.h, d, P(opened), P(s), m, one, P(pw0), P(ybig), P(coef), P(planes), width, m, kappa, P(p0), P(p1), 0, st) == 0
    assert lib.hb_fxlog_finish(ctx.h, P(opened), P(s), m, one, P(ipart), P(ob), 0, st) == 0
    torch.cuda.synchronize()
    assert bool((ob == 7).all()) and torch.equal(b0, fm) and torch.equal(lb, lm) and torch.equal(pwb, pw1) and torch.equal(p0, pm) and torch.equal(p1, ks)
    assert all(torch.equal(t, cp) for t, cp in zip(ops, copies))


# ---- the protocol, end to end ---------------------------------------------------------------------------------------------------
async def _composed(co, x, bits, triples, f, k, kappa, base):
    """the chain of fixedpoint_log from what the package offered before: bit_decompose, _prefix_or_in_place, share_arithmetic,
    fixedpoint.trunc_mask / trunc_pr_finish; the same preprocessing in the same order -> the result shares"""
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd.progs import bit_decomposition as bd
    from honeybadgermpc_amd.progs import fixedpoint as fx
    from honeybadgermpc_amd.progs import fixedpoint_division as fd
    from honeybadgermpc_amd.progs import fixedpoint_log as fl

    ctx = co.ctx
    torch = ctx.torch
    lay = fl.log_layout(k, f, kappa, None, base)
    d, width = lay["degree"], lay["width"]
    n, nb, p = k - 1, width + kappa, ctx.modulus
    count = x.shape[0]
    rows = fd._Rows(bits, triples)
    shifts = iter(fl.log_shifts(k, f, None, base))

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
    weights = fl.log_weights(k, f, base)[0]
    v, ipart = ctx.upload_ints([0] * count), ctx.upload_ints([0] * count)
    for i in range(n):
        z = sa.sub(ctx, y[i], y[i + 1]) if i + 1 < n else y[i]
        v = sa.add(ctx, v, sa.mul(ctx, z, 1 << (n - 1 - i)))
        ipart = sa.add(ctx, ipart, sa.mul(ctx, z, weights[i] % p))
    big = sa.mul(ctx, y[0], 1 << n)
    c, = await products([(x, v)])
    powers = {1: sa.sub(ctx, sa.mul(ctx, c, 4), sa.mul(ctx, big, 3))}
    for level in range(1, lay["levels"] + 1):
        half = 1 << (level - 1)
        js = lc.level_powers(level, d)
        for j, t in zip(js, await truncate(await products([(powers[half], powers[j - half]) for j in js]))):
            powers[j] = t
    coef = fl.log_coefficients(k, f, base)
    poly = sa.mul(ctx, big, coef[0] % p)
    for j in range(1, d + 1):
        poly = sa.add(ctx, poly, sa.mul(ctx, powers[j], coef[j] % p))
    t, = await truncate([poly])
    return sa.add(ctx, t, ipart)


SMALL = [(8, 4, 8), (16, 8, 8)]
E2E = [(p, shape) for p in (BLS, bc.P64) for shape in SMALL] + [(BLS, (64, 32, 32))]
E2E_IDS = [f"{'bls' if p == BLS else '2^64-59'}-k{k}-f{f}" for p, (k, f, kappa) in E2E]


@pytest.mark.parametrize("base", [2, E], ids=["log2", "log"])
@pytest.mark.parametrize("p, shape", E2E, ids=E2E_IDS)
def test_protocol_end_to_end(p, shape, base):
    from honeybadgermpc_amd.progs import fixedpoint_log as fl

    k, f, kappa = shape
    n, t = 4, 1
    ctx = gpu_ctx(p)
    torch = ctx.torch
    rnd = random.Random(100 * k + f + (base == E) + p % 7)
    xs = lc.e2e_inputs(rnd, k, f, 16)
    count = len(xs)                                                        # 16, and 37 at k = 64: a power of two at every second bit
    bad = set(rnd.sample(range(n), 1))
    honest = [i for i in range(n) if i not in bad]
    lay = fl.log_layout(k, f, kappa, None, base)
    d, n_planes, n_triples, width = lay["degree"], lay["n_planes"], lay["n_triples"], lay["width"]
    assert d == fl.log_degree(k, f, base) and width + kappa + 1 <= p.bit_length() - 1          # the width fits both field classes at the small shapes
    assert count == (16 if k < 64 else 37) and xs[0] == 0 and xs[1] == 1 and all(1 << i in xs for i in range(1, k - 1, 2))
    bit_rows = [[rnd.getrandbits(1) for _ in range(count)] for _ in range(n_planes)]
    starts, limits = lc.truncation_planes(lay, kappa), fl.log_shifts(k, f, None, base)
    assert len(starts) == len(limits) == d
    for which in (0, d // 2, d - 1):                                       # an all-ones r1 under the first, one middle and the last truncation, element 1
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
    fn = fl.log2 if base == 2 else fl.log

    async def body(co, i):
        x = vals[i][0]
        triples = tuple(tr[i] for tr in trip)
        exact_bits, exact_triples = bits[i][:n_planes], tuple(v[:n_triples] for v in triples)
        keep = (vals[i].clone(), bits[i].clone(), [v.clone() for v in triples])
        for short in (lambda: fn(co, x, exact_bits, tuple(v[:n_triples - 1] for v in triples), f, k, kappa),
                      lambda: fn(co, x, exact_bits[:n_planes - 1], exact_triples, f, k, kappa),
                      lambda: fn(co, x, exact_bits, exact_triples, k - 1, k, kappa),
                      lambda: fn(co, x, exact_bits, exact_triples, f, k, 250)):
            with pytest.raises(ValueError):
                await short()
        assert co.batches == 0                                             # refused before anything was opened
        before = co.batches
        fused = await fn(co, x, bits[i], triples, f, k, kappa)
        batches = co.batches - before
        exact = await fl.log_base(co, x, exact_bits, exact_triples, f, k, kappa, base)
        before = co.batches
        composed = await _composed(co, x, exact_bits, exact_triples, f, k, kappa, base)
        assert co.batches - before == batches                               # the same opens, composed or fused
        assert torch.equal(fused, exact) and torch.equal(fused, composed), i          # share for share
        opened = ctx.download_ints(await co.open_share_array(fused))
        assert torch.equal(vals[i], keep[0]) and torch.equal(bits[i], keep[1]) and all(torch.equal(v, w) for v, w in zip(triples, keep[2]))
        return opened, batches

    results = bc.run_parties(p, n, t, bad, rnd, body)
    want = [fl.log_model(xs[e], p, k, f, r1s[e], base) for e in range(count)]
    bound = fl.log_error_bound(k, f, None, base)
    assert want[0] == 0                                                     # x = 0: nothing raised, and what log_model gives
    for e, w in enumerate(want):                                            # the fixed inputs are in range: the model is within the bound
        if xs[e]:
            assert lc.distance(lc.centered(w, p), lc.log_enclosure(xs[e], f, base)) <= bound, (xs[e], w)
    for i in honest:
        opened, batches = results[i]
        assert opened == want, i
        assert batches == lay["opens"] == fl.log_opens(k, f, None, base)


def test_fixed_point_array_log2_and_log():
    from honeybadgermpc_amd.progs import fixedpoint as fx
    from honeybadgermpc_amd.progs import fixedpoint_log as fl

    p, (k, f, kappa), n, t, count = BLS, (16, 8, 8), 4, 1, 16
    ctx = gpu_ctx(p)
    rnd = random.Random(169)
    xs = lc.e2e_inputs(rnd, k, f, count)
    assert len(xs) == count
    lay = fl.log_layout(k, f, kappa, None, 2)
    assert (lay["n_planes"], lay["n_triples"]) == (fl.log_planes(k, f, kappa, None, E), fl.log_triples(k, f, None, E))
    bit_rows = [[rnd.getrandbits(1) for _ in range(count)] for _ in range(lay["n_planes"])]
    starts, limits = lc.truncation_planes(lay, kappa), fl.log_shifts(k, f)
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
        for res in (await arr.log2(bits[i], triples), await arr.log(bits[i], triples)):
            assert isinstance(res, fx.FixedPointArray) and (res.f, res.k, res.kappa) == (f, k, kappa)
            out.append(ctx.download_ints(await co.open_share_array(res.shares)))
        return out

    for got in bc.run_parties(p, n, t, set(), rnd, body):
        assert got[0] == [fl.log_model(xs[e], p, k, f, r1s[e], 2) for e in range(count)]
        assert got[1] == [fl.log_model(xs[e], p, k, f, r1s[e], E) for e in range(count)]

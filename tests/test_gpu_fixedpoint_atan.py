"""GPU: honeybadgermpc_amd.progs.fixedpoint_atan -- every step of csrc/hb_fxatan.hip bit-equal to its host self-test row (the same row, the
same step function) and to the step composed from share_arithmetic and fixedpoint.trunc_mask / trunc_pr_finish; inputs untouched, out=
honoured, overlaps refused, nothing synchronises; the whole protocol among n = 4 parties in one process: atan2 opens to exactly
atan2_model for the dealt r1 -- no tolerance --, in atan2_opens batches, share for share what the composed protocol gives;
FixedPointArray.atan2 / .atan; and one round trip through sincos_turns."""
import random
from fractions import Fraction
from math import isqrt

import pytest

import atan_cases as ac
import bitdec_cases as bc
from atan_cases import ABS, ASSEMBLE, DEGREES, FINISH, FIRST, LEVEL, POLY_MASK, SELECT, SELECT_MASK, SIGN_MASK
from bitdec_cases import COUNTS, gpu_ctx, random_tensor
from conftest import BLS

pytestmark = pytest.mark.gpu


def _sigma(ctx, sa, b):
    """1 - 2 b"""
    return sa.add(ctx, sa.neg(ctx, sa.mul(ctx, b, 2)), 1)


# ---- the kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", bc.GPU_FIELDS, ids=bc.GPU_FIELD_IDS)
def test_every_step_equals_its_selftest_row(p):
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd.progs import fixedpoint as fx
    from honeybadgermpc_amd.progs import fixedpoint_atan as fa

    ctx = gpu_ctx(p)
    torch = ctx.torch
    L = ctx.n_limbs
    k, kappa = 16, 8
    same = lambda got, want: torch.equal(got.cpu(), want)
    shifts = (1, 8) + ((64, 127, 140) if p >> 64 else (61,))
    consts = [p - 3, (p + 1) // 2]
    for count in COUNTS:
        compose = count in (1, 257)
        zero = ctx.upload_ints([0] * count)
        opened, s, ta, tb, tab, powers0 = (random_tensor(ctx, 700 + q + count, count, rows=12) for q in range(6))
        x, y, c, w, g = (random_tensor(ctx, 710 + q + count, count) for q in range(5))
        bits = ctx.upload_ints([(i * 5 + r * 3 + (i * r) % 7) & 1 for r in range(k + kappa) for i in range(count)]).view(k + kappa, count, L)
        inputs = [opened, s, ta, tb, tab, powers0, x, y, c, w, g, bits]
        copies = [t.clone() for t in inputs]
        s2, sx, sy = s[:2].reshape(2 * count, L), s[0], s[1]
        # the masks of the abs and of the select step
        masked = fa.sign_mask(ctx, s2, x, y, ta[:3], tb[:3])
        assert tuple(masked.shape) == (6, count, L)
        assert same(masked, ac.selftest_on_tensors(ctx, SIGN_MASK, [s[:2], x, y, ta[:3], tb[:3]], [], [6], count)[0]), count
        if compose:
            for r, (u, v) in enumerate([(sx, x), (sy, y), (_sigma(ctx, sa, sy), sx)]):
                assert torch.equal(masked[2 * r], sa.sub(ctx, u, ta[r])) and torch.equal(masked[2 * r + 1], sa.sub(ctx, v, tb[r])), r
        masked = fa.select_mask(ctx, c, w, sx, ta[:2], tb[:2])
        assert tuple(masked.shape) == (4, count, L)
        assert same(masked, ac.selftest_on_tensors(ctx, SELECT_MASK, [c, w, sx, ta[:2], tb[:2]], [], [4], count)[0]), count
        if compose:
            for r, (u, v) in enumerate([(c, w), (_sigma(ctx, sa, c), _sigma(ctx, sa, sx))]):
                assert torch.equal(masked[2 * r], sa.sub(ctx, u, ta[r])) and torch.equal(masked[2 * r + 1], sa.sub(ctx, v, tb[r])), r
        # the abs step
        masked, kept = fa.abs_step(ctx, opened[:6], ta[:3], tb[:3], tab[:3], x, y, bits, k, kappa)
        assert tuple(masked.shape) == (1, count, L) and tuple(kept.shape) == (5, count, L)
        want = ac.selftest_on_tensors(ctx, ABS, [opened[:6], ta[:3], tb[:3], tab[:3], x, y, bits], [k, kappa], [1, 5], count)
        assert same(masked, want[0]) and same(kept, want[1]), count
        if compose:
            pr = [sa.beaver_combine(ctx, opened[2 * r], opened[2 * r + 1], ta[r], tb[r], tab[r]) for r in range(3)]
            ax, ay = sa.sub(ctx, x, sa.mul(ctx, pr[0], 2)), sa.sub(ctx, y, sa.mul(ctx, pr[1], 2))
            ww = sa.sub(ctx, ax, ay)
            mk, r1 = fx.trunc_mask(ctx, ww, bits, k, k - 1, kappa)
            assert all(torch.equal(a, b) for a, b in zip(kept, (ax, ay, pr[2], ww, r1))) and torch.equal(masked[0], mk)
        # the select step and the finish
        out = fa.select(ctx, opened[:4], ta[:2], tb[:2], tab[:2], x, y)
        assert tuple(out.shape) == (3, count, L)
        assert same(out, ac.selftest_on_tensors(ctx, SELECT, [opened[:4], ta[:2], tb[:2], tab[:2], x, y], [], [3], count)[0]), count
        if compose:
            pr = [sa.beaver_combine(ctx, opened[2 * r], opened[2 * r + 1], ta[r], tb[r], tab[r]) for r in range(2)]
            assert torch.equal(out[0], sa.add(ctx, y, pr[0])) and torch.equal(out[1], sa.sub(ctx, x, pr[0])) and torch.equal(out[2], pr[1])
        out = fa.atan_finish(ctx, opened[:2], ta[0], tb[0], tab[0], c)
        assert tuple(out.shape) == (count, L)
        assert same(out.view(1, count, L), ac.selftest_on_tensors(ctx, FINISH, [opened[:2], ta[:1], tb[:1], tab[:1], c], [], [1], count)[0]), count
        if compose:
            assert torch.equal(out, sa.add(ctx, c, sa.beaver_combine(ctx, opened[0], opened[1], ta[0], tb[0], tab[0])))
        # the ladder's first step
        for shift in (0, 7, 31) + ((140,) if p >> 64 else ()):
            masked, powers = fa.atan_first(ctx, x, shift, sy, g, ta[:2], tb[:2], 7)
            assert tuple(masked.shape) == (4, count, L) and tuple(powers.shape) == (4, count, L)
            want = ac.selftest_on_tensors(ctx, FIRST, [x, sy, g, ta[:2], tb[:2]], [shift], [4, 1], count)
            assert same(masked, want[0]) and same(powers[:1], want[1]), (shift, count)
            if compose:
                t = sa.mul(ctx, x, pow(2, shift, p))
                rows = [sa.sub(ctx, t, ta[0]), sa.sub(ctx, t, tb[0]), sa.sub(ctx, _sigma(ctx, sa, sy), ta[1]), sa.sub(ctx, g, tb[1])]
                assert torch.equal(powers[0], t) and all(torch.equal(a, b) for a, b in zip(masked, rows)), shift
        # the assemble step
        for m in shifts:
            masked, cst = fa.atan_assemble(ctx, opened[0], s[:1], m, opened[2:4], ta[1], tb[1], tab[1], sy, g, consts, ta[2], tb[2])
            assert tuple(masked.shape) == (2, count, L) and tuple(cst.shape) == (count, L)
            want = ac.selftest_on_tensors(ctx, ASSEMBLE, [opened[:1], s[:1], [pow(2, -m, p)], opened[2:4], ta[1:2], tb[1:2], tab[1:2], sy, g, consts, ta[2:3], tb[2:3]], [m],
                                          [2, 1], count)
            assert same(masked, want[0]) and same(cst.view(1, count, L), want[1]), (m, count)
            if compose:
                a = fx.trunc_pr_finish(ctx, s[0], opened[0], zero, m)
                e = sa.beaver_combine(ctx, opened[2], opened[3], ta[1], tb[1], tab[1])
                cc = sa.add(ctx, sa.mul(ctx, g, consts[0]), sa.mul(ctx, sa.sub(ctx, _sigma(ctx, sa, sy), e), consts[1]))
                assert torch.equal(masked[0], sa.sub(ctx, e, ta[2])) and torch.equal(masked[1], sa.sub(ctx, a, tb[2])) and torch.equal(cst, cc), m
        # a level and the polynomial, at every degree, at every level
        for d in DEGREES:
            rows = (d + 1) // 2
            coef = random_tensor(ctx, 720 + d, rows)
            coef_ints = ctx.download_ints(coef)
            for level in range(ac.levels(d) + 1):
                done = ac.level_products(level, d)
                half = 1 << (level - 1) if level else 0
                for m in shifts if (d, level) in ((13, 2), (5, 0), (23, 3), (23, 4), (3, 1)) else (8,):
                    new = [fx.trunc_pr_finish(ctx, s[q], opened[q], zero, m) for q in range(done)] if compose else None
                    if level < ac.levels(d):
                        nxt, odd = ac.level_products(level + 1, d), len(ac.level_odd(level + 1, d))
                        pw = powers0[:rows].clone()
                        masked = fa.atan_level(ctx, level, d, opened[:done], s[:done], m, ta[:nxt], tb[:nxt], pw)
                        assert tuple(masked.shape) == (2 * nxt, count, L)
                        want = ac.selftest_on_tensors(ctx, LEVEL, [opened[:done], s[:done], [pow(2, -m, p)], ta[:nxt], tb[:nxt]], [level, d, m], [2 * nxt, rows], count,
                                                      preset={1: powers0[:rows]})
                        assert same(masked, want[0]) and same(pw, want[1]), (d, level, m, count)
                        if compose:
                            allp = [powers0[j] for j in range(max(half, 1))] + new[:done - 1]
                            square = new[done - 1]
                            assert all(torch.equal(pw[half + q], new[q]) for q in range(done - 1)) and torch.equal(pw[:max(half, 1)], powers0[:max(half, 1)])
                            assert torch.equal(pw[half + done - 1:] if level else pw[1:], powers0[half + done - 1:rows] if level else powers0[1:rows])
                            for q in range(nxt):
                                first = allp[q] if q < odd else square
                                assert torch.equal(masked[2 * q], sa.sub(ctx, first, ta[q])) and torch.equal(masked[2 * q + 1], sa.sub(ctx, square, tb[q])), (d, level, q)
                    else:
                        m_out = m if m + 5 + kappa + 1 <= p.bit_length() - 1 else 8
                        width = m_out + 5
                        planes = ctx.upload_ints([(i * 7 + r * 3 + (i * r) % 5) & 1 for r in range(width + kappa) for i in range(count)]).view(width + kappa, count, L)
                        masked, kept = fa.atan_poly_mask(ctx, d, opened[:done], s[:done], m, powers0[:rows], coef, planes, width, m_out, kappa)
                        assert tuple(masked.shape) == (1, count, L) and tuple(kept.shape) == (1, count, L)
                        want = ac.selftest_on_tensors(ctx, POLY_MASK, [opened[:done], s[:done], [pow(2, -m, p)], powers0[:rows], coef, planes], [d, m, width, m_out, kappa],
                                                      [1, 1], count)
                        assert same(masked, want[0]) and same(kept, want[1]), (d, m, count)
                        if compose:
                            allp = [powers0[j] for j in range(half)] + new
                            poly = sa.mul(ctx, allp[0], coef_ints[0])
                            for j in range(1, rows):
                                poly = sa.add(ctx, poly, sa.mul(ctx, allp[j], coef_ints[j]))
                            mk, r1 = fx.trunc_mask(ctx, poly, planes, width, m_out, kappa)
                            assert torch.equal(masked[0], mk) and torch.equal(kept[0], sa.add(ctx, poly, r1)), (d, m, count)
        assert all(torch.equal(t, cp) for t, cp in zip(inputs, copies))


def test_inputs_untouched_out_honoured_overlap_refused_and_asynchronous():
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd._capi import HB_ERR_BAD_ARG, HbmpcBackendError
    from honeybadgermpc_amd.progs import fixedpoint_atan as fa

    p, count, d, m, kappa, width, k = BLS, 600, 5, 8, 8, 24, 16
    ctx = gpu_ctx(p)
    torch = ctx.torch
    L = ctx.n_limbs
    opened, s, ta, tb, tab, pw0 = (random_tensor(ctx, 800 + q, count, rows=6) for q in range(6))
    x, y, c, w, g = (random_tensor(ctx, 810 + q, count) for q in range(5))
    coef = random_tensor(ctx, 820, 3)
    planes = ctx.upload_ints([(i + r) & 1 for r in range(width + kappa) for i in range(count)]).view(width + kappa, count, L)
    ops = [opened, s, ta, tb, tab, pw0, x, y, c, w, g, coef, planes]
    copies = [t.clone() for t in ops]
    s2, consts = s[:2].reshape(2 * count, L), (5, 7)

    def run():
        sm = fa.sign_mask(ctx, s2, x, y, ta[:3], tb[:3])
        am, ak = fa.abs_step(ctx, opened, ta[:3], tb[:3], tab[:3], x, y, planes, k, kappa)
        lm = fa.select_mask(ctx, c, w, s[0], ta[:2], tb[:2])
        so = fa.select(ctx, opened[:4], ta[:2], tb[:2], tab[:2], x, y)
        fm, pw = fa.atan_first(ctx, x, 7, s[1], g, ta[:2], tb[:2], d)
        pw1 = pw0[:3].clone()
        l0 = fa.atan_level(ctx, 0, d, opened[:1], s[:1], m, ta[:2], tb[:2], pw1)
        pw2 = pw0[:3].clone()
        l1 = fa.atan_level(ctx, 1, d, opened[:2], s[:2], m, ta[:1], tb[:1], pw2)
        pm, ks = fa.atan_poly_mask(ctx, d, opened[:1], s[:1], m, pw0[:3], coef, planes, width, m, kappa)
        asm, cst = fa.atan_assemble(ctx, opened[0], s[:1], m, opened[2:4], ta[1], tb[1], tab[1], s[1], g, consts, ta[2], tb[2])
        out = fa.atan_finish(ctx, opened[:2], ta[0], tb[0], tab[0], c)
        return [sm, am, ak, lm, so, fm, pw[:1], l0, pw1, l1, pw2, pm, ks, asm, cst, out]

    first = run()
    out = first[-1]
    assert torch.equal(sa.sub(ctx, sa.add(ctx, out, out), out), out)               # consumed on the current stream without a synchronise
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        second = run()
    side.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    sm, am, ak, lm, so, fm, pwr, l0, pw1, l1, pw2, pm, ks, asm, cst, out = first
    # out given: written where asked, and handed back
    new = lambda like: torch.empty_like(like)
    b = new(sm)
    assert fa.sign_mask(ctx, s2, x, y, ta[:3], tb[:3], out=b).data_ptr() == b.data_ptr() and torch.equal(b, sm)
    b0, b1 = new(am), new(ak)
    got = fa.abs_step(ctx, opened, ta[:3], tb[:3], tab[:3], x, y, planes, k, kappa, out=(b0, b1))
    assert got[0].data_ptr() == b0.data_ptr() and got[1].data_ptr() == b1.data_ptr() and torch.equal(b0, am) and torch.equal(b1, ak)
    b = new(lm)
    assert fa.select_mask(ctx, c, w, s[0], ta[:2], tb[:2], out=b).data_ptr() == b.data_ptr() and torch.equal(b, lm)
    b = new(so)
    assert fa.select(ctx, opened[:4], ta[:2], tb[:2], tab[:2], x, y, out=b).data_ptr() == b.data_ptr() and torch.equal(b, so)
    f0, f1 = new(fm), torch.empty((3, count, L), dtype=torch.int64, device=fm.device)
    got = fa.atan_first(ctx, x, 7, s[1], g, ta[:2], tb[:2], d, out=(f0, f1))
    assert got[0].data_ptr() == f0.data_ptr() and got[1].data_ptr() == f1.data_ptr() and torch.equal(f0, fm) and torch.equal(f1[:1], pwr)
    lb, pwb = new(l1), pw0[:3].clone()
    assert fa.atan_level(ctx, 1, d, opened[:2], s[:2], m, ta[:1], tb[:1], pwb, out=lb).data_ptr() == lb.data_ptr() and torch.equal(lb, l1) and torch.equal(pwb, pw2)
    p0, p1 = new(pm), new(ks)
    got = fa.atan_poly_mask(ctx, d, opened[:1], s[:1], m, pw0[:3], coef, planes, width, m, kappa, out=(p0, p1))
    assert got[0].data_ptr() == p0.data_ptr() and got[1].data_ptr() == p1.data_ptr() and torch.equal(p0, pm) and torch.equal(p1, ks)
    a0, a1 = new(asm), new(cst)
    got = fa.atan_assemble(ctx, opened[0], s[:1], m, opened[2:4], ta[1], tb[1], tab[1], s[1], g, consts, ta[2], tb[2], out=(a0, a1))
    assert got[0].data_ptr() == a0.data_ptr() and got[1].data_ptr() == a1.data_ptr() and torch.equal(a0, asm) and torch.equal(a1, cst)
    ob = new(out)
    assert fa.atan_finish(ctx, opened[:2], ta[0], tb[0], tab[0], c, out=ob).data_ptr() == ob.data_ptr() and torch.equal(ob, out)
    assert all(torch.equal(t, cp) for t, cp in zip(ops, copies))
    # argument checks raise before C and nothing is launched: the buffers keep their contents
    ob.fill_(7)
    bad_calls = [
        lambda: fa.sign_mask(ctx, s[0], x, y, ta[:3], tb[:3]),
        lambda: fa.sign_mask(ctx, s2, x, y, ta[:2], tb[:3]),
        lambda: fa.sign_mask(ctx, s2, x, y[:-1], ta[:3], tb[:3]),
        lambda: fa.abs_step(ctx, opened[:5], ta[:3], tb[:3], tab[:3], x, y, planes, k, kappa),
        lambda: fa.abs_step(ctx, opened, ta[:3], tb[:3], tab[:3], x, y, planes[:k + kappa - 1], k, kappa),
        lambda: fa.abs_step(ctx, opened, ta[:3], tb[:3], tab[:3], x, y, planes, k, 250),
        lambda: fa.abs_step(ctx, opened, ta[:3], tb[:3], tab[:3], x, y, planes, 1, kappa),
        lambda: fa.select_mask(ctx, c, w, s[0], ta[:3], tb[:2]),
        lambda: fa.select(ctx, opened[:3], ta[:2], tb[:2], tab[:2], x, y),
        lambda: fa.select(ctx, opened[:4], ta[:2], tb[:2], tab[:1], x, y),
        lambda: fa.atan_first(ctx, x, 7, s[1], g, ta[:2], tb[:2], 4),
        lambda: fa.atan_first(ctx, x, 7, s[1], g, ta[:2], tb[:2], 65),
        lambda: fa.atan_first(ctx, x, 256, s[1], g, ta[:2], tb[:2], d),
        lambda: fa.atan_first(ctx, x, -1, s[1], g, ta[:2], tb[:2], d),
        lambda: fa.atan_first(ctx, x, 7, s[1], g, ta[:1], tb[:2], d),
        lambda: fa.atan_level(ctx, 2, d, opened[:1], s[:1], m, ta[:1], tb[:1], pwb),
        lambda: fa.atan_level(ctx, -1, d, opened[:1], s[:1], m, ta[:1], tb[:1], pwb),
        lambda: fa.atan_level(ctx, 1, 6, opened[:2], s[:2], m, ta[:1], tb[:1], pwb),
        lambda: fa.atan_level(ctx, 1, d, opened[:2], s[:2], 0, ta[:1], tb[:1], pwb),
        lambda: fa.atan_level(ctx, 1, d, opened[:2], s[:2], 254, ta[:1], tb[:1], pwb),
        lambda: fa.atan_level(ctx, 1, d, opened[:1], s[:1], m, ta[:1], tb[:1], pwb),
        lambda: fa.atan_level(ctx, 1, d, opened[:2], s[:2], m, ta[:2], tb[:2], pwb),
        lambda: fa.atan_level(ctx, 1, d, opened[:2], s[:2], m, ta[:1], tb[:1], pwb[:2]),
        lambda: fa.atan_poly_mask(ctx, 1, opened[:1], s[:1], m, pw0[:3], coef, planes, width, m, kappa),
        lambda: fa.atan_poly_mask(ctx, d, opened[:2], s[:2], m, pw0[:3], coef, planes, width, m, kappa),
        lambda: fa.atan_poly_mask(ctx, d, opened[:1], s[:1], m, pw0[:2], coef, planes, width, m, kappa),
        lambda: fa.atan_poly_mask(ctx, d, opened[:1], s[:1], m, pw0[:3], coef[:2], planes, width, m, kappa),
        lambda: fa.atan_poly_mask(ctx, d, opened[:1], s[:1], m, pw0[:3], coef, planes[:-1], width, m, kappa),
        lambda: fa.atan_poly_mask(ctx, d, opened[:1], s[:1], m, pw0[:3], coef, planes, width, width, kappa),
        lambda: fa.atan_poly_mask(ctx, d, opened[:1], s[:1], m, pw0[:3], coef, planes, 250, m, kappa),
        lambda: fa.atan_assemble(ctx, opened[0], s[:1], 0, opened[2:4], ta[1], tb[1], tab[1], s[1], g, consts, ta[2], tb[2]),
        lambda: fa.atan_assemble(ctx, opened[0], s[:1], m, opened[2:3], ta[1], tb[1], tab[1], s[1], g, consts, ta[2], tb[2]),
        lambda: fa.atan_assemble(ctx, opened[0], s[:1], m, opened[2:4], ta[1], tb[1], tab[1], s[1], g, (5,), ta[2], tb[2]),
        lambda: fa.atan_finish(ctx, opened[:1], ta[0], tb[0], tab[0], c),
        lambda: fa.atan_finish(ctx, opened[:2], ta[0], tb[0], tab[0], c, out=ob[:-1]),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"bad call {i} was accepted")
    # an output laid over an input is refused by the C ABI, through Python too
    buf = random_tensor(ctx, 830, count, rows=8)
    for call in (lambda: fa.sign_mask(ctx, s2, x, y, ta[:3], tb[:3], out=ta),
                 lambda: fa.sign_mask(ctx, s2, buf[1], y, ta[:3], tb[:3], out=buf[:6]),
                 lambda: fa.abs_step(ctx, opened, ta[:3], tb[:3], tab[:3], x, y, planes, k, kappa, out=(b0, opened[1:6])),
                 lambda: fa.abs_step(ctx, opened, ta[:3], tb[:3], tab[:3], x, y, planes, k, kappa, out=(planes[3:4], b1)),
                 lambda: fa.abs_step(ctx, opened, ta[:3], tb[:3], tab[:3], x, y, planes, k, kappa, out=(buf[:1], buf[:5])),
                 lambda: fa.select_mask(ctx, c, w, buf[2], ta[:2], tb[:2], out=buf[:4]),
                 lambda: fa.select(ctx, opened[:4], ta[:2], tb[:2], tab[:2], x, buf[0], out=buf[:3]),
                 lambda: fa.atan_first(ctx, x, 7, s[1], g, ta[:2], tb[:2], d, out=(ta[:4], f1)),
                 lambda: fa.atan_first(ctx, buf[0], 7, s[1], g, ta[:2], tb[:2], d, out=(f0, buf[:3])),
                 lambda: fa.atan_first(ctx, x, 7, s[1], g, ta[:2], tb[:2], d, out=(buf[:4], buf[3:6])),
                 lambda: fa.atan_level(ctx, 1, d, opened[:2], s[:2], m, ta[:1], tb[:1], pwb, out=pwb[:2]),
                 lambda: fa.atan_level(ctx, 1, d, buf[:2], s[:2], m, ta[:1], tb[:1], pwb, out=buf[1:3]),
                 lambda: fa.atan_level(ctx, 1, d, opened[:2], s[:2], m, buf[:1], tb[:1], buf[:3]),
                 lambda: fa.atan_poly_mask(ctx, d, opened[:1], s[:1], m, pw0[:3], coef, planes, width, m, kappa, out=(pw0[:1], p1)),
                 lambda: fa.atan_poly_mask(ctx, d, opened[:1], s[:1], m, pw0[:3], coef, planes, width, m, kappa, out=(p0, planes[3:4])),
                 lambda: fa.atan_poly_mask(ctx, d, opened[:1], s[:1], m, pw0[:3], coef, planes, width, m, kappa, out=(p0, p0)),
                 lambda: fa.atan_assemble(ctx, opened[0], s[:1], m, opened[2:4], ta[1], tb[1], tab[1], s[1], g, consts, ta[2], tb[2], out=(a0, g)),
                 lambda: fa.atan_assemble(ctx, opened[0], s[:1], m, opened[2:4], ta[1], tb[1], tab[1], s[1], g, consts, ta[2], tb[2], out=(opened[3:5], a1)),
                 lambda: fa.atan_finish(ctx, opened[:2], ta[0], tb[0], tab[0], c, out=c),
                 lambda: fa.atan_finish(ctx, opened[:2], ta[0], tb[0], tab[0], c, out=opened[1])):
        with pytest.raises(HbmpcBackendError):
            call()
    # ... and the C ABI itself
    lib, st, P = ctx.lib, ctx.stream(), ctx.ptr
    one_elem, two_elems = ctx.host_elems([1]), ctx.host_elems([5, 7])
    one, two = one_elem.ctypes.data, two_elems.ctypes.data
    A = HB_ERR_BAD_ARG
    assert lib.hb_fxatan_sign_mask(ctx.h, P(s), P(x), None, P(ta), P(tb), P(b), count, st) == A
    assert lib.hb_fxatan_sign_mask(ctx.h, P(s), P(x), P(y), P(ta), P(tb), P(b), -1, st) == A
    assert lib.hb_fxatan_abs(ctx.h, P(opened), P(ta), P(tb), P(tab), P(x), P(y), P(planes), 1, kappa, P(b0), P(b1), count, st) == A
    assert lib.hb_fxatan_abs(ctx.h, P(opened), P(ta), P(tb), P(tab), P(x), P(y), P(planes), k, 250, P(b0), P(b1), count, st) == A
    assert lib.hb_fxatan_abs(ctx.h, P(opened), P(ta), P(tb), P(tab), P(x), P(y), P(planes), k, kappa, P(b0), P(x), count, st) == A
    assert lib.hb_fxatan_select_mask(ctx.h, P(c), P(w), P(s), P(ta), P(tb), P(c), count, st) == A
    assert lib.hb_fxatan_select(ctx.h, P(opened), P(ta), P(tb), P(tab), P(x), None, P(b), count, st) == A
    assert lib.hb_fxatan_first(ctx.h, P(x), 256, P(s), P(g), P(ta), P(tb), P(f0), P(f1), count, st) == A
    assert lib.hb_fxatan_first(ctx.h, P(x), -1, P(s), P(g), P(ta), P(tb), P(f0), P(f1), count, st) == A
    assert lib.hb_fxatan_first(ctx.h, P(x), 7, P(s), P(g), P(ta), P(tb), P(f0), P(g), count, st) == A
    assert lib.hb_fxatan_level(ctx.h, 1, 1, P(opened), P(s), m, one, P(ta), P(tb), P(lb), P(pwb), count, st) == A
    assert lib.hb_fxatan_level(ctx.h, 1, 65, P(opened), P(s), m, one, P(ta), P(tb), P(lb), P(pwb), count, st) == A
    assert lib.hb_fxatan_level(ctx.h, 1, 6, P(opened), P(s), m, one, P(ta), P(tb), P(lb), P(pwb), count, st) == A
    assert lib.hb_fxatan_level(ctx.h, 2, d, P(opened), P(s), m, one, P(ta), P(tb), P(lb), P(pwb), count, st) == A
    assert lib.hb_fxatan_level(ctx.h, -1, d, P(opened), P(s), m, one, P(ta), P(tb), P(lb), P(pwb), count, st) == A
    assert lib.hb_fxatan_level(ctx.h, 1, d, P(opened), P(s), m, None, P(ta), P(tb), P(lb), P(pwb), count, st) == A
    assert lib.hb_fxatan_level(ctx.h, 1, d, P(opened), P(s), 254, one, P(ta), P(tb), P(lb), P(pwb), count, st) == A
    assert lib.hb_fxatan_level(ctx.h, 1, d, P(opened), P(s), m, one, P(ta), P(tb), P(lb), None, count, st) == A
    assert lib.hb_fxatan_level(ctx.h, 1, d, P(opened), P(s), m, one, P(ta), P(tb), P(ta), P(pwb), count, st) == A
    assert lib.hb_fxatan_poly_mask(ctx.h, 1, P(opened), P(s), m, one, P(pw0), P(coef), P(planes), width, m, kappa, P(p0), P(p1), count, st) == A
    assert lib.hb_fxatan_poly_mask(ctx.h, d, P(opened), P(s), m, one, P(pw0), None, P(planes), width, m, kappa, P(p0), P(p1), count, st) == A
    assert lib.hb_fxatan_poly_mask(ctx.h, d, P(opened), P(s), m, one, P(pw0), P(coef), P(planes), 250, m, kappa, P(p0), P(p1), count, st) == A
    assert lib.hb_fxatan_poly_mask(ctx.h, d, P(opened), P(s), m, one, P(pw0), P(coef), P(planes), width, m, kappa, P(p0), P(coef), count, st) == A
    assert lib.hb_fxatan_assemble(ctx.h, P(opened), P(s), 0, one, P(opened[2]), P(ta), P(tb), P(tab), P(s[1]), P(g), two, P(ta[2]), P(tb[2]), P(a0), P(a1), count, st) == A
    assert lib.hb_fxatan_assemble(ctx.h, P(opened), P(s), m, one, P(opened[2]), P(ta), P(tb), P(tab), P(s[1]), P(g), None, P(ta[2]), P(tb[2]), P(a0), P(a1), count, st) == A
    assert lib.hb_fxatan_assemble(ctx.h, P(opened), P(s), m, one, P(opened[2]), P(ta), P(tb), P(tab), P(s[1]), P(g), two, P(ta[2]), P(tb[2]), P(a0), P(g), count, st) == A
    assert lib.hb_fxatan_finish(ctx.h, P(opened), P(ta), P(tb), P(tab), P(c), P(c), count, st) == A
    assert lib.hb_fxatan_finish(ctx.h, P(opened), P(ta), P(tb), P(tab), P(c), None, count, st) == A
    # count == 0: a successful call that launches nothing
    assert lib.hb_fxatan_sign_mask(ctx.h, P(s), P(x), P(y), P(ta), P(tb), P(b), 0, st) == 0
    assert lib.hb_fxatan_abs(ctx.h, P(opened), P(ta), P(tb), P(tab), P(x), P(y), P(planes), k, kappa, P(b0), P(b1), 0, st) == 0
    assert lib.hb_fxatan_select_mask(ctx.h, P(c), P(w), P(s), P(ta), P(tb), P(b), 0, st) == 0
    assert lib.hb_fxatan_select(ctx.h, P(opened), P(ta), P(tb), P(tab), P(x), P(y), P(b), 0, st) == 0
    assert lib.hb_fxatan_first(ctx.h, P(x), 7, P(s), P(g), P(ta), P(tb), P(f0), P(f1), 0, st) == 0
    assert lib.hb_fxatan_level(ctx.h, 1, d, P(opened), P(s), m, one, P(ta), P(tb), P(lb), P(pwb), 0, st) == 0
    assert lib.hb_fxatan_poly_mask(ctx.h, d, P(opened), P(s), m, one, P(pw0), P(coef), P(planes), width, m, kappa, P(p0), P(p1), 0, st) == 0
    assert lib.hb_fxatan_assemble(ctx.h, P(opened), P(s), m, one, P(opened[2]), P(ta), P(tb), P(tab), P(s[1]), P(g), two, P(ta[2]), P(tb[2]), P(a0), P(a1), 0, st) == 0
    assert lib.hb_fxatan_finish(ctx.h, P(opened), P(ta), P(tb), P(tab), P(c), P(ob), 0, st) == 0
    torch.cuda.synchronize()
    assert bool((ob == 7).all()) and torch.equal(b0, am) and torch.equal(b1, ak) and torch.equal(f0, fm) and torch.equal(lb, l1) and torch.equal(pwb, pw2)
    assert torch.equal(p0, pm) and torch.equal(p1, ks) and torch.equal(a0, asm) and torch.equal(a1, cst)
    assert all(torch.equal(t, cp) for t, cp in zip(ops, copies))


# ---- the protocol, end to end ---------------------------------------------------------------------------------------------------
async def _composed(co, y, x, bits, triples, f, k, kappa, turns):
    """the chain of fixedpoint_atan from what the package offered before: ltz, div, share_arithmetic, fixedpoint.trunc_mask /
    trunc_pr_finish; the same preprocessing in the same order, several products in ONE open where the fused steps have them so -> the
    result shares"""
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd.progs import fixedpoint as fx
    from honeybadgermpc_amd.progs import fixedpoint_atan as fa
    from honeybadgermpc_amd.progs import fixedpoint_division as fd

    ctx = co.ctx
    torch = ctx.torch
    lay = fa.atan_layout(k, f, kappa, turns)
    d, width, dlay = lay["degree"], lay["width"], lay["div"]
    n, nb, p, L = k - 1, width + kappa, ctx.modulus, ctx.n_limbs
    count = x.shape[0]
    rows = fd._Rows(bits, triples)
    n_div = len(dlay["planes"]) - 1                                        # every range of the division's planes but the bit decomposition's is a truncation
    shifts = iter(fa.atan_shifts(k, f, turns)[n_div:])
    sigma = lambda b: _sigma(ctx, sa, b)

    async def products(pairs):
        t = rows.take(len(pairs))
        opened = await co.open_share_array(torch.cat([m for q, (u, v) in enumerate(pairs) for m in (sa.sub(ctx, u, t[0][q]), sa.sub(ctx, v, t[1][q]))]))
        return [sa.beaver_combine(ctx, opened[2 * q * count:(2 * q + 1) * count], opened[(2 * q + 1) * count:(2 * q + 2) * count], t[0][q], t[1][q], t[2][q]) for q in range(len(pairs))]

    async def truncate(vals):
        ms = [next(shifts) for _ in vals]
        masks = [fx.trunc_mask(ctx, v, rows.planes(nb), width, m, kappa) for v, m in zip(vals, ms)]
        opened = await co.open_share_array(torch.cat([mk for mk, _ in masks]))
        return [fx.trunc_pr_finish(ctx, v, opened[q * count:(q + 1) * count], masks[q][1], m) for q, (v, m) in enumerate(zip(vals, ms))]

    ct = fx.carry_triples(n)
    s = await fx.ltz(co, torch.cat([x, y]), rows.planes(2 * (k + kappa)).view(k + kappa, 2 * count, L), tuple(v.view(ct, 2 * count, L) for v in rows.take(2 * ct)), k, kappa)
    sx, sy = s[:count], s[count:]
    px, py, g = await products([(sx, x), (sy, y), (sigma(sy), sx)])
    ax, ay = sa.sub(ctx, x, sa.mul(ctx, px, 2)), sa.sub(ctx, y, sa.mul(ctx, py, 2))
    w = sa.sub(ctx, ax, ay)
    c = await fx.ltz(co, w, rows.planes(k + kappa), rows.take(ct), k, kappa)
    cw, e1 = await products([(c, w), (sigma(c), sigma(sx))])
    num, den = sa.add(ctx, ay, cw), sa.sub(ctx, ax, cw)
    q = await fd.div(co, num, den, rows.planes(dlay["n_planes"]), rows.take(dlay["n_triples"]), f, k, kappa, None, False)
    t = {0: sa.mul(ctx, q, 1 << (n - f))}
    uu, e = await products([(t[0], t[0]), (sigma(sy), e1)])
    u, = await truncate([uu])
    for level in range(1, lay["levels"] + 1):
        js = ac.level_odd(level, d)
        pairs = [(t[j - (1 << (level - 1))], u) for j in js] + ([(u, u)] if ac.level_square(level, d) else [])
        done = await truncate(await products(pairs))
        for j, v in zip(js, done):
            t[j] = v
        if ac.level_square(level, d):
            u = done[-1]
    coef = fa.atan_coefficients(k, f, turns)
    poly = sa.mul(ctx, t[0], coef[0] % p)
    for j in range(1, len(coef)):
        poly = sa.add(ctx, poly, sa.mul(ctx, t[j], coef[j] % p))
    a, = await truncate([poly])
    ca, cb = fa.assemble_constants(p, f, turns)
    cst = sa.add(ctx, sa.mul(ctx, g, ca), sa.mul(ctx, sa.sub(ctx, sigma(sy), e), cb))
    ea, = await products([(e, a)])
    return sa.add(ctx, cst, ea)


def _deal(ctx, fa, rnd, p, n, t, lay, limits, kappa, count):
    """bit planes with an all-ones r1 planted under the first, one middle and the last truncation of element 1, and triples, each with
    a canary row after its last -> (bits, trip [party], r1s [element])"""
    n_planes, n_triples = lay["n_planes"], lay["n_triples"]
    bit_rows = [[rnd.getrandbits(1) for _ in range(count)] for _ in range(n_planes)]
    starts = ac.truncation_planes(lay, kappa)
    assert len(starts) == len(limits)
    for which in (0, len(starts) // 2, len(starts) - 1):
        for i in range(limits[which]):
            bit_rows[starts[which] + i][1] = 1
    r1s = [[sum(bit_rows[s + i][e] << i for i in range(m)) for s, m in zip(starts, limits)] for e in range(count)]
    bit_rows.append([rnd.randrange(p) for _ in range(count)])              # a canary plane and a canary row: reading either would spoil the results
    ta, tb = ([[rnd.randrange(p) for _ in range(count)] for _ in range(n_triples)] for _ in range(2))
    tab = [[a * b % p for a, b in zip(ra, rb)] for ra, rb in zip(ta, tb)]
    for v in (ta, tb, tab):
        v.append([rnd.randrange(p) for _ in range(count)])
    return bc.deal_planes(ctx, rnd, p, n, t, bit_rows), [bc.deal_planes(ctx, rnd, p, n, t, v) for v in (ta, tb, tab)], r1s


@pytest.mark.parametrize("turns", [False, True], ids=["radians", "turns"])
@pytest.mark.parametrize("p", [BLS, bc.P64], ids=["bls", "2^64-59"])
def test_protocol_end_to_end(p, turns):
    from honeybadgermpc_amd.progs import fixedpoint_atan as fa

    k, f, kappa = 16, 8, 8
    n, t, count = 4, 1, 16
    ctx = gpu_ctx(p)
    torch = ctx.torch
    rnd = random.Random(100 * k + f + turns + p % 7)
    pairs = ac.e2e_pairs(rnd, k, f, count)
    assert len(pairs) == count and pairs[0] == (0, 0) and {(y > 0) - (y < 0) for y, _ in pairs} == {(x > 0) - (x < 0) for _, x in pairs} == {-1, 0, 1}
    bad = set(rnd.sample(range(n), 1))
    honest = [i for i in range(n) if i not in bad]
    lay = fa.atan_layout(k, f, kappa, turns)
    n_planes, n_triples = lay["n_planes"], lay["n_triples"]
    assert lay["degree"] == fa.atan_degree(k, f, turns) and lay["width"] + kappa + 1 <= p.bit_length() - 1          # the width fits both field classes
    limits = fa.atan_shifts(k, f, turns)
    bits, trip, r1s = _deal(ctx, fa, rnd, p, n, t, lay, limits, kappa, count)
    vals = bc.deal_planes(ctx, rnd, p, n, t, [[y % p for y, _ in pairs], [x % p for _, x in pairs]])

    async def body(co, i):
        y, x = vals[i][0], vals[i][1]
        triples = tuple(tr[i] for tr in trip)
        exact_bits, exact_triples = bits[i][:n_planes], tuple(v[:n_triples] for v in triples)
        keep = (vals[i].clone(), bits[i].clone(), [v.clone() for v in triples])
        for short in (lambda: fa.atan2(co, y, x, exact_bits, tuple(v[:n_triples - 1] for v in triples), f, k, kappa, turns),
                      lambda: fa.atan2(co, y, x, exact_bits[:n_planes - 1], exact_triples, f, k, kappa, turns),
                      lambda: fa.atan2(co, y, x[:-1], exact_bits, exact_triples, f, k, kappa, turns),
                      lambda: fa.atan2(co, y, x, exact_bits, exact_triples, k - 2, k, kappa, turns),
                      lambda: fa.atan2(co, y, x, exact_bits, exact_triples, k // 2 - 1, k, kappa, turns),
                      lambda: fa.atan2(co, y, x, exact_bits, exact_triples, f, k, 250, turns),
                      lambda: fa.atan(co, y, exact_bits, exact_triples, k - 2, k, kappa, turns)):
            with pytest.raises(ValueError):
                await short()
        assert co.batches == 0                                             # refused before anything was opened
        fused = await fa.atan2(co, y, x, bits[i], triples, f, k, kappa, turns)
        batches = co.batches
        exact = await fa.atan2(co, y, x, exact_bits, exact_triples, f, k, kappa, turns)
        before = co.batches
        composed = await _composed(co, y, x, exact_bits, exact_triples, f, k, kappa, turns)
        assert co.batches - before == batches                               # the same opens, composed or fused
        assert torch.equal(fused, exact) and torch.equal(fused, composed), i          # share for share
        opened = ctx.download_ints(await co.open_share_array(fused))
        assert torch.equal(vals[i], keep[0]) and torch.equal(bits[i], keep[1]) and all(torch.equal(v, w) for v, w in zip(triples, keep[2]))
        return opened, batches

    results = bc.run_parties(p, n, t, bad, rnd, body)
    want = [fa.atan2_model(y, x, p, k, f, r1s[e], turns) for e, (y, x) in enumerate(pairs)]
    bound = fa.atan_error_bound(k, f, turns)
    big, half = fa.atan_constants(f, turns)
    assert [ac.centered(w, p) for w in want[:5]] == [0, 0, big, half, -half]        # (0, 0), (0, +), (0, -): +pi, (+, 0), (-, 0), exactly
    for e, w in enumerate(want):                                            # the model is within the bound
        assert ac.distance(ac.centered(w, p), ac.atan2_enclosure(*pairs[e], f, turns)) <= bound, (pairs[e], w)
    for i in honest:
        opened, batches = results[i]
        assert opened == want, i
        assert batches == lay["opens"] == fa.atan2_opens(k, f, turns)


def test_fixed_point_array_atan2_and_atan():
    from honeybadgermpc_amd.progs import fixedpoint as fx
    from honeybadgermpc_amd.progs import fixedpoint_atan as fa

    p, (k, f, kappa), n, t, count = BLS, (16, 8, 8), 4, 1, 16
    ctx = gpu_ctx(p)
    rnd = random.Random(173)
    pairs = ac.e2e_pairs(rnd, k, f, count)
    cases = [("atan2", False), ("atan2", True), ("atan", False), ("atan", True)]
    prep = [_deal(ctx, fa, rnd, p, n, t, fa.atan_layout(k, f, kappa, turns), fa.atan_shifts(k, f, turns), kappa, count) for _, turns in cases]
    vals = bc.deal_planes(ctx, rnd, p, n, t, [[y % p for y, _ in pairs], [x % p for _, x in pairs]])

    async def body(co, i):
        ya, xa = (fx.FixedPointArray(co, vals[i][r], f, k, kappa) for r in range(2))
        out = []
        for (name, turns), (bits, trip, _) in zip(cases, prep):
            triples = tuple(tr[i] for tr in trip)
            res = await (ya.atan2(xa, bits[i], triples, turns) if name == "atan2" else ya.atan(bits[i], triples, turns))
            assert isinstance(res, fx.FixedPointArray) and (res.f, res.k, res.kappa) == (f, k, kappa)
            out.append(ctx.download_ints(await co.open_share_array(res.shares)))
        return out

    for got in bc.run_parties(p, n, t, set(), rnd, body):
        for (name, turns), (_, _, r1s), res in zip(cases, prep, got):
            assert res == [fa.atan2_model(y, x if name == "atan2" else 1 << f, p, k, f, r1s[e], turns) for e, (y, x) in enumerate(pairs)], (name, turns)


def test_round_trip_through_sincos_turns():
    """sincos_turns of atan2(y, x, turns=True) against (y, x) / R, R = sqrt(x^2 + y^2) from the opened inputs: the angle is within
    atan_error_bound ulps of a turn of the true one, the sine and the cosine are 2 pi-Lipschitz in turns (710 / 113 > 2 pi), and
    sincos_turns adds trig_error_bound of its own: |R s - y 2^f| <= R (710 / 113 atan_error_bound + trig_error_bound), and likewise x"""
    import exp_cases as ec

    from honeybadgermpc_amd.progs import demux as dx
    from honeybadgermpc_amd.progs import fixedpoint_atan as fa
    from honeybadgermpc_amd.progs import fixedpoint_trig as ft

    p, (k, f, kappa), n, t, count = BLS, (16, 8, 8), 4, 1, 16
    ctx = gpu_ctx(p)
    rnd = random.Random(179)
    pairs = ac.e2e_pairs(rnd, k, f, count + 1)[1:]                          # (0, 0) has no direction
    lay = fa.atan_layout(k, f, kappa, True)
    bits, trip, _ = _deal(ctx, fa, rnd, p, n, t, lay, fa.atan_shifts(k, f, True), kappa, count)
    tlay = ft.trig_layout(k, f, kappa)
    tbits = bc.deal_planes(ctx, rnd, p, n, t, [[rnd.getrandbits(1) for _ in range(count)] for _ in range(tlay["n_planes"])])
    ta, tb = ([[rnd.randrange(p) for _ in range(count)] for _ in range(tlay["n_triples"])] for _ in range(2))
    ttrip = [bc.deal_planes(ctx, rnd, p, n, t, v) for v in (ta, tb, [[a * b % p for a, b in zip(ra, rb)] for ra, rb in zip(ta, tb)])]
    demux = ec.deal_demux_triples(ctx, ft, dx, rnd, p, n, t, tlay, [w for _, w in tlay["groups"]], count)
    vals = bc.deal_planes(ctx, rnd, p, n, t, [[y % p for y, _ in pairs], [x % p for _, x in pairs]])

    async def body(co, i):
        angle = await fa.atan2(co, vals[i][0], vals[i][1], bits[i], tuple(tr[i] for tr in trip), f, k, kappa, True)
        sin, cos = await ft.sincos_turns(co, angle, tbits[i], tuple(tr[i] for tr in ttrip), [(a[:-1], b[:-1]) for a, b in demux[i]], f, k, kappa)
        return [ctx.download_ints(await co.open_share_array(v)) for v in (sin, cos, vals[i][0], vals[i][1])]

    tol = Fraction(710, 113) * fa.atan_error_bound(k, f, True) + ft.trig_error_bound(k, f)
    for sin, cos, ys, xs in bc.run_parties(p, n, t, set(), rnd, body):
        assert [(ac.centered(y, p), ac.centered(x, p)) for y, x in zip(ys, xs)] == pairs
        worst = Fraction(0)
        for (y, x), s, c in zip(pairs, sin, cos):
            r_hi = Fraction(isqrt((x * x + y * y) << 128) + 1, 1 << 64)     # the opened radius, from above
            r_lo = r_hi - Fraction(1, 1 << 64)
            for got, true in ((ac.centered(s, p), y), (ac.centered(c, p), x)):
                err = max(abs(got * r_lo - (true << f)), abs(got * r_hi - (true << f)))
                worst = max(worst, err / r_lo)
                assert err <= tol * r_hi, (y, x, got, float(tol))
        print(f"round trip at (16, 8): worst {float(worst):.4f} ulps, bound {float(tol):.4f}")

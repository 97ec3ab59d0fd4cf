"""k_pair_product (csrc/hb_pair.hip) and the verifier of PolyCommitConst on the device.  The kernel's words are compared with
hb_selftest_pairing, which runs the same bodies on the host (pairing_support), with the Python-int model on a few items, and with the
reference crate's recorded e(G1 generator, G2 generator).  Every comparison is exact.

W = 64 is the number of items a workgroup of k_pair_product takes: the batches are 1, W - 1, W and W + 1 items.  The host reference of
the largest batch is computed once a K and shared."""
import ctypes
import functools
import json
import os
import random

import numpy as np
import pytest

import pairing_support as ps
from conftest import GOLDEN

from honeybadgermpc_amd import _capi
from honeybadgermpc_amd.bls12_381 import G1, R
from honeybadgermpc_amd.bls12_381_pairing import G2

pytestmark = pytest.mark.gpu

W = 64
ALL_IDENTITY, MODEL_ITEMS = 3, (0, 3, 5, 64)


@pytest.fixture(scope="module")
def ctx():
    from honeybadgermpc_amd._capi import Context

    return Context.get(R)


@functools.lru_cache(maxsize=None)
def qs():
    h = G2.generator()
    return [h, h ** 0xABCDEF, h ** (R - 2)]


@functools.lru_cache(maxsize=None)
def prepared(ctx):
    from honeybadgermpc_amd import pairing

    return [pairing.PreparedG2(ctx, q) for q in qs()]


@functools.lru_cache(maxsize=None)
def rows(K):
    """W + 1 items of K points: small and full-width multiples of the generator, identities scattered through the batch (item 5: the
    first point; item 9: the last), item ALL_IDENTITY all identities"""
    rnd = random.Random(40 + K)
    g = G1.generator()
    out = []
    for m in range(W + 1):
        row = [g ** (rnd.randrange(R) if m % 4 == 0 else rnd.randrange(1, 1 << 16)) for _ in range(K)]
        if m == ALL_IDENTITY:
            row = [G1.one()] * K
        if m in (5, 40):
            row[0] = G1.one()
        if m in (9, W):
            row[K - 1] = G1.one() if K > 1 else row[K - 1]
        out.append(row)
    return out


@functools.lru_cache(maxsize=None)
def reference(K):
    """(W + 1, 72) uint64 from the self test"""
    return ps.gt_words(ps.host_product(rows(K), qs()[:K]))


def device_product(ctx, K, count):
    from honeybadgermpc_amd import g1, pairing

    pairs = [(g1.upload([r[k] for r in rows(K)[:count]], ctx), prepared(ctx)[k]) for k in range(K)]
    return pairing.product(ctx, pairs)


@pytest.mark.parametrize("count", [1, W - 1, W, W + 1])
@pytest.mark.parametrize("K", [1, 2, 3])
def test_product_is_bit_equal_to_the_selftest(ctx, K, count):
    out = device_product(ctx, K, count)
    assert tuple(out.shape) == (count, 12, 6)
    got = out.cpu().numpy().view(np.uint64).reshape(count, 72)
    assert np.array_equal(got, reference(K)[:count])


def test_product_equals_the_model_on_four_items_and_identities_contribute_one(ctx):
    from honeybadgermpc_amd import pairing

    out = pairing.download_gt(device_product(ctx, 2, W + 1))
    for m in MODEL_ITEMS:
        assert out[m] == ps.model_product(rows(2)[m], qs()[:2]), m
    assert out[ALL_IDENTITY].is_one()
    assert out[5] == ps.model_product(rows(2)[5][1:], qs()[1:2])      # the first pair is skipped


def test_pair_of_the_generators_is_the_recorded_value(ctx):
    from honeybadgermpc_amd import pairing

    with open(os.path.join(GOLDEN, "pairing_generators_gt.json")) as f:
        want = [int(v) for v in json.load(f)["coords"]]
    out = pairing.pair(ctx, G1.generator(), prepared(ctx)[0])
    assert tuple(out.shape) == (1, 12, 6)
    assert ps.s.unwords(out.cpu().numpy().view(np.uint64).reshape(-1), 6) == want
    assert pairing.download_gt(out)[0].coords() == want


def test_verdict_mode_flags_exactly_the_planted_rejections(ctx):
    from honeybadgermpc_amd import g1, pairing

    g, h = G1.generator(), G2.generator()
    count, bad = W + 1, (0, 31, W)
    first = [g ** (3 * (m + 1) + (1 if m in bad else 0)) for m in range(count)]
    second = [(g ** (m + 1)).invert() for m in range(count)]
    first[7], second[7] = G1.one(), G1.one()                          # both identities: 1
    p3 = pairing.PreparedG2(ctx, h ** 3)
    ok, counter = pairing.product_is_one(ctx, [(g1.upload(first, ctx), prepared(ctx)[0]), (g1.upload(second, ctx), p3)])
    assert ok.dtype == ctx.torch.bool and tuple(ok.shape) == (count,)
    assert [m for m in range(count) if not ok[m].item()] == list(bad)
    assert int(counter.item()) == len(bad)
    verdicts, rejected = ps.host_product([[a, b] for a, b in zip(first, second)], [h, h ** 3], mode=ps.VERDICT)
    assert verdicts == [int(v) for v in ok.cpu().tolist()] and rejected == len(bad)
    # a point off the curve is rejected whatever the product
    raw = ctx.torch.from_numpy(ps.s.points([ps.s.off_curve_raw(), G1.one()]).view(np.int64).reshape(2, 2, 6)).to(ctx.tdev)
    ok, counter = pairing.product_is_one(ctx, [(raw, prepared(ctx)[0])])
    assert ok.cpu().tolist() == [False, True] and int(counter.item()) == 1


# ---------------------------------------------------------------- PolyCommitConst
def test_poly_commit_const_verifier_end_to_end(ctx):
    from honeybadgermpc_amd import g1
    from honeybadgermpc_amd.field import GF
    from honeybadgermpc_amd.poly_commit_const import PolyCommitConst, gen_pc_const_crs
    from honeybadgermpc_amd.polynomial import polynomials_over

    t, n, B = 3, 4, 5
    torch = ctx.torch
    g = G1.generator()
    gh = ps.ghats()
    crs = gen_pc_const_crs(t, alpha=ps.ALPHA, g=g, h=g ** ps.LAM, ctx=ctx, ghat=gh[0])
    assert crs[1] == gh and crs[0] == ps.cs.crs_points(t + 1)[0]
    pc = PolyCommitConst(crs, ctx=ctx)
    pc.preprocess_verifier(4)
    rnd = random.Random(8)
    phis = [[rnd.randrange(R) for _ in range(t + 1)] for _ in range(B)]
    coeffs = ctx.upload_ints([v for p in phis for v in p]).reshape(B, t + 1, 4)
    c, hat = pc.commit_batch(coeffs)
    xs = list(range(1, n + 1))
    w, shares, aux = pc.witness_batch(coeffs, hat, xs)
    # one shared index
    for i, x in enumerate(xs):
        ok = pc.verify_batch(c, x, shares[:, i], aux[:, i], w[:, i])
        assert ok.dtype == torch.bool and ok.cpu().tolist() == [True] * B, x
    # an index an item: item b opens at xs[b % n]
    pick = [b % n for b in range(B)]
    idx = torch.tensor(pick, device=ctx.tdev)
    ar = torch.arange(B, device=ctx.tdev)
    sh, au, wi = shares[ar, idx].contiguous(), aux[ar, idx].contiguous(), w[ar, idx].contiguous()
    per_item = [xs[k] for k in pick]
    assert pc.verify_batch(c, per_item, sh, au, wi).cpu().tolist() == [True] * B
    assert pc.verify_batch(c, ctx.upload_ints(per_item), sh, au, wi).cpu().tolist() == [True] * B
    wrong_index = list(per_item)
    wrong_index[2] += 1
    assert pc.verify_batch(c, wrong_index, sh, au, wi).cpu().tolist() == [b != 2 for b in range(B)]
    # a corrupted share, aux and witness flip exactly their slot
    for slot, what in ((0, "share"), (3, "aux"), (4, "witness")):
        s2, a2, w2 = sh.clone(), au.clone(), wi.clone()
        if what == "share":
            s2[slot] = ctx.upload_ints([(ctx.download_ints(sh[slot:slot + 1])[0] + 1) % R])[0]
        elif what == "aux":
            a2[slot] = ctx.upload_ints([(ctx.download_ints(au[slot:slot + 1])[0] + 1) % R])[0]
        else:
            w2[slot] = g1.add(ctx, wi[slot:slot + 1].contiguous(), g1.upload([g], ctx))[0]
        assert pc.verify_batch(c, per_item, s2, a2, w2).cpu().tolist() == [b != slot for b in range(B)], what
    # the reference's surface on host objects
    poly = polynomials_over(GF(R))
    phi_list = [poly(p) for p in phis[:3]]
    opened = []
    for phi in phi_list:
        ch, phi_hat = pc.commit(phi)
        wh = pc.create_witness(phi, phi_hat, 2)
        opened.append((ch, phi(2), phi_hat(2), wh))
    ch, s2, a2, wh = opened[0]
    assert pc.verify_eval(ch, 2, s2, a2, wh) is True
    assert pc.verify_eval(ch, 2, s2 + 1, a2, wh) is False
    assert pc.verify_eval(ch, 3, s2, a2, wh) is False
    assert pc.verify_eval(ch * g, 2, s2, a2, wh) is False
    cols = list(zip(*opened))
    assert pc.batch_verify_eval(cols[0], 2, cols[1], cols[2], cols[3]) is True
    bad_shares = list(cols[1])
    bad_shares[1] = bad_shares[1] + 1
    assert pc.batch_verify_eval(cols[0], 2, bad_shares, cols[2], cols[3]) is False
    # the reference's batch check is ONE equation over sums: errors that cancel pass, as they do there
    bad_shares[2] = bad_shares[2] - 1
    assert pc.batch_verify_eval(cols[0], 2, bad_shares, cols[2], cols[3]) is True
    assert pc.batch_verify_eval([], 2, [], [], []) is True
    # a CRS without ghats raises as before
    pc0 = PolyCommitConst([crs[0], None, crs[2]], ctx=ctx)
    for call in (lambda: pc0.verify_eval(ch, 2, s2, a2, wh), lambda: pc0.batch_verify_eval([ch], 2, [s2], [a2], [wh]), lambda: pc0.preprocess_verifier(),
                 lambda: pc0.verify_batch(c, 1, sh, au, wi)):
        with pytest.raises(NotImplementedError, match="pairing"):
            call()


def test_poly_commit_const_verifier_degree_zero(ctx):
    """t = 0: every witness is the identity, so the second pair is skipped on the device too"""
    from honeybadgermpc_amd.poly_commit_const import PolyCommitConst

    gs, hs = ps.cs.crs_points(1)
    pc = PolyCommitConst([gs, ps.ghats(), hs], ctx=ctx)
    coeffs, hat = ctx.upload_ints([5, R - 1]).reshape(2, 1, 4), ctx.upload_ints([7, 0]).reshape(2, 1, 4)
    c, _ = pc.commit_batch(coeffs, hat)
    w, shares, aux = pc.witness_batch(coeffs, hat, [9])
    assert (w == 0).all().item()
    assert pc.verify_batch(c, 9, shares[:, 0], aux[:, 0], w[:, 0]).cpu().tolist() == [True, True]
    assert pc.verify_batch(c, 9, aux[:, 0], shares[:, 0], w[:, 0]).cpu().tolist() == [False, False]


# ---------------------------------------------------------------- arguments
def test_argument_errors(ctx):
    from honeybadgermpc_amd import g1, pairing

    p0, p1 = prepared(ctx)[:2]
    pts = g1.upload([G1.generator()] * 3, ctx)
    with pytest.raises(ValueError, match="pairs"):
        pairing.product(ctx, [])
    with pytest.raises(ValueError, match="pairs"):
        pairing.product(ctx, [(pts, p0)] * 5)
    with pytest.raises(ValueError, match="points"):
        pairing.product(ctx, [(pts, p0), (pts[:2], p1)])
    with pytest.raises(TypeError):
        pairing.product(ctx, [(pts, p0.table)])
    with pytest.raises(ValueError, match="identity"):
        pairing.PreparedG2(ctx, G2.one())
    short = pairing.PreparedG2(ctx, G2.generator())
    short.table = short.table[:-4]
    with pytest.raises(ValueError, match="bytes"):
        pairing.product(ctx, [(pts, short)])
    # the C ABI itself
    lib, s = ctx.lib, ctx.stream()
    tabs = (ctypes.c_void_p * 5)(*[p0.table.data_ptr()] * 5)
    out = ctx.torch.empty((3, 12, 6), dtype=ctx.torch.int64, device=ctx.tdev)
    flags = ctx.torch.zeros((4,), dtype=ctx.torch.int32, device=ctx.tdev)
    call = lambda K, points, mode, o, f, r, count: lib.hb_pair_product(ctx.h, tabs, K, points, mode, o, f, r, count, s)
    P, O, F = ctx.ptr(pts), ctx.ptr(out), ctx.ptr(flags)
    Rj = ctypes.c_void_p(flags.data_ptr() + 12)
    for K in (0, 5):
        assert call(K, P, 0, O, None, None, 3) == _capi.HB_ERR_BAD_ARG
    assert call(1, P, 2, O, None, None, 3) == _capi.HB_ERR_BAD_ARG
    assert call(1, P, 0, O, None, None, -1) == _capi.HB_ERR_BAD_ARG
    assert call(1, None, 0, O, None, None, 3) == _capi.HB_ERR_BAD_ARG
    assert call(1, P, 0, None, None, None, 3) == _capi.HB_ERR_BAD_ARG
    assert call(1, P, 1, None, F, None, 3) == _capi.HB_ERR_BAD_ARG
    assert call(1, P, 0, P, None, None, 3) == _capi.HB_ERR_BAD_ARG                 # out overlaps the points
    assert call(1, P, 1, None, P, Rj, 3) == _capi.HB_ERR_BAD_ARG
    assert call(1, P, 1, None, F, F, 3) == _capi.HB_ERR_BAD_ARG                    # the counter inside the verdicts
    assert lib.hb_pair_product(ctx.h, None, 1, P, 0, O, None, None, 3, s) == _capi.HB_ERR_BAD_ARG
    assert call(1, None, 0, None, None, None, 0) == _capi.HB_OK                    # nothing to do, nothing launched
    co = ps.coeff_words(G2.generator())
    tab = ctx.torch.empty_like(p0.table)
    assert lib.hb_pair_prepare(ctx.h, co.ctypes.data, 203, ctx.ptr(tab), s) == _capi.HB_ERR_BAD_ARG
    bad = co.copy()
    bad[0] = ps.s.words([ps.Q], 6)[0]
    assert lib.hb_pair_prepare(ctx.h, bad.ctypes.data, 204, ctx.ptr(tab), s) == _capi.HB_ERR_BAD_ARG
    assert lib.hb_pair_prepare(ctx.h, co.ctypes.data, 204, ctx.ptr(tab), s) == _capi.HB_OK and ctx.torch.equal(tab, p0.table)
    host = ps.host_table(G2.generator())
    assert np.array_equal(tab.cpu().numpy().view(np.uint64), host)

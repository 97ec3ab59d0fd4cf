"""GPU: multi-scalar multiplication in G1 (csrc/hb_msm.hip) through honeybadgermpc_amd.g1.msm, interpolate_at and interpolate_g1_at_x,
against the Python-int model of g1_msm_support and bit-equal to hb_selftest_g1_msm (the kernels' per-lane steps on the host) on the same
inputs.  Exact equality of affine words; the workspace's partials are never compared (their representation depends on the order the LDS
atomics were served in).

Reference parity: the reference's interpolate_g1_at_x (betterpairing.py:800) needs its pairing extension, which cannot be imported
where this suite is built; the Python-int model and the host G1 product of powers stand in for it."""
import random

import numpy as np
import pytest

import g1_msm_support as ms
import g1_support as s
from g1_msm_support import BUCKET, DIRECT

from honeybadgermpc_amd.bls12_381 import G1, R

pytestmark = pytest.mark.gpu

METHODS = ["direct", "bucket", "auto"]
CODE = {"direct": DIRECT, "bucket": BUCKET, "auto": 0}


@pytest.fixture(scope="module")
def ctx():
    from honeybadgermpc_amd._capi import Context

    return Context.get(R)


def dev_points(ctx, arr, *shape):
    return ctx.torch.from_numpy(np.ascontiguousarray(arr).view(np.int64).reshape(*shape, 2, 6)).to(ctx.tdev)


def dev_scalars(ctx, rows):
    M, K = len(rows), len(rows[0]) if rows else 0
    flat = s.words([v for row in rows for v in row], 4) if M * K else np.zeros((0, 4), dtype=np.uint64)
    return ctx.torch.from_numpy(flat.view(np.int64).reshape(M, K, 4)).to(ctx.tdev)


def host(t):
    return t.cpu().numpy().view(np.uint64).reshape(-1, 12)


def device_msm(ctx, scalars, pts, method, chunk=None, per_row=False):
    from honeybadgermpc_amd import g1

    M, K = len(scalars), len(scalars[0])
    dp = dev_points(ctx, pts, M, K) if per_row else dev_points(ctx, pts, K)
    out = g1.msm(ctx, dev_scalars(ctx, scalars), dp, method=method, chunk=chunk)
    assert tuple(out.shape) == (M, 2, 6)
    return host(out)


def check(ctx, scalars, pts, want, method, chunk=None, per_row=False):
    got = device_msm(ctx, scalars, pts, method, chunk, per_row)
    rc, ref = ms.selftest(scalars, pts, len(scalars), len(scalars[0]), CODE[method], chunk or 0, per_row)
    assert rc == 0 and np.array_equal(got, ref), (method, chunk)
    assert np.array_equal(got, want), (method, chunk)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("K", [1, 2, 255, 256, 257])
def test_rows_of_k_terms(ctx, method, K):
    M = 3 if K != 256 else 1
    per_row = K in (2, 257)
    scalars, logs, pts = ms.random_case(M, K, seed=K + M, per_row=per_row)
    check(ctx, scalars, pts, ms.model_logs(scalars, logs, per_row), method, per_row=per_row)


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("K", [1, 63, 64, 65, 129])
def test_bucket_path_at_chunk_64(ctx, M, K):
    per_row = K in (63, 129)
    scalars, logs, pts = ms.random_case(M, K, seed=100 + K + M, per_row=per_row)
    check(ctx, scalars, pts, ms.model_logs(scalars, logs, per_row), "bucket", 64, per_row)


def test_no_terms_and_no_rows(ctx):
    from honeybadgermpc_amd import g1

    torch = ctx.torch
    for method in METHODS:
        out = torch.full((3, 2, 6), 7, dtype=torch.int64, device=ctx.tdev)
        sc = torch.empty((3, 0, 4), dtype=torch.int64, device=ctx.tdev)
        assert g1.msm(ctx, sc, torch.empty((0, 2, 6), dtype=torch.int64, device=ctx.tdev), out=out, method=method) is out
        assert not out.cpu().numpy().any()
        sc = torch.empty((0, 5, 4), dtype=torch.int64, device=ctx.tdev)
        assert g1.msm(ctx, sc, dev_points(ctx, ms.log_points([1, 2, 3, 4, 5]), 5), method=method).shape == (0, 2, 6)


@pytest.mark.parametrize("name", ["all-zero rows", "all-equal scalars", "every byte 255", "single top byte", "identity bases", "all bases the identity",
                                  "one base repeated", "P and -P"])
def test_special_inputs(ctx, name):
    scalars, _, pts, want = ms.special_cases()[name]
    for method, chunk in (("bucket", 64), ("bucket", None), ("direct", None), ("auto", None)):
        got = device_msm(ctx, scalars, pts, method, chunk)
        assert np.array_equal(got, want), (name, method, chunk)
    rc, ref = ms.selftest(scalars, pts, len(scalars), len(scalars[0]), BUCKET, 64)
    assert rc == 0 and np.array_equal(ref, want)


def test_generic_bases_against_the_host_product(ctx):
    scalars, pts, want = ms.generic_case()
    for method, chunk in (("direct", None), ("bucket", None), ("bucket", 64), ("auto", None)):
        check(ctx, scalars, pts, want, method, chunk)


def test_default_chunk_edge(ctx):
    """K = the default chunk + 1: the second chunk of every window holds ONE term; also the all-equal row at the default chunk, whose
    every window is one heavy bucket of 4096 entries"""
    from honeybadgermpc_amd import g1

    K = g1.MSM_CHUNK + 1
    rnd = random.Random(41)
    logs = [1 + k % 999 for k in range(K)]
    scalars = [[rnd.randrange(1 << 256) for _ in range(K)]]
    scalars[0][-1] = (1 << 256) - 1
    pts = ms.log_points(logs)
    check(ctx, scalars, pts, ms.model_logs(scalars, logs), "bucket")
    equal = [[0xA5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A501] * K]
    assert np.array_equal(device_msm(ctx, equal, pts, "bucket"), ms.model_logs(equal, logs))


def test_out_reuse_and_argument_errors(ctx):
    from honeybadgermpc_amd import g1
    from honeybadgermpc_amd._capi import Context, HbmpcBackendError

    torch = ctx.torch
    scalars, logs, pts = ms.random_case(2, 70, seed=3)
    want = ms.model_logs(scalars, logs)
    sc, dp = dev_scalars(ctx, scalars), dev_points(ctx, pts, 70)
    out = torch.empty((2, 2, 6), dtype=torch.int64, device=ctx.tdev)
    for method in METHODS:
        out.fill_(-1)
        assert g1.msm(ctx, sc, dp, out=out, method=method) is out and np.array_equal(host(out), want)
    # (K, 4) scalars are one row; per-row bases of one row
    assert np.array_equal(host(g1.msm(ctx, sc[1], dp)), want[1:])
    assert np.array_equal(host(g1.msm(ctx, sc[:1], dp.reshape(1, 70, 2, 6))), want[:1])
    wide = torch.empty((2, 2, 12), dtype=torch.int64, device=ctx.tdev)
    with pytest.raises(ValueError, match="out"):
        g1.msm(ctx, sc, dp, out=wide[:, :, :6])
    with pytest.raises(ValueError, match="out"):
        g1.msm(ctx, sc, dp, out=torch.empty((3, 2, 6), dtype=torch.int64, device=ctx.tdev))
    with pytest.raises(ValueError, match="method"):
        g1.msm(ctx, sc, dp, method="pippenger")
    for chunk in (32, 100, 8192, 64.0, True):
        with pytest.raises(ValueError, match="chunk"):
            g1.msm(ctx, sc, dp, chunk=chunk)
    with pytest.raises(ValueError, match="scalars"):
        g1.msm(ctx, sc[:, :69], dp)
    with pytest.raises(ValueError, match="scalars and points"):
        g1.msm(ctx, sc, dp.reshape(1, 70, 2, 6))
    with pytest.raises(ValueError, match="points"):
        g1.msm(ctx, sc, dp.reshape(70 * 2, 6))
    with pytest.raises(TypeError, match="scalars"):
        g1.msm(ctx, sc.to(torch.int32), dp)
    with pytest.raises(ValueError, match="ctx"):
        g1.msm(Context.get((1 << 255) - 19), sc, dp)
    # the C ABI: aliasing, the workspace, null pointers, method and chunk
    lib, stream = ctx.lib, ctx.stream()
    need = lib.hb_g1_msm_workspace_bytes(2, 70, 2, 0)
    ws = torch.empty((need // 8,), dtype=torch.int64, device=ctx.tdev)

    def call(s_t, p_t, out_t, method=2, chunk=0, w=ws, nbytes=need, rows=2, terms=70):
        return lib.hb_g1_msm(ctx.h, ctx.ptr(s_t), ctx.ptr(p_t), 0, ctx.ptr(out_t) if out_t is not None else None, rows, terms, method, chunk,
                             ctx.ptr(w) if w is not None else None, nbytes, stream)

    ctx.check(call(sc, dp, out), "hb_g1_msm")
    assert np.array_equal(host(out), want)
    for rc in (call(sc, dp, sc), call(sc, dp, dp), call(sc, dp, dp[35:]), call(sc, dp, ws), call(sc, dp, out, nbytes=need - 8), call(sc, dp, out, w=None),
               call(sc, dp, None), call(sc, dp, out, method=3), call(sc, dp, out, chunk=96), call(sc, dp, out, rows=-1), call(sc, dp, out, terms=-1)):
        assert rc == 2
        with pytest.raises(HbmpcBackendError, match="hb_g1_msm"):
            ctx.check(rc, "hb_g1_msm")
    assert np.array_equal(host(out), want)                    # a refused call writes nothing


def test_interpolate_at_the_reference_shape(ctx):
    """nodes 0 .. K - 1, targets 0 .. n - 1, K = 22, n = 4 (hbavss.py:499-512): node targets return the input points word for word"""
    from honeybadgermpc_amd import g1

    K, n = 22, 4
    rnd = random.Random(8)
    a, b = rnd.randrange(1, 40), rnd.randrange(1, 20)
    f = lambda x: a + b * x + x * x                                       # below 1000 on the nodes: vectors()[f(x)] = f(x) g
    logs = [f(x) for x in range(K)]
    assert max(logs) < 1000
    pts = ms.log_points(logs)
    dp = dev_points(ctx, pts, K)
    got = host(g1.interpolate_at(ctx, range(K), dp, range(n)))
    assert np.array_equal(got, pts[:n])
    # beyond the nodes, and a negative target: f continues as a polynomial over GF(R)
    targets = [K, 1000, R - 1, -2, 5]
    g = G1.generator()
    out = ctx.torch.empty((len(targets), 2, 6), dtype=ctx.torch.int64, device=ctx.tdev)
    assert g1.interpolate_at(ctx, range(K), dp, targets, out=out) is out
    assert s.unpoints(host(out)) == [g ** (f(t) % R) for t in targets]
    # general nodes: a quadratic through opaque values
    xs = [9, 2, 30, 4, 11]
    q = lambda x: (3 + 5 * x + 7 * x * x) % R
    qp = s.points([g ** q(x) for x in xs])
    assert s.unpoints(host(g1.interpolate_at(ctx, xs, dev_points(ctx, qp, 5), [0, 30, 77]))) == [g ** q(t) for t in (0, 30, 77)]
    with pytest.raises(ValueError, match="points"):
        g1.interpolate_at(ctx, range(K - 1), dp, [0])


def test_interpolate_g1_at_x_unsorted_with_an_order(ctx):
    """the reference's semantics: sort by x, take the first `order` coordinates; against the host product of powers with the weights of
    the reference's lagrange_at_x (g1_msm_support.lagrange_definition)"""
    from honeybadgermpc_amd import g1

    rnd = random.Random(12)
    vs = s.vectors()
    h = G1.rand("h")
    coords = [(x, vs[rnd.randrange(1, 1000)] * h ** x) for x in (7, 2, 11, 5, 3, 1)]
    for order, x in ((4, 0), (-1, 9), (6, 7), (1, 100)):
        used = sorted(coords, key=lambda c: c[0])[:order if order != -1 else len(coords)]
        w = ms.lagrange_definition([c[0] for c in used], [x])[0]
        want = G1.one()
        for wk, (_, p) in zip(w, used):
            want = want * p ** wk
        got = g1.interpolate_g1_at_x(coords, x, order, ctx=ctx)
        assert isinstance(got, G1) and got == want, (order, x)
    assert g1.interpolate_g1_at_x(coords, 5) == dict(coords)[5]
    assert g1.interpolate_g1_at_x([], 5, ctx=ctx) == G1.one()


def test_msm_against_the_composed_schedule(ctx):
    """scalar_mul on the expanded operands, then add in a loop: what a caller did before msm existed"""
    from honeybadgermpc_amd import g1

    M, K = 2, 33
    scalars, _, pts = ms.random_case(M, K, seed=21)
    sc, dp = dev_scalars(ctx, scalars), dev_points(ctx, pts, K)
    terms = g1.scalar_mul(ctx, sc.reshape(M * K, 4), dp.repeat(M, 1, 1)).reshape(M, K, 2, 6)
    acc = terms[:, 0].contiguous()
    for k in range(1, K):
        acc = g1.add(ctx, acc, terms[:, k].contiguous())
    for method in METHODS:
        assert ctx.torch.equal(g1.msm(ctx, sc, dp, method=method), acc), method

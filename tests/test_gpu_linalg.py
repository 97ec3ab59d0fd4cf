"""GPU: products of share matrices (honeybadgermpc_amd.linalg over csrc/hb_mat.hip).  The kernel through linalg.matmul and linalg.dot
against Python ints at every arithmetic and tile boundary, with all three epilogues, the split over the inner dimension at and around
its threshold, and -- where hb_matvec accepts the shape -- against hb_matrix_from_host + hb_matvec, an independent route; then the two
protocols, the matrix-triple generator and the fixed-point product with n parties in one process over an in-process tagged network,
checked on Python ints: the opened product, the degree of every party's output, the number of opened elements.  Exact equality."""
import asyncio
import ctypes
import random

import numpy as np
import pytest

from conftest import BLS

pytestmark = pytest.mark.gpu

P64 = (1 << 64) - 59
P256 = (1 << 256) - 189
FIELDS = [BLS, P256, P64, 13]
FIELD_IDS = ["bls", "2^256-189", "2^64-59", "13"]
NONE, ADD, SUB = "none", "add", "sub"


def _ctx(p):
    from honeybadgermpc_amd._capi import Context

    return Context.get(p)


def _random_tensor(ctx, seed, count):
    g = np.random.default_rng(seed)
    limbs = g.integers(-(1 << 63), (1 << 63) - 1, size=(max(count, 0), ctx.n_limbs), dtype=np.int64, endpoint=True)
    return ctx.reduce_(ctx.to_device(limbs))


def _generator(seed):
    import torch

    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return g


def _sums(a, b, batch, m, k, n):
    """the integer products, unreduced: [batch m n]"""
    out = []
    for bt in range(batch):
        cols = [[b[(bt * k + l) * n + j] for l in range(k)] for j in range(n)]
        for i in range(m):
            row = a[(bt * m + i) * k:(bt * m + i + 1) * k]
            out += [sum(x * y for x, y in zip(row, col)) for col in cols]
    return out


def _apply(p, sums, c, op):
    return [(s + (v if op == ADD else -v if op == SUB else 0)) % p for s, v in zip(sums, c)]


def _matmul(ctx, a, b, c, op, out=None):
    from honeybadgermpc_amd import linalg

    return linalg.matmul(ctx, a, b, add=c if op == ADD else None, sub=c if op == SUB else None, out=out)


def _case(ctx, seed, batch, m, k, n, fill=None):
    """-> tensors (a, b, c) in matrix shape (batched when batch > 1) and their ints"""
    p, L = ctx.modulus, ctx.n_limbs
    lead = (batch,) if batch > 1 else ()
    if fill is None:
        flat = [_random_tensor(ctx, seed + i, cnt) for i, cnt in enumerate((batch * m * k, batch * k * n, batch * m * n))]
    else:
        flat = [ctx.upload_ints([fill] * cnt) if cnt else ctx.empty(0) for cnt in (batch * m * k, batch * k * n, batch * m * n)]
    ints = [ctx.download_ints(t) if t.shape[0] else [] for t in flat]
    shapes = (lead + (m, k, L), lead + (k, n, L), lead + (m, n, L))
    return [t.view(s) for t, s in zip(flat, shapes)], ints


def _check_all_epilogues(ctx, seed, batch, m, k, n, fill=None):
    p = ctx.modulus
    (a, b, c), (ai, bi, ci) = _case(ctx, seed, batch, m, k, n, fill)
    keep = [t.clone() for t in (a, b, c)]
    sums = _sums(ai, bi, batch, m, k, n)
    outs = {}
    for op in (NONE, ADD, SUB):
        got = _matmul(ctx, a, b, c, op)
        assert tuple(got.shape) == tuple(c.shape)
        assert ctx.download_ints(got.view(-1, ctx.n_limbs)) == _apply(p, sums, ci, op), (batch, m, k, n, op)
        outs[op] = got
    for op in (ADD, SUB):                                                 # out over c
        cc = c.clone()
        assert _matmul(ctx, a, b, cc, op, out=cc) is cc and ctx.torch.equal(cc, outs[op]), (batch, m, k, n, op)
    assert all(ctx.torch.equal(x, y) for x, y in zip((a, b, c), keep)), "inputs were written"
    return a, b, ai, bi, outs[NONE]


def _matvec_route(ctx, a_ints, m, k, b, n):
    """a b by the route that was there before: the left factor as a host-built table, the right one as n columns of a mat-vec"""
    from honeybadgermpc_amd._capi import HbView, np_ptr

    host = ctx.host_elems(a_ints)
    h = ctypes.c_void_p()
    ctx.check(ctx.lib.hb_matrix_from_host(ctx.h, np_ptr(host), m, k, ctypes.byref(h), ctx.stream()), "hb_matrix_from_host")
    out = ctx.empty(m * n)
    view = HbView(1, n)                                                    # element (column j, row l) at l n + j, in and out
    try:
        ctx.check(ctx.lib.hb_matvec(ctx.h, h, ctx.ptr(b), view, None, ctx.ptr(out), view, n, ctx.stream()), "hb_matvec")
        ctx.torch.cuda.synchronize()
    finally:
        ctx.lib.hb_matrix_destroy(h)
    return out.view(m, n, ctx.n_limbs)


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", FIELDS, ids=FIELD_IDS)
def test_matmul_against_python_ints(p):
    from honeybadgermpc_amd import linalg

    ctx = _ctx(p)
    G, L = linalg.LAZY_GROUP[ctx.n_limbs], linalg.LAZY_L[ctx.n_limbs]
    TM, TN, TK = linalg.TILE_M, linalg.TILE_N, linalg.TILE_K
    for e, k in enumerate(sorted({1, G - 1, G, G + 1, L - 1, L, L + 1, 2 * L, 4 * L + 3, TK - 1, TK + 1})):
        _check_all_epilogues(ctx, 10 * e, 1, 2 + e % 2, k, 3 - e % 2)
    for e, (batch, m, k, n) in enumerate(((1, 1, 1, 1), (1, 1, 29, 1), (1, 3, 7, 5), (1, TM + 1, L + 1, TN - 1), (1, 65, 57, 63), (3, 5, 9, 4), (1, 2, 1, 300))):
        a, b, ai, bi, plain = _check_all_epilogues(ctx, 1000 + 10 * e, batch, m, k, n)
        if batch == 1 and (m, k, n) != (1, 1, 1):
            assert ctx.torch.equal(_matvec_route(ctx, ai, m, k, b, n), plain), (m, k, n)
    if p in (P256, P64):                                                   # every operand p - 1: the tight case of the reduction
        for k in (L, L + 1, 4 * L):
            _check_all_epilogues(ctx, 0, 1, 2, k, 3, fill=p - 1)


@pytest.mark.parametrize("p", [BLS, P64], ids=["bls", "2^64-59"])
def test_zero_sized_shapes_and_arguments(p):
    from honeybadgermpc_amd import linalg

    ctx = _ctx(p)
    torch, L = ctx.torch, ctx.n_limbs
    for m, k, n in ((0, 3, 2), (2, 3, 0), (0, 0, 0)):
        a, b = ctx.empty(m * k).view(m, k, L), ctx.empty(k * n).view(k, n, L)
        assert tuple(linalg.matmul(ctx, a, b).shape) == (m, n, L)
        assert tuple(linalg.matmul(ctx, a, b, add=ctx.empty(m * n).view(m, n, L)).shape) == (m, n, L)
    c = _random_tensor(ctx, 5, 6).view(2, 3, L)                           # k == 0: 0 (op) C
    a, b = ctx.empty(0).view(2, 0, L), ctx.empty(0).view(0, 3, L)
    ci = ctx.download_ints(c.view(6, L))
    assert ctx.download_ints(linalg.matmul(ctx, a, b).view(6, L)) == [0] * 6
    assert ctx.download_ints(linalg.matmul(ctx, a, b, add=c).view(6, L)) == ci
    assert ctx.download_ints(linalg.matmul(ctx, a, b, sub=c).view(6, L)) == [-v % p for v in ci]
    assert tuple(linalg.dot(ctx, ctx.empty(0), ctx.empty(0)).shape) == (1, L) and ctx.download_ints(linalg.dot(ctx, ctx.empty(0), ctx.empty(0))) == [0]
    # shapes that do not fit name the operand
    a, b = _random_tensor(ctx, 1, 6).view(2, 3, L), _random_tensor(ctx, 2, 12).view(3, 4, L)
    for kwargs, word in (({"add": c}, "add"), ({"sub": c.view(6, L)[:5]}, "sub"), ({"out": ctx.empty(7)}, "out")):
        with pytest.raises(ValueError, match=word):
            linalg.matmul(ctx, a, b, **kwargs)
    with pytest.raises(ValueError, match="b"):
        linalg.matmul(ctx, a, b.view(4, 3, L))
    with pytest.raises(ValueError, match="b"):
        linalg.matmul(ctx, a, b.view(1, 3, 4, L))
    with pytest.raises(ValueError, match="a"):
        linalg.matmul(ctx, a.view(6, L), b)
    with pytest.raises(ValueError, match="mutually exclusive"):
        linalg.matmul(ctx, a, b, add=ctx.empty(8), sub=ctx.empty(8))
    with pytest.raises(ValueError, match="y"):
        linalg.dot(ctx, a.view(6, L), b.view(12, L))
    with pytest.raises(TypeError):
        linalg.matmul(ctx, a.cpu().numpy(), b)
    sq = _random_tensor(ctx, 3, 9).view(3, 3, L)
    with pytest.raises(ValueError, match="out"):
        linalg.matmul(ctx, sq, sq.clone(), out=sq)
    # the C entry point's own table
    st, P = ctx.stream(), ctx.ptr
    out = ctx.empty(8)
    call = ctx.lib.hb_mat_mul
    assert call(ctx.h, P(a), P(b), None, 0, P(out), 1, 2, 3, 4, st) == 0
    torch.cuda.synchronize()
    good = out.clone()
    assert torch.equal(good.view(2, 4, L), linalg.matmul(ctx, a, b))
    for args in ((P(a), P(b), None, 0, P(a), 1, 2, 3, 4), (P(a), P(b), None, 0, P(b), 1, 2, 3, 4), (None, P(b), None, 0, P(out), 1, 2, 3, 4),
                 (P(a), None, None, 0, P(out), 1, 2, 3, 4), (P(a), P(b), None, 0, None, 1, 2, 3, 4), (P(a), P(b), None, 0, P(out), -1, 2, 3, 4),
                 (P(a), P(b), None, 0, P(out), 1, -2, 3, 4), (P(a), P(b), None, 0, P(out), 1, 2, -3, 4), (P(a), P(b), None, 0, P(out), 1, 2, 3, -4),
                 (P(a), P(b), None, 3, P(out), 1, 2, 3, 4), (P(a), P(b), None, -1, P(out), 1, 2, 3, 4), (P(a), P(b), None, 1, P(out), 1, 2, 3, 4),
                 (P(a), P(b), None, 2, P(out), 1, 2, 3, 4)):
        assert call(ctx.h, *args, st) == 2, args[3:]
    assert call(ctx.h, None, None, None, 0, None, 0, 2, 3, 4, st) == 0 and call(ctx.h, None, None, None, 0, None, 1, 0, 3, 4, st) == 0
    assert call(None, P(a), P(b), None, 0, P(out), 1, 2, 3, 4, st) == 2
    torch.cuda.synchronize()
    assert torch.equal(out, good), "a refused call launched"


@pytest.mark.parametrize("p", [BLS, P64], ids=["bls", "2^64-59"])
def test_dot_and_the_split_threshold(p):
    from honeybadgermpc_amd import linalg

    ctx = _ctx(p)
    torch, L = ctx.torch, ctx.n_limbs
    T = linalg.SPLIT_MIN_K
    lib = ctx.lib
    for k in (5000, T - 1, T, T + 1):
        x, y = _random_tensor(ctx, k, k), _random_tensor(ctx, k + 1, k)
        xi, yi = ctx.download_ints(x), ctx.download_ints(y)
        want = sum(u * v for u, v in zip(xi, yi)) % p
        assert linalg.takes_split(1, 1, k, 1) == (k >= T)
        got = linalg.dot(ctx, x, y)
        assert tuple(got.shape) == (1, L) and ctx.download_ints(got) == [want], k
        try:                                                              # the other path on the same operands: the same bits
            lib.hb_debug_mat_split(-1 if k >= T else 1)
            assert torch.equal(linalg.dot(ctx, x, y), got), k
        finally:
            lib.hb_debug_mat_split(0)
    # batched vectors, and a batch of matrices whose output is few tiles: slices of one tile depth against the single launch
    x, y = _random_tensor(ctx, 1, 3 * 70).view(3, 70, L), _random_tensor(ctx, 2, 3 * 70).view(3, 70, L)
    xi, yi = ctx.download_ints(x.view(-1, L)), ctx.download_ints(y.view(-1, L))
    want = [sum(u * v for u, v in zip(xi[b * 70:(b + 1) * 70], yi[b * 70:(b + 1) * 70])) % p for b in range(3)]
    assert ctx.download_ints(linalg.dot(ctx, x, y)) == want
    (a, b, c), (ai, bi, ci) = _case(ctx, 77, 2, linalg.TILE_M + 1, 3 * linalg.TILE_K + 5, 5)
    plain = {op: _matmul(ctx, a, b, c, op) for op in (NONE, ADD, SUB)}
    try:
        lib.hb_debug_mat_split(1)
        assert ctx.download_ints(linalg.dot(ctx, x, y)) == want
        for op in (NONE, ADD, SUB):
            assert torch.equal(_matmul(ctx, a, b, c, op), plain[op]), op
            cc = c.clone()
            assert torch.equal(_matmul(ctx, a, b, cc, op, out=cc), plain[op]), op
    finally:
        lib.hb_debug_mat_split(0)
    sums = _sums(ai, bi, 2, linalg.TILE_M + 1, 3 * linalg.TILE_K + 5, 5)
    assert ctx.download_ints(plain[SUB].view(-1, L)) == _apply(p, sums, ci, SUB)


def test_256_cubed_at_sampled_outputs():
    from honeybadgermpc_amd import linalg

    ctx = _ctx(BLS)
    p, L, d = BLS, ctx.n_limbs, 256
    a, b, c = (_random_tensor(ctx, 40 + i, d * d).view(d, d, L) for i in range(3))
    got = linalg.matmul(ctx, a, b, add=c)
    rnd = random.Random(9)
    where = sorted({(0, 0), (d - 1, d - 1), (0, d - 1), (d - 1, 0), (15, 31), (16, 32)} | {(rnd.randrange(d), rnd.randrange(d)) for _ in range(300)})
    rows = {i: ctx.download_ints(a[i]) for i in {i for i, _ in where}}
    cols = {j: ctx.download_ints(b[:, j].contiguous()) for j in {j for _, j in where}}
    idx = ctx.torch.tensor([i * d + j for i, j in where], device=ctx.tdev)
    gi, ci = ctx.download_ints(got.view(-1, L)[idx]), ctx.download_ints(c.view(-1, L)[idx])
    for e, (i, j) in enumerate(where):
        assert gi[e] == (sum(u * v for u, v in zip(rows[i], cols[j])) + ci[e]) % p, (i, j)


def test_side_stream_and_two_contexts_in_turn():
    """the split path's partial products live in a scratch slot per context and stream"""
    import torch

    from honeybadgermpc_amd import linalg

    k = 5000
    ctxs = [_ctx(BLS), _ctx(P64)]
    data = []
    for ctx in ctxs:
        x, y = _random_tensor(ctx, 3, k), _random_tensor(ctx, 4, k)
        data.append((x, y, sum(u * v for u, v in zip(ctx.download_ints(x), ctx.download_ints(y))) % ctx.modulus))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    results = []
    for turn in range(3):
        for ctx, (x, y, _) in zip(ctxs, data):
            results.append(linalg.dot(ctx, x, y))
            with torch.cuda.stream(side):
                results.append(linalg.dot(ctx, x, y))
                a = x[:6 * 7].view(6, 7, ctx.n_limbs)
                results.append(linalg.matmul(ctx, a, y[:7 * 3].view(7, 3, ctx.n_limbs)))
    torch.cuda.synchronize()
    at = 0
    for turn in range(3):
        for ctx, (x, y, want) in zip(ctxs, data):
            assert ctx.download_ints(results[at]) == [want] and ctx.download_ints(results[at + 1]) == [want], (turn, ctx.modulus)
            xi, yi = ctx.download_ints(x[:42]), ctx.download_ints(y[:21])
            assert ctx.download_ints(results[at + 2].view(18, ctx.n_limbs)) == [v % ctx.modulus for v in _sums(xi, yi, 1, 6, 7, 3)]
            at += 3


# ---- the protocols over the in-process tagged network ------------------------------------------------------------------------------
class _TaggedNet:
    """get_send_recv(i)(tag) -> (send, recv) for party i; hook(sender, tag, dest, msg) -> the message that travels"""

    def __init__(self, n, hook=None):
        self.n, self.q, self.hook = n, [dict() for _ in range(n)], hook

    def _queue(self, party, tag):
        return self.q[party].setdefault(tag, asyncio.Queue())

    def get_send_recv(self, i):
        def factory(tag):
            def send(dest, msg):
                self._queue(dest, tag).put_nowait((i, self.hook(i, tag, dest, msg) if self.hook else msg))

            return send, self._queue(i, tag).get

        return factory


def _run_parties(p, n, t, body, hook=None, return_exceptions=False):
    from honeybadgermpc_amd.open_coalescer import OpenCoalescer

    async def main():
        net = _TaggedNet(n, hook)
        work = asyncio.gather(*[body(OpenCoalescer(p, n, t, i, net.get_send_recv(i)), i) for i in range(n)], return_exceptions=return_exceptions)
        return await asyncio.wait_for(work, 20)

    results = asyncio.run(main())
    _ctx(p).torch.cuda.synchronize()
    return results


def _coefficients(ys, p):
    """the polynomial of degree < n through (1, ys[0]) .. (n, ys[n-1]) on Python ints -> n coefficients"""
    n = len(ys)
    out = [0] * n
    for i in range(n):
        num, den = [1], 1
        for j in range(n):
            if j != i:
                num = [(a - (j + 1) * b) % p for a, b in zip([0] + num, num + [0])]
                den = den * (i - j) % p
        scale = ys[i] * pow(den, -1, p) % p
        for e in range(n):
            out[e] = (out[e] + scale * num[e]) % p
    return out


def _check_sharings(p, n, t, per_party):
    """every column of per_party ([party][index] ints) is a sharing of degree <= t -> the constants"""
    secrets = []
    for idx in range(len(per_party[0])):
        ct = _coefficients([per_party[i][idx] for i in range(n)], p)
        assert not any(ct[t + 1:]), idx
        secrets.append(ct[0])
    return secrets


_DEALERS = {}


def _deal(ctx, n, t, degree, values, seed):
    """values: ints (the secrets) -> (n, len(values), limbs): row i = party i's shares, dealt by ShareDealer at `degree`"""
    from honeybadgermpc_amd.offline import ShareDealer

    key = (ctx.modulus, n, t, degree)
    if key not in _DEALERS:
        _DEALERS[key] = ShareDealer(ctx.modulus, n, t, max_polys=1 << 13, device=ctx.device, degree=degree)
    shares, _ = _DEALERS[key].deal_secrets(ctx.upload_ints([v % ctx.modulus for v in values]), _generator(seed))
    return shares.view(n, len(values), ctx.n_limbs)


def _count_opens(co, log):
    inner = co.open_share_array

    def counting(shares, degree=None):
        log.append((len(shares), degree))
        return inner(shares, degree)

    co.open_share_array = counting


@pytest.mark.parametrize("n, t", [(4, 1), (7, 2)])
@pytest.mark.parametrize("m, k, nn", [(1, 1, 1), (3, 5, 2), (4, 29, 4)])
def test_shared_matmul_protocols(n, t, m, k, nn):
    from honeybadgermpc_amd import linalg

    p = BLS
    ctx = _ctx(p)
    L = ctx.n_limbs
    rnd = random.Random(100 * n + m * k)
    xs, ys = [rnd.randrange(p) for _ in range(m * k)], [rnd.randrange(p) for _ in range(k * nn)]
    rs = [rnd.randrange(p) for _ in range(m * nn)]
    ps, qs = [rnd.randrange(p) for _ in range(m * k)], [rnd.randrange(p) for _ in range(k * nn)]
    want = [v % p for v in _sums(xs, ys, 1, m, k, nn)]
    pqs = [v % p for v in _sums(ps, qs, 1, m, k, nn)]
    X, Y = _deal(ctx, n, t, t, xs, 1).view(n, m, k, L), _deal(ctx, n, t, t, ys, 2).view(n, k, nn, L)
    r_t, r_2t = _deal(ctx, n, t, t, rs, 3), _deal(ctx, n, t, 2 * t, rs, 4)
    P, Q, PQ = _deal(ctx, n, t, t, ps, 5).view(n, m, k, L), _deal(ctx, n, t, t, qs, 6).view(n, k, nn, L), _deal(ctx, n, t, t, pqs, 7).view(n, m, nn, L)

    async def body(co, i):
        log = []
        _count_opens(co, log)
        keep = (X[i].clone(), Y[i].clone())
        before = co.batches
        ds = await linalg.double_sharing_matmul(co, X[i], Y[i], r_t[i], r_2t[i])
        ds_batches, ds_log = co.batches - before, list(log)
        del log[:]
        before = co.batches
        bv = await linalg.beaver_matmul(co, X[i], Y[i], (P[i], Q[i], PQ[i]))
        bv_batches, bv_log = co.batches - before, list(log)
        assert tuple(ds.shape) == tuple(bv.shape) == (m, nn, L)
        assert ctx.torch.equal(X[i], keep[0]) and ctx.torch.equal(Y[i], keep[1])
        opened = [ctx.download_ints(await co.open_share_array(v.view(m * nn, L))) for v in (ds, bv)]
        return ctx.download_ints(ds.view(-1, L)), ctx.download_ints(bv.view(-1, L)), opened, (ds_batches, ds_log), (bv_batches, bv_log)

    results = _run_parties(p, n, t, body)
    for which in (0, 1):
        assert _check_sharings(p, n, t, [r[which] for r in results]) == want, which      # every party's output: a degree-t sharing of X Y
    for r in results:
        assert r[2] == [want, want]
        ds_batches, ds_log = r[3]
        bv_batches, bv_log = r[4]
        assert ds_batches == 1 and ds_log == [(m * nn, 2 * t)]
        assert bv_batches == 1 and sorted(bv_log) == sorted([(m * k, None), (k * nn, None)])
        assert sum(c for c, _ in ds_log) == linalg.count_opens(linalg.DOUBLE_SHARING, m, k, nn) == m * nn
        assert sum(c for c, _ in bv_log) == linalg.count_opens(linalg.BEAVER, m, k, nn) == m * k + k * nn
        if (m, k, nn) != (1, 1, 1):
            assert m * k * nn not in (sum(c for c, _ in ds_log), sum(c for c, _ in bv_log))
    assert linalg.count_triples(linalg.DOUBLE_SHARING, m, k, nn) == linalg.count_triples(linalg.BEAVER, m, k, nn) == 0


@pytest.mark.parametrize("n, t", [(4, 1), (7, 2)])
def test_generate_matrix_triples(n, t):
    from honeybadgermpc_amd import linalg, offline

    p = BLS
    ctx = _ctx(p)
    L = ctx.n_limbs
    m, k, nn, count = 3, 5, 2, 2
    rnd = random.Random(n)
    xs, ys = [rnd.randrange(p) for _ in range(m * k)], [rnd.randrange(p) for _ in range(k * nn)]
    X, Y = _deal(ctx, n, t, t, xs, 11).view(n, m, k, L), _deal(ctx, n, t, t, ys, 12).view(n, k, nn, L)

    async def body(co, i):
        P, Q, PQ = await offline.generate_matrix_triples(co, m, k, nn, count, generator=_generator(700 + i))
        assert tuple(P.shape) == (count, m, k, L) and tuple(Q.shape) == (count, k, nn, L) and tuple(PQ.shape) == (count, m, nn, L) and co.batches == 1
        flat = [v.reshape(-1, L) for v in (P, Q, PQ)]
        handles = [co.open_share_array(v) for v in flat]
        out = [ctx.download_ints(v) for v in flat] + [ctx.download_ints(await h) for h in handles]
        prod = await linalg.beaver_matmul(co, X[i], Y[i], (P[1], Q[1], PQ[1]))       # end to end: the second triple multiplies two dealt matrices
        out.append(ctx.download_ints(await co.open_share_array(prod.view(m * nn, L))))
        return out

    results = _run_parties(p, n, t, body)
    for part in range(3):
        assert _check_sharings(p, n, t, [r[part] for r in results]) == results[0][3 + part]       # all three of degree t
    for r in results:
        assert r[3:6] == results[0][3:6]
        ps, qs, pqs = r[3:6]
        assert pqs == [v % p for v in _sums(ps, qs, count, m, k, nn)]
        assert r[6] == [v % p for v in _sums(xs, ys, 1, m, k, nn)]
    assert len(set(results[0][3] + results[0][4])) == count * (m * k + k * nn)


def test_generate_matrix_triples_aborts_with_randousha():
    """an "A" verdict from a checker: every party raises HoneyBadgerMPCError, and none waits for a message that will not come"""
    from honeybadgermpc_amd import offline
    from honeybadgermpc_amd.exceptions import HoneyBadgerMPCError

    p, n, t = BLS, 7, 2

    def hook(sender, tag, dest, msg):
        return "A" if tag[-1] == "H3" and sender == n - 1 else msg

    async def body(co, i):
        return await offline.generate_matrix_triples(co, 2, 3, 2, generator=_generator(40 + i))

    results = _run_parties(p, n, t, body, hook, return_exceptions=True)
    assert all(isinstance(r, HoneyBadgerMPCError) for r in results), results


@pytest.mark.parametrize("m, inner, nn", [(2, 3, 2), (4, 28, 4)])
def test_fixedpoint_matmul(m, inner, nn):
    from honeybadgermpc_amd import linalg
    from honeybadgermpc_amd.progs import fixedpoint as fx

    p, n, t = BLS, 4, 1
    ctx = _ctx(p)
    L = ctx.n_limbs
    f, k, kappa = fx.F, fx.K, fx.KAPPA
    rnd = random.Random(m * inner)
    top = (1 << (k - 1)) - 1
    xs = ([top, -top, top, -top, 0, 1, -1] + [rnd.randrange(-top, top + 1) for _ in range(m * inner)])[:m * inner]
    ys = ([top, top, -top, -top, -1, 0, 1] + [rnd.randrange(-top, top + 1) for _ in range(inner * nn)])[:inner * nn]
    if inner == 28:                                                        # one output is the largest sum there is: inner products of two extremes
        xs[:inner] = [top] * inner
        ys[0::nn] = [top] * inner
        xs[inner:2 * inner] = [-top] * inner
    exact = _sums(xs, ys, 1, m, inner, nn)
    assert inner != 28 or (exact[0] == inner * top * top and exact[nn] == -inner * top * top)
    count = m * nn
    width = fx.matmul_width(k, inner)
    assert width == 2 * k + (2 if inner == 3 else 5)
    bit_rows = [[rnd.getrandbits(1) for _ in range(count)] for _ in range(width + kappa)]
    bit_rows[0] = [1] * count
    bits = _deal(ctx, n, t, t, [v for row in bit_rows for v in row], 21).view(n, width + kappa, count, L)
    X, Y = _deal(ctx, n, t, t, xs, 22).view(n, m, inner, L), _deal(ctx, n, t, t, ys, 23).view(n, inner, nn, L)
    rs, ps, qs = ([rnd.randrange(p) for _ in range(c)] for c in (count, m * inner, inner * nn))
    r_t, r_2t = _deal(ctx, n, t, t, rs, 24), _deal(ctx, n, t, 2 * t, rs, 25)
    pqs = [v % p for v in _sums(ps, qs, 1, m, inner, nn)]
    P, Q, PQ = _deal(ctx, n, t, t, ps, 26).view(n, m, inner, L), _deal(ctx, n, t, t, qs, 27).view(n, inner, nn, L), _deal(ctx, n, t, t, pqs, 28).view(n, m, nn, L)

    async def body(co, i):
        log, out = [], []
        _count_opens(co, log)
        for method, prep in ((linalg.DOUBLE_SHARING, (r_t[i], r_2t[i])), (linalg.BEAVER, (P[i], Q[i], PQ[i]))):
            before = co.batches
            z = await fx.matmul(co, X[i], Y[i], prep, bits[i], method, f, k, kappa)
            assert tuple(z.shape) == (m, nn, L) and co.batches - before == 2
            out.append(list(log))
            del log[:]
            out.append(ctx.download_ints(await co.open_share_array(z.view(count, L))))
            del log[:]
        A, B = fx.FixedPointArray(co, X[i].view(-1, L), f, k, kappa), fx.FixedPointArray(co, Y[i].view(-1, L), f, k, kappa)
        out.append(ctx.download_ints(await co.open_share_array((await A.matmul(B, m, inner, nn, (r_t[i], r_2t[i]), bits[i], linalg.DOUBLE_SHARING)).shares)))
        # a width that does not fit the modulus: refused before anything is opened
        del log[:]
        opens = co.opens
        for method, prep in ((linalg.DOUBLE_SHARING, (r_t[i], r_2t[i])), (linalg.BEAVER, (P[i], Q[i], PQ[i]))):
            with pytest.raises(ValueError):
                await fx.matmul(co, X[i], Y[i], prep, bits[i], method, f, 110, kappa)
        with pytest.raises(ValueError):
            await fx.matmul(co, X[i], Y[i], (r_t[i], r_2t[i]), bits[i], "guess", f, k, kappa)
        with pytest.raises(ValueError):
            await fx.matmul(co, X[i], Y[i], (r_t[i], r_2t[i]), bits[i], linalg.BEAVER, f, k, kappa)
        with pytest.raises(ValueError):
            await fx.matmul(co, X[i], Y[i], (r_t[i], r_2t[i]), bits[i][:width], linalg.DOUBLE_SHARING, f, k, kappa)
        assert log == [] and co.opens == opens
        return out

    results = _run_parties(p, n, t, body)
    masks = [(sum(bit_rows[i][e] << i for i in range(f)), sum(bit_rows[f + i][e] << i for i in range(width + kappa - f))) for e in range(count)]
    want = [fx.trunc_pr_model(v % p, *masks[e], p, width, f, kappa) for e, v in enumerate(exact)]
    for e, v in enumerate(exact):                                          # the model's own meaning: the product over 2^f, rounded up or down
        signed = want[e] if want[e] < p // 2 else want[e] - p
        assert signed in (v >> f, (v >> f) + 1)
    for r in results:
        assert r[1] == want and r[3] == want and r[4] == want
        assert r[0] == [(count, 2 * t), (count, None)]                     # m n opened for the product, m n for the truncation
        assert sorted(r[2][:2]) == sorted([(m * inner, None), (inner * nn, None)]) and r[2][2:] == [(count, None)]

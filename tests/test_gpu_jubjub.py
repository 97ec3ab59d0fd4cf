"""GPU: honeybadgermpc_amd.progs.jubjub and progs.mimc_jubjub_pkc -- the kernels of csrc/hb_jj.hip against tests/golden/jubjub.json (the
reference's own Point and mimc_plain), the host model and Python ints, the addition of shared points against the same addition composed
from share_arithmetic, and the protocols over an OpenCoalescer (shared_add, share_mul, key_generation, mimc_encrypt -> mimc_decrypt).
Exact equality everywhere."""
import asyncio
import json
import math
import os
import random

import pytest

from conftest import BLS, REPO

from honeybadgermpc_amd.elliptic_curve import Ideal, Jubjub, Point

pytestmark = pytest.mark.gpu

P64 = (1 << 64) - 59
COUNTS = [1, 255, 256, 257]


def _ctx(p):
    from honeybadgermpc_amd._capi import Context

    return Context.get(p)


_CACHE = {}


def _golden():
    if "g" not in _CACHE:
        with open(os.path.join(REPO, "tests", "golden", "jubjub.json")) as f:
            _CACHE["g"] = json.load(f)
    return _CACHE["g"]


def _xy(v):
    return int(v[0]), int(v[1])


def _curve(p):
    return Jubjub() if p == BLS else Jubjub(-1, 2, p)


def _pool(p):
    """a pool of curve points, computed once: the golden points over BLS12-381 Fr; multiples of a found point over 2^64 - 59"""
    if p not in _CACHE:
        curve = _curve(p)
        if p == BLS:
            g = _golden()
            pts = {_xy(c[k]) for c in g["adds"] for k in ("P", "Q", "sum")} | {_xy(c["out"]) for c in g["muls"]}
            _CACHE[p] = [Point(x, y, curve) for x, y in sorted(pts)]
        else:
            x = 2
            while True:                                            # y^2 = (1 + x^2) / (1 - d x^2); p = 5 mod 8: Atkin's square root
                y2 = (1 + x * x) * pow(1 - curve.d * x * x, -1, p) % p
                if pow(y2, (p - 1) // 2, p) == 1:
                    break
                x += 1
            assert p % 8 == 5
            v = pow(2 * y2, (p - 5) // 8, p)
            i = 2 * y2 * v * v % p
            base = Point(x, y2 * v * (i - 1) % p, curve)
            pts, cur = [Point(0, 1, curve), Point(0, -1, curve)], base
            for _ in range(40):
                pts.append(cur)
                cur = cur + base
            _CACHE[p] = pts
    return _CACHE[p]


def _upload_points(ctx, pts):
    return ctx.upload_ints([q.x for q in pts]), ctx.upload_ints([q.y for q in pts])


def _download_points(ctx, pair):
    return list(zip(ctx.download_ints(pair[0]), ctx.download_ints(pair[1])))


# ---- the cleartext kernels ------------------------------------------------------------------------------------------------
def test_scalar_mul_equals_the_golden_file():
    from honeybadgermpc_amd.progs import jubjub

    ctx = _ctx(BLS)
    g = _golden()
    for c in g["muls"]:                                             # a host point and an int, sign included
        assert _download_points(ctx, jubjub.scalar_mul(ctx, int(c["n"]), Point(*_xy(c["P"])))) == [_xy(c["out"])]
    pos = [c for c in g["muls"] if int(c["n"]) > 0]
    ns = ctx.upload_ints([int(c["n"]) for c in pos])
    pts = _upload_points(ctx, [Point(*_xy(c["P"])) for c in pos])
    assert _download_points(ctx, jubjub.scalar_mul(ctx, ns, pts)) == [_xy(c["out"]) for c in pos]
    assert _download_points(ctx, jubjub.scalar_mul(ctx, 0, pts)) == [(0, 1)] * len(pos)
    with pytest.raises(ValueError):
        jubjub.scalar_mul(ctx, 3, Ideal(Jubjub()))
    with pytest.raises(ValueError):
        jubjub.scalar_mul(ctx, 3, Point(0, 1, Jubjub(-1, 2, P64)))   # another field's curve
    with pytest.raises(ValueError):
        jubjub.scalar_mul(ctx, ns[:3], pts)
    with pytest.raises(ValueError):
        jubjub.scalar_mul(ctx, BLS, pts)


@pytest.mark.parametrize("p", [BLS, P64], ids=["bls", "2^64-59"])
@pytest.mark.parametrize("count", COUNTS)
def test_scalar_mul_and_double_table_equal_the_host_model(p, count):
    from honeybadgermpc_amd.progs import jubjub

    ctx = _ctx(p)
    curve = _curve(p)
    rnd = random.Random(p % 997 + count)
    pool = _pool(p)
    pts = [rnd.choice(pool) for _ in range(count)]
    ns = [rnd.choice([0, 1, 2, p - 1, rnd.randrange(p), rnd.randrange(p)]) for _ in range(count)]
    ns[-1] = p - 1
    products = {}

    def times(q, n):
        if (q, n) not in products:
            products[q, n] = q * n if n else Point(0, 1, curve)
        return products[q, n].x, products[q, n].y

    n_dev, p_dev = ctx.upload_ints(ns), _upload_points(ctx, pts)
    keep = [t.clone() for t in (n_dev, *p_dev)]
    check = sorted({0, count - 1} | {rnd.randrange(count) for _ in range(12)})
    got = jubjub.scalar_mul(ctx, n_dev, p_dev, curve)
    assert tuple(got[0].shape) == tuple(got[1].shape) == (count, ctx.n_limbs)
    got = _download_points(ctx, got)
    assert [got[i] for i in check] == [times(pts[i], ns[i]) for i in check]
    # one scalar for all (an int, a one-element tensor), one point for all (a host Point, a one-element pair)
    n1, q1 = ns[check[-1]] or 5, pts[check[0]]
    got = _download_points(ctx, jubjub.scalar_mul(ctx, n1, p_dev, curve))
    assert [got[i] for i in check] == [times(pts[i], n1) for i in check]
    assert _download_points(ctx, jubjub.scalar_mul(ctx, ctx.upload_ints([n1]), p_dev, curve)) == got
    got = _download_points(ctx, jubjub.scalar_mul(ctx, n_dev, q1))
    assert [got[i] for i in check] == [times(q1, ns[i]) for i in check]
    assert _download_points(ctx, jubjub.scalar_mul(ctx, n_dev, _upload_points(ctx, [q1]), curve)) == got
    out = (ctx.empty(count), ctx.empty(count))
    res = jubjub.scalar_mul(ctx, n1, p_dev, curve, out=out)
    assert res[0] is out[0] and res[1] is out[1] and [_download_points(ctx, out)[i] for i in check] == [times(pts[i], n1) for i in check]
    # the doubling table: rows of 2^j P
    K = 5
    xs, ys = jubjub.double_table(ctx, p_dev, K, curve)
    assert tuple(xs.shape) == tuple(ys.shape) == (K, count, ctx.n_limbs)
    for j in range(K):
        row = _download_points(ctx, (xs[j], ys[j]))
        assert [row[i] for i in check] == [times(pts[i], 1 << j) for i in check], j
    hx, hy = jubjub.double_table(ctx, q1, K)
    assert tuple(hx.shape) == (K, 1, ctx.n_limbs) and _download_points(ctx, (hx, hy)) == [times(q1, 1 << j) for j in range(K)]
    assert all(ctx.torch.equal(a, b) for a, b in zip((n_dev, *p_dev), keep))
    with pytest.raises(ValueError):
        jubjub.double_table(ctx, p_dev, 0, curve)


# ---- the stage kernels against Python ints ------------------------------------------------------------------------------------
def _beaver(p, d, e, tp, tq, tpq):
    return (d * e + d * tq + e * tp + tpq) % p


@pytest.mark.parametrize("p", [BLS, P64], ids=["bls", "2^64-59"])
@pytest.mark.parametrize("m", COUNTS)
def test_stage_kernels_equal_python_ints(p, m):
    from honeybadgermpc_amd.progs import jubjub

    ctx = _ctx(p)
    curve = _curve(p)
    d = curve.d
    rnd = random.Random(p % 991 + m)

    def draw(count):
        return [rnd.choice([0, 1, p - 1, rnd.randrange(p), rnd.randrange(p), rnd.randrange(p)]) for _ in range(count)]

    big = m + 3                                                       # the triples are a column slice of a larger tensor: no copy, a row stride
    tp, tq, tpq = ([draw(big) for _ in range(9)] for _ in range(3))
    if m == 257:
        tp, tq, tpq = ([[p - 1] * big for _ in range(9)] for _ in range(3))
    full = [ctx.upload_ints([v for row in comp for v in row]).reshape(9, big, ctx.n_limbs) for comp in (tp, tq, tpq)]
    trip = tuple(t[:, 2:2 + m] for t in full)
    tp, tq, tpq = ([row[2:2 + m] for row in comp] for comp in (tp, tq, tpq))
    rx, ry = draw(m), draw(m)
    rs = ctx.upload_ints(rx + ry).reshape(2, m, ctx.n_limbs)
    x1, y1, x2, y2 = (draw(m) for _ in range(4))
    ops = [ctx.upload_ints(v) for v in (x1, y1, x2, y2)]
    keep = [t.clone() for t in ops + full + [rs]]
    A = jubjub.add_mask(ctx, (ops[0], ops[1]), (ops[2], ops[3]), trip)
    assert tuple(A.shape) == (8 * m, ctx.n_limbs)
    want = [[(v - k) % p for v, k in zip(src, mask[k_])] for src, mask, k_ in ((x1, tp, 0), (x2, tq, 0), (y1, tp, 1), (y2, tq, 1), (x1, tp, 2), (y2, tq, 2),
                                                                                   (y1, tp, 3), (x2, tq, 3))]
    assert ctx.download_ints(A) == [v for row in want for v in row]
    Ao = [draw(m) for _ in range(8)]
    B = jubjub.add_stage1(ctx, ctx.upload_ints([v for row in Ao for v in row]), trip, rs)
    prod = [[_beaver(p, Ao[2 * k][i], Ao[2 * k + 1][i], tp[k][i], tq[k][i], tpq[k][i]) for i in range(m)] for k in range(4)]
    want = [[(prod[0][i] - tp[4][i]) % p for i in range(m)], [(prod[1][i] - tq[4][i]) % p for i in range(m)],
            [(prod[2][i] + prod[3][i] - tp[5][i]) % p for i in range(m)], [(rx[i] - tq[5][i]) % p for i in range(m)],
            [(prod[1][i] + prod[0][i] - tp[6][i]) % p for i in range(m)], [(ry[i] - tq[6][i]) % p for i in range(m)]]
    assert ctx.download_ints(B) == [v for row in want for v in row]
    Bo = [draw(m) for _ in range(6)]
    uv, C = jubjub.add_stage2(ctx, ctx.upload_ints([v for row in Bo for v in row]), trip, rs, curve)
    w, u, v = ([_beaver(p, Bo[2 * (k - 4)][i], Bo[2 * (k - 4) + 1][i], tp[k][i], tq[k][i], tpq[k][i]) for i in range(m)] for k in (4, 5, 6))
    assert ctx.download_ints(uv) == u + v
    want = [[(1 + d * w[i] - tp[7][i]) % p for i in range(m)], [(rx[i] - tq[7][i]) % p for i in range(m)],
            [(1 - d * w[i] - tp[8][i]) % p for i in range(m)], [(ry[i] - tq[8][i]) % p for i in range(m)]]
    assert ctx.download_ints(C) == [v_ for row in want for v_ in row]
    Co = [draw(m) for _ in range(4)]
    D = jubjub.add_stage3(ctx, ctx.upload_ints([v_ for row in Co for v_ in row]), trip)
    assert ctx.download_ints(D) == [_beaver(p, Co[2 * (k - 7)][i], Co[2 * (k - 7) + 1][i], tp[k][i], tq[k][i], tpq[k][i]) for k in (7, 8) for i in range(m)]
    sig = [rnd.randrange(1, p) for _ in range(2 * m)]
    uvv = draw(2 * m)
    x3, y3 = jubjub.add_finish(ctx, ctx.upload_ints(sig), ctx.upload_ints(uvv))
    assert ctx.download_ints(x3) + ctx.download_ints(y3) == [a * pow(s, -1, p) % p for a, s in zip(uvv, sig)]
    sig[m - 1] = 0                                                    # a zero sig: counted, not fatal, unless asked
    (x3, y3), zeros = jubjub.add_finish(ctx, ctx.upload_ints(sig), ctx.upload_ints(uvv), check=False)
    assert int(zeros.item()) == 1 and ctx.download_ints(x3)[m - 1] == 0 and ctx.download_ints(y3) == [a * pow(s, -1, p) % p for a, s in zip(uvv[m:], sig[m:])]
    with pytest.raises(ZeroDivisionError):
        jubjub.add_finish(ctx, ctx.upload_ints(sig), ctx.upload_ints(uvv))
    assert all(ctx.torch.equal(a, b) for a, b in zip(ops + full + [rs], keep))


def test_arguments_checked_and_asynchronous():
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd._capi import HB_ERR_BAD_ARG
    from honeybadgermpc_amd.progs import jubjub

    p, m = BLS, 70
    ctx = _ctx(p)
    torch = ctx.torch
    rnd = random.Random(3)
    pool = _pool(p)
    Pp, Qp = [rnd.choice(pool) for _ in range(m)], [rnd.choice(pool) for _ in range(m)]
    P, Q = _upload_points(ctx, Pp), _upload_points(ctx, Qp)
    trip = tuple(ctx.upload_ints([rnd.randrange(p) for _ in range(9 * m)]).reshape(9, m, ctx.n_limbs) for _ in range(3))
    rs = ctx.upload_ints([rnd.randrange(1, p) for _ in range(2 * m)]).reshape(2, m, ctx.n_limbs)
    # consumed on the current stream and on a side stream through other kernels of the library, no synchronise in between
    A = jubjub.add_mask(ctx, P, Q, trip)
    twice = sa.add(ctx, A, A)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        A2 = sa.add(ctx, jubjub.add_mask(ctx, P, Q, trip), 0)
        prod = jubjub.scalar_mul(ctx, 3, P)
        neg_x = sa.neg(ctx, prod[0])
    side.synchronize()
    assert torch.equal(A, A2) and ctx.download_ints(twice) == [2 * v % p for v in ctx.download_ints(A)]
    assert ctx.download_ints(neg_x) == [-(q * 3).x % p for q in Pp]
    bad_calls = [
        lambda: jubjub.add_mask(ctx, P, (Q[0], Q[1][:-1]), trip),
        lambda: jubjub.add_mask(ctx, P, Q, (trip[0], trip[1])),
        lambda: jubjub.add_mask(ctx, P, Q, (trip[0], trip[1], trip[2][:8])),
        lambda: jubjub.add_mask(ctx, P, Q, (trip[0], trip[1], trip[2][:, :5])),
        lambda: jubjub.add_mask(ctx, P, Q, (trip[0], trip[1], trip[2].cpu())),
        lambda: jubjub.add_stage1(ctx, A[:-1], trip, rs),
        lambda: jubjub.add_stage1(ctx, A, trip, rs[:1]),
        lambda: jubjub.add_stage2(ctx, A[:6 * m], trip, rs, Jubjub(-1, 2, P64)),
        lambda: jubjub.add_stage2(ctx, A[:6 * m], trip, rs, Jubjub(1, 5)),          # a = 1: not the reference's law
        lambda: jubjub.add_stage3(ctx, A[:4 * m + 1], trip),
        lambda: jubjub.add_finish(ctx, A[:2 * m + 1], A[:2 * m]),
        lambda: jubjub.add_finish(ctx, A[:2 * m], A[:2 * m - 1]),
        lambda: jubjub.scalar_mul(ctx, 3, P, out=(ctx.empty(m), ctx.empty(m - 1))),
        lambda: jubjub.double_table(ctx, P, -1),
    ]
    for call in bad_calls:
        with pytest.raises(ValueError):
            call()
    for call in (lambda: jubjub.add_mask(ctx, P, Q, (trip[0], trip[1], trip[2].to(torch.int32))), lambda: jubjub.add_mask(ctx, P, 5, trip),
                 lambda: jubjub.add_stage1(ctx, A, trip, [1, 2]), lambda: jubjub.scalar_mul(ctx, 3, P, curve="jubjub"), lambda: jubjub.scalar_mul(ctx, 1.5, P)):
        with pytest.raises(TypeError):
            call()
    # ... and the C ABI refuses what gets past Python
    lib, st, ptr = ctx.lib, ctx.stream(), ctx.ptr
    buf = ctx.empty(8 * m)
    buf.fill_(7)
    seven = buf.clone()
    a_h, d_h = ctx.host_elems([p - 1]), ctx.host_elems([Jubjub().d])
    big = ctx.host_elems([0])
    big[:] = [int.from_bytes(int(p).to_bytes(32, "little")[8 * i:8 * i + 8], "little") for i in range(4)]
    x1, y1, x2, y2 = (ptr(t) for t in (*P, *Q))
    tp, tq, tpq = (ptr(t) for t in trip)
    assert lib.hb_jj_add_mask(ctx.h, x1, y1, x2, y2, tp, tq, m - 1, ptr(buf), m, st) == HB_ERR_BAD_ARG          # row stride below m
    assert lib.hb_jj_add_mask(ctx.h, x1, y1, x2, y2, tp, tq, m, ptr(buf), -1, st) == HB_ERR_BAD_ARG
    assert lib.hb_jj_add_mask(ctx.h, x1, None, x2, y2, tp, tq, m, ptr(buf), m, st) == HB_ERR_BAD_ARG
    assert lib.hb_jj_add_mask(ctx.h, x1, y1, x2, y2, tp, tq, m, None, m, st) == HB_ERR_BAD_ARG
    assert lib.hb_jj_add_stage1(ctx.h, ptr(A), tp, tq, None, m, ptr(rs), ptr(rs), ptr(buf), m, st) == HB_ERR_BAD_ARG
    assert lib.hb_jj_add_stage2(ctx.h, ptr(A), tp, tq, tpq, m, ptr(rs), ptr(rs), None, ptr(buf), ptr(buf), m, st) == HB_ERR_BAD_ARG      # no d
    assert lib.hb_jj_add_stage2(ctx.h, ptr(A), tp, tq, tpq, m, ptr(rs), ptr(rs), big.ctypes.data, ptr(buf), ptr(buf), m, st) == HB_ERR_BAD_ARG
    assert lib.hb_jj_add_stage3(ctx.h, None, tp, tq, tpq, m, ptr(buf), m, st) == HB_ERR_BAD_ARG
    assert lib.hb_jj_add_finish(ctx.h, ptr(A), ptr(A), ptr(buf), ptr(buf), ptr(buf), m, None, st) == HB_ERR_BAD_ARG            # outputs not distinct
    assert lib.hb_jj_scalar_mul(ctx.h, x1, 0, x1, y1, 0, a_h.ctypes.data, None, ptr(buf), ptr(buf[m:]), m, st) == HB_ERR_BAD_ARG
    assert lib.hb_jj_scalar_mul(ctx.h, x1, 0, x1, y1, 0, big.ctypes.data, d_h.ctypes.data, ptr(buf), ptr(buf[m:]), m, st) == HB_ERR_BAD_ARG
    assert lib.hb_jj_scalar_mul(ctx.h, x1, 0, x1, y1, 0, a_h.ctypes.data, d_h.ctypes.data, ptr(buf), ptr(buf), m, st) == HB_ERR_BAD_ARG
    assert lib.hb_jj_double_table(ctx.h, x1, y1, a_h.ctypes.data, 0, ptr(buf), ptr(buf[m:]), ptr(buf[2 * m:]), m, None, st) == HB_ERR_BAD_ARG
    assert lib.hb_jj_add_mask(ctx.h, x1, y1, x2, y2, tp, tq, m, ptr(buf), 0, st) == 0                           # m == 0: nothing launched
    torch.cuda.synchronize()
    assert torch.equal(buf, seven)


# ---- the protocols, end to end over the in-process tagged network of tests/test_gpu_butterfly_network.py ------------------------
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


def _run_parties(p, n, t, bad, rnd, body):
    """every party runs `body(co, i)` over its own OpenCoalescer -> ([result per party], {batches per party})"""
    from honeybadgermpc_amd import wire
    from honeybadgermpc_amd.open_coalescer import OpenCoalescer

    def garble(msg):
        tag, blob = msg
        count = wire.unpack_limbs(blob).shape[0]
        return (tag, wire.pack_ints([rnd.randrange(p) for _ in range(count)], p))

    batches = set()

    async def party(i, net):
        co = OpenCoalescer(p, n, t, i, net.get_send_recv(i, garble if i in bad else None))
        res = await body(co, i)
        batches.add(co.batches)
        return res

    async def main():
        net = _TaggedNet(n)
        return await asyncio.gather(*[party(i, net) for i in range(n)])

    results = asyncio.run(main())
    _ctx(p).torch.cuda.synchronize()
    return results, batches


def _deal_tensor(ctx, rnd, p, n, t, values, shape):
    """-> [party] tensors of `shape` + (limbs,)"""
    dealt = _deal(rnd, p, n, t, values)
    return [ctx.upload_ints(dealt[i]).reshape(*shape, ctx.n_limbs) for i in range(n)]


def _deal_add_preprocessing(ctx, rnd, p, n, t, pairs, zero_r=None):
    """-> [party] of ((p, q, pq), rs): 9 triples and 2 non-zero random values a pair"""
    a = [rnd.randrange(p) for _ in range(9 * pairs)]
    b = [rnd.randrange(p) for _ in range(9 * pairs)]
    r = [rnd.randrange(1, p) for _ in range(2 * pairs)]
    if zero_r is not None:
        r[zero_r] = 0
    comps = [_deal_tensor(ctx, rnd, p, n, t, v, (9, pairs)) for v in (a, b, [x * y % p for x, y in zip(a, b)])]
    rs = _deal_tensor(ctx, rnd, p, n, t, r, (2, pairs))
    return [((comps[0][i], comps[1][i], comps[2][i]), rs[i]) for i in range(n)]


async def _composed_add(co, P, Q, d, triples, rs):
    """the same addition from share_arithmetic alone, line by line as SharedPoint.add reads (progs/jubjub.py:99-113)"""
    from honeybadgermpc_amd import share_arithmetic as sa

    ctx = co.ctx
    (x1, y1), (x2, y2) = P, Q
    tp, tq, tpq = triples

    def tr(k):
        return tp[k], tq[k], tpq[k]

    x_prod = await sa.beaver_multiply_arrays(co, x1, x2, tr(0))
    y_prod = await sa.beaver_multiply_arrays(co, y1, y2, tr(1))
    d_prod = sa.mul(ctx, await sa.beaver_multiply_arrays(co, x_prod, y_prod, tr(2)), d)
    a = await sa.beaver_multiply_arrays(co, x1, y2, tr(3))
    b = await sa.beaver_multiply_arrays(co, y1, x2, tr(4))
    x3 = await sa.divide_share_arrays(co, sa.add(ctx, a, b), sa.add(ctx, d_prod, 1), rs[0], tr(5), tr(6))
    one_minus = sa.add(ctx, sa.neg(ctx, d_prod), 1)
    y3 = await sa.divide_share_arrays(co, sa.add(ctx, y_prod, x_prod), one_minus, rs[1], tr(7), tr(8))
    return x3, y3


@pytest.mark.parametrize("n, t, liars", [(4, 1, 0), (7, 2, 0), (4, 1, 1), (7, 2, 2)])
@pytest.mark.parametrize("m", [1, 20, 257])
def test_shared_add_end_to_end(n, t, liars, m):
    from honeybadgermpc_amd.progs import jubjub

    p = BLS
    ctx = _ctx(p)
    rnd = random.Random(1000 * n + 10 * m + liars)
    bad = set(rnd.sample(range(n), liars))
    honest = [i for i in range(n) if i not in bad]
    g = _golden()
    cases = [(Point(*_xy(c["P"])), Point(*_xy(c["Q"])), _xy(c["sum"])) for c in g["adds"]]
    cases = cases[-m:] if m < len(cases) else cases                  # the golden pairs go first
    pool = _pool(p)
    Ps = [c[0] for c in cases] + [rnd.choice(pool) for _ in range(m - len(cases))]
    Qs = [c[1] for c in cases] + [rnd.choice(pool) for _ in range(m - len(cases))]
    want = [c[2] for c in cases] + [((a + b).x, (a + b).y) for a, b in zip(Ps[len(cases):], Qs[len(cases):])]
    shares = [_deal_tensor(ctx, rnd, p, n, t, v, (m,)) for v in ([q.x for q in Ps], [q.y for q in Ps], [q.x for q in Qs], [q.y for q in Qs])]
    pre = _deal_add_preprocessing(ctx, rnd, p, n, t, m)

    async def fused(co, i):
        ops = [s[i] for s in shares]
        keep = [v.clone() for v in ops + list(pre[i][0]) + [pre[i][1]]]
        x3, y3 = await jubjub.shared_add(co, (ops[0], ops[1]), (ops[2], ops[3]), *pre[i])
        assert all(ctx.torch.equal(a, b) for a, b in zip(ops + list(pre[i][0]) + [pre[i][1]], keep))
        assert tuple(x3.shape) == tuple(y3.shape) == (m, ctx.n_limbs)
        fx, fy = co.open_share_array(x3), co.open_share_array(y3)
        return list(zip(ctx.download_ints(await fx), ctx.download_ints(await fy)))

    results, batches = _run_parties(p, n, t, bad, rnd, fused)
    for i in honest:
        assert results[i] == want, i
    assert batches == {4 + 1}

    async def composed(co, i):
        ops = [s[i] for s in shares]
        x3, y3 = await _composed_add(co, (ops[0], ops[1]), (ops[2], ops[3]), Jubjub().d, *pre[i])
        fx, fy = co.open_share_array(x3), co.open_share_array(y3)
        return list(zip(ctx.download_ints(await fx), ctx.download_ints(await fy)))

    composed_results, _ = _run_parties(p, n, t, bad, rnd, composed)
    for i in honest:
        assert composed_results[i] == results[i], i                   # the opened points: the shares differ by design


def test_shared_neg_sub_double_mul_and_the_narrow_field():
    from honeybadgermpc_amd.progs import jubjub

    p, n, t, m = P64, 4, 1, 33
    ctx = _ctx(p)
    curve = _curve(p)
    rnd = random.Random(64)
    pool = _pool(p)
    Ps, Qs = [rnd.choice(pool) for _ in range(m)], [rnd.choice(pool) for _ in range(m)]
    shares = [_deal_tensor(ctx, rnd, p, n, t, v, (m,)) for v in ([q.x for q in Ps], [q.y for q in Ps], [q.x for q in Qs], [q.y for q in Qs])]
    k = 11
    pairs = 2 + jubjub.shared_mul_pairs(k) + jubjub.shared_mul_pairs(-6)
    pre = _deal_add_preprocessing(ctx, rnd, p, n, t, pairs * m)

    async def body(co, i):
        P, Q = (shares[0][i], shares[1][i]), (shares[2][i], shares[3][i])
        (tp, tq, tpq), rs = pre[i]
        used = 0

        def take(count):
            nonlocal used
            s = slice(used * m, (used + count) * m)
            used += count
            return (tp[:, s], tq[:, s], tpq[:, s]), rs[:, s]

        outs = [await jubjub.shared_sub(co, P, Q, *take(1), curve), await jubjub.shared_double(co, P, *take(1), curve),
                await jubjub.shared_mul(co, P, k, *take(jubjub.shared_mul_pairs(k)), curve), await jubjub.shared_mul(co, Q, -6, *take(jubjub.shared_mul_pairs(-6)), curve),
                await jubjub.shared_mul(co, P, 1, *take(0), curve)]
        with pytest.raises(ValueError):
            await jubjub.shared_mul(co, P, 0, *take(0), curve)
        for bad_triples, bad_rs, error in (((tp, tq), rs, ValueError), (None, rs, ValueError), ((tp, tq, tpq[:8]), rs, ValueError), ((tp, tq, tpq), rs[:, :m], ValueError),
                                           ((tp, tq, tpq), [1, 2], TypeError), ((tp, tq, 5), rs, TypeError)):
            with pytest.raises(error):
                await jubjub.shared_mul(co, P, 3, bad_triples, bad_rs, curve)     # nothing is opened: the batch count below holds
        with pytest.raises(ValueError):
            await jubjub.shared_add(co, P, Q, *take(0))                # the default curve lives over another field
        futures = [co.open_share_array(v) for pair in outs for v in pair]
        opened = [ctx.download_ints(await f) for f in futures]
        return [list(zip(opened[2 * j], opened[2 * j + 1])) for j in range(len(outs))]

    results, batches = _run_parties(p, n, t, set(), rnd, body)
    want = [[((a - b).x, (a - b).y) for a, b in zip(Ps, Qs)], [((a + a).x, (a + a).y) for a in Ps], [((a * k).x, (a * k).y) for a in Ps],
            [((b * -6).x, (b * -6).y) for b in Qs], [(a.x, a.y) for a in Ps]]
    assert all(res == want for res in results)
    assert batches == {4 * pairs + 1}


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("K", [1, 2, 5, 8])
def test_share_mul(K, B):
    from honeybadgermpc_amd.progs import jubjub

    p, n, t = BLS, 4, 1
    ctx = _ctx(p)
    rnd = random.Random(10 * K + B)
    pool = _pool(p)
    host_point = rnd.choice(pool[2:])
    pts = [rnd.choice(pool) for _ in range(B)]
    xs = [rnd.getrandbits(K) | 1 for _ in range(B)]
    xs[0] = (1 << K) - 1
    bit_values = [(xs[i] >> j) & 1 for j in range(K) for i in range(B)]
    bits = _deal_tensor(ctx, rnd, p, n, t, bit_values, (K, B))
    need = max((K - 1) * B, 1)
    pre = [_deal_add_preprocessing(ctx, rnd, p, n, t, need) for _ in range(2)]
    dev_pts = _upload_points(ctx, pts)

    async def body(co, i):
        keep = bits[i].clone()
        one = await jubjub.share_mul(co, bits[i], host_point, *pre[0][i])
        before = co.batches
        per = await jubjub.share_mul(co, bits[i], dev_pts, *pre[1][i])
        assert co.batches - before == 4 * math.ceil(math.log2(K)) == before and ctx.torch.equal(bits[i], keep)
        assert tuple(one[0].shape) == tuple(per[1].shape) == (B, ctx.n_limbs)
        with pytest.raises(ValueError):
            await jubjub.share_mul(co, bits[i], Ideal(Jubjub()), *pre[0][i])
        if K > 1:
            with pytest.raises(ValueError):
                await jubjub.share_mul(co, bits[i], host_point, tuple(v[:, :need - 1] for v in pre[0][i][0]), pre[0][i][1])
        futures = [co.open_share_array(v) for v in (*one, *per)]
        o = [ctx.download_ints(await f) for f in futures]
        return list(zip(o[0], o[1])), list(zip(o[2], o[3]))

    results, batches = _run_parties(p, n, t, set(), rnd, body)
    want_one = [((host_point * x).x, (host_point * x).y) for x in xs]
    want_per = [((q * x).x, (q * x).y) for q, x in zip(pts, xs)]
    assert all(res == (want_one, want_per) for res in results)
    assert batches == {2 * 4 * math.ceil(math.log2(K)) + 1}


def test_key_generation_encrypt_and_decrypt():
    """K = 32 bit shares of the golden private keys: key_generation opens the golden public key, mimc_encrypt reproduces the golden
    ciphertexts (the reference's mimc_encrypt lines on its own Point and mimc_plain), mimc_decrypt opens to the messages: 3 blocks, the
    full 161 rounds, n = 4 -- one client with a host point, then all four clients in one batch"""
    from honeybadgermpc_amd.progs import mimc, mimc_jubjub_pkc as pkc

    p, n, t, K = BLS, 4, 1, 32
    ctx = _ctx(p)
    rnd = random.Random(32)
    cases = _golden()["encrypts"]
    c0 = cases[0]
    priv = int(c0["priv"])
    bits = _deal_tensor(ctx, rnd, p, n, t, [(priv >> j) & 1 for j in range(K)], (K, 1))
    pre_keygen = _deal_add_preprocessing(ctx, rnd, p, n, t, K - 1)

    async def keygen(co, i):
        kept, pub = await pkc.key_generation(co, bits[i], *pre_keygen[i])
        assert kept is bits[i]
        return pub

    results, batches = _run_parties(p, n, t, set(), rnd, keygen)
    pub = Point(*_xy(c0["pub"]))
    assert all(r == pub for r in results) and batches == {4 * 5 + 1}
    ms = [int(v) for v in c0["ms"]]
    cs, a_ = pkc.mimc_encrypt(ctx, pub, ctx.upload_ints(ms), int(c0["a"]))
    assert ctx.download_ints(cs) == [int(v) for v in c0["cs"]] and a_ == Point(*_xy(c0["a_"]))
    blocks = len(ms)

    def deal_cubes(count):
        r = [rnd.randrange(p) for _ in range(mimc.ROUND * count)]
        dealt = [_deal(rnd, p, n, t, vals) for vals in (r, [v * v % p for v in r], [v * v * v % p for v in r])]
        return [tuple(ctx.upload_ints(d[i]).reshape(mimc.ROUND, count, ctx.n_limbs) for d in dealt) for i in range(n)]

    pre_dec, cubes = _deal_add_preprocessing(ctx, rnd, p, n, t, K - 1), deal_cubes(blocks)

    async def decrypt(co, i):
        shares = await pkc.mimc_decrypt(co, bits[i], (cs, a_), *pre_dec[i], cubes[i])
        return ctx.download_ints(await co.open_share_array(shares))

    results, batches = _run_parties(p, n, t, set(), rnd, decrypt)
    assert all(r == ms for r in results) and batches == {4 * 5 + mimc.ROUND + 1}
    # every client at once: a scalar, a message row and a private key each (the system holds B key pairs here)
    B = len(cases)
    privs = [int(c["priv"]) for c in cases]
    all_ms = [[int(v) for v in c["ms"]] for c in cases]
    batch_cs, batch_a = [], []
    for c in cases:                                                  # the batched encryption takes ONE public key: client by client keys differ
        one_cs, one_a = pkc.mimc_encrypt(ctx, Point(*_xy(c["pub"])), ctx.upload_ints([int(v) for v in c["ms"]]).reshape(1, blocks, ctx.n_limbs),
                                         ctx.upload_ints([int(c["a"])]))
        assert ctx.download_ints(one_cs) == [int(v) for v in c["cs"]] and _download_points(ctx, one_a) == [_xy(c["a_"])]
        batch_cs.append(one_cs), batch_a.append(one_a)
    many_cs, many_a = pkc.mimc_encrypt(ctx, pub, ctx.upload_ints([v for row in all_ms for v in row]).reshape(B, blocks, ctx.n_limbs),
                                       ctx.upload_ints([int(c["a"]) for c in cases]))
    assert tuple(many_cs.shape) == (B, blocks, ctx.n_limbs) and ctx.torch.equal(many_cs[0], cs) and _download_points(ctx, many_a) == [_xy(c["a_"]) for c in cases]
    cs_all = ctx.torch.cat(batch_cs)
    a_all = (ctx.torch.cat([a[0] for a in batch_a]), ctx.torch.cat([a[1] for a in batch_a]))
    bits_all = _deal_tensor(ctx, rnd, p, n, t, [(privs[i] >> j) & 1 for j in range(K) for i in range(B)], (K, B))
    pre_all, cubes_all = _deal_add_preprocessing(ctx, rnd, p, n, t, (K - 1) * B), deal_cubes(B * blocks)

    async def decrypt_all(co, i):
        shares = await pkc.mimc_decrypt(co, bits_all[i], (cs_all, a_all), *pre_all[i], cubes_all[i])
        assert tuple(shares.shape) == (B, blocks, ctx.n_limbs)
        return ctx.download_ints(await co.open_share_array(shares.reshape(B * blocks, ctx.n_limbs)))

    results, batches = _run_parties(p, n, t, set(), rnd, decrypt_all)
    assert all(r == [v for row in all_ms for v in row] for r in results) and batches == {4 * 5 + mimc.ROUND + 1}


def test_a_zero_random_share_raises_on_every_party():
    from honeybadgermpc_amd.progs import jubjub

    p, n, t, m = BLS, 4, 1, 20
    ctx = _ctx(p)
    rnd = random.Random(0)
    pool = _pool(p)
    Ps, Qs = [rnd.choice(pool) for _ in range(m)], [rnd.choice(pool) for _ in range(m)]
    shares = [_deal_tensor(ctx, rnd, p, n, t, v, (m,)) for v in ([q.x for q in Ps], [q.y for q in Ps], [q.x for q in Qs], [q.y for q in Qs])]
    pre = _deal_add_preprocessing(ctx, rnd, p, n, t, m, zero_r=m + 7)             # ry of pair 7

    async def body(co, i):
        with pytest.raises(ZeroDivisionError, match="Cannot invert zero"):
            await jubjub.shared_add(co, (shares[0][i], shares[1][i]), (shares[2][i], shares[3][i]), *pre[i])
        return co.batches

    results, _ = _run_parties(p, n, t, set(), rnd, body)
    assert results == [4] * n


@pytest.mark.parametrize("p", [BLS, P64], ids=["bls", "2^64-59"])
@pytest.mark.parametrize("m", [1, 257])
def test_every_step_equals_the_host_self_test(p, m):
    """One row body: for every step of csrc/hb_jj.hip the device's output equals, bit for bit, what hb_selftest_jj computes on the host
    from the same random inputs -- the self test runs the rows the kernels run, addressing included.  The triples' row stride is
    m + 3, so it and m are different offsets; scalar_mul with each broadcast flag on and off; double_table with 3 rows, whose device
    result is affine where the self test's is projective ((X R, Y R, Z R) -> X R / Z R, Y R / Z R: the division is done on ints here).
    m = 1 is one partial workgroup, 257 a second workgroup that holds one element."""
    import numpy as np
    import selftest_cases as stc
    from honeybadgermpc_amd.progs import jubjub

    ctx, curve = _ctx(p), _curve(p)
    torch, nl = ctx.torch, ctx.n_limbs
    SCALAR_MUL, DOUBLE_TABLE, MASK, STAGE1, STAGE2, STAGE3, SCALE = range(7)
    seeds = iter(range(700, 800))

    def rnd(rows, cols=m):
        limbs = np.random.default_rng(next(seeds)).integers(-(1 << 63), (1 << 63) - 1, size=(rows * cols, nl), dtype=np.int64, endpoint=True)
        return ctx.reduce_(ctx.to_device(limbs)).view(rows, cols, nl)

    def ints(t):
        return ctx.download_ints(t.reshape(-1, nl))

    def host(what, operands, out_rows, count=m, **kw):
        rc, outs = stc.run_jj(p, nl, what, [o if isinstance(o, list) else ints(o) for o in operands], count, out_rows, **kw)
        assert rc == 0
        return outs

    def same(dev, want_rows):
        return ints(dev) == [v for row in want_rows for v in row]

    # ---- cleartext
    pool = _pool(p)
    pts = [pool[(7 * i + 3) % len(pool)] for i in range(m)]
    px, py = _upload_points(ctx, pts)
    ns = rnd(1)[0]
    a_h, d_h = ctx.host_elems([curve.a]), ctx.host_elems([curve.d])
    for n_b, p_b in ((0, 0), (1, 0), (0, 1), (1, 1)):
        n_dev, x_dev, y_dev = ns[:1] if n_b else ns, px[:1] if p_b else px, py[:1] if p_b else py
        ox, oy = ctx.empty(m), ctx.empty(m)
        ctx.check(ctx.lib.hb_jj_scalar_mul(ctx.h, ctx.ptr(n_dev), n_b, ctx.ptr(x_dev), ctx.ptr(y_dev), p_b, a_h.ctypes.data, d_h.ctypes.data, ctx.ptr(ox), ctx.ptr(oy), m,
                                           ctx.stream()), "hb_jj_scalar_mul")
        h = host(SCALAR_MUL, [n_dev, x_dev, y_dev], 2, a=curve.a, d=curve.d, flags=n_b | 2 * p_b)
        assert same(ox, h[:1]) and same(oy, h[1:]), (n_b, p_b)
    K = 3
    xs, ys = jubjub.double_table(ctx, (px, py), K, curve)
    h = host(DOUBLE_TABLE, [px, py], 3 * K, a=curve.a, arg=K)
    X, Y, Z = ([v for row in h[k * K:(k + 1) * K] for v in row] for k in range(3))
    assert ints(xs) == [x * pow(z, -1, p) % p for x, z in zip(X, Z)] and ints(ys) == [y * pow(z, -1, p) % p for y, z in zip(Y, Z)]
    # ---- the five stages of the shared addition
    stride = m + 3
    wide = tuple(rnd(9, stride) for _ in range(3))
    trip = tuple(v[:, :m] for v in wide)                                   # a column slice: taken as it is, row stride m + 3
    P, Q, rs = rnd(2), rnd(2), rnd(2)
    assert same(jubjub.add_mask(ctx, (P[0], P[1]), (Q[0], Q[1]), trip), host(MASK, [P[0], P[1], Q[0], Q[1], wide[0], wide[1]], 8, arg=stride))
    A, B, C, D = rnd(8), rnd(6), rnd(4), rnd(2)
    assert same(jubjub.add_stage1(ctx, A, trip, rs), host(STAGE1, [A, *wide, rs[0], rs[1]], 6, arg=stride))
    uv, c_out = jubjub.add_stage2(ctx, B, trip, rs, curve)
    h = host(STAGE2, [B, *wide, rs[0], rs[1]], 6, d=curve.d, arg=stride)
    assert same(uv, h[:2]) and same(c_out, h[2:])
    assert same(jubjub.add_stage3(ctx, C, trip), host(STAGE3, [C, *wide], 2, arg=stride))
    (x3, y3), zeros = jubjub.add_finish(ctx, D, uv, check=False)
    assert int(zeros.item()) == 0
    h = host(SCALE, [[pow(v, -1, p) for v in ints(D)], uv], 2)
    assert same(x3, h[:1]) and same(y3, h[1:])
    torch.cuda.synchronize()

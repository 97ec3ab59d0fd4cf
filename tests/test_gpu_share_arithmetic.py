"""GPU: honeybadgermpc_amd.share_arithmetic -- the element-wise kernels of csrc/hb_ew.hip through the tensor-level
functions, and the Beaver / double-sharing / inversion / division protocols over an OpenCoalescer -- against Python int
arithmetic.  Exact equality everywhere."""
import asyncio
import random

import pytest

from conftest import BLS

pytestmark = pytest.mark.gpu

WIDE = [BLS, (1 << 256) - 189, (1 << 255) - 19, 53]
NARROW = [(1 << 64) - 59, 0xFFFFFFFF00000001, 13]
FIELDS = [(p, 4) for p in WIDE] + [(p, 1) for p in NARROW]
FIELD_IDS = ["bls", "2^256-189", "2^255-19", "53w", "2^64-59", "goldilocks", "13n"]
COUNTS = [0, 1, 63, 64, 65, 3001]


def _ctx(p, nl):
    from honeybadgermpc_amd._capi import Context

    return Context.get(p, 0, nl)


def _rand(rnd, p, count, corners=True):
    xs = [rnd.randrange(p) for _ in range(count)]
    for k, v in enumerate((0, 1, p - 1, p - 1, 0)):
        if corners and k < count:
            xs[k] = v
    return xs


@pytest.mark.parametrize("p, nl", FIELDS, ids=FIELD_IDS)
def test_ops_beaver_and_inverse_over_the_counts(p, nl):
    from honeybadgermpc_amd import share_arithmetic as sa

    ctx = _ctx(p, nl)
    rnd = random.Random(p % 997 + nl)
    for count in COUNTS:
        a, b = _rand(rnd, p, count), _rand(rnd, p, count)[::-1]
        ta, tb = ctx.upload_ints(a), ctx.upload_ints(b)
        assert ctx.download_ints(sa.add(ctx, ta, tb)) == [(x + y) % p for x, y in zip(a, b)], count
        assert ctx.download_ints(sa.sub(ctx, ta, tb)) == [(x - y) % p for x, y in zip(a, b)], count
        assert ctx.download_ints(sa.mul(ctx, ta, tb)) == [x * y % p for x, y in zip(a, b)], count
        assert ctx.download_ints(sa.neg(ctx, ta)) == [-x % p for x in a], count
        # a Python int broadcast over the array
        for s in (0, 1, p - 1, rnd.randrange(p), p + 5, -3):
            assert ctx.download_ints(sa.add(ctx, ta, s)) == [(x + s) % p for x in a], (count, s)
            assert ctx.download_ints(sa.sub(ctx, ta, s)) == [(x - s) % p for x in a], (count, s)
            assert ctx.download_ints(sa.mul(ctx, ta, s)) == [x * s % p for x in a], (count, s)
        # the fused Beaver step, and the same by six launches
        cols = [_rand(rnd, p, count, corners=(k % 2 == 0)) for k in range(5)]
        d, e, pp, q, pq = (ctx.upload_ints(c) for c in cols)
        want = [(cols[0][i] * cols[1][i] + cols[0][i] * cols[3][i] + cols[1][i] * cols[2][i] + cols[4][i]) % p for i in range(count)]
        fused = sa.beaver_combine(ctx, d, e, pp, q, pq)
        assert ctx.download_ints(fused) == want, count
        composed = sa.add(ctx, sa.add(ctx, sa.add(ctx, sa.mul(ctx, d, e), sa.mul(ctx, d, q)), sa.mul(ctx, e, pp)), pq)
        assert ctx.torch.equal(fused, composed), count
        # inverses of non-zero elements
        nz = [x or 1 for x in a]
        assert ctx.download_ints(sa.inv(ctx, ctx.upload_ints(nz))) == [pow(x, -1, p) for x in nz], count
    ctx.torch.cuda.synchronize()


@pytest.mark.parametrize("p, nl", [(BLS, 4), ((1 << 256) - 189, 4), ((1 << 64) - 59, 1)], ids=["bls", "2^256-189", "2^64-59"])
def test_large_arrays_sampled(p, nl):
    """2^20 elements (and a ragged count beside it): a few thousand sampled positions and the first and last inversion tile"""
    from honeybadgermpc_amd import share_arithmetic as sa

    ctx = _ctx(p, nl)
    torch = ctx.torch
    rnd = random.Random(20)
    tile = 64 * (8 if nl == 4 else 16)
    for count in ((1 << 20), (1 << 20) - 37):
        gen = torch.Generator(device="cuda")
        gen.manual_seed(count)
        ts = [ctx.reduce_(torch.randint(-(1 << 63), (1 << 63) - 1, (count, nl), dtype=torch.int64, device="cuda", generator=gen)) for _ in range(5)]
        idx = sorted(set(list(range(tile)) + list(range(count - tile - 70, count)) + [rnd.randrange(count) for _ in range(3000)]))
        sel = torch.tensor(idx, device="cuda")
        cols = [ctx.download_ints(tt[sel]) for tt in ts]
        d, e, pp, q, pq = cols

        def at(tensor):
            return ctx.download_ints(tensor[sel])

        assert at(sa.mul(ctx, ts[0], ts[1])) == [x * y % p for x, y in zip(d, e)]
        assert at(sa.add(ctx, ts[0], ts[1])) == [(x + y) % p for x, y in zip(d, e)]
        assert at(sa.sub(ctx, ts[0], ts[1])) == [(x - y) % p for x, y in zip(d, e)]
        assert at(sa.neg(ctx, ts[0])) == [-x % p for x in d]
        fused = sa.beaver_combine(ctx, *ts)
        assert at(fused) == [(d[i] * e[i] + d[i] * q[i] + e[i] * pp[i] + pq[i]) % p for i in range(len(idx))]
        composed = sa.add(ctx, sa.add(ctx, sa.add(ctx, sa.mul(ctx, ts[0], ts[1]), sa.mul(ctx, ts[0], ts[3])), sa.mul(ctx, ts[1], ts[2])), ts[4])
        assert torch.equal(fused, composed)
        inverses, zeros = sa.inv(ctx, ts[0], check=False)
        assert at(inverses) == [pow(x, -1, p) if x else 0 for x in d]
        # the whole array: a * (1 / a) == 1 wherever a != 0 (a consistency check beside the sampled Python-int one)
        ones = sa.mul(ctx, ts[0], inverses)
        nonzero = (ts[0] != 0).any(dim=1)
        one = ctx.upload_ints([1])
        assert bool((ones[nonzero] == one).all()) and int(zeros.item()) == int((~nonzero).sum().item())
    torch.cuda.synchronize()


@pytest.mark.parametrize("p, nl", [(BLS, 4), ((1 << 64) - 59, 1)], ids=["bls", "2^64-59"])
def test_out_aliases_an_input(p, nl):
    from honeybadgermpc_amd import share_arithmetic as sa

    ctx = _ctx(p, nl)
    rnd = random.Random(5)
    count = 1000
    a, b = _rand(rnd, p, count), _rand(rnd, p, count)[::-1]
    for fn, ref in ((sa.add, lambda x, y: (x + y) % p), (sa.sub, lambda x, y: (x - y) % p), (sa.mul, lambda x, y: x * y % p)):
        ta, tb = ctx.upload_ints(a), ctx.upload_ints(b)
        assert fn(ctx, ta, tb, out=ta) is ta and ctx.download_ints(ta) == [ref(x, y) for x, y in zip(a, b)]
        ta = ctx.upload_ints(a)
        assert fn(ctx, ta, tb, out=tb) is tb and ctx.download_ints(tb) == [ref(x, y) for x, y in zip(a, b)]
        ta = ctx.upload_ints(a)
        assert fn(ctx, ta, ta, out=ta) is ta and ctx.download_ints(ta) == [ref(x, x) for x in a]
        ta = ctx.upload_ints(a)
        assert fn(ctx, ta, 7, out=ta) is ta and ctx.download_ints(ta) == [ref(x, 7) for x in a]
    ta = ctx.upload_ints(a)
    assert sa.neg(ctx, ta, out=ta) is ta and ctx.download_ints(ta) == [-x % p for x in a]
    cols = [_rand(rnd, p, count) for _ in range(5)]
    want = [(cols[0][i] * cols[1][i] + cols[0][i] * cols[3][i] + cols[1][i] * cols[2][i] + cols[4][i]) % p for i in range(count)]
    for k in range(5):
        ts = [ctx.upload_ints(c) for c in cols]
        assert sa.beaver_combine(ctx, *ts, out=ts[k]) is ts[k] and ctx.download_ints(ts[k]) == want, k
    nz = [x or 1 for x in a]
    ta = ctx.upload_ints(nz)
    assert sa.inv(ctx, ta, out=ta) is ta and ctx.download_ints(ta) == [pow(x, -1, p) for x in nz]
    ctx.torch.cuda.synchronize()


@pytest.mark.parametrize("p, nl", [(BLS, 4), ((1 << 255) - 19, 4), ((1 << 64) - 59, 1), (13, 1)], ids=["bls", "2^255-19", "2^64-59", "13n"])
def test_inverse_with_zeros(p, nl):
    """zeros in the first lane, the last lane, the last slot of a tile and the ragged tail: check=True raises, check=False
    counts them exactly, answers 0 for them and the right inverse everywhere else"""
    from honeybadgermpc_amd import share_arithmetic as sa

    ctx = _ctx(p, nl)
    rnd = random.Random(9)
    tile = 64 * (8 if nl == 4 else 16)
    count = 2 * tile + 129
    placements = [[0], [63], [tile - 1], [tile], [count - 1], [2 * tile + 64 + 3], [0, 64, 128, 63, tile - 1, 2 * tile, count - 1], list(range(count))]
    for zeros_at in placements:
        xs = [rnd.randrange(1, p) for _ in range(count)]
        for i in zeros_at:
            xs[i] = 0
        tx = ctx.upload_ints(xs)
        with pytest.raises(ZeroDivisionError, match="Cannot invert zero"):
            sa.inv(ctx, tx)
        out, counter = sa.inv(ctx, tx, check=False)
        assert ctx.download_ints(out) == [pow(x, -1, p) if x else 0 for x in xs], zeros_at[:4]
        assert counter.dtype == ctx.torch.int32 and int(counter.item()) == len(zeros_at)
    out, counter = sa.inv(ctx, ctx.upload_ints([rnd.randrange(1, p) for _ in range(count)]), check=False)
    assert int(counter.item()) == 0
    ctx.torch.cuda.synchronize()


def test_arguments_are_checked_before_c():
    import torch

    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd._capi import HB_ERR_BAD_ARG

    ctx = _ctx(BLS, 4)
    good = ctx.upload_ints([1, 2, 3])
    with pytest.raises(TypeError):
        sa.add(ctx, good.to(torch.int32), good)
    with pytest.raises(TypeError):
        sa.mul(ctx, good, good.to(torch.float64))
    with pytest.raises(TypeError):
        sa.neg(ctx, [1, 2, 3])
    with pytest.raises(ValueError):
        sa.add(ctx, good, torch.zeros((3, 1), dtype=torch.int64, device="cuda"))     # limb count
    with pytest.raises(ValueError):
        sa.sub(ctx, good, ctx.upload_ints([1, 2]))                                     # length
    with pytest.raises(ValueError):
        sa.mul(ctx, good.cpu(), good)                                                  # device
    with pytest.raises(ValueError):
        sa.inv(ctx, good.cpu())
    with pytest.raises(ValueError):
        sa.beaver_combine(ctx, good, good, good, good, ctx.upload_ints([1]))
    with pytest.raises(ValueError):
        sa.add(ctx, good, good, out=ctx.empty(2))
    with pytest.raises(ValueError):
        sa.add(ctx, good, good, out=ctx.empty(6)[::2])                                 # a strided output
    with pytest.raises(TypeError):
        sa.beaver_combine(ctx, good, good, good, good, good, out=good.to(torch.int32))
    # the raw C ABI: an unknown op, a negative count and null pointers return an error code and launch nothing
    lib, out = ctx.lib, ctx.upload_ints([7, 7, 7])
    torch.cuda.synchronize()
    for op in (4, -1, 99):
        assert lib.hb_ew_op(ctx.h, op, ctx.ptr(good), ctx.ptr(good), 0, ctx.ptr(out), 3, ctx.stream()) == HB_ERR_BAD_ARG
    assert lib.hb_ew_op(ctx.h, 0, ctx.ptr(good), ctx.ptr(good), 0, ctx.ptr(out), -1, ctx.stream()) == HB_ERR_BAD_ARG
    assert lib.hb_ew_op(ctx.h, 0, ctx.ptr(good), None, 0, ctx.ptr(out), 3, ctx.stream()) == HB_ERR_BAD_ARG
    assert lib.hb_ew_op(ctx.h, 0, None, ctx.ptr(good), 0, ctx.ptr(out), 3, ctx.stream()) == HB_ERR_BAD_ARG
    assert lib.hb_ew_op(ctx.h, 0, ctx.ptr(good), ctx.ptr(good), 0, None, 3, ctx.stream()) == HB_ERR_BAD_ARG
    assert lib.hb_ew_op(ctx.h, 0, ctx.ptr(good), ctx.ptr(out), 1, ctx.ptr(out), 3, ctx.stream()) == HB_ERR_BAD_ARG   # out = broadcast b
    assert lib.hb_ew_op(None, 0, ctx.ptr(good), ctx.ptr(good), 0, ctx.ptr(out), 3, ctx.stream()) == HB_ERR_BAD_ARG
    assert lib.hb_ew_beaver(ctx.h, ctx.ptr(good), ctx.ptr(good), None, ctx.ptr(good), ctx.ptr(good), ctx.ptr(out), 3, ctx.stream()) == HB_ERR_BAD_ARG
    assert lib.hb_ew_beaver(ctx.h, ctx.ptr(good), ctx.ptr(good), ctx.ptr(good), ctx.ptr(good), ctx.ptr(good), ctx.ptr(out), -2, ctx.stream()) == HB_ERR_BAD_ARG
    assert lib.hb_ew_inv(ctx.h, None, ctx.ptr(out), 3, None, ctx.stream()) == HB_ERR_BAD_ARG
    assert lib.hb_ew_inv(ctx.h, ctx.ptr(good), ctx.ptr(out), -1, None, ctx.stream()) == HB_ERR_BAD_ARG
    # count == 0 with null pointers is fine and launches nothing; NEG takes no b
    assert lib.hb_ew_op(ctx.h, 2, None, None, 0, None, 0, ctx.stream()) == 0
    assert lib.hb_ew_inv(ctx.h, None, None, 0, None, ctx.stream()) == 0
    assert lib.hb_ew_op(ctx.h, 3, ctx.ptr(good), None, 0, ctx.ptr(good), 3, ctx.stream()) == 0
    torch.cuda.synchronize()
    assert ctx.download_ints(out) == [7, 7, 7] and ctx.download_ints(good) == [BLS - 1, BLS - 2, BLS - 3]


# ---- the protocols, end to end over the in-process tagged network of tests/test_gpu_offline.py --------------------------
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
    polys = [[v] + [rnd.randrange(p) for _ in range(degree)] for v in values]
    return [[sum(co * pow(x, e, p) for e, co in enumerate(poly)) % p for poly in polys] for x in range(1, n + 1)]


def _triples(rnd, p, n, t, length):
    a, b = [rnd.randrange(p) for _ in range(length)], [rnd.randrange(p) for _ in range(length)]
    return _deal(rnd, p, n, t, a), _deal(rnd, p, n, t, b), _deal(rnd, p, n, t, [x * y % p for x, y in zip(a, b)])


def _run_parties(n, bad, garble, program):
    """every party runs program(i, co) -> tensor of result shares; the results are then opened; -> ([party] opened ints, [party] (opens, batches) before the final open)"""
    from honeybadgermpc_amd._capi import Context
    from honeybadgermpc_amd.open_coalescer import OpenCoalescer

    async def party(i, net, p, t):
        co = OpenCoalescer(p, n, t, i, net.get_send_recv(i, garble if i in bad else None))
        shares = await program(i, co)
        counters = (co.opens, co.batches)
        opened = await co.open_share_array(shares)
        return Context.get(p).download_ints(opened), counters

    return party


@pytest.mark.parametrize("n, t, liars", [(4, 1, 0), (7, 2, 0), (7, 2, 2)])
def test_beaver_multiply_arrays_end_to_end(n, t, liars):
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd import wire
    from honeybadgermpc_amd._capi import Context

    p = BLS
    ctx = Context.get(p)
    rnd = random.Random(100 * n + liars)
    length = 257
    x, y = [rnd.randrange(p) for _ in range(length)], [rnd.randrange(p) for _ in range(length)]
    x[0], y[1], x[2], y[2] = 0, 0, p - 1, p - 1
    xs, ys = _deal(rnd, p, n, t, x), _deal(rnd, p, n, t, y)
    ta, tb, tab = _triples(rnd, p, n, t, length)
    bad = set(rnd.sample(range(n), liars))

    def garble(msg):
        tag, blob = msg
        count = wire.unpack_limbs(blob).shape[0]
        return (tag, wire.pack_ints([rnd.randrange(p) for _ in range(count)], p))

    async def program(i, co):
        up = ctx.upload_ints
        return await sa.beaver_multiply_arrays(co, up(xs[i]), up(ys[i]), (up(ta[i]), up(tb[i]), up(tab[i])))

    party = _run_parties(n, bad, garble, program)

    async def main():
        net = _TaggedNet(n)
        return await asyncio.gather(*[party(i, net, p, t) for i in range(n)])

    results = asyncio.run(main())
    for i in range(n):
        opened, (opens, batches) = results[i]
        assert (opens, batches) == (2, 1), "the two masked opens of a Beaver multiplication travel as one coalesced batch"
        if i not in bad:
            assert opened == [a * b % p for a, b in zip(x, y)], i
    ctx.torch.cuda.synchronize()


@pytest.mark.parametrize("n, t", [(4, 1), (7, 2)])
def test_invert_and_divide_share_arrays_end_to_end(n, t):
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd._capi import Context

    p = BLS
    ctx = Context.get(p)
    rnd = random.Random(7 * n)
    length = 130
    x = [rnd.randrange(p) for _ in range(length)]
    y = [rnd.randrange(1, p) for _ in range(length)]
    x[0], y[1], y[2] = 0, 1, p - 1
    r = [rnd.randrange(1, p) for _ in range(length)]
    xs, ys, rs = _deal(rnd, p, n, t, x), _deal(rnd, p, n, t, y), _deal(rnd, p, n, t, r)
    t1, t2 = _triples(rnd, p, n, t, length), _triples(rnd, p, n, t, length)
    up = ctx.upload_ints

    def trip(tr, i):
        return tuple(up(part[i]) for part in tr)

    async def invert(i, co):
        return await sa.invert_share_array(co, up(ys[i]), up(rs[i]), trip(t1, i))

    async def divide(i, co):
        return await sa.divide_share_arrays(co, up(xs[i]), up(ys[i]), up(rs[i]), trip(t1, i), trip(t2, i))

    for program, want, counters in ((invert, [pow(v, -1, p) for v in y], (3, 2)), (divide, [a * pow(b, -1, p) % p for a, b in zip(x, y)], (5, 3))):
        party = _run_parties(n, set(), None, program)

        async def main():
            net = _TaggedNet(n)
            return await asyncio.gather(*[party(i, net, p, t) for i in range(n)])

        for i, (opened, seen) in enumerate(asyncio.run(main())):
            assert opened == want, i
            assert seen == counters, seen          # per Beaver multiplication two opens in one batch, plus the open of sig

    # a zero among the values to invert: the opened sig is zero and every party is told so
    y0 = list(y)
    y0[5] = 0
    ys0 = _deal(rnd, p, n, t, y0)

    async def invert_zero(i, co):
        with pytest.raises(ZeroDivisionError, match="Cannot invert zero"):
            await sa.invert_share_array(co, up(ys0[i]), up(rs[i]), trip(t1, i))
        return up([0])

    party = _run_parties(n, set(), None, invert_zero)

    async def main_zero():
        net = _TaggedNet(n)
        return await asyncio.gather(*[party(i, net, p, t) for i in range(n)])

    asyncio.run(main_zero())
    ctx.torch.cuda.synchronize()


def test_double_sharing_multiply_arrays_end_to_end():
    """n = 7, t = 2: the local products are opened at degree 2t = 4 (5 columns needed, 7 arrive)"""
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd._capi import Context

    p, n, t = BLS, 7, 2
    ctx = Context.get(p)
    rnd = random.Random(72)
    length = 200
    x, y = [rnd.randrange(p) for _ in range(length)], [rnd.randrange(p) for _ in range(length)]
    r = [rnd.randrange(p) for _ in range(length)]
    xs, ys = _deal(rnd, p, n, t, x), _deal(rnd, p, n, t, y)
    r_t, r_2t = _deal(rnd, p, n, t, r), _deal(rnd, p, n, 2 * t, r)
    up = ctx.upload_ints

    async def program(i, co):
        return await sa.double_sharing_multiply_arrays(co, up(xs[i]), up(ys[i]), up(r_t[i]), up(r_2t[i]))

    party = _run_parties(n, set(), None, program)

    async def main():
        net = _TaggedNet(n)
        return await asyncio.gather(*[party(i, net, p, t) for i in range(n)])

    for i, (opened, seen) in enumerate(asyncio.run(main())):
        assert opened == [a * b % p for a, b in zip(x, y)], i
        assert seen == (1, 1)
    ctx.torch.cuda.synchronize()


def test_narrow_field_beaver_end_to_end():
    """the same Beaver multiplication over the 8-byte prime 2^64 - 59"""
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd._capi import Context

    p, n, t = (1 << 64) - 59, 4, 1
    ctx = Context.get(p)
    assert ctx.n_limbs == 1
    rnd = random.Random(64)
    length = 100
    x, y = [rnd.randrange(p) for _ in range(length)], [rnd.randrange(p) for _ in range(length)]
    xs, ys = _deal(rnd, p, n, t, x), _deal(rnd, p, n, t, y)
    ta, tb, tab = _triples(rnd, p, n, t, length)
    up = ctx.upload_ints

    async def program(i, co):
        return await sa.beaver_multiply_arrays(co, up(xs[i]), up(ys[i]), (up(ta[i]), up(tb[i]), up(tab[i])))

    party = _run_parties(n, set(), None, program)

    async def main():
        net = _TaggedNet(n)
        return await asyncio.gather(*[party(i, net, p, t) for i in range(n)])

    for i, (opened, seen) in enumerate(asyncio.run(main())):
        assert opened == [a * b % p for a, b in zip(x, y)], i
        assert seen == (2, 1)
    ctx.torch.cuda.synchronize()


def _with_corners(rnd, p, count, shift):
    """random residues with 0, 1 and p - 1 among them, at positions that differ from operand to operand"""
    xs = [rnd.randrange(p) for _ in range(count)]
    for k, v in enumerate((0, 1, p - 1)):
        xs[(shift + k) % count] = v
    return xs


@pytest.mark.parametrize("count", (1, 255, 256, 257, 513))
@pytest.mark.parametrize("p, nl", [(BLS, 4), ((1 << 64) - 59, 1)], ids=["bls", "2^64-59"])
def test_every_row_equals_the_host_self_test(p, nl, count):
    """One row body: the device's output of every binary op -- with and without a broadcast b, in place on a and on b -- and of the
    Beaver step equals, bit for bit, what hb_selftest_ew computes on the host from the same inputs: the self test runs the rows the
    kernel runs, addressing included.  Both instantiations; one lane, a full workgroup, one lane into a second, a ragged third."""
    import selftest_cases as stc
    from honeybadgermpc_amd import share_arithmetic as sa

    ADD, SUB, MUL, NEG, BEAVER, BROADCAST = 0, 1, 2, 3, 4, 0x100
    ctx = _ctx(p, nl)
    torch = ctx.torch
    rnd = random.Random(1000 * nl + count)
    a, b = _with_corners(rnd, p, count, 0), _with_corners(rnd, p, count, 1)

    def same(dev, host):
        return tuple(dev.shape) == (count, nl) and torch.equal(dev, ctx.upload_ints(host))

    for op, fn in ((ADD, sa.add), (SUB, sa.sub), (MUL, sa.mul)):
        want = stc.run_ew(p, nl, op, [a, b], count)
        ta, tb = ctx.upload_ints(a), ctx.upload_ints(b)
        assert same(fn(ctx, ta, tb), want), op
        assert fn(ctx, ta, tb, out=ta) is ta and same(ta, want), (op, "in place on a")
        ta = ctx.upload_ints(a)
        assert fn(ctx, ta, tb, out=tb) is tb and same(tb, want), (op, "in place on b")
        for s in (0, 1, p - 1, rnd.randrange(p)):
            want = stc.run_ew(p, nl, op | BROADCAST, [a, [s]], count)
            ta = ctx.upload_ints(a)
            assert same(fn(ctx, ta, s), want), (op, s)
            assert fn(ctx, ta, s, out=ta) is ta and same(ta, want), (op, s, "in place on a")
    want = stc.run_ew(p, nl, NEG, [a], count)
    ta = ctx.upload_ints(a)
    assert same(sa.neg(ctx, ta), want)
    assert sa.neg(ctx, ta, out=ta) is ta and same(ta, want)
    cols = [_with_corners(rnd, p, count, k) for k in range(5)]
    assert same(sa.beaver_combine(ctx, *(ctx.upload_ints(c) for c in cols)), stc.run_ew(p, nl, BEAVER, cols, count))
    torch.cuda.synchronize()

"""GPU: the less-than half of honeybadgermpc_amd.share_comparison -- the kernels of csrc/hb_lt.hip, bit for bit, against the same steps
composed from share_arithmetic (sub, mul, add, beaver_combine) with the public bits taken from the limbs by torch, and against Python
ints; and the whole protocol over an OpenCoalescer: less_than opens to the host model's value, which is [a < b], in the stated number of
batches, in both modes, the reference's recorded runs among them.  Exact equality everywhere."""
import asyncio
import json
import os
import random

import numpy as np
import pytest

from conftest import BLS, REPO

pytestmark = pytest.mark.gpu

GOLDILOCKS = 0xFFFFFFFF00000001
P64 = (1 << 64) - 59
P256 = (1 << 256) - 189
FIELDS = [BLS, P256, P64, GOLDILOCKS]
FIELD_IDS = ["bls", "2^256-189", "2^64-59", "goldilocks"]
COUNTS = (0, 1, 255, 256, 257, 5000)


# ---- the helpers of tests/test_gpu_share_comparison.py (restated) ------------------------------------------------------------
def _ctx(p):
    from honeybadgermpc_amd._capi import Context

    return Context.get(p)


def _random_tensor(ctx, seed, count, rows=None):
    """uniform canonical residues made on the device side (numpy limbs, reduced by hb_reduce)"""
    g = np.random.default_rng(seed)
    n = count if rows is None else rows * count
    limbs = g.integers(-(1 << 63), (1 << 63) - 1, size=(n, ctx.n_limbs), dtype=np.int64, endpoint=True)
    t = ctx.reduce_(ctx.to_device(limbs))
    return t if rows is None else t.view(rows, count, ctx.n_limbs)


def _ints(ctx, t):
    return ctx.download_ints(t.reshape(-1, ctx.n_limbs))


def _sample(count):
    return list(range(count)) if count <= 257 else sorted({0, 1, 2, 3, 4, 255, 256, 257, count - 1} | set(random.Random(count).sample(range(count), 40)))


def _const(ctx, v, like):
    """the residue v in every element of a tensor shaped like `like`"""
    return ctx.upload_ints([v % ctx.modulus]).expand(like.numel() // ctx.n_limbs, ctx.n_limbs).contiguous().view(like.shape)


class _TaggedNet:
    def __init__(self, n):
        self.n, self.q = n, [dict() for _ in range(n)]

    def _queue(self, party, tag):
        return self.q[party].setdefault(tag, asyncio.Queue())

    def get_send_recv(self, i):
        def factory(tag):
            def send(dest, msg):
                self._queue(dest, tag).put_nowait((i, msg))

            return send, self._queue(i, tag).get

        return factory


def _run_parties(p, n, t, body):
    from honeybadgermpc_amd.open_coalescer import OpenCoalescer

    async def party(i, net):
        return await body(OpenCoalescer(p, n, t, i, net.get_send_recv(i)), i)

    async def main():
        net = _TaggedNet(n)
        return await asyncio.gather(*[party(i, net) for i in range(n)])

    results = asyncio.run(main())
    _ctx(p).torch.cuda.synchronize()
    return results


def _deal(ctx, seed, values, n):
    """degree-1 Shamir shares of a tensor of values at the points 1..n, dealt on the device: value + point * slope"""
    from honeybadgermpc_amd import share_arithmetic as sa

    flat = values.reshape(-1, ctx.n_limbs)
    slope = _random_tensor(ctx, seed, flat.shape[0])
    return [sa.add(ctx, flat, sa.mul(ctx, slope, i + 1)).view(values.shape) for i in range(n)]


# ---- bits of canonical residues, by torch on the limbs (limb 0 is the least significant) ------------------------------------
def _bit(t, i):
    """bit i of every element of a (count, limbs) tensor -> bool (count, 1)"""
    return (((t[:, i // 64] >> (i % 64)) & 1) != 0).unsqueeze(1)


def _bit_planes(ctx, t):
    """(count, limbs) -> (L, count, limbs): plane i holds bit i of every element, as the residue 0 or 1"""
    L = ctx.modulus.bit_length()
    out = ctx.torch.zeros((L, t.shape[0], ctx.n_limbs), dtype=ctx.torch.int64, device=ctx.tdev)
    for i in range(L):
        out[i, :, 0] = (t[:, i // 64] >> (i % 64)) & 1
    return out


def edge_pairs(p):
    """(c, r): c on the corners and with single bits at the words' edges; r equal to c, beside it, and differing in bit 0 or the top bit only"""
    L = p.bit_length()
    cs = [0, 1, p - 1, (1 << (L - 1)) - 1] + [1 << k for k in (31, 32, 63, 64) if k < L and (1 << k) < p] + [(1 << k) - 1 for k in (32, 64) if k < L]
    return [(c, r) for c in cs for r in (c, c + 1, c - 1, c ^ 1, c ^ (1 << (L - 1))) if 0 <= r < p]


def edge_masks(p):
    """s and d on both sides of 2^(L-2), 2^(L-1) and their sum, p - 1 and 0"""
    L = p.bit_length()
    lo, hi = 1 << (L - 2), 1 << (L - 1)
    return [v for v in (lo - 1, lo, hi - 1, hi, lo + hi - 1, lo + hi, p - 1, 0) if v < p]


def d0_select(d, s1, s2, sp, L, p):
    d0 = d & 1
    x1, x2, x12 = d0 ^ (d < (1 << (L - 1))), d0 ^ (d < (1 << (L - 2))), d0 ^ (d < ((1 << (L - 1)) + (1 << (L - 2))))
    return ((1 - s1 - s2 + sp) * d0 + (s2 - sp) * x2 + (s1 - sp) * x1 + sp * x12) % p


# ---- the kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", FIELDS, ids=FIELD_IDS)
def test_wrappers_equal_their_compositions(p):
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd import share_comparison as sc

    ctx = _ctx(p)
    torch = ctx.torch
    L = p.bit_length()
    pairs, masks = edge_pairs(p), edge_masks(p)
    flat = lambda t: t.reshape(-1, ctx.n_limbs)                                             # noqa: E731
    for count in COUNTS:
        sd = 1000 + 40 * count
        a, b, r, c, w, x, s = (_random_tensor(ctx, sd + k, count) for k in range(7))
        r_bits, s_bits = _random_tensor(ctx, sd + 7, count, L), _random_tensor(ctx, sd + 8, count, L)     # a share of a bit is any residue
        if count >= 255:                                                 # the edge values in front: c, and exact bits of the r beside it
            c[:len(pairs)] = ctx.upload_ints([v for v, _ in pairs])
            r_bits[:, :len(pairs)] = _bit_planes(ctx, ctx.upload_ints([v for _, v in pairs]))
            s[:len(masks)] = ctx.upload_ints(masks)
            s_bits[:, :len(masks)] = _bit_planes(ctx, s[:len(masks)])
        ta, tb, tc = (tuple(_random_tensor(ctx, sd + 9 + 3 * k + j, count) for j in range(3)) for k in range(3))
        opened, opened2 = _random_tensor(ctx, sd + 20, count, 5), _random_tensor(ctx, sd + 21, count, 2)
        if count >= 255:
            opened[0, :len(masks)] = ctx.upload_ints(masks)               # d on both sides of the three thresholds
        inputs = [a, b, r, c, w, x, s, r_bits, s_bits, *ta, *tb, *tc, opened, opened2]
        keep = [v.clone() for v in inputs]
        zero, one, two = (_const(ctx, v, a) for v in (0, 1, 2))
        # lt_mask
        assert torch.equal(sc.lt_mask(ctx, a, b, r), sa.add(ctx, sa.mul(ctx, sa.sub(ctx, a, b), 2), r)), count
        assert torch.equal(sc.lt_mask(ctx, a, None, r), sa.add(ctx, sa.mul(ctx, a, 2), r)), count
        # lt_leaves: plane j against bit L - 1 - j
        for mode in (sc.DIRECT, sc.REFERENCE):
            g, q = sc.lt_leaves(ctx, c, r_bits, mode)
            assert tuple(g.shape) == tuple(q.shape) == (L, count, ctx.n_limbs)
            for j in (sorted({j for j in (0, 1, L // 2, L - 65, L - 64, L - 33, L - 32, L - 2, L - 1) if 0 <= j < L}) if count == 5000 else range(L)):
                i = L - 1 - j
                cb, rb = _bit(c, i), r_bits[i]
                assert torch.equal(g[j], torch.where(cb, zero, rb)), (count, mode, j)
                if mode == sc.DIRECT:
                    want = torch.where(cb, rb, sa.sub(ctx, one, rb))
                else:
                    want = torch.where(cb, sa.sub(ctx, two, rb), sa.add(ctx, rb, 1))
                assert torch.equal(q[j], want), (count, mode, j)
            if count >= 255:                                             # Python ints at the edge values, every plane
                n = len(pairs)
                gi, qi = _ints(ctx, g[:, :n].contiguous()), _ints(ctx, q[:, :n].contiguous())
                for e, (cv, rv) in enumerate(pairs):
                    for j in range(L):
                        cb, rb = (cv >> (L - 1 - j)) & 1, (rv >> (L - 1 - j)) & 1
                        want = (0 if cb else rb, (rb if cb else 1 - rb) if mode == sc.DIRECT else (2 - rb if cb else 1 + rb))
                        assert (gi[j * n + e], qi[j * n + e]) == want, (mode, cv, rv, j)
        # lt_xor_mask, lt_dmask
        r0, s0, s1, s2 = r_bits[0], s_bits[0], s_bits[L - 1], s_bits[L - 2]
        want_u = torch.where(_bit(c, 0), sa.sub(ctx, one, r0), r0) if count else a
        u, masked = sc.lt_xor_mask(ctx, c, r0, w, ta[0], ta[1])
        assert torch.equal(u, want_u) and tuple(masked.shape) == (2, count, ctx.n_limbs)
        assert torch.equal(flat(masked), torch.cat((sa.sub(ctx, want_u, ta[0]), sa.sub(ctx, w, ta[1])))), count
        u, masked = sc.lt_dmask(ctx, c, r0, x, s, s_bits, ta[0], ta[1], tb[0], tb[1])
        assert torch.equal(u, want_u) and tuple(masked.shape) == (5, count, ctx.n_limbs)
        assert torch.equal(flat(masked), torch.cat((sa.add(ctx, s, x), sa.sub(ctx, want_u, ta[0]), sa.sub(ctx, s0, ta[1]), sa.sub(ctx, s1, tb[0]), sa.sub(ctx, s2, tb[1])))), count
        # lt_mid
        v, d0, masked2 = sc.lt_mid(ctx, opened, want_u, s_bits, ta, tb, tc[0], tc[1])
        us0 = sa.beaver_combine(ctx, opened[1], opened[2], *ta)
        sp = sa.beaver_combine(ctx, opened[3], opened[4], *tb)
        want_v = sa.sub(ctx, sa.sub(ctx, sa.add(ctx, want_u, s0), us0), us0)
        if count:
            d = opened[0]
            lsb, t1, t2 = _bit(d, 0), _bit(d, L - 1), _bit(d, L - 2)
            terms = ((lsb, sa.add(ctx, sa.sub(ctx, sa.sub(ctx, one, s1), s2), sp)), (lsb ^ ~(t1 | t2), sa.sub(ctx, s2, sp)), (lsb ^ ~t1, sa.sub(ctx, s1, sp)), (lsb ^ ~(t1 & t2), sp))
            want_d0 = zero
            for sel, term in terms:
                want_d0 = sa.add(ctx, want_d0, torch.where(sel, term, zero))
        else:
            want_d0 = a
        assert torch.equal(v, want_v) and torch.equal(d0, want_d0), count
        assert torch.equal(flat(masked2), torch.cat((sa.sub(ctx, want_v, tc[0]), sa.sub(ctx, want_d0, tc[1])))) and tuple(masked2.shape) == (2, count, ctx.n_limbs)
        if count >= 255:                                                 # Python ints at the thresholds of d
            n = len(masks)
            got = _ints(ctx, d0[:n])
            for e, (dv, a1, a2, a3) in enumerate(zip(masks, _ints(ctx, s1[:n]), _ints(ctx, s2[:n]), _ints(ctx, sp[:n]))):
                assert got[e] == d0_select(dv, a1, a2, a3, L, p), dv
        # lt_xor_finish
        m = sa.beaver_combine(ctx, opened2[0], opened2[1], *tc)
        assert torch.equal(sc.lt_xor_finish(ctx, opened2, want_v, want_d0, tc), sa.sub(ctx, sa.sub(ctx, sa.add(ctx, want_v, want_d0), m), m)), count
        assert torch.equal(sc.lt_xor_finish(ctx, flat(opened2), want_v, want_d0, tc), sc.lt_xor_finish(ctx, opened2, want_v, want_d0, tc))
        assert all(torch.equal(i, k) for i, k in zip(inputs, keep)), "inputs were written"


def test_arguments_are_checked():
    from honeybadgermpc_amd import share_comparison as sc

    ctx = _ctx(BLS)
    torch = ctx.torch
    L, count = BLS.bit_length(), 9
    e = [_random_tensor(ctx, 1 + k, count) for k in range(12)]
    bits = _random_tensor(ctx, 20, count, L)
    with pytest.raises(ValueError):
        sc.lt_mask(ctx, e[0], e[1][:4], e[2])
    with pytest.raises(ValueError):
        sc.lt_leaves(ctx, e[0], bits[:L - 1])
    with pytest.raises(ValueError):
        sc.lt_leaves(ctx, e[0], _random_tensor(ctx, 21, count, L + 1))
    with pytest.raises(ValueError):
        sc.lt_leaves(ctx, e[0], bits, mode=2)
    with pytest.raises(ValueError):
        sc.lt_xor_mask(ctx, e[0], e[1], e[2], e[3], e[4][:3])
    with pytest.raises(ValueError):
        sc.lt_dmask(ctx, e[0], e[1], e[2], e[3], bits[:2], e[4], e[5], e[6], e[7])
    with pytest.raises(ValueError):
        sc.lt_mid(ctx, _random_tensor(ctx, 22, count, 4), e[0], bits, tuple(e[1:4]), tuple(e[4:7]), e[7], e[8])
    with pytest.raises(ValueError):
        sc.lt_mid(ctx, _random_tensor(ctx, 22, count, 5), e[0], bits, tuple(e[1:3]), tuple(e[4:7]), e[7], e[8])
    with pytest.raises(ValueError):
        sc.lt_xor_finish(ctx, _random_tensor(ctx, 23, count, 3), e[0], e[1], tuple(e[2:5]))
    with pytest.raises(TypeError):
        sc.lt_mask(ctx, e[0].cpu().numpy(), None, e[1])
    # the C ABI: return code 2 and nothing written
    st, P = ctx.stream(), ctx.ptr
    lib, h = ctx.lib, ctx.h
    buf = torch.zeros((2 * L + 8, count, ctx.n_limbs), dtype=torch.int64, device=ctx.tdev)
    o = [buf[0], buf[1], buf[2:4], buf[8:8 + L], buf[8 + L:8 + 2 * L], buf[2:7]]
    assert lib.hb_lt_mask(h, None, P(e[1]), P(e[2]), P(o[0]), count, st) == 2 and lib.hb_lt_mask(h, P(e[0]), None, P(e[2]), P(o[0]), -1, st) == 2
    assert lib.hb_lt_mask(h, P(e[0]), None, P(e[2]), None, count, st) == 2 and lib.hb_lt_mask(h, P(e[0]), P(e[1]), P(e[1]), P(e[1]), count, st) == 2     # masked over b
    assert lib.hb_lt_mask(h, None, None, None, None, 0, st) == 0
    assert lib.hb_lt_leaves(h, P(e[0]), P(bits), L, 2, P(o[3]), P(o[4]), count, st) == 2 and lib.hb_lt_leaves(h, P(e[0]), P(bits), L - 1, 0, P(o[3]), P(o[4]), count, st) == 2
    assert lib.hb_lt_leaves(h, P(e[0]), P(bits), L + 1, 1, P(o[3]), P(o[4]), count, st) == 2 and lib.hb_lt_leaves(h, P(e[0]), P(bits), L, 0, P(o[3]), P(o[3]), count, st) == 2
    assert lib.hb_lt_leaves(h, P(e[0]), None, L, 0, P(o[3]), P(o[4]), count, st) == 2 and lib.hb_lt_leaves(h, None, None, L, 0, None, None, 0, st) == 0
    assert lib.hb_lt_leaves(h, None, None, L, 5, None, None, 0, st) == 2
    assert lib.hb_lt_xor_mask(h, P(e[0]), P(e[1]), P(e[2]), P(e[3]), P(e[4]), P(o[0]), P(buf[0:2]), count, st) == 2           # u inside masked
    assert lib.hb_lt_xor_mask(h, P(e[0]), P(e[1]), P(e[2]), P(e[3]), None, P(o[0]), P(o[2]), count, st) == 2
    assert lib.hb_lt_dmask(h, P(e[0]), P(e[1]), P(e[2]), P(e[3]), P(bits), L - 1, P(e[4]), P(e[5]), P(e[6]), P(e[7]), P(o[0]), P(o[5]), count, st) == 2
    assert lib.hb_lt_dmask(h, P(e[0]), P(e[1]), P(e[2]), P(e[3]), P(bits), L, P(e[4]), P(e[5]), P(e[6]), P(e[7]), P(o[0]), P(buf[0:5]), count, st) == 2
    opened = _random_tensor(ctx, 24, count, 5)
    assert lib.hb_lt_mid(h, P(opened), P(e[0]), P(bits), L + 1, *(P(v) for v in e[1:9]), P(o[0]), P(o[1]), P(o[2]), count, st) == 2
    assert lib.hb_lt_mid(h, P(opened), P(e[0]), P(bits), L, *(P(v) for v in e[1:9]), P(o[0]), P(o[0]), P(o[2]), count, st) == 2          # v is d0
    assert lib.hb_lt_mid(h, P(opened), P(e[0]), P(bits), L, *(P(v) for v in e[1:9]), P(o[0]), P(o[1]), P(o[2]), -3, st) == 2
    assert lib.hb_lt_xor_finish(h, P(opened), P(e[0]), P(e[1]), P(e[2]), P(e[3]), P(e[4]), P(e[0]), count, st) == 2                     # out over u
    assert lib.hb_lt_xor_finish(h, P(opened), P(e[0]), P(e[1]), P(e[2]), P(e[3]), None, P(o[0]), count, st) == 2
    torch.cuda.synchronize()
    assert not buf.any()


# ---- the protocol, end to end over the in-process tagged network ------------------------------------------------------------
def _valid_pairs(p, count, seed, equal_every=4):
    """a, b < (p - 1) / 2: every equal_every-th pair equal, the one after it b = a + 1, the one after that b = a - 1"""
    rnd = random.Random(seed)
    half = (p - 1) // 2
    a = [rnd.randrange(1, half - 1) for _ in range(count)]
    b = [a[i] if i % equal_every == 0 else (a[i] + 1 if i % equal_every == 1 and i % 3 == 0 else (a[i] - 1 if i % equal_every == 1 and i % 3 == 1 else rnd.randrange(half)))
         for i in range(count)]
    return a, b


def _setup(ctx, a, b, r, s, seed, n, rows):
    """upload and deal: -> per-party lists (a, b, r, r_bits, s, s_bits, [p, q, pq]); s None: no second mask"""
    from honeybadgermpc_amd import share_arithmetic as sa

    count = len(a)
    ta, tb, tr = (ctx.upload_ints(v) for v in (a, b, r))
    tp, tq = _random_tensor(ctx, seed, count, rows), _random_tensor(ctx, seed + 1, count, rows)
    tpq = sa.mul(ctx, tp.view(-1, ctx.n_limbs), tq.view(-1, ctx.n_limbs)).view(tp.shape)
    dealt = [_deal(ctx, seed + 10 + k, v, n) for k, v in enumerate((ta, tb, tr, _bit_planes(ctx, tr)))]
    if s is None:
        dealt += [[None] * n, [None] * n]
    else:
        ts = ctx.upload_ints(s)
        dealt += [_deal(ctx, seed + 14 + k, v, n) for k, v in enumerate((ts, _bit_planes(ctx, ts)))]
    return dealt + [[_deal(ctx, seed + 20 + k, v, n) for k, v in enumerate((tp, tq, tpq))]]


def _protocol(p, count, seed, modes, n=4, t=1):
    from honeybadgermpc_amd import share_comparison as sc

    ctx = _ctx(p)
    L = p.bit_length()
    rnd = random.Random(seed)
    a, b = _valid_pairs(p, count, seed + 1)
    r, s = [rnd.randrange(p) for _ in range(count)], [rnd.randrange(p) for _ in range(count)]
    da, db, dr, drb, ds, dsb, dtrip = _setup(ctx, a, b, r, s, seed + 2, n, sc.less_than_triples(L, sc.REFERENCE))

    async def body(co, i):
        got = {}
        tr = tuple(v[i] for v in dtrip)
        held = (da[i], db[i], dr[i], drb[i], ds[i], dsb[i], *tr)
        keep = [v.clone() for v in held] if i == 0 else None
        for mode in modes:
            before = co.batches
            shares = await sc.less_than(co, da[i], db[i], dr[i], drb[i], tr, ds[i], dsb[i], mode)
            batches = co.batches - before
            got[mode] = (ctx.download_ints(await co.open_share_array(shares)), batches)
        if keep:
            assert all(ctx.torch.equal(x, y) for x, y in zip(keep, held)), "inputs were written"
        return got

    results = _run_parties(p, n, t, body)
    for mode in modes:
        want = [sc.less_than_model(x, y, u, v, p, mode)["out"] for x, y, u, v in zip(a, b, r, s)]
        assert want == [1 if x < y else 0 for x, y in zip(a, b)]
        for got in results:
            assert got[mode] == (want, sc.less_than_opens(L, mode)), (count, mode)


@pytest.mark.parametrize("p", (BLS, P64), ids=("bls", "2^64-59"))
@pytest.mark.parametrize("count", (1, 257))
def test_less_than_opens_to_the_model(p, count):
    from honeybadgermpc_amd import share_comparison as sc

    _protocol(p, count, 7000 + count + p % 97, (sc.DIRECT, sc.REFERENCE))


def test_reference_runs_are_replayed():
    """the reference's recorded _prog runs, their draws r and s shared out freshly: REFERENCE mode opens to the reference's result"""
    from honeybadgermpc_amd import share_comparison as sc

    with open(os.path.join(REPO, "tests", "golden", "less_than.json")) as f:
        cases = json.load(f)["cases"]
    p, n = BLS, 4
    ctx = _ctx(p)
    a, b, r, s = ([int(c[k]) for c in cases] for k in "abrs")
    assert len(cases) >= 40
    da, db, dr, drb, ds, dsb, dtrip = _setup(ctx, a, b, r, s, 410, n, sc.less_than_triples(p.bit_length(), sc.REFERENCE))

    async def body(co, i):
        shares = await sc.less_than(co, da[i], db[i], dr[i], drb[i], tuple(v[i] for v in dtrip), ds[i], dsb[i], sc.REFERENCE)
        return ctx.download_ints(await co.open_share_array(shares))

    for got in _run_parties(p, n, 1, body):
        assert got == [int(c["out"]) for c in cases]


def test_less_than_is_the_comparison_on_5000_valid_pairs():
    """5000 pairs a, b < (p - 1) / 2 at a fixed seed, DIRECT mode, a quarter of them equal pairs: the host model alone gives [a < b] for
    every pair, asserted before the device is asked, and so does the device"""
    from honeybadgermpc_amd import share_comparison as sc

    p, count, n, seed = BLS, 5000, 4, 5255
    ctx = _ctx(p)
    L = p.bit_length()
    rnd = random.Random(seed)
    a, b = _valid_pairs(p, count, seed + 1)
    r = [rnd.randrange(p) for _ in range(count)]
    want = [sc.less_than_model(x, y, u, None, p, sc.DIRECT)["out"] for x, y, u in zip(a, b, r)]
    assert want == [1 if x < y else 0 for x, y in zip(a, b)] and sum(x == y for x, y in zip(a, b)) == 1250 and 0 < sum(want) < count
    da, db, dr, drb, _, _, dtrip = _setup(ctx, a, b, r, None, seed + 2, n, sc.less_than_triples(L))

    async def body(co, i):
        shares = await sc.less_than(co, da[i], db[i], dr[i], drb[i], tuple(v[i] for v in dtrip))
        return ctx.download_ints(await co.open_share_array(shares)), co.batches

    for got in _run_parties(p, n, 1, body):
        assert got == (want, sc.less_than_opens(L) + 1)


def test_protocol_arguments_are_checked():
    from honeybadgermpc_amd import share_comparison as sc
    from honeybadgermpc_amd.open_coalescer import OpenCoalescer

    p, count = P64, 3
    ctx = _ctx(p)
    L = p.bit_length()
    co = OpenCoalescer(p, 4, 1, 0, _TaggedNet(4).get_send_recv(0))
    e = [_random_tensor(ctx, 50 + k, count) for k in range(3)]
    bits = _random_tensor(ctx, 60, count, L)
    trip = tuple(_random_tensor(ctx, 61 + k, count, 2 * L) for k in range(3))

    async def main():
        for args, kw in (((e[0], e[1], e[2], bits, trip), {"mode": sc.REFERENCE}),                          # no s, s_bits
                         ((e[0], e[1], e[2], bits, trip), {"mode": sc.REFERENCE, "s": e[0]}),
                         ((e[0], e[1], e[2], bits, trip), {"mode": 3}),
                         ((e[0], e[1][:2], e[2], bits, trip), {}),
                         ((e[0], e[1], e[2], bits[:L - 1], trip), {}),
                         ((e[0], e[1], e[2], bits, tuple(v[:2 * L - 3] for v in trip)), {}),                   # the last xor's row is missing
                         ((e[0], e[1], e[2], bits, tuple(v[:2 * L - 1] for v in trip)), {"mode": sc.REFERENCE, "s": e[0], "s_bits": bits}),
                         ((e[0], e[1], e[2], bits, trip[:2]), {})):
            with pytest.raises(ValueError):
                await sc.less_than(co, *args, **kw)
        empty = await sc.less_than(co, ctx.empty(0), ctx.empty(0), ctx.empty(0), bits[:, :0], tuple(v[:, :0] for v in trip))
        assert tuple(empty.shape) == (0, ctx.n_limbs) and co.batches == 0 and co.opens == 0

    asyncio.run(main())


@pytest.mark.parametrize("count", (1, 257))
@pytest.mark.parametrize("p", (BLS, P64), ids=("bls", "2^64-59"))
def test_every_step_equals_the_host_self_test(p, count):
    """One row body: for every step of csrc/hb_lt.hip the device's output equals, bit for bit, what hb_selftest_lt computes on the host
    from the same random inputs -- the self test runs the rows the kernels run, addressing included.  Both instantiations, L = 255 and
    64; the mask with and without b, the leaves in both modes.  count 1 is one partial workgroup, 257 a second workgroup that holds
    one element."""
    import selftest_cases as stc
    from honeybadgermpc_amd import share_comparison as sc

    ctx = _ctx(p)
    torch, nl, L = ctx.torch, ctx.n_limbs, p.bit_length()
    MASK, LEAVES, XOR_MASK, DMASK, MID, XOR_FINISH = range(6)
    seeds = iter(range(500, 600))

    def rnd(rows=None):
        return _random_tensor(ctx, next(seeds), count, rows)

    def host(what, operands, out_rows, mode=sc.DIRECT):
        rc, outs = stc.run_lt(p, nl, what, [None if o is None else _ints(ctx, o) for o in operands], mode, out_rows, count)
        assert rc == 0
        return [ctx.upload_ints(o) for o in outs]

    def same(dev, want):
        return torch.equal(dev.reshape(-1, nl), want)

    a, b, r, c, w, x, s, u, v = (rnd() for _ in range(9))
    r_bits, s_bits = rnd(L), rnd(L)                                       # a share of a bit is any residue
    ta, tb, tc = ((rnd(), rnd(), rnd()) for _ in range(3))
    assert same(sc.lt_mask(ctx, a, b, r), host(MASK, [a, b, r], [1])[0])
    assert same(sc.lt_mask(ctx, a, None, r), host(MASK, [a, None, r], [1])[0])
    for mode in (sc.DIRECT, sc.REFERENCE):
        g, q = sc.lt_leaves(ctx, c, r_bits, mode)
        h = host(LEAVES, [c, r_bits], [L, L], mode)
        assert same(g, h[0]) and same(q, h[1]), mode
    got = sc.lt_xor_mask(ctx, c, r_bits[0], w, ta[0], ta[1])
    h = host(XOR_MASK, [c, r_bits[0], w, ta[0], ta[1]], [1, 2])
    assert same(got[0], h[0]) and same(got[1], h[1])
    got = sc.lt_dmask(ctx, c, r_bits[0], x, s, s_bits, ta[0], ta[1], tb[0], tb[1])
    h = host(DMASK, [c, r_bits[0], x, s, s_bits, ta[0], ta[1], tb[0], tb[1]], [1, 5], sc.REFERENCE)
    assert same(got[0], h[0]) and same(got[1], h[1])
    opened = rnd(5)
    got = sc.lt_mid(ctx, opened, u, s_bits, ta, tb, tc[0], tc[1])
    h = host(MID, [opened, u, s_bits, *ta, *tb, tc[0], tc[1]], [1, 1, 2], sc.REFERENCE)
    assert same(got[0], h[0]) and same(got[1], h[1]) and same(got[2], h[2])
    opened = rnd(2)
    assert same(sc.lt_xor_finish(ctx, opened, u, v, tc), host(XOR_FINISH, [opened, u, v, *tc], [1])[0])

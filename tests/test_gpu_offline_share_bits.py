"""GPU: the share bits of the offline phase.  The two kernels of csrc/hb_offsb.hip through their wrappers, bit for bit against the host run
of the same rows (hb_selftest_off_share_bits) and against Python ints, at every edge candidate; and the protocol -- share_bits_round on
dealt planes, generate_share_bits with its own sources and with injected ones, generate_less_than_preprocessing handed unchanged to
share_comparison.less_than -- with n parties in one process over an in-process tagged network.  Exact equality."""
import random

import numpy as np
import pytest

from conftest import BLS
from offline_support import _check_sharings, _coefficients, _deal, _run_parties

pytestmark = pytest.mark.gpu

P64 = (1 << 64) - 59
P256 = (1 << 256) - 189
FIELDS = [BLS, P256, P64, 13]
FIELD_IDS = ["bls", "2^256-189", "2^64-59", "13"]
COUNTS = (0, 1, 255, 256, 257, 1000)
LEAVES, FINISH = 0, 1


def _ctx(p):
    from honeybadgermpc_amd._capi import Context

    return Context.get(p)


def _generator(seed):
    import torch

    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return g


def _np(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint64)


def _raw(value, nl):
    return np.array([(value >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(nl)], dtype=np.uint64)


def _host(ctx, what, bits, L, bound, candidates, index, out0, out1, count):
    """the same step on host copies through hb_selftest_off_share_bits"""
    ptr = lambda a: None if a is None else a.ctypes.data
    mod = _raw(ctx.modulus, ctx.n_limbs)
    return ctx.lib.hb_selftest_off_share_bits(mod.ctypes.data, ctx.n_limbs, what, ptr(bits), L, ptr(bound), candidates, ptr(index), ptr(out0), ptr(out1), count)


def _edge_candidates(p):
    """the candidates at which the comparison can go wrong, and p - 1 with each single bit flipped: every leaf position decides once"""
    L = p.bit_length()
    return [0, 1, p - 2, p - 1, p, p + 1, 1 << (L - 1), (1 << L) - 1] + [(p - 1) ^ (1 << i) for i in range(L)]


def _candidates(p, count, rnd):
    """count candidates: the edge candidates first, as many as fit, then random ones"""
    edge = _edge_candidates(p)
    return (edge + [rnd.randrange(1 << p.bit_length()) for _ in range(max(0, count - len(edge)))])[:count]


def _upload_planes(ctx, planes):
    """[L][count] ints -> (L, count, limbs)"""
    L, count = len(planes), len(planes[0])
    flat = [v for plane in planes for v in plane]
    return (ctx.upload_ints(flat) if flat else ctx.empty(0)).view(L, count, ctx.n_limbs)


def _fold(g, q, p):
    G, Q = g[0], q[0]
    for gi, qi in zip(g[1:], q[1:]):
        G, Q = (G + Q * gi) % p, Q * qi % p
    return G


class _Sharings:
    """_check_sharings for many columns: the interpolation through the points 1 .. n as one matrix (its columns are _coefficients of the
    unit vectors), so a column costs n^2 products"""

    def __init__(self, p, n, t):
        self.p, self.n, self.t = p, n, t
        cols = [_coefficients([int(i == j) for i in range(n)], p) for j in range(n)]
        self.rows = [[cols[j][e] for j in range(n)] for e in range(n)]

    def constants(self, per_party):
        """per_party [party][index] -> the constants; every column is of degree <= t"""
        out = []
        for idx in range(len(per_party[0])):
            ys = [per_party[i][idx] for i in range(self.n)]
            for e in range(self.t + 1, self.n):
                assert sum(m * y for m, y in zip(self.rows[e], ys)) % self.p == 0, idx
            out.append(sum(m * y for m, y in zip(self.rows[0], ys)) % self.p)
        return out


# ---- the kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", FIELDS, ids=FIELD_IDS)
def test_kernels_equal_the_host_rows_and_the_model(p):
    from honeybadgermpc_amd import offline

    ctx = _ctx(p)
    torch, nl, L = ctx.torch, ctx.n_limbs, p.bit_length()
    rnd = random.Random(p % 1013)
    for count in COUNTS:
        cands = _candidates(p, count, rnd)
        planes = [[(v >> i) & 1 for v in cands] for i in range(L)]
        bits = _upload_planes(ctx, planes)
        keep = bits.clone()
        # the leaves against p - 1 and against an explicit bound
        for bound in (None, rnd.randrange(1 << L)):
            g, q = offline.sb_leaves(ctx, bits, bound)
            assert tuple(g.shape) == tuple(q.shape) == (L, count, nl) and g.is_contiguous() and q.is_contiguous()
            assert torch.equal(bits, keep), "the leaves wrote their input"
            if not count:
                continue
            hg, hq = np.zeros((L * count, nl), dtype=np.uint64), np.zeros((L * count, nl), dtype=np.uint64)
            assert _host(ctx, LEAVES, _np(bits), L, None if bound is None else _raw(bound, nl), 0, None, hg, hq, count) == 0
            assert np.array_equal(_np(g).reshape(-1, nl), hg) and np.array_equal(_np(q).reshape(-1, nl), hq), (count, bound)
            gi, qi = ctx.download_ints(g.view(-1, nl)), ctx.download_ints(q.view(-1, nl))
            c = p - 1 if bound is None else bound
            some = min(count, 300)                                             # the edge candidates come first: all of them are folded
            roots = [_fold(gi[i::count], qi[i::count], p) for i in range(some)]
            assert roots == [int(v > c) for v in cands[:some]], (count, bound)
        # on residues that are no bits: the affine maps
        if count:
            shares = [[rnd.randrange(p) for _ in range(count)] for _ in range(L)] if count <= 257 else None
            if shares:
                g, q = offline.sb_leaves(ctx, _upload_planes(ctx, shares))
                gi, qi = ctx.download_ints(g.view(-1, nl)), ctx.download_ints(q.view(-1, nl))
                for y in range(L):
                    b = shares[L - 1 - y]
                    one = ((p - 1) >> (L - 1 - y)) & 1
                    assert gi[y * count:(y + 1) * count] == ([0] * count if one else b), (count, y)
                    assert qi[y * count:(y + 1) * count] == (b if one else [(1 - v) % p for v in b]), (count, y)
        # the finish: the kept candidates in order, reversed, repeated
        kept = [i for i, v in enumerate(cands) if v < p]
        for index in (kept, kept[::-1], [kept[0]] * 3 + kept[-2:] + [kept[0]] if kept else [], []):
            idx = torch.tensor(index, dtype=torch.int64, device=ctx.tdev)
            r, r_bits = offline.sb_finish(ctx, bits, idx)
            k = len(index)
            assert tuple(r.shape) == (k, nl) and tuple(r_bits.shape) == (L, k, nl) and r_bits.is_contiguous()
            assert torch.equal(bits, keep) and idx.tolist() == index
            if not k:
                continue
            hr, hb = np.zeros((k, nl), dtype=np.uint64), np.zeros((L * k, nl), dtype=np.uint64)
            assert _host(ctx, FINISH, _np(bits), L, None, count, np.array(index, dtype=np.int64), hr, hb, k) == 0
            assert np.array_equal(_np(r), hr) and np.array_equal(_np(r_bits).reshape(-1, nl), hb), (count, k)
            assert ctx.download_ints(r) == [offline.share_bits_model([planes[i][c] for i in range(L)], p)[0] for c in index] == [cands[c] for c in index]
            assert torch.equal(r_bits, bits[:, idx]), (count, k)
    # shares, not bits, in the planes: r = sum_q 2^q b_q mod p
    shares = [[rnd.randrange(p) for _ in range(300)] for _ in range(L)]
    idx = torch.tensor([299, 0, 256, 255, 17], dtype=torch.int64, device=ctx.tdev)
    r, r_bits = offline.sb_finish(ctx, _upload_planes(ctx, shares), idx)
    assert ctx.download_ints(r) == [sum(shares[q][c] << q for q in range(L)) % p for c in idx.tolist()]
    assert ctx.download_ints(r_bits.view(-1, nl)) == [shares[q][c] for q in range(L) for c in idx.tolist()]


def test_an_index_out_of_range_is_never_an_address():
    """the wrapper refuses it; the entry point, asked directly, zeroes the slot and writes nothing else"""
    from honeybadgermpc_amd import offline

    p = BLS
    ctx = _ctx(p)
    torch, nl, L, count = ctx.torch, ctx.n_limbs, 255, 40
    rnd = random.Random(9)
    bits = _upload_planes(ctx, [[rnd.randrange(p) for _ in range(count)] for _ in range(L)])
    index = [3, -1, count, 0, 1 << 40, -(1 << 63), (1 << 63) - 1, count - 1]
    idx = torch.tensor(index, dtype=torch.int64, device=ctx.tdev)
    with pytest.raises(ValueError):
        offline.sb_finish(ctx, bits, idx)
    k = len(index)
    r = torch.full((k + 1, nl), 7, dtype=torch.int64, device=ctx.tdev)
    r_bits = torch.full((L * k + 1, nl), 7, dtype=torch.int64, device=ctx.tdev)
    assert ctx.lib.hb_off_sb_finish(ctx.h, ctx.ptr(bits), L, count, ctx.ptr(idx), ctx.ptr(r), ctx.ptr(r_bits), k, ctx.stream()) == 0
    torch.cuda.synchronize()
    assert (r[k:] == 7).all() and (r_bits[L * k:] == 7).all()
    planes = r_bits[:L * k].view(L, k, nl)
    for j, c in enumerate(index):
        if 0 <= c < count:
            assert torch.equal(planes[:, j], bits[:, c])
        else:
            assert not planes[:, j].any() and not r[j].any(), (j, c)


def test_wrappers_and_entry_points_refuse_bad_arguments():
    from honeybadgermpc_amd import offline

    ctx = _ctx(BLS)
    torch, nl, L, count = ctx.torch, ctx.n_limbs, 255, 6
    bits = ctx.upload_ints([1] * (L * count)).view(L, count, nl)
    idx = torch.arange(count, dtype=torch.int64, device=ctx.tdev)
    keep = bits.clone()
    for bad in (bits[:-1], bits.view(L * count, nl), bits[:, :, :3], bits.transpose(0, 1), bits[:, ::2], ctx.upload_ints([1] * (L * count)).view(count, L, nl).transpose(0, 1),
                bits.cpu(), bits.to(torch.int32), None):
        with pytest.raises((ValueError, TypeError)):
            offline.sb_leaves(ctx, bad)
        with pytest.raises((ValueError, TypeError)):
            offline.sb_finish(ctx, bad, idx)
    for bad in (bits[:-1], bits.view(L * count, nl), bits.transpose(0, 1), bits[:, ::2]):          # shapes and strides: ValueError
        with pytest.raises(ValueError):
            offline.sb_leaves(ctx, bad)
    for bound in (-1, 1 << 255, 1 << 256, 1.0, True, "3"):
        with pytest.raises(ValueError):
            offline.sb_leaves(ctx, bits, bound)
    for bad in (idx.to(torch.int32), idx.cpu(), idx.view(count, 1), list(range(count)), None, torch.arange(2 * count, dtype=torch.int64, device=ctx.tdev)[::2],
                torch.tensor([0, count], device=ctx.tdev), torch.tensor([-1], device=ctx.tdev)):
        with pytest.raises(ValueError):
            offline.sb_finish(ctx, bits, bad)
    st, P = ctx.stream(), ctx.ptr
    leaves, finish = ctx.lib.hb_off_sb_leaves, ctx.lib.hb_off_sb_finish
    g, q = torch.zeros_like(bits), torch.zeros_like(bits)
    r = torch.zeros_like(ctx.empty(count))
    for bad_L in (254, 256, 0, -1):
        assert leaves(ctx.h, P(bits), bad_L, None, P(g), P(q), count, st) == 2 and finish(ctx.h, P(bits), bad_L, count, P(idx), P(r), P(g), count, st) == 2
    assert leaves(ctx.h, P(bits), L, None, P(g), P(q), -1, st) == 2 and finish(ctx.h, P(bits), L, count, P(idx), P(r), P(g), -1, st) == 2
    assert finish(ctx.h, P(bits), L, -1, P(idx), P(r), P(g), count, st) == 2
    assert leaves(ctx.h, None, L, None, P(g), P(q), count, st) == 2 and leaves(ctx.h, P(bits), L, None, None, P(q), count, st) == 2
    assert leaves(ctx.h, P(bits), L, None, P(g), None, count, st) == 2
    assert finish(ctx.h, None, L, count, P(idx), P(r), P(g), count, st) == 2 and finish(ctx.h, P(bits), L, count, None, P(r), P(g), count, st) == 2
    assert finish(ctx.h, P(bits), L, count, P(idx), None, P(g), count, st) == 2 and finish(ctx.h, P(bits), L, count, P(idx), P(r), None, count, st) == 2
    big, fits = _raw(1 << 255, nl), _raw((1 << 255) - 1, nl)
    assert leaves(ctx.h, P(bits), L, big.ctypes.data, P(g), P(q), count, st) == 2 and leaves(ctx.h, P(bits), L, big.ctypes.data, P(g), P(q), 0, st) == 2
    assert leaves(ctx.h, None, L, fits.ctypes.data, None, None, 0, st) == 0
    assert leaves(ctx.h, P(bits), L, None, P(bits), P(q), count, st) == 2 and leaves(ctx.h, P(bits), L, None, P(g), P(g), count, st) == 2
    assert finish(ctx.h, P(bits), L, count, P(idx), P(r), P(bits), count, st) == 2 and finish(ctx.h, P(bits), L, count, P(idx), P(g), P(g), count, st) == 2
    assert finish(ctx.h, P(bits), L, count, P(idx), P(idx), P(g), count, st) == 2
    assert leaves(ctx.h, None, L, None, None, None, 0, st) == 0 and finish(ctx.h, None, L, 0, None, None, None, 0, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(bits, keep) and not g.any() and not q.any() and not r.any(), "a refused call wrote"


# ---- one round on dealt planes ----------------------------------------------------------------------------------------------
_TRIPLE_POOL = 61                                  # dealt triples, reused across rows and candidates (a prime: no row repeats a pattern)


def _dealt_round(p, n, t, cands, seed, planes=None):
    """-> per party (bits [L][m] ints, pool: 3 lists of _TRIPLE_POOL ints): the bit planes of the candidates dealt with _deal at degree
    t, and a pool of triples dealt the same way"""
    L, m = p.bit_length(), len(cands)
    rnd = random.Random(seed)
    planes = planes or [[(v >> i) & 1 for v in cands] for i in range(L)]
    dealt = [[_deal(b, t, n, p, rnd) for b in plane] for plane in planes]                       # [plane][candidate][party]
    pool = []
    for _ in range(_TRIPLE_POOL):
        a, b = rnd.randrange(p), rnd.randrange(p)
        pool.append((_deal(a, t, n, p, rnd), _deal(b, t, n, p, rnd), _deal(a * b % p, t, n, p, rnd)))
    return [([[dealt[q][c][i] for c in range(m)] for q in range(L)], tuple([tr[part][i] for tr in pool] for part in range(3))) for i in range(n)]


def _tile_triples(ctx, pool, m):
    """a party's pool -> triples (p, q, pq), each (2 L - 3, m, limbs): element e is triple e mod _TRIPLE_POOL of the pool"""
    rows = 2 * ctx.modulus.bit_length() - 3
    which = ctx.torch.arange(rows * m, device=ctx.tdev) % _TRIPLE_POOL
    return tuple(ctx.upload_ints(part)[which].view(rows, m, ctx.n_limbs).contiguous() for part in pool)


ROUND_CASES = [(BLS, 4, 1), (P64, 4, 1), (BLS, 7, 2)]


@pytest.mark.parametrize("p, n, t", ROUND_CASES, ids=["bls-4-1", "2^64-59-4-1", "bls-7-2"])
def test_share_bits_round_on_the_edge_candidates(p, n, t):
    from honeybadgermpc_amd import offline
    from honeybadgermpc_amd.progs.fixedpoint import carry_levels

    ctx = _ctx(p)
    nl, L = ctx.n_limbs, p.bit_length()
    cands = _edge_candidates(p)
    m = len(cands)
    dealt = _dealt_round(p, n, t, cands, 100 * n + L)

    async def body(co, i):
        bits = _upload_planes(ctx, dealt[i][0])
        trip = _tile_triples(ctx, dealt[i][1], m)
        keep =[v.clone() for v in (bits,) + trip]
        before = co.batches
        r, r_bits, verdicts = await offline.share_bits_round(co, bits, trip)
        assert co.batches - before == carry_levels(L - 1) + 1                 # the tree's levels and the verdicts' open
        assert all(ctx.torch.equal(v, w) for v, w in zip((bits,) + trip, keep)), "the round wrote its inputs"
        kept = int(verdicts.sum())
        assert verdicts.dtype == ctx.torch.bool and tuple(verdicts.shape) == (m,)
        assert tuple(r.shape) == (kept, nl) and tuple(r_bits.shape) == (L, kept, nl)
        empty = await offline.share_bits_round(co, bits[:, :0].contiguous(), tuple(v[:, :0].contiguous() for v in trip))
        assert co.batches - before == carry_levels(L - 1) + 1 and [tuple(v.shape) for v in empty] == [(0, nl), (L, 0, nl), (0,)]
        return verdicts.tolist(), ctx.download_ints(r), ctx.download_ints(r_bits.reshape(-1, nl))

    results = _run_parties(p, n, t, body)
    accepted = [v for v in cands if v < p]
    for verdicts, _, _ in results:
        assert verdicts == [v < p for v in cands]
    assert _check_sharings(p, n, t, [res[1] for res in results]) == accepted                  # degree <= t, the kept candidates in order
    bits_open = _Sharings(p, n, t).constants([res[2] for res in results])
    assert bits_open == [(v >> q) & 1 for q in range(L) for v in accepted]


@pytest.mark.parametrize("p", (BLS, P64), ids=("bls", "2^64-59"))
def test_a_plane_that_is_no_bit_raises_on_every_party(p):
    """the top plane a sharing of 2 over lower bits that are all 1: the leaf (0, 2) scales the first g = 1 below it, the verdict opens to 2"""
    from honeybadgermpc_amd import offline
    from honeybadgermpc_amd.exceptions import HoneyBadgerMPCError

    n, t = 4, 1
    ctx = _ctx(p)
    L = p.bit_length()
    cands = [0, p - 1, (1 << L) - 1, 5]
    planes = [[(v >> i) & 1 for v in cands] for i in range(L)]
    planes[L - 1][2] = 2
    dealt = _dealt_round(p, n, t, cands, 77, planes)

    async def body(co, i):
        return await offline.share_bits_round(co, _upload_planes(ctx, dealt[i][0]), _tile_triples(ctx, dealt[i][1], len(cands)))

    results = _run_parties(p, n, t, body, return_exceptions=True)
    assert all(isinstance(r, HoneyBadgerMPCError) for r in results), results


# ---- the generator ----------------------------------------------------------------------------------------------------------
def _check_share_bits(p, n, t, results, count):
    """results [party] = (r ints, r_bits ints flat [L][count]): degree <= t, r < p, planes of 0 / 1, sum_i 2^i bit_i = r -> the r"""
    L = p.bit_length()
    assert all(len(res[0]) == count and len(res[1]) == L * count for res in results)
    r = _check_sharings(p, n, t, [res[0] for res in results])
    planes = _Sharings(p, n, t).constants([res[1] for res in results])
    assert all(v < p for v in r) and set(planes) <= {0, 1}
    assert r == [sum(planes[q * count + j] << q for q in range(L)) for j in range(count)]
    return r


@pytest.mark.parametrize("p", (BLS, P64), ids=("bls", "2^64-59"))
def test_generate_share_bits(p):
    from honeybadgermpc_amd import offline

    n, t, count = 4, 1, 5
    ctx = _ctx(p)
    nl, L = ctx.n_limbs, p.bit_length()

    async def body(co, i):
        r, r_bits = await offline.generate_share_bits(co, count, generator=_generator(2100 + i))
        assert tuple(r.shape) == (count, nl) and tuple(r_bits.shape) == (L, count, nl) and r.is_contiguous() and r_bits.is_contiguous()
        return ctx.download_ints(r), ctx.download_ints(r_bits.view(-1, nl))

    r = _check_share_bits(p, n, t, _run_parties(p, n, t, body), count)
    assert len(set(r)) == count


def test_generate_share_bits_draws_again_when_a_round_keeps_too_few():
    """an injected bit source whose first round holds more candidates >= p than below: a second round under another tag makes up for it"""
    from honeybadgermpc_amd import offline

    p, n, t, count = BLS, 4, 1, 5
    ctx = _ctx(p)
    nl, L = ctx.n_limbs, p.bit_length()
    m0 = offline.share_bits_candidates(p, count)
    calls = [[] for _ in range(n)]
    dealt = {}

    def planes_of(tag, k):
        """every party deals the same polynomials for a tag: [plane * m + candidate][party]"""
        if tag not in dealt:
            rnd = random.Random(len(dealt) + 31)
            m = k // L
            first = not dealt
            cands = [(1 << L) - 1 - c if first and c >= 2 else rnd.randrange(p) for c in range(m)]            # round 0 keeps two
            dealt[tag] = (cands, [_deal((v >> q) & 1, t, n, p, rnd) for q in range(L) for v in cands])
        return dealt[tag]

    async def body(co, i):
        async def bit_source(branch, k, tag):
            assert k % L == 0 and branch.myid == i
            calls[i].append((tag, k))
            return ctx.upload_ints([share[i] for share in planes_of(tag, k)[1]])

        r, r_bits = await offline.generate_share_bits(co, count, generator=_generator(2200 + i), bit_source=bit_source)
        return ctx.download_ints(r), ctx.download_ints(r_bits.view(-1, nl))

    results = _run_parties(p, n, t, body)
    r = _check_share_bits(p, n, t, results, count)
    assert all(c == calls[0] for c in calls) and len(calls[0]) == 2
    (tag0, k0), (tag1, k1) = calls[0]
    assert tag0 != tag1 and k0 == L * m0 and k1 == L * offline.share_bits_candidates(p, count - 2)
    kept = [v for tag in (tag0, tag1) for v in dealt[tag][0] if v < p]
    assert r == kept[:count] and len(kept) >= count                                                # in order, the surplus dropped


def test_generate_share_bits_in_chunks():
    from honeybadgermpc_amd import offline

    p, n, t, count, chunk = BLS, 4, 1, 5, 3
    ctx = _ctx(p)
    nl, L = ctx.n_limbs, p.bit_length()
    calls = [[] for _ in range(n)]

    async def body(co, i):
        gen_bits, gen_triples = _generator(2300 + i), _generator(2350 + i)

        async def bit_source(branch, k, tag):
            calls[i].append((tag, k))
            return await offline.generate_bits(branch, k, encoding=offline.ZERO_ONE, tag=tag, generator=gen_bits)

        async def triple_source(branch, k, tag):
            return await offline.generate_triples(branch, k, tag=tag, generator=gen_triples)

        r, r_bits = await offline.generate_share_bits(co, count, chunk=chunk, bit_source=bit_source, triple_source=triple_source)
        return ctx.download_ints(r), ctx.download_ints(r_bits.view(-1, nl))

    results = _run_parties(p, n, t, body)
    _check_share_bits(p, n, t, results, count)
    assert all(c == calls[0] for c in calls) and len(calls[0]) >= 2 and len({tag for tag, _ in calls[0]}) == len(calls[0])
    assert all(k <= L * chunk for _, k in calls[0]) and calls[0][0][1] == L * chunk


def test_generate_share_bits_aborts_with_randousha():
    """a perturbed H1 share of the bit source's randousha: every party raises HoneyBadgerMPCError, and none waits for a message that will
    not come -- the triple source's branch ends with the call"""
    from honeybadgermpc_amd import offline, wire
    from honeybadgermpc_amd.exceptions import HoneyBadgerMPCError

    p, n, t = BLS, 4, 1

    def flat(tag):
        return [x for part in tag for x in (flat(part) if isinstance(part, tuple) else [part])]

    def hook(sender, tag, dest, msg):
        names = flat(tag)
        if names[-1] == "H1" and "bits" in names and sender == 1 and dest == 2:
            values = wire.unpack_ints(msg)
            values[0] += 1
            return wire.pack_ints([v % p for v in values], p)
        return msg

    async def body(co, i):
        return await offline.generate_share_bits(co, 3, generator=_generator(2500 + i))

    results = _run_parties(p, n, t, body, hook, return_exceptions=True)
    assert all(isinstance(r, HoneyBadgerMPCError) for r in results), results


# ---- end to end: less-than on preprocessing no dealer made --------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("DIRECT", "REFERENCE"))
def test_less_than_on_generated_preprocessing(mode):
    from honeybadgermpc_amd import offline, share_comparison as sc

    p, n, t, count = BLS, 4, 1, 6
    mode = getattr(sc, mode)
    ctx = _ctx(p)
    nl, L = ctx.n_limbs, p.bit_length()
    rnd = random.Random(41)
    half = (p - 1) // 2                                                        # operands lie below it
    x, y = rnd.randrange(half - 1), rnd.randrange(half)
    pairs = [(min(x, y), max(x, y) + 1), (max(x, y) + 1, min(x, y)), (x, x), (y, y + 1), (0, rnd.randrange(1, half)), (rnd.randrange(half), (p - 3) // 2)]
    assert len(pairs) == count and all(0 <= a < half and 0 <= b < half for a, b in pairs)
    slopes = [(rnd.randrange(p), rnd.randrange(p)) for _ in pairs]

    async def body(co, i):
        pre = await offline.generate_less_than_preprocessing(co, count, mode=mode, generator=_generator(2400 + i))
        assert tuple(pre.r.shape) == (count, nl) and tuple(pre.r_bits.shape) == (L, count, nl)
        assert all(tuple(v.shape) == (sc.less_than_triples(L, mode), count, nl) for v in pre.triples)
        if mode == sc.DIRECT:
            assert pre.s is None and pre.s_bits is None
        else:
            assert tuple(pre.s.shape) == (count, nl) and tuple(pre.s_bits.shape) == (L, count, nl)
        a = ctx.upload_ints([(v + (i + 1) * s) % p for (v, _), (s, _) in zip(pairs, slopes)])
        b = ctx.upload_ints([(v + (i + 1) * s) % p for (_, v), (_, s) in zip(pairs, slopes)])
        out = await sc.less_than(co, a, b, pre.r, pre.r_bits, pre.triples, pre.s, pre.s_bits, mode)
        return ctx.download_ints(await co.open_share_array(out))

    for opened in _run_parties(p, n, t, body):
        assert opened == [int(a < b) for a, b in pairs]

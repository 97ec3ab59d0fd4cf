"""GPU: honeybadgermpc_amd.power_mixing -- the kernels of csrc/hb_pm.hip through the tensor-level functions and the power-mixing
protocol over an OpenCoalescer -- against Python ints and the binomial formula [a^m] = sum_j C(m, j) c^(m-j) [b^j].
Exact equality everywhere."""
import asyncio
import random

import numpy as np
import pytest

from conftest import BLS

pytestmark = pytest.mark.gpu

GOLDILOCKS = 0xFFFFFFFF00000001
P64 = (1 << 64) - 59
FIELDS = [BLS, (1 << 256) - 189, P64, GOLDILOCKS]
FIELD_IDS = ["bls", "2^256-189", "2^64-59", "goldilocks"]


def _ctx(p):
    from honeybadgermpc_amd._capi import Context

    return Context.get(p)


def _binomial_rows(p, k):
    rows, row = [], [1]
    for _ in range(k):
        row = [1] + [(row[i] + row[i + 1]) % p for i in range(len(row) - 1)] + [1]
        rows.append(row)
    return rows                                     # rows[m - 1][j] = C(m, j) mod p


def _powers_ref(p, c, shares, k, binom, ms=None):
    """[a^m] for m in ms (default 1 .. k) from c and the values standing for [b^1] .. [b^k]"""
    b = [1] + list(shares)
    cp = [1]
    for _ in range(k):
        cp.append(cp[-1] * c % p)
    return [sum(binom[m - 1][j] * (cp[m - j] * b[j] % p) for j in range(m + 1)) % p for m in (ms or range(1, k + 1))]


def _draw(rnd, p, m, k):
    cs = [rnd.choice([0, 1, p - 1, rnd.randrange(p), rnd.randrange(p)]) for _ in range(m)]
    powers = [[rnd.choice([0, 1, p - 1, rnd.randrange(p), rnd.randrange(p), rnd.randrange(p)]) for _ in range(k)] for _ in range(m)]
    if m:
        cs[0] = 0
    return cs, powers


def _upload(ctx, cs, powers, k):
    m = len(cs)
    flat = [x for row in powers for x in row]
    pw = ctx.upload_ints(flat).reshape(m, k, ctx.n_limbs) if m else ctx.empty(0).reshape(0, k, ctx.n_limbs)
    return (ctx.upload_ints(cs) if m else ctx.empty(0)), pw


def _random_tensor(ctx, seed, count):
    """`count` uniform canonical residues made on the device side (numpy limbs, reduced by hb_reduce)"""
    g = np.random.default_rng(seed)
    limbs = g.integers(-(1 << 63), (1 << 63) - 1, size=(count, ctx.n_limbs), dtype=np.int64, endpoint=True)
    return ctx.reduce_(ctx.to_device(limbs))


@pytest.mark.parametrize("p", FIELDS, ids=FIELD_IDS)
def test_direct_path_and_powers_equal_python_ints(p):
    from honeybadgermpc_amd import power_mixing as pm

    ctx = _ctx(p)
    rnd = random.Random(p % 997)
    for k in (1, 2, 27, 28, 29, 100, 128):
        binom = _binomial_rows(p, k)
        for m in sorted({0, 1, 3, k, 2 * k}):
            cs, powers = _draw(rnd, p, m, k)
            c_dev, p_dev = _upload(ctx, cs, powers, k)
            want = [_powers_ref(p, c, row, k, binom) for c, row in zip(cs, powers)]
            got = pm.powers_from_masked(ctx, c_dev, p_dev)
            assert tuple(got.shape) == (m, k, ctx.n_limbs)
            assert ctx.download_ints(got.reshape(-1, ctx.n_limbs)) == [x for row in want for x in row], (k, m)
            if m:
                assert want[0] == powers[0]                      # c = 0 passes [b^m] through
            sums = pm.local_power_sums(ctx, c_dev, p_dev, method="direct")
            assert ctx.download_ints(sums) == [sum(row[i] for row in want) % p for i in range(k)], (k, m)


def test_direct_path_k_1000_sampled():
    from honeybadgermpc_amd import power_mixing as pm

    p, k, m = BLS, 1000, 5
    ctx = _ctx(p)
    rnd = random.Random(11)
    cs, powers = _draw(rnd, p, m, k)
    c_dev, p_dev = _upload(ctx, cs, powers, k)
    binom = _binomial_rows(p, k)
    ms = [1, 2, 255, 256, 257, 512, 999, 1000]
    want = [_powers_ref(p, c, row, k, binom, ms) for c, row in zip(cs, powers)]
    got = ctx.download_ints(pm.powers_from_masked(ctx, c_dev, p_dev).reshape(-1, ctx.n_limbs))
    assert [[got[c * k + mm - 1] for mm in ms] for c in range(m)] == want
    sums = ctx.download_ints(pm.local_power_sums(ctx, c_dev, p_dev, method="direct"))
    assert [sums[mm - 1] for mm in ms] == [sum(row[i] for row in want) % p for i in range(len(ms))]
    assert sums == [sum(got[c * k + i] for c in range(m)) % p for i in range(k)]


@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 1000, 1024, 2048, 4096])
@pytest.mark.parametrize("p", [BLS, GOLDILOCKS], ids=["bls", "goldilocks"])
def test_ntt_path_bit_equal_to_the_direct_path(p, k):
    from honeybadgermpc_amd import power_mixing as pm

    ctx = _ctx(p)
    m = min(k, 1024)
    c_dev = _random_tensor(ctx, 1000 + k, m)
    p_dev = _random_tensor(ctx, 2000 + k, m * k).reshape(m, k, ctx.n_limbs)
    direct = pm.local_power_sums(ctx, c_dev, p_dev, method="direct")
    ntt = pm.local_power_sums(ctx, c_dev, p_dev, method="ntt")
    assert ctx.torch.equal(direct, ntt)
    auto = pm.local_power_sums(ctx, c_dev, p_dev, method="auto")
    assert ctx.torch.equal(direct, auto)
    if k == 1024:
        ms = [1, 2, 27, 28, 500, 777, 1023, 1024]
        cs = ctx.download_ints(c_dev)
        flat = ctx.download_ints(p_dev.reshape(-1, ctx.n_limbs))
        binom = _binomial_rows(p, k)
        want = [0] * len(ms)
        for c in range(m):
            row = _powers_ref(p, cs[c], flat[c * k:(c + 1) * k], k, binom, ms)
            want = [(w + r) % p for w, r in zip(want, row)]
        got = ctx.download_ints(ntt)
        assert [got[mm - 1] for mm in ms] == want


@pytest.mark.parametrize("p", [BLS, GOLDILOCKS], ids=["bls", "goldilocks"])
def test_slab_boundary_inside_the_clients(p):
    """a cap on the working set small enough that 37 clients take several slabs (the last one ragged), both paths"""
    from honeybadgermpc_amd import power_mixing as pm

    ctx = _ctx(p)
    k, m = 65, 37
    c_dev = _random_tensor(ctx, 5, m)
    p_dev = _random_tensor(ctx, 6, m * k).reshape(m, k, ctx.n_limbs)
    whole = [pm.local_power_sums(ctx, c_dev, p_dev, method=meth) for meth in ("direct", "ntt")]
    whole_powers = pm.powers_from_masked(ctx, c_dev, p_dev)
    ctx.torch.cuda.synchronize()
    per_client = (2 * (k + 1) + 2 * pm.transform_order(k)) * ctx.nbytes
    try:
        ctx.lib.hb_debug_pm_slab_bytes(5 * per_client)         # five clients a slab on the NTT path, ten on the direct one
        parts = [pm.local_power_sums(ctx, c_dev, p_dev, method=meth) for meth in ("direct", "ntt")]
        parts_powers = pm.powers_from_masked(ctx, c_dev, p_dev)
        ctx.torch.cuda.synchronize()
    finally:
        ctx.lib.hb_debug_pm_slab_bytes(0)
    assert ctx.torch.equal(whole[0], whole[1])
    assert ctx.torch.equal(parts[0], whole[0]) and ctx.torch.equal(parts[1], whole[0])
    assert ctx.torch.equal(parts_powers, whole_powers)
    flat = ctx.download_ints(whole_powers.reshape(-1, ctx.n_limbs))
    assert ctx.download_ints(whole[0]) == [sum(flat[c * k + i] for c in range(m)) % p for i in range(k)]


def test_prime_without_the_root_of_unity():
    from honeybadgermpc_amd import power_mixing as pm
    from honeybadgermpc_amd._capi import HB_ERR_UNSUPPORTED, HB_PM_NTT

    p, k, m = P64, 100, 7                                      # p - 1 = 2 * odd: no root of order 256
    ctx = _ctx(p)
    rnd = random.Random(3)
    cs, powers = _draw(rnd, p, m, k)
    c_dev, p_dev = _upload(ctx, cs, powers, k)
    auto = pm.local_power_sums(ctx, c_dev, p_dev, method="auto")
    assert ctx.torch.equal(auto, pm.local_power_sums(ctx, c_dev, p_dev, method="direct"))
    binom = _binomial_rows(p, k)
    want = [_powers_ref(p, c, row, k, binom) for c, row in zip(cs, powers)]
    assert ctx.download_ints(auto) == [sum(row[i] for row in want) % p for i in range(k)]
    with pytest.raises(ValueError):
        pm.local_power_sums(ctx, c_dev, p_dev, method="ntt")
    out = ctx.empty(k)
    assert ctx.lib.hb_pm_power_sums(ctx.h, ctx.ptr(c_dev), ctx.ptr(p_dev), m, k, HB_PM_NTT, None, 0, ctx.ptr(out), ctx.stream()) == HB_ERR_UNSUPPORTED


def test_inputs_untouched_arguments_checked_and_asynchronous():
    from honeybadgermpc_amd import power_mixing as pm
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd._capi import HB_ERR_BAD_ARG

    p, k, m = BLS, 70, 9
    ctx = _ctx(p)
    torch = ctx.torch
    rnd = random.Random(4)
    cs, powers = _draw(rnd, p, m, k)
    c_dev, p_dev = _upload(ctx, cs, powers, k)
    c_copy, p_copy = c_dev.clone(), p_dev.clone()
    binom = _binomial_rows(p, k)
    want = [_powers_ref(p, c, row, k, binom) for c, row in zip(cs, powers)]
    sums_want = [sum(row[i] for row in want) % p for i in range(k)]
    # results consumed on the current stream without a synchronise: S + S through another kernel of the library
    for meth in ("direct", "ntt"):
        s = pm.local_power_sums(ctx, c_dev, p_dev, method=meth)
        twice = sa.add(ctx, s, s)
        assert ctx.download_ints(twice) == [2 * x % p for x in sums_want]
    pw = pm.powers_from_masked(ctx, c_dev, p_dev)
    neg = sa.neg(ctx, pw.reshape(-1, ctx.n_limbs))
    assert ctx.download_ints(neg) == [-x % p for row in want for x in row]
    # on a side stream as well
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s2 = pm.local_power_sums(ctx, c_dev, p_dev, method="ntt")
        twice = sa.add(ctx, s2, s2)
    side.synchronize()
    assert ctx.download_ints(twice) == [2 * x % p for x in sums_want]
    assert torch.equal(c_dev, c_copy) and torch.equal(p_dev, p_copy)
    assert pw.data_ptr() != p_dev.data_ptr() and s2.data_ptr() not in (c_dev.data_ptr(), p_dev.data_ptr())
    # a strided view of the powers is taken as its values
    wide = torch.zeros((m, k + 3, ctx.n_limbs), dtype=torch.int64, device=ctx.tdev)
    wide[:, :k] = p_dev
    assert ctx.download_ints(pm.local_power_sums(ctx, c_dev, wide[:, :k], method="direct")) == sums_want
    # argument checks raise before C
    with pytest.raises(ValueError):
        pm.local_power_sums(ctx, c_dev, p_dev, method="fast")
    with pytest.raises(ValueError):
        pm.local_power_sums(ctx, c_dev, p_dev.reshape(m * k, ctx.n_limbs))
    with pytest.raises(ValueError):
        pm.local_power_sums(ctx, c_dev[:-1], p_dev)
    with pytest.raises(ValueError):
        pm.powers_from_masked(ctx, c_dev, p_dev[:, :0])
    with pytest.raises(TypeError):
        pm.powers_from_masked(ctx, c_dev.to(torch.int32), p_dev)
    with pytest.raises(ValueError):
        pm.powers_from_masked(ctx, c_dev.cpu(), p_dev)
    small = _ctx(13)
    with pytest.raises(ValueError):
        pm.local_power_sums(small, small.upload_ints([1]), small.upload_ints([1] * 13).reshape(1, 13, 1))
    assert small.download_ints(pm.local_power_sums(small, small.upload_ints([5]), small.upload_ints([pow(3, j, 13) for j in range(1, 13)]).reshape(1, 12, 1))) == [
        pow(8, j, 13) for j in range(1, 13)]
    # ... and the C ABI refuses what gets past Python
    lib, out = ctx.lib, ctx.empty(k)
    st = ctx.stream()
    assert lib.hb_pm_power_sums(ctx.h, ctx.ptr(c_dev), ctx.ptr(p_dev), m, 0, 0, None, 0, ctx.ptr(out), st) == HB_ERR_BAD_ARG
    assert lib.hb_pm_power_sums(ctx.h, ctx.ptr(c_dev), ctx.ptr(p_dev), -1, k, 0, None, 0, ctx.ptr(out), st) == HB_ERR_BAD_ARG
    assert lib.hb_pm_power_sums(ctx.h, None, ctx.ptr(p_dev), m, k, 0, None, 0, ctx.ptr(out), st) == HB_ERR_BAD_ARG
    assert lib.hb_pm_power_sums(ctx.h, ctx.ptr(c_dev), ctx.ptr(p_dev), m, k, 0, None, 0, None, st) == HB_ERR_BAD_ARG
    assert lib.hb_pm_power_sums(ctx.h, ctx.ptr(c_dev), ctx.ptr(p_dev), m, k, 9, None, 0, ctx.ptr(out), st) == HB_ERR_BAD_ARG
    assert lib.hb_pm_powers(ctx.h, ctx.ptr(c_dev), None, m, k, ctx.ptr(out), st) == HB_ERR_BAD_ARG
    assert lib.hb_pm_powers(small.h, None, None, 1, 13, None, st) == HB_ERR_BAD_ARG
    # no clients: zeros
    out.fill_(7)
    assert lib.hb_pm_power_sums(ctx.h, None, None, 0, k, 0, None, 0, ctx.ptr(out), st) == 0
    assert ctx.download_ints(out) == [0] * k
    # the temporaries go back with the cache
    ctx.cache_clear()
    assert ctx.download_ints(pm.local_power_sums(ctx, c_dev, p_dev, method="ntt")) == sums_want


# ---- the protocol, end to end over the in-process tagged network of tests/test_gpu_share_arithmetic.py ---------------------
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


@pytest.mark.parametrize("n, t, liars", [(4, 1, 0), (7, 2, 0), (4, 1, 1), (7, 2, 2)])
@pytest.mark.parametrize("k", [16, 64])
def test_power_mix_end_to_end(n, t, liars, k):
    from honeybadgermpc_amd import power_mixing as pm
    from honeybadgermpc_amd import wire
    from honeybadgermpc_amd.open_coalescer import OpenCoalescer

    p = BLS
    ctx = _ctx(p)
    rnd = random.Random(1000 * n + 10 * k + liars)
    msgs = [rnd.randrange(p) for _ in range(k)]
    msgs[0], msgs[1] = 0, p - 1
    bs = [rnd.randrange(p) for _ in range(k)]
    msg_shares = _deal(rnd, p, n, t, msgs)                                               # [party][client]
    pow_shares = _deal(rnd, p, n, t, [pow(b, j, p) for b in bs for j in range(1, k + 1)])   # [party][client * k + j - 1]
    bad = set(rnd.sample(range(n), liars))

    def garble(msg):
        tag, blob = msg
        count = wire.unpack_limbs(blob).shape[0]
        return (tag, wire.pack_ints([rnd.randrange(p) for _ in range(count)], p))

    async def party(i, net):
        co = OpenCoalescer(p, n, t, i, net.get_send_recv(i, garble if i in bad else None))
        sums = await pm.power_mix(co, ctx.upload_ints(msg_shares[i]), ctx.upload_ints(pow_shares[i]).reshape(k, k, ctx.n_limbs))
        return ctx.download_ints(sums)

    async def main():
        net = _TaggedNet(n)
        return await asyncio.gather(*[party(i, net) for i in range(n)])

    results = asyncio.run(main())
    want = [sum(pow(a, m, p) for a in msgs) % p for m in range(1, k + 1)]
    for i in range(n):
        if i in bad:
            continue
        assert results[i] == want, i
        coeffs = pm.newton_coefficients(results[i], p)
        assert coeffs[k] == 1 and all(sum(c * pow(a, e, p) for e, c in enumerate(coeffs)) % p == 0 for a in msgs)
    ctx.torch.cuda.synchronize()

"""GPU: shared powers and cubes of the offline phase.  The two kernels of csrc/hb_offpow.hip through their wrappers, bit for bit against the
host run of the same rows (hb_selftest_off_powers) and against Python ints, in both layouts at every level; and the protocol --
generate_powers, generate_cubes -- with n parties in one process over an in-process tagged network: degrees, constants b^e, the number of
opens, and the programs the preprocessing is for (power_mix and the solver, mimc_mpc_batch) run on what no dealer made.  Exact equality."""
import ctypes
import random

import numpy as np
import pytest

from conftest import BLS
from offline_support import _check_sharings, _run_parties

pytestmark = pytest.mark.gpu

P64 = (1 << 64) - 59
FIELDS = [BLS, P64, 13]
FIELD_IDS = ["bls", "2^64-59", "13"]
COUNTS = (0, 1, 255, 256, 257)
KS = (2, 3, 5, 8, 9)
LAYOUTS = ("item", "power")
MASK, FINISH = 0, 1


def _ctx(p):
    from honeybadgermpc_amd._capi import Context

    return Context.get(p)


def _generator(seed):
    import torch

    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return g


def _values(p, count, rnd, salt):
    corners = (0, 1, p - 1)
    return [corners[(i + salt) % 3] if (i + salt) % 4 != 3 else rnd.randrange(p) for i in range(count)]


def _host(ctx, what, powers, strides, x, r, m, w, out, count):
    """the same level on host copies through hb_selftest_off_powers"""
    from honeybadgermpc_amd._capi import ints_to_limbs

    ptr = lambda a: None if a is None else a.ctypes.data
    mod = ints_to_limbs([ctx.modulus], ctx.modulus + 1, ctx.nbytes)
    return ctx.lib.hb_selftest_off_powers(mod.ctypes.data, ctx.n_limbs, what, ptr(powers), strides[0], strides[1], ptr(x), ptr(r), m, w, ptr(out), count)


def _np(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint64)


# ---- the kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("p", FIELDS, ids=FIELD_IDS)
def test_kernels_equal_the_host_rows_and_the_model(p, layout):
    from honeybadgermpc_amd import offline

    ctx = _ctx(p)
    torch, L = ctx.torch, ctx.n_limbs
    rnd = random.Random(p % 1013 + len(layout))
    for count in COUNTS:
        for k in KS:
            # one array of true powers and sentinels a (count, k): the levels are run on it one after the other
            cols = [_values(p, count, rnd, q) for q in range(k)]         # column q, one value an item; any residues serve a level
            flat = [cols[q][c] for c in range(count) for q in range(k)] if layout == "item" else [v for col in cols for v in col]
            shape = (count, k, L) if layout == "item" else (k, count, L)
            strides = (k, 1) if layout == "item" else (1, count)
            powers = (ctx.upload_ints(flat) if count else ctx.empty(0)).view(shape)
            for m, w in offline.power_levels(k):
                total = count * w
                r2t, opened, rt = (_values(p, total, rnd, s) for s in (1, 2, 0))
                r2t_d, opened_d, rt_d = (ctx.upload_ints(v) if total else ctx.empty(0) for v in (r2t, opened, rt))
                keep = [v.clone() for v in (powers, r2t_d, opened_d, rt_d)]
                # mask
                got = offline.pow_mask(ctx, powers, r2t_d, m, w, layout)
                assert tuple(got.shape) == (total, L) and got.is_contiguous()
                assert torch.equal(powers, keep[0]) and torch.equal(r2t_d, keep[1]), "the mask wrote its inputs"
                if total:
                    host_out = np.zeros((total, L), dtype=np.uint64)
                    assert _host(ctx, MASK, _np(powers), strides, None, _np(r2t_d), m, w, host_out, count) == 0
                    assert np.array_equal(_np(got), host_out), (count, k, m, w)
                    assert ctx.download_ints(got) == [(cols[m - 1][c] * cols[j][c] + r2t[c * w + j]) % p for c in range(count) for j in range(w)]
                    buf = ctx.empty(total + 1)
                    assert offline.pow_mask(ctx, powers, r2t_d, m, w, layout, out=buf[1:]).data_ptr() == buf[1:].data_ptr() and torch.equal(buf[1:], got)
                # finish, on a copy: the levels above go on reading the columns as they were dealt
                work = powers.clone()
                assert offline.pow_finish(ctx, opened_d, rt_d, work, m, w, layout) is work
                assert torch.equal(opened_d, keep[2]) and torch.equal(rt_d, keep[3])
                if total:
                    host_powers = _np(powers).copy()
                    assert _host(ctx, FINISH, host_powers, strides, _np(opened_d), _np(rt_d), m, w, None, count) == 0
                    assert np.array_equal(_np(work), host_powers), (count, k, m, w)
                col = (lambda t, q: t[:, q]) if layout == "item" else (lambda t, q: t[q])
                for q in range(k):
                    if m <= q < m + w:
                        assert ctx.download_ints(col(work, q).contiguous()) == [(opened[c * w + q - m] - rt[c * w + q - m]) % p for c in range(count)]
                    else:
                        assert torch.equal(col(work, q), col(powers, q)), (count, k, m, w, q)


def test_wrappers_and_entry_points_refuse_bad_arguments():
    from honeybadgermpc_amd import offline

    ctx = _ctx(BLS)
    torch, L = ctx.torch, ctx.n_limbs
    count, k = 5, 4
    powers = ctx.upload_ints(list(range(1, count * k + 1))).view(count, k, L)
    r = ctx.upload_ints([1] * (2 * count))
    x = ctx.upload_ints([2] * (2 * count))
    out = torch.zeros_like(ctx.empty(2 * count))
    keep = powers.clone()
    for bad in (dict(m=1, w=2), dict(m=0, w=0), dict(m=2, w=0), dict(m=3, w=2), dict(m=2, w=True), dict(m=2.0, w=2)):      # m + w > k is the wrapper's
        with pytest.raises(ValueError):
            offline.pow_mask(ctx, powers, r, layout="item", **bad)
        with pytest.raises(ValueError):
            offline.pow_finish(ctx, x, r, powers, layout="item", **bad)
    with pytest.raises(ValueError):
        offline.pow_mask(ctx, powers, r, 2, 2, layout="rows")
    with pytest.raises(ValueError):
        offline.pow_mask(ctx, powers, r[:3], 2, 2)
    with pytest.raises(ValueError):
        offline.pow_mask(ctx, powers.transpose(0, 1), r, 2, 2)               # the finish writes in place: no silent copy
    with pytest.raises(ValueError):
        offline.pow_finish(ctx, x[:3], r, powers, 2, 2)
    with pytest.raises(ValueError):
        offline.pow_mask(ctx, powers.view(count * k, L), r, 2, 2)
    st, P = ctx.stream(), ctx.ptr
    mask, finish = ctx.lib.hb_off_pow_mask, ctx.lib.hb_off_pow_finish
    at = lambda t, e: ctypes.c_void_p(t.data_ptr() + e * 8 * L)
    assert mask(ctx.h, P(powers), k, 1, P(r), 1, 2, P(out), count, st) == 2 and finish(ctx.h, P(x), P(r), P(powers), k, 1, 1, 2, count, st) == 2      # w > m
    assert mask(ctx.h, P(powers), k, 1, P(r), 0, 0, P(out), count, st) == 2 and mask(ctx.h, P(powers), k, 1, P(r), 2, 0, P(out), count, st) == 2
    assert mask(ctx.h, P(powers), k, 1, P(r), 2, 2, P(out), -1, st) == 2 and finish(ctx.h, P(x), P(r), P(powers), k, 1, 2, 2, -1, st) == 2
    for strides in ((3, 1), (1, 1), (1, 4), (2, 2), (0, 1), (4, 0), (-4, 1)):
        assert mask(ctx.h, P(powers), strides[0], strides[1], P(r), 2, 2, P(out), count, st) == 2, strides
        assert finish(ctx.h, P(x), P(r), P(powers), strides[0], strides[1], 2, 2, count, st) == 2, strides
    assert mask(ctx.h, None, k, 1, P(r), 2, 2, P(out), count, st) == 2 and mask(ctx.h, P(powers), k, 1, None, 2, 2, P(out), count, st) == 2
    assert mask(ctx.h, P(powers), k, 1, P(r), 2, 2, None, count, st) == 2
    assert finish(ctx.h, None, P(r), P(powers), k, 1, 2, 2, count, st) == 2 and finish(ctx.h, P(x), None, P(powers), k, 1, 2, 2, count, st) == 2
    assert finish(ctx.h, P(x), P(r), None, k, 1, 2, 2, count, st) == 2
    assert mask(ctx.h, P(powers), k, 1, P(r), 2, 2, P(powers), count, st) == 2 and mask(ctx.h, P(powers), k, 1, P(r), 2, 2, P(r), count, st) == 2
    assert mask(ctx.h, P(powers), k, 1, P(r), 2, 2, at(powers, count * k - 1), count, st) == 2
    assert finish(ctx.h, at(powers, 2), P(r), P(powers), k, 1, 2, 2, count, st) == 2 and finish(ctx.h, P(x), at(powers, 2), P(powers), k, 1, 2, 2, count, st) == 2
    assert mask(ctx.h, None, k, 1, None, 2, 2, None, 0, st) == 0 and finish(ctx.h, None, None, None, k, 1, 2, 2, 0, st) == 0
    assert mask(ctx.h, None, 1, 0, None, 2, 2, None, 0, st) == 0                 # the power-major strides of no item
    torch.cuda.synchronize()
    assert torch.equal(powers, keep) and not out.any(), "a refused call wrote"


# ---- the protocol over the in-process tagged network ------------------------------------------------------------------------
CASES = [(BLS, 4, 1, 1, 1), (BLS, 4, 1, 3, 2), (BLS, 4, 1, 5, 9), (BLS, 7, 2, 4, 8), (BLS, 4, 1, 2, 33), (P64, 4, 1, 5, 9)]


@pytest.mark.parametrize("p, n, t, count, k", CASES, ids=["4-1-1-1", "4-1-3-2", "4-1-5-9", "7-2-4-8", "4-1-2-33", "4-1-5-9-2^64-59"])
def test_generate_powers(p, n, t, count, k):
    from honeybadgermpc_amd import offline

    ctx = _ctx(p)
    L = ctx.n_limbs
    levels = offline.power_levels(k)
    both = (count, k) == (5, 9) and p == BLS

    async def body(co, i):
        before = co.batches
        powers = await offline.generate_powers(co, count, k, generator=_generator(1200 + i))
        assert tuple(powers.shape) == (count, k, L) and powers.is_contiguous() and co.batches - before == len(levels)
        opened = await co.open_share_array(powers.view(count * k, L))
        out = [ctx.download_ints(powers.view(count * k, L)), ctx.download_ints(opened)]
        if both:                                                          # the same randomness in the other layout: the same shares, transposed
            before = co.batches
            other = await offline.generate_powers(co, count, k, tag="powers-2", generator=_generator(1200 + i), layout="power")
            assert tuple(other.shape) == (k, count, L) and other.is_contiguous() and co.batches - before == len(levels)
            assert ctx.torch.equal(other.transpose(0, 1), powers)
        return out

    results = _run_parties(p, n, t, body)
    opened = results[0][1]
    assert all(r[1] == opened for r in results)
    assert _check_sharings(p, n, t, [r[0] for r in results]) == opened
    b = [opened[c * k] for c in range(count)]
    assert len(set(b)) == count
    assert opened == [pow(v, e, p) for v in b for e in range(1, k + 1)]
    assert [offline.powers_model(v, k, p) for v in b] == [opened[c * k:(c + 1) * k] for c in range(count)]


def test_generate_cubes_feed_mimc():
    from honeybadgermpc_amd import offline
    from honeybadgermpc_amd.progs import mimc

    p, n, t, rounds, count = BLS, 4, 1, 3, 10
    ctx = _ctx(p)
    L = ctx.n_limbs
    rnd = random.Random(17)
    xs, slopes = [rnd.randrange(p) for _ in range(count)], [rnd.randrange(p) for _ in range(count)]
    key, key_slope = rnd.randrange(p), rnd.randrange(p)

    async def body(co, i):
        before = co.batches
        cubes = await offline.generate_cubes(co, rounds, count, generator=_generator(1300 + i))
        assert co.batches - before == 2 and len(cubes) == 3
        assert all(tuple(v.shape) == (rounds, count, L) and v.is_contiguous() for v in cubes)
        assert [v.data_ptr() - cubes[0].data_ptr() for v in cubes] == [e * rounds * count * 8 * L for e in range(3)]      # one buffer, no copy
        handles = [co.open_share_array(v.reshape(rounds * count, L)) for v in cubes]
        out = [ctx.download_ints(v.reshape(rounds * count, L)) for v in cubes] + [ctx.download_ints(await h) for h in handles]
        x = ctx.upload_ints([(v + (i + 1) * s) % p for v, s in zip(xs, slopes)])
        key_share = ctx.upload_ints([(key + (i + 1) * key_slope) % p])
        keep = [v.clone() for v in cubes]
        shares = await mimc.mimc_mpc_batch(co, x, key_share, cubes, rounds=rounds)
        assert all(ctx.torch.equal(v, w) for v, w in zip(cubes, keep))
        out.append(ctx.download_ints(await co.open_share_array(shares)))
        return out

    results = _run_parties(p, n, t, body)
    for part in range(3):
        assert _check_sharings(p, n, t, [r[part] for r in results]) == results[0][3 + part]
    for res in results:
        assert res[3:] == results[0][3:]
    r, r2, r3 = results[0][3:6]
    assert len(set(r)) == rounds * count and r2 == [v * v % p for v in r] and r3 == [pow(v, 3, p) for v in r]
    assert results[0][6] == [mimc.mimc_plain(x, key, p, rounds=rounds) for x in xs]


def test_generate_powers_feed_the_mixer_and_the_solver():
    from honeybadgermpc_amd import offline, solver
    from honeybadgermpc_amd import power_mixing as pm

    p, n, t, k = BLS, 4, 1, 4
    ctx = _ctx(p)
    rnd = random.Random(23)
    msgs, slopes = [rnd.randrange(p) for _ in range(k)], [rnd.randrange(p) for _ in range(k)]

    async def body(co, i):
        a = ctx.upload_ints([(v + (i + 1) * s) % p for v, s in zip(msgs, slopes)])
        powers = await offline.generate_powers(co, k, k, generator=_generator(1400 + i))
        sums = await pm.power_mix(co, a, powers)
        again = await offline.generate_powers(co, k, k, tag="powers-2", generator=_generator(1500 + i))
        return ctx.download_ints(sums), solver.solve(ctx, sums), await solver.mix(co, a, again)

    results = _run_parties(p, n, t, body)
    for sums, solved, mixed in results:
        assert sums == [sum(pow(a, j, p) for a in msgs) % p for j in range(1, k + 1)]
        assert solved == sorted(msgs) and mixed == sorted(msgs)


def test_generate_powers_aborts_with_randousha():
    """a perturbed H1 share of the inner randousha: every party raises HoneyBadgerMPCError, and none waits for a message that will not come"""
    from honeybadgermpc_amd import offline, wire
    from honeybadgermpc_amd.exceptions import HoneyBadgerMPCError

    p, n, t = BLS, 4, 1

    def hook(sender, tag, dest, msg):
        if tag[-1] == "H1" and sender == 1 and dest == 2:
            values = wire.unpack_ints(msg)
            values[0] += 1
            return wire.pack_ints([v % p for v in values], p)
        return msg

    async def body(co, i):
        return await offline.generate_powers(co, 3, 5, generator=_generator(1600 + i))

    results = _run_parties(p, n, t, body, hook, return_exceptions=True)
    assert all(isinstance(r, HoneyBadgerMPCError) for r in results), results

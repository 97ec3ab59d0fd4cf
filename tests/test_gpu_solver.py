"""GPU: honeybadgermpc_amd.solver -- Newton's identities, the root finder of csrc/hb_rf.hip and the mixing protocol end to end.
The expected outputs are mathematics: the sorted roots a test started from, or None; for the case table of tests/rootfind_cases.py also
the walk of the same level loop over host memory, root by root in the order found.  Exact equality everywhere."""
import asyncio
import ctypes
import random

import pytest

from conftest import BLS

import rootfind_cases as cases
import rootfind_model as model
import test_solver_host as host

pytestmark = pytest.mark.gpu

P64 = (1 << 64) - 59
P256 = (1 << 256) - 189


def _ctx(p, n_limbs=None):
    from honeybadgermpc_amd._capi import Context

    return Context.get(p, n_limbs=n_limbs)


def _both(ctx, coeffs, seed=0):
    """solve (from the power sums of the polynomial) and roots (from its coefficients): both answers as lists, or None"""
    from honeybadgermpc_amd import solver

    p = ctx.modulus
    got_solve = solver.solve(ctx, model.power_sums_from_poly(coeffs, p), seed=seed)
    found = solver.roots(ctx, ctx.upload_ints(coeffs), seed=seed)
    if found is not None:
        assert tuple(found.shape) == (len(coeffs) - 1, ctx.n_limbs)
    return got_solve, (None if found is None else ctx.download_ints(found))


def _check_roots(ctx, rts, seed=0):
    p = ctx.modulus
    want = sorted(r % p for r in rts)
    got_solve, got_roots = _both(ctx, model.poly_from_roots(want, p), seed=seed)
    assert got_solve == want
    assert got_roots == want


def _check_invalid(ctx, coeffs):
    got_solve, got_roots = _both(ctx, coeffs)
    assert got_solve is None and got_roots is None


def test_two_and_three_distinct_roots():
    ctx = _ctx(BLS)
    rnd = random.Random(1)
    _check_roots(ctx, [rnd.randrange(BLS) for _ in range(2)])
    _check_roots(ctx, [rnd.randrange(BLS) for _ in range(3)])


def test_two_equal_roots():
    _check_roots(_ctx(BLS), [12345, 12345])


def test_the_references_workload_around_the_small_degree():
    """roots 1001 .. 1000 + k (powermixing.py:186) at the threshold between the one-launch chain and the tiled one, and at 200"""
    from honeybadgermpc_amd import solver

    ctx = _ctx(BLS)
    for k in (solver.SMALL_DEGREE, solver.SMALL_DEGREE + 1, 200):
        _check_roots(ctx, list(range(1001, 1001 + k)))


def test_k_1024_random_roots():
    from honeybadgermpc_amd import solver

    ctx = _ctx(BLS)
    rnd = random.Random(1024)
    want = sorted(rnd.randrange(BLS) for _ in range(1024))
    assert len(set(want)) == 1024
    # (the polynomial through the library's own Newton kernel: 1024^2 / 2 products are slow in Python; bit-equality of the two is a test below)
    sums = model.power_sums_from_roots(want, BLS)
    assert solver.solve(ctx, sums) == want


def test_roots_at_the_edges_of_the_field():
    _check_roots(_ctx(BLS), [0, 1, BLS - 1, BLS - 2, 7])


def test_multiplicities():
    ctx = _ctx(BLS)
    _check_roots(ctx, [5, 5, 5, 7])
    _check_roots(ctx, [BLS - 3] * 8)
    rnd = random.Random(40)
    singles = [rnd.randrange(BLS) for _ in range(20)]
    doubles = [rnd.randrange(BLS) for _ in range(7)]
    triples = [rnd.randrange(BLS) for _ in range(2)]
    rts = singles + 2 * doubles + 3 * triples
    assert len(rts) == 40
    _check_roots(ctx, rts)


def test_invalid_inputs_give_none():
    p = BLS
    ctx = _ctx(p)
    rnd = random.Random(9)
    c = model.non_residue(p)
    quad = [(-c) % p, 0, 1]
    _check_invalid(ctx, quad)                                                                   # k = 2: nothing but the quadratic
    _check_invalid(ctx, model.poly_mul(quad, model.poly_from_roots([rnd.randrange(p) for _ in range(32)], p), p))      # k = 34
    cubic = model.irreducible_cubic(p)
    _check_invalid(ctx, model.poly_mul(cubic, model.poly_from_roots([rnd.randrange(p) for _ in range(5)], p), p))
    _check_invalid(ctx, model.poly_mul(model.poly_mul(quad, quad, p), [p - 1, 1], p))           # (x^2 - c)^2 (x - 1)


def test_two_seeds_one_answer():
    from honeybadgermpc_amd import solver

    ctx = _ctx(BLS)
    rnd = random.Random(77)
    rts = sorted([rnd.randrange(BLS) for _ in range(60)] + [3, 3])
    sums = model.power_sums_from_roots(rts, BLS)
    assert solver.solve(ctx, sums, seed=1) == rts
    assert solver.solve(ctx, sums, seed=2**63 + 5) == rts


@pytest.mark.parametrize("k", [2, 33, 300])
def test_newton_on_the_device_is_bit_equal_to_the_host_function(k):
    from honeybadgermpc_amd import power_mixing, solver

    ctx = _ctx(BLS)
    rnd = random.Random(k)
    sums = [rnd.choice([0, 1, BLS - 1, rnd.randrange(BLS), rnd.randrange(BLS)]) for _ in range(k)]
    got = solver.newton_coefficients_device(ctx, ctx.upload_ints(sums))
    assert tuple(got.shape) == (k + 1, ctx.n_limbs)
    assert ctx.download_ints(got) == power_mixing.newton_coefficients(sums, BLS)


def test_small_fields():
    """shifts hit roots and a node's shifts run out: the answer is still exact"""
    for p, k in ((97, 20), (13, 12), (3, 2)):
        ctx = _ctx(p)
        rnd = random.Random(p)
        _check_roots(ctx, rnd.sample(range(p), k))
        if p == 13:
            _check_roots(ctx, [4] * 5 + [0, 0, 12])
            _check_invalid(ctx, model.poly_mul([(-model.non_residue(p)) % p, 0, 1], [p - 3, 1], p))


def test_word_size_prime_on_a_one_limb_context():
    ctx = _ctx(P64, n_limbs=1)
    rnd = random.Random(64)
    _check_roots(ctx, [rnd.randrange(P64) for _ in range(98)] + [0, P64 - 1])


def test_a_256_bit_prime():
    ctx = _ctx(P256)
    rnd = random.Random(256)
    _check_roots(ctx, [rnd.randrange(P256) for _ in range(31)] + [P256 - 1, P256 - 1])


def test_arguments_refused_on_the_device():
    from honeybadgermpc_amd import solver
    from honeybadgermpc_amd._capi import HB_ERR_BAD_ARG

    ctx = _ctx(BLS)
    with pytest.raises(ValueError):
        solver.roots(ctx, ctx.upload_ints([1, 2, 3]))                    # not monic
    with pytest.raises(ValueError):
        solver.roots(ctx, ctx.upload_ints([1]))
    small = _ctx(13)
    with pytest.raises(ValueError):
        solver.solve(small, [1] * 13)
    out = ctx.empty(4)
    assert ctx.lib.hb_rf_newton(ctx.h, None, 3, ctx.ptr(out), ctx.stream()) == HB_ERR_BAD_ARG
    assert ctx.lib.hb_rf_newton(ctx.h, ctx.ptr(out), 0, ctx.ptr(out), ctx.stream()) == HB_ERR_BAD_ARG
    # the temporaries go back with the cache, and the next call regrows them
    ctx.cache_clear()
    _check_roots(ctx, [9, 8, 7])


# ---- the case table of tests/rootfind_cases.py: the device's walk against the host's ------------------------------------------
# hb_rf_roots writes the roots in the order found, and so does the level loop over host memory (HB_RF_SELFTEST_ROOTS: the same bodies,
# the same driver, RfRun<.., DEV = false>) for the same seed: the two UNSORTED lists are equal exactly when every split of every node
# came out the same on both sides.  solver.roots sorts, so these tests call the library directly.
def device_walk(ctx, coeffs, seed=0):
    """hb_rf_roots on the current stream -> host.HostWalk: n_roots, the roots as the library wrote them, levels, rounds, nodes"""
    k = len(coeffs) - 1
    dev = ctx.upload_ints(list(coeffs))
    out = ctx.empty(k)
    n = ctypes.c_int32(0)
    ctx.check(ctx.lib.hb_rf_roots(ctx.h, ctx.ptr(dev), k, ctypes.c_uint64(seed), ctx.ptr(out), ctypes.byref(n), ctx.stream()), "hb_rf_roots")
    stats = (ctypes.c_int64 * 8)()
    ctx.lib.hb_debug_rf_stats(stats)
    return host.HostWalk(n.value, tuple(ctx.download_ints(out)) if n.value >= 0 else None, int(stats[0]), int(stats[3]), int(stats[7]))


def _case_on_the_device(case_id, seed=0):
    """one case, one seed: the device's walk is the host's, and the host's is right; -> the device's walk"""
    case = cases.BY_ID[case_id]
    want = host.host_walk(case_id, seed)
    host.check_walk(case, want)
    got = device_walk(_ctx(case.p, case.n_limbs), cases.coeffs_of(case_id), seed)
    assert got.n == want.n, (case_id, seed)
    assert got.roots == want.roots, (case_id, seed)
    assert (got.levels, got.rounds, got.nodes) == (want.levels, want.rounds, want.nodes), (case_id, seed)
    host.check_walk(case, got)
    return got


@pytest.mark.parametrize("case", cases.CASES, ids=[c.id for c in cases.CASES])
def test_case_device_walk_is_the_host_walk(case):
    from honeybadgermpc_amd import solver

    _case_on_the_device(case.id)
    ctx = _ctx(case.p, case.n_limbs)
    assert solver.solve(ctx, list(cases.power_sums_of(case.id))) == case.expected


@pytest.mark.parametrize("case_id", sorted(cases.SEEDS))
def test_case_under_other_seeds(case_id):
    case = cases.BY_ID[case_id]
    for seed in (0,) + cases.SEEDS[case_id]:
        assert sorted(_case_on_the_device(case_id, seed).roots) == case.expected, seed


def _run_sequence():
    """a large solve, then small ones, on one context and the current stream: the arenas, the table and h hold what the larger call left"""
    walks = [_case_on_the_device(cid) for cid in cases.SEQUENCE]
    assert cases.SEQUENCE[0] == cases.SEQUENCE[-1] and walks[0] == walks[-1]
    assert [cases.degree(cases.BY_ID[cid]) for cid in cases.SEQUENCE] == [200, 3, 129, 2, 65, 200]
    assert walks[4].n == -1


def test_a_small_solve_after_a_large_one_on_the_same_context():
    _run_sequence()


def test_the_same_calls_on_a_stream_of_their_own():
    import torch

    ctx = _ctx(BLS)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert ctx.stream().value == side.cuda_stream
        _run_sequence()
    side.synchronize()


def test_two_contexts_in_turn():
    assert len({cases.BY_ID[cid].p for cid in cases.ALTERNATING}) == 2
    assert all(cases.BY_ID[a].p != cases.BY_ID[b].p for a, b in zip(cases.ALTERNATING, cases.ALTERNATING[1:]))
    for cid in cases.ALTERNATING:
        _case_on_the_device(cid)


@pytest.mark.parametrize("nc", cases.NEWTON, ids=[c.id for c in cases.NEWTON])
def test_newton_kernel_is_the_host_body_where_the_run_of_a_thread_grows(nc):
    from honeybadgermpc_amd import solver

    ctx = _ctx(nc.p, nc.n_limbs)
    got = solver.newton_coefficients_device(ctx, ctx.upload_ints(list(nc.sums)))
    assert tuple(ctx.download_ints(got)) == host.newton_body(nc.id)


def test_newton_kernel_on_1024_pool_values():
    from honeybadgermpc_amd import power_mixing, solver

    ctx = _ctx(BLS)
    sums = cases.newton_pool_vector(1024)
    got = solver.newton_coefficients_device(ctx, ctx.upload_ints(sums))
    assert ctx.download_ints(got) == power_mixing.newton_coefficients(sums, BLS)


# ---- the protocol, end to end over an in-process tagged network ---------------------------------------------------------------
class _TaggedNet:
    """get_send_recv(tag) -> (send, recv) for party i, as the runtime hands out per-share-id channels"""

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


def _deal(rnd, p, n, degree, values):
    """-> [party][k]: Shamir shares of values[k] at the points 1..n"""
    polys = [[v] + [rnd.randrange(p) for _ in range(degree)] for v in values]
    return [[sum(co * pow(x, e, p) for e, co in enumerate(poly)) % p for poly in polys] for x in range(1, n + 1)]


def test_mix_end_to_end():
    from honeybadgermpc_amd import solver
    from honeybadgermpc_amd.open_coalescer import OpenCoalescer

    p, n, t, k = BLS, 4, 1, 16
    ctx = _ctx(p)
    rnd = random.Random(416)
    msgs = [rnd.randrange(p) for _ in range(k)]
    msgs[0], msgs[1], msgs[2] = 0, p - 1, msgs[3]
    bs = [rnd.randrange(p) for _ in range(k)]
    msg_shares = _deal(rnd, p, n, t, msgs)
    pow_shares = _deal(rnd, p, n, t, [pow(b, j, p) for b in bs for j in range(1, k + 1)])

    async def party(i, net):
        co = OpenCoalescer(p, n, t, i, net.get_send_recv(i))
        return await solver.mix(co, ctx.upload_ints(msg_shares[i]), ctx.upload_ints(pow_shares[i]).reshape(k, k, ctx.n_limbs), seed=i)

    async def main():
        net = _TaggedNet(n)
        return await asyncio.gather(*[party(i, net) for i in range(n)])

    results = asyncio.run(main())
    for i in range(n):
        assert results[i] == sorted(msgs), i
    ctx.torch.cuda.synchronize()

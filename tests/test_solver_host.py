"""CPU-only: the bodies of the root-finding kernels (csrc/hb_rf.hip) run on the host through hb_selftest_rf -- the same HB_HD phases
the kernels run, walked thread by thread -- against the plain-Python model of tests/rootfind_model.py and
power_mixing.newton_coefficients; and what honeybadgermpc_amd.solver checks before it touches a device.  Exact equality."""
import collections
import ctypes
import functools
import os
import random
import re

import numpy as np
import pytest

from conftest import BLS, REPO

import rootfind_cases as cases
import rootfind_model as model

P256 = (1 << 256) - 189
P64 = (1 << 64) - 59
PRIMES = [(BLS, 4), (P256, 4), (97, 4), (13, 4), (P64, 1), (13, 1)]
IDS = ["bls", "2^256-189", "97", "13w", "2^64-59", "13n"]
NEWTON, STEP, GCD, SHIFT, ROOTS = 0, 1, 2, 3, 4


def run(p, nl, what, operands, params, n_out):
    """hb_selftest_rf over lists of ints -> (rc, (n_out, nl) uint64 array)"""
    from honeybadgermpc_amd._capi import ints_to_limbs, load_library, np_ptr

    lib = load_library()
    nb = 8 * nl
    arrs = [ints_to_limbs(list(o), p, nb) for o in operands]
    ptrs = (ctypes.c_void_p * max(len(arrs), 1))(*[a.ctypes.data for a in arrs])
    pr = np.array([x - (1 << 64) if x >= 1 << 63 else x for x in params], dtype=np.int64)
    out = np.zeros((max(n_out, 1), nl), dtype=np.uint64)
    rc = lib.hb_selftest_rf(np_ptr(ints_to_limbs([p], p + 1, nb)), nl, what, ctypes.cast(ptrs, ctypes.c_void_p), np_ptr(pr), np_ptr(out))
    return rc, out


def ints(out, nl):
    from honeybadgermpc_amd._capi import limbs_to_ints

    return limbs_to_ints(out, 8 * nl)


def small_degree():
    from honeybadgermpc_amd import solver

    return solver.SMALL_DEGREE


@pytest.mark.parametrize("p, nl", PRIMES, ids=IDS)
def test_newton_body_against_the_host_function(p, nl):
    from honeybadgermpc_amd.power_mixing import newton_coefficients

    rnd = random.Random(p % 1000 + nl)
    for k in (2, 3, 33):
        if k >= p:
            continue
        for sums in ([rnd.randrange(p) for _ in range(k)], [p - 1] * k, model.power_sums_from_roots([rnd.randrange(p) for _ in range(k)], p)):
            rc, out = run(p, nl, NEWTON, [sums], [k], k + 1)
            assert rc == 0 and ints(out, nl) == newton_coefficients(sums, p), k


def test_newton_body_across_several_runs_of_integers_a_thread():
    """k above the 256 threads of the workgroup: every thread owns a run of two integers of the 1 / m table, and a step's sum spans them"""
    from honeybadgermpc_amd.power_mixing import newton_coefficients

    rnd = random.Random(5)
    k = 300
    sums = [rnd.randrange(P64) for _ in range(k)]
    rc, out = run(P64, 1, NEWTON, [sums], [k], k + 1)
    assert rc == 0 and ints(out, 1) == newton_coefficients(sums, P64)


def _step_want(p, s, h, a, mul):
    want = model.poly_mul(h, h, p)
    if mul:
        want = model.poly_mul(want, [a, 1], p)
    return model.poly_rem(want, s, p)


@pytest.mark.parametrize("p, nl", PRIMES, ids=IDS)
def test_one_step_of_the_chain(p, nl):
    """h^2 mod s (mul = 0) and h^2 (x + a) mod s (mul = 1: the multiplication by x + a is a shift and an axpy on the product) at degree 2,
    at SMALL_DEGREE (the one-workgroup step) and one above (table, tiled square, vector-matrix reduction); random operands, every
    coefficient p - 1 (the accumulation bound: hb_pm.hip:28-35), and h = 1, where the step is the multiplication alone"""
    rnd = random.Random(p % 1000 + 7 * nl)
    sd = small_degree()
    for d in (2, sd, sd + 1, 3 * sd + 5):
        cases = [([rnd.randrange(p) for _ in range(d)] + [1], [rnd.randrange(p) for _ in range(d)], rnd.randrange(p)),
                 ([p - 1] * d + [1], [p - 1] * d, p - 1),
                 ([rnd.randrange(p) for _ in range(d)] + [1], [1] + [0] * (d - 1), rnd.randrange(p)),
                 ([0] * d + [1], [rnd.randrange(p) for _ in range(d)], 0)]
        for s, h, a in cases:
            for mul in (0, 1):
                rc, out = run(p, nl, STEP, [s, h, [a]], [d, mul], d)
                assert rc == 0 and ints(out, nl) == _step_want(p, s, h, a, mul), (d, mul)


@pytest.mark.parametrize("p, nl", [(BLS, 4), (P64, 1)], ids=["bls", "2^64-59"])
def test_a_step_across_several_tiles(p, nl):
    """degree 200: four tiles of outputs in the reduction, seven in the square (the pairing t / T-1-t with a middle tile), sums split over the waves"""
    rnd = random.Random(200 + nl)
    d = 200
    s, h, a = [rnd.randrange(p) for _ in range(d)] + [1], [rnd.randrange(p) for _ in range(d)], rnd.randrange(p)
    rc, out = run(p, nl, STEP, [s, h, [a]], [d, 1], d)
    assert rc == 0 and ints(out, nl) == _step_want(p, s, h, a, 1)


def _gcd_check(p, nl, a, b):
    a, b = model.trim(x % p for x in a), model.trim(x % p for x in b)
    if len(b) > len(a):
        a, b = b, a
    want = model.poly_gcd(a, b, p)
    rc, out = run(p, nl, GCD, [a, b], [len(a) - 1, len(b) - 1], len(a) + 1)
    assert rc == 0 and int(out[0, 0]) == len(want) - 1, (a, b)
    assert ints(out[1:1 + len(want)], nl) == want, (a, b)


@pytest.mark.parametrize("p, nl", PRIMES, ids=IDS)
def test_gcd_body(p, nl):
    rnd = random.Random(p % 1000 + 11 * nl)

    def rand_monic(d):
        return [rnd.randrange(p) for _ in range(d)] + [1]

    def scaled(f):
        c = rnd.randrange(1, p)
        return [x * c % p for x in f]

    for _ in range(4):
        # coprime (almost surely for the large primes; whatever the model says otherwise)
        _gcd_check(p, nl, rand_monic(9), scaled(rand_monic(6)))
        # a common factor
        c = rand_monic(3)
        _gcd_check(p, nl, model.poly_mul(c, rand_monic(8), p), scaled(model.poly_mul(c, rand_monic(4), p)))
    # one divides the other; equal inputs; a constant
    f = rand_monic(5)
    _gcd_check(p, nl, model.poly_mul(f, rand_monic(7), p), scaled(f))
    _gcd_check(p, nl, f, f)
    _gcd_check(p, nl, f, scaled(f))
    _gcd_check(p, nl, f, [rnd.randrange(1, p)])
    # the remainder's degree drops by more than one in a step: x^10 + x + 1 against x^9 leaves x + 1 at once
    _gcd_check(p, nl, [1, 1] + [0] * 8 + [1], [0] * 9 + [1])
    _gcd_check(p, nl, [3 % p, 0, 0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 1])
    # products of linear factors, as the split tree meets them (more than one 256-thread stride at degree 300)
    rts = [rnd.randrange(p) for _ in range(300)] if p > 1000 else [rnd.randrange(p) for _ in range(10)]
    half = len(rts) // 2
    _gcd_check(p, nl, model.poly_from_roots(rts, p), scaled(model.poly_from_roots(rts[:half] + [rnd.randrange(p) for _ in range(half - 1)], p)))


@pytest.mark.parametrize("p, nl", PRIMES + [(3, 4)], ids=IDS + ["3"])
def test_shift_generator(p, nl):
    def shift(seed, level, node, draw):
        rc, out = run(p, nl, SHIFT, [], [seed, level, node, draw], 1)
        assert rc == 0
        return ints(out, nl)[0]

    assert shift(5, 2, 3, 4) == shift(5, 2, 3, 4)
    for seed, level, node in ((0, 0, 0), (1, 0, 0), (0, 3, 17), ((1 << 64) - 1, 9, 511)):
        draws = [shift(seed, level, node, j) for j in range(64)]
        assert all(0 <= a < p for a in draws)
        assert len(set(draws)) == min(64, p)                          # distinct mod p while that is possible
        if p < 64:
            assert set(draws) == set(range(p))
    if p > 1 << 60:
        # the base depends on each of seed, level and node
        base = shift(0, 0, 0, 0)
        assert len({base, shift(1, 0, 0, 0), shift(0, 1, 0, 0), shift(0, 0, 1, 0)}) == 4


@pytest.mark.parametrize("p, nl", PRIMES + [(3, 4)], ids=IDS + ["3"])
def test_the_whole_level_loop_on_the_host(p, nl):
    """hb_rf_roots' loop over host memory: distinct roots, multiplicities, the threshold between the two chains, invalid inputs, two seeds"""
    rnd = random.Random(p % 1000 + 13 * nl)
    sd = small_degree()

    def roots_of(coeffs, seed=0):
        k = len(coeffs) - 1
        rc, out = run(p, nl, ROOTS, [coeffs], [k, seed], k + 1)
        assert rc == 0
        n = int(out[0].view(np.int64)[0])
        return None if n < 0 else sorted(ints(out[1:], nl))

    cases = []
    if p > 1000:
        cases += [[rnd.randrange(p) for _ in range(k)] for k in (2, 3, sd, sd + 1)]
        cases += [[5, 5, 5, 7], [p - 2] * 8, [0, 1, p - 1, p - 2], [rnd.randrange(p) for _ in range(8)] * 2 + [11] * 3]
    elif p > 3:
        cases += [rnd.sample(range(p), p - 1), rnd.sample(range(p), min(p - 1, 20)), [4] * 5 + [0, 0, 12]]
    else:
        cases += [[0, 1], [2, 2], [1, 2]]
    for rts in cases:
        want = sorted(rts)
        f = model.poly_from_roots(want, p)
        assert roots_of(f) == want, want
        assert roots_of(f, seed=(1 << 64) - 3) == want
    c = model.non_residue(p)
    quad = [(-c) % p, 0, 1]
    assert roots_of(quad) is None
    if p > 5:
        assert roots_of(model.poly_mul(quad, model.poly_from_roots([1, 2, 2], p), p)) is None
        assert roots_of(model.poly_mul(model.poly_mul(quad, quad, p), [p - 1, 1], p)) is None
        assert roots_of(model.poly_mul(model.irreducible_cubic(p), model.poly_from_roots([3, 4], p), p)) is None


# ---- the case table of tests/rootfind_cases.py: every case here, and then on the device against this walk (test_gpu_solver.py) ----
HostWalk = collections.namedtuple("HostWalk", "n roots levels rounds nodes")


@functools.lru_cache(maxsize=None)
def host_walk(case_id, seed=0):
    """The level loop over host memory (RfRun<.., DEV = false>) on a case of the table: the number of roots (-1: invalid), the roots
    in the order found, and the walk's counters.  Kept for the process: the GPU tests hold the device's output against it."""
    from honeybadgermpc_amd._capi import load_library

    c = cases.BY_ID[case_id]
    coeffs = list(cases.coeffs_of(case_id))
    k = len(coeffs) - 1
    rc, out = run(c.p, c.n_limbs, ROOTS, [coeffs], [k, seed], k + 1)
    assert rc == 0, (case_id, seed, rc)
    stats = (ctypes.c_int64 * 8)()
    load_library().hb_debug_rf_stats(stats)
    n = int(out[0].view(np.int64)[0])
    return HostWalk(n, tuple(ints(out[1:], c.n_limbs)) if n >= 0 else None, int(stats[0]), int(stats[3]), int(stats[7]))


def check_walk(case, walk):
    """what mathematics says about a walk of the level loop, host or device"""
    if case.expected is None:
        # the first level decides: every node is fresh there, and the one that holds the factor of degree above one fails the count
        assert walk.n == -1 and walk.levels == 1, (case.id, walk)
        return
    assert walk.n == len(case.expected) and sorted(walk.roots) == case.expected, case.id
    assert walk.rounds == cases.multiplicity(case), (case.id, walk.rounds)
    # every level works on at least one node; a single root, however often repeated, is the one input that needs no level
    assert walk.nodes >= walk.levels and (walk.levels >= 1 or len(set(case.expected)) == 1), (case.id, walk)


def test_the_case_table_is_what_it_says():
    assert cases.BLS == BLS and cases.P256 == P256 and cases.P64 == P64
    sd = small_degree()
    by_group = collections.Counter(c.id.split("-")[0] for c in cases.CASES)
    assert set(by_group) == {"tile", "seq", "edge", "small", "mult", "invalid", "seeds"}
    for c in cases.CASES:
        f = cases.coeffs_of(c.id)
        assert f[-1] == 1 and len(f) - 1 == cases.degree(c) < c.p and all(0 <= v < c.p for v in f)
        if c.roots is None:
            assert len(f) - 1 > 2 * sd, c.id                                           # the node that holds the factor is in the tiled chain
        elif not c.id.startswith(("seq-", "mult-65x-", "small-13-")):
            assert len(set(c.roots)) > sd, c.id                                        # so is the first node of a valid case
    # every wide modulus has a case above degree 128
    for name in cases.WIDE:
        assert any(c.p == cases.MODULI[name][0] and c.roots is not None and len(set(c.roots)) > 128 for c in cases.CASES), name
    # the pool is 35 .. 55 roots; with the pre-images it crosses a tile (Goldilocks: 62, where many pre-images are pool values)
    for name in cases.LARGE:
        assert sd < cases.degree(cases.BY_ID[f"edge-pool-{name}"]) < 64
        assert cases.degree(cases.BY_ID[f"edge-operands-{name}"]) > (sd if name == "gold" else 64)
    for cid, seeds in cases.SEEDS.items():
        assert cid in cases.BY_ID and 0 not in seeds
    assert all(cid in cases.BY_ID for cid in cases.SEQUENCE + cases.ALTERNATING)


@pytest.mark.parametrize("case", cases.CASES, ids=[c.id for c in cases.CASES])
def test_case_on_the_host(case):
    """the whole level loop on a case of the table: the roots, the rounds of the repeated-root loop, an invalid input's one level"""
    check_walk(case, host_walk(case.id))


@pytest.mark.parametrize("case_id", sorted(cases.SEEDS))
def test_case_under_other_seeds_on_the_host(case_id):
    case = cases.BY_ID[case_id]
    orders = {host_walk(case_id).roots}
    for seed in cases.SEEDS[case_id]:
        walk = host_walk(case_id, seed)
        check_walk(case, walk)
        orders.add(walk.roots)
    assert len(orders) > 1                       # the seed does choose the shifts: the walks differ, the answer does not


@pytest.mark.parametrize("case", cases.CASES, ids=[c.id for c in cases.CASES])
def test_newton_body_gives_back_the_polynomial_of_a_case(case):
    """power sums of the case's polynomial (Newton run backwards in Python ints) -> the Newton body -> the polynomial, invalid ones too"""
    k = cases.degree(case)
    rc, out = run(case.p, case.n_limbs, NEWTON, [list(cases.power_sums_of(case.id))], [k], k + 1)
    assert rc == 0 and ints(out, case.n_limbs) == list(cases.coeffs_of(case.id))


@pytest.mark.parametrize("nc", cases.NEWTON, ids=[c.id for c in cases.NEWTON])
def test_newton_body_where_the_run_of_a_thread_grows(nc):
    """k = 255, 256, 257: the last thread idle, every thread one integer, every thread a run of two (and a step's sum two terms a thread)"""
    from honeybadgermpc_amd.power_mixing import newton_coefficients

    assert newton_body(nc.id) == tuple(newton_coefficients(list(nc.sums), nc.p))


@functools.lru_cache(maxsize=None)
def newton_body(newton_id):
    """the Newton body over host memory on a case of cases.NEWTON (kept: the GPU test holds the kernel against it)"""
    nc = next(c for c in cases.NEWTON if c.id == newton_id)
    k = len(nc.sums)
    rc, out = run(nc.p, nc.n_limbs, NEWTON, [list(nc.sums)], [k], k + 1)
    assert rc == 0
    return tuple(ints(out, nc.n_limbs))


def test_model_power_sums_run_backwards():
    p = 97
    rts = [3, 3, 50, 96, 0]
    assert model.power_sums_from_poly(model.poly_from_roots(rts, p), p) == model.power_sums_from_roots(rts, p)
    from honeybadgermpc_amd.power_mixing import newton_coefficients

    f = model.poly_mul([(-model.non_residue(p)) % p, 0, 1], [5, 1], p)
    assert newton_coefficients(model.power_sums_from_poly(f, p), p) == f


class _Ctx:
    """what solve() looks at before any device call"""

    def __init__(self, modulus, n_limbs):
        self.modulus, self.n_limbs = modulus, n_limbs


def test_argument_checks_of_solve_need_no_device():
    from honeybadgermpc_amd import solver

    assert solver.MAX_K >= 1024 and 2 <= solver.SMALL_DEGREE < solver.MAX_K
    ctx = _Ctx(BLS, 4)
    with pytest.raises(ValueError):
        solver.solve(ctx, [])
    with pytest.raises(ValueError):
        solver.solve(ctx, [5])                                      # k < 2
    with pytest.raises(ValueError):
        solver.solve(_Ctx(13, 1), [1] * 13)                          # modulus <= k
    with pytest.raises(ValueError):
        solver.solve(ctx, [1] * (solver.MAX_K + 1))
    with pytest.raises(ValueError):
        solver.solve(ctx, np.zeros((5, 3), dtype=np.int64))          # wrong limb count
    with pytest.raises(ValueError):
        solver.solve(ctx, np.zeros((5,), dtype=np.int64))
    with pytest.raises(ValueError):
        solver.solve(ctx, np.zeros((1, 4), dtype=np.int64))          # k < 2 as a tensor


def test_no_cpu_fallback():
    import torch

    if torch.cuda.is_available():
        return
    from honeybadgermpc_amd._capi import Context, HbmpcBackendError

    with pytest.raises(HbmpcBackendError):
        Context.get(BLS)


def test_selftest_refuses_bad_arguments():
    assert run(13, 4, NEWTON, [[1] * 13], [13], 14)[0] == 2            # k >= p
    assert run(BLS, 4, 9, [[1]], [1], 1)[0] == 2                       # unknown `what`
    assert run(BLS, 4, GCD, [[1, 1], [1, 1, 1]], [1, 2], 3)[0] == 2    # db > da
    assert run(BLS, 4, STEP, [[1, 1], [1], [1]], [1, 0], 1)[0] == 2    # d < 2


def test_abi_names_in_header_and_ctypes_table():
    from honeybadgermpc_amd import _capi, solver

    text = open(os.path.join(REPO, "include", "hbmpc_hip.h")).read()
    for name in ("hb_rf_newton", "hb_rf_roots", "hb_selftest_rf"):
        assert re.search(r"\bint " + name + r"\s*\(", text) and name in _capi.SYMBOLS
    for name, value in (("HB_RF_MAX_K", solver.MAX_K), ("HB_RF_SMALL_DEGREE", solver.SMALL_DEGREE), ("HB_RF_SELFTEST_NEWTON", 0), ("HB_RF_SELFTEST_STEP", 1),
                        ("HB_RF_SELFTEST_GCD", 2), ("HB_RF_SELFTEST_SHIFT", 3), ("HB_RF_SELFTEST_ROOTS", 4)):
        assert re.search(r"#define " + name + r" " + str(value) + r"\b", text) and getattr(_capi, name) == value
    debug = open(os.path.join(REPO, "include", "hbmpc_hip_debug.h")).read()
    for name in ("hb_debug_rf_stats", "hb_debug_rf_profile"):
        assert name in debug and name in _capi.DEBUG_SYMBOLS

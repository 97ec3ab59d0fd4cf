"""CPU-only: the edge-value helper (tests/edge_values.py) itself, and the radix-2^29 arithmetic the kernels share (csrc/fp29.hpp through
hb_selftest_mulmod and hb_selftest_ew) over every ordered pair of pool values and their Montgomery pre-images, against Python ints.
Exact equality."""
import ctypes
import itertools

import numpy as np
import pytest

import edge_values as ev
from conftest import BLS
from test_share_arithmetic_host import ADD, BEAVER, BROADCAST, IDS, INV, MUL, NEG, PRIMES, SUB, run

SECP_N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
# the moduli of tests/test_gpu_edge_values.py
GPU_PRIMES = [BLS, (1 << 256) - 189, SECP_N, (1 << 255) - 19, (1 << 255) + 95, (1 << 64) - 59, 0xFFFFFFFF00000001, (1 << 61) - 1]
GPU_IDS = ["bls", "2^256-189", "secp256k1-n", "2^255-19", "2^255+95", "2^64-59", "goldilocks", "2^61-1"]
POOL_SIZES = {BLS: 55, (1 << 256) - 189: 55, (1 << 255) - 19: 55, (1 << 64) - 59: 37, 0xFFFFFFFF00000001: 35}


# ---- the helper ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", GPU_PRIMES, ids=GPU_IDS)
def test_pool_members(p):
    nl = ev.n_limbs_of(p)
    bits = 64 * nl
    pool = ev.edge_pool(p, nl)
    assert pool == sorted(set(pool)) and all(0 <= v < p for v in pool)
    if p in POOL_SIZES:
        assert len(pool) == POOL_SIZES[p]
    have = set(pool)
    want = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, (1 << bits) - p - 1, (1 << bits) - p, (1 << bits) - p + 1]
    want += [(1 << (32 * j)) + s for j in range(1, bits // 32 + 1) for s in (-1, 0, 1)]
    want += [(1 << (29 * j)) + s for j in range(1, 10) for s in (-1, 0)]
    want += [int(b * (bits // 8), 16) for b in ("80", "7f", "ff", "01", "fe")] + [int("ff00" * (bits // 16), 16), int("00ff" * (bits // 16), 16)]
    assert all(v % p in have for v in want) and len(have) <= len(want)
    big_r = ev.montgomery_radix(nl)
    assert [v * big_r % p for v in ev.montgomery_preimages(p, nl)] == pool


@pytest.mark.parametrize("p", GPU_PRIMES, ids=GPU_IDS)
def test_targeted_rows_hit_their_targets(p):
    pool = ev.edge_pool(p, ev.n_limbs_of(p))
    count = len(pool) + 3
    for x, where in [(list(range(1, 65)), list(range(40, 62))), (list(range(1, 25)), [23, 0, 7, 5, 11, 2]), ([pow(7, i, p) for i in range(16)], [15, 3, 9, 1, 0, 8]),
                     (list(range(1, 8)), [6, 2, 4])]:
        d = len(where)
        rows = ev.targeted_rows(p, x, where, d, count, seed=3)
        assert len(rows) == count and all(len(r) == d and all(0 <= v < p for v in r) for r in rows)
        vals = ev.evaluate_rows(p, x, rows)
        tg = ev.targets(p, d, count, seed=3)
        hit = sum(vals[k][j] == tg[k][i] and tg[k][i] in pool for k in range(count) for i, j in enumerate(where))
        assert hit == count * d                                    # 100 % of the targeted positions hold their pool value
        for i in range(d):                                         # every value at every position once
            assert sorted(tg[k][i] for k in range(len(pool))) == pool
    rows = ev.edge_rows(p, 6, count, seed=1)
    assert all(v in set(pool) | set(ev.montgomery_preimages(p, ev.n_limbs_of(p))) for r in rows for v in r) and rows[len(pool)] == [p - 1] * 6
    for i in range(6):
        assert sorted(r[i] for r in rows[: len(pool)]) == pool


# ---- fp29.hpp on the host ---------------------------------------------------------------------------------------------------
operands, reduced_pool = ev.operands, ev.reduced_pool


@pytest.mark.parametrize("p, nl", PRIMES, ids=IDS)
def test_mulmod_every_ordered_pair(p, nl):
    from honeybadgermpc_amd._capi import ints_to_limbs, limbs_to_ints, load_library, np_ptr

    lib = load_library()
    vs = operands(p, nl)
    arr = ints_to_limbs(vs, p, 8 * nl)
    pl = np_ptr(ints_to_limbs([p], p + 1, 8 * nl))
    step = arr.strides[0]
    out = np.zeros((len(vs) * len(vs), nl), dtype=np.uint64)
    k = 0
    for i in range(len(vs)):
        for j in range(len(vs)):
            rc = lib.hb_selftest_mulmod(pl, nl, ctypes.c_void_p(arr.ctypes.data + i * step), ctypes.c_void_p(arr.ctypes.data + j * step),
                                        ctypes.c_void_p(out.ctypes.data + k * out.strides[0]))
            assert rc == 0
            k += 1
    assert limbs_to_ints(out, 8 * nl) == [a * b % p for a in vs for b in vs]


@pytest.mark.parametrize("p, nl", PRIMES, ids=IDS)
def test_binary_ops_every_ordered_pair(p, nl):
    vs = operands(p, nl)
    pairs = list(itertools.product(vs, repeat=2))
    a, b = [x for x, _ in pairs], [y for _, y in pairs]
    assert run(p, nl, ADD, [a, b], len(pairs)) == [(x + y) % p for x, y in pairs]
    assert run(p, nl, SUB, [a, b], len(pairs)) == [(x - y) % p for x, y in pairs]
    assert run(p, nl, MUL, [a, b], len(pairs)) == [x * y % p for x, y in pairs]
    assert run(p, nl, NEG, [vs], len(vs)) == [-x % p for x in vs]
    for s in vs:                                                   # the broadcast forms: the same pairs with b as one element
        assert run(p, nl, ADD | BROADCAST, [vs, [s]], len(vs)) == [(x + s) % p for x in vs]
        assert run(p, nl, SUB | BROADCAST, [vs, [s]], len(vs)) == [(x - s) % p for x in vs]
        assert run(p, nl, MUL | BROADCAST, [vs, [s]], len(vs)) == [x * s % p for x in vs]


@pytest.mark.parametrize("p, nl", PRIMES, ids=IDS)
def test_beaver_step_every_tuple_of_the_reduced_pool(p, nl):
    ts = list(itertools.product(reduced_pool(p, nl), repeat=5))
    cols = [[tp[k] for tp in ts] for k in range(5)]
    assert run(p, nl, BEAVER, cols, len(ts)) == [(d * e + d * q + e * pp + pq) % p for d, e, pp, q, pq in ts]


@pytest.mark.parametrize("p, nl", PRIMES, ids=IDS)
def test_inversion_of_the_pool(p, nl):
    xs = [v for v in operands(p, nl) if v]
    zeros = np.zeros(1, dtype=np.uint64)
    assert run(p, nl, INV, [xs], len(xs), extra=zeros) == [pow(x, -1, p) for x in xs]
    assert int(zeros[0]) == 0
    xs = operands(p, nl)                                           # with the zero among them
    assert run(p, nl, INV, [xs], len(xs), extra=zeros) == [pow(x, -1, p) if x else 0 for x in xs]
    assert int(zeros[0]) == 1


def test_interpolate_and_balanced_digits():
    p = (1 << 255) - 19
    xs, ys = [5, 1, 9, 2], [0, p - 1, 7, 1 << 200]
    co = ev.interpolate(p, xs, ys)
    assert len(co) == 4 and ev.evaluate_rows(p, xs, [co]) == [ys]
    # 32 digits in -128 .. 127: the largest such value is 0x7f7f..7f, and a byte of 0x80 or more carries into the next
    assert ev.fits_32_balanced_digits(int("7f" * 32, 16)) and not ev.fits_32_balanced_digits(int("7f" * 31 + "80", 16))
    assert ev.fits_32_balanced_digits(int("7e" + "ff" * 31, 16)) and not ev.fits_32_balanced_digits(int("7f" + "ff" * 31, 16))
    assert ev.fits_32_balanced_digits(0) and not ev.fits_32_balanced_digits(1 << 255) and not ev.fits_32_balanced_digits(1 << 256)

"""CPU-only: the per-element bodies of the element-wise kernels (csrc/hb_ew.hip) run on the host through hb_selftest_ew --
the rows EwBinaryRow and EwBeaverRow that the device runs and the lane function k_ew_inv calls -- against Python int arithmetic.  Exact equality."""
import ctypes
import itertools
import random

import numpy as np
import pytest

from conftest import BLS
from selftest_cases import run_ew as run

PRIMES = [(BLS, 4), (13, 4), (53, 4), ((1 << 256) - 189, 4), ((1 << 255) - 19, 4), (13, 1), ((1 << 64) - 59, 1), (0xFFFFFFFF00000001, 1)]
IDS = ["bls", "13w", "53w", "2^256-189", "2^255-19", "13n", "2^64-59", "goldilocks"]
ADD, SUB, MUL, NEG, BEAVER, INV, BROADCAST = 0, 1, 2, 3, 4, 5, 0x100


def tuples(p, arity, rnd, n_random=200):
    corners = [0, 1, p - 1]
    return [tuple(c) for c in itertools.product(corners, repeat=arity)] + [tuple(rnd.randrange(p) for _ in range(arity)) for _ in range(n_random)]


@pytest.mark.parametrize("p, nl", PRIMES, ids=IDS)
def test_binary_ops_on_the_host(p, nl):
    rnd = random.Random(p % 1000 + nl)
    ts = tuples(p, 2, rnd)
    a, b = [x for x, _ in ts], [y for _, y in ts]
    assert run(p, nl, ADD, [a, b], len(ts)) == [(x + y) % p for x, y in ts]
    assert run(p, nl, SUB, [a, b], len(ts)) == [(x - y) % p for x, y in ts]
    assert run(p, nl, MUL, [a, b], len(ts)) == [x * y % p for x, y in ts]
    assert run(p, nl, NEG, [a], len(ts)) == [-x % p for x in a]
    # one element broadcast over the array
    for s in (0, 1, p - 1, rnd.randrange(p)):
        assert run(p, nl, ADD | BROADCAST, [a, [s]], len(ts)) == [(x + s) % p for x in a]
        assert run(p, nl, SUB | BROADCAST, [a, [s]], len(ts)) == [(x - s) % p for x in a]
        assert run(p, nl, MUL | BROADCAST, [a, [s]], len(ts)) == [x * s % p for x in a]


@pytest.mark.parametrize("p, nl", PRIMES, ids=IDS)
def test_beaver_step_on_the_host(p, nl):
    """d e + d q + e p + pq over all 3^5 corner tuples of {0, 1, p - 1} (every operand p - 1 over 2^256 - 189 is the largest
    value the lazy columns of the fused step ever hold) and 200 random ones"""
    rnd = random.Random(p % 1000 + 7 * nl)
    ts = tuples(p, 5, rnd)
    assert len(ts) == 243 + 200 and (p - 1,) * 5 in ts
    cols = [[tp[k] for tp in ts] for k in range(5)]
    want = [(d * e + d * q + e * pp + pq) % p for d, e, pp, q, pq in ts]
    assert run(p, nl, BEAVER, cols, len(ts)) == want


@pytest.mark.parametrize("p, nl", PRIMES, ids=IDS)
def test_inversion_tiles_on_the_host(p, nl):
    """Montgomery's trick as the kernel's waves walk it: no zero, one zero (first lane, last lane, ragged tail), all zeros,
    and lengths that are not a multiple of the tile (64 x 8 elements wide, 64 x 16 narrow)"""
    rnd = random.Random(p % 1000 + 11 * nl)
    tile = 64 * (8 if nl == 4 else 16)

    def check(xs):
        zeros = np.zeros(1, dtype=np.uint64)
        got = run(p, nl, INV, [xs], len(xs), extra=zeros)
        assert got == [pow(x, -1, p) if x else 0 for x in xs]
        assert int(zeros[0]) == sum(1 for x in xs if x == 0)

    def nonzero(k):
        return [rnd.randrange(1, p) for _ in range(k)]

    check(nonzero(tile))
    check(nonzero(1))
    check(nonzero(tile + 65))                      # a second, ragged tile
    check([1, p - 1] + nonzero(61))                # less than a wave
    for pos in (0, 63, tile - 1, tile, tile + 64):  # first lane, last lane, last slot of a tile, the ragged tail
        xs = nonzero(tile + 65)
        xs[pos] = 0
        check(xs)
    xs = nonzero(tile + 65)
    for pos in (0, 64, 128, tile + 64):            # several zeros in one lane's chain
        xs[pos] = 0
    check(xs)
    check([0] * tile)
    check([0] * 3)
    check([])


def test_selftest_rejects_bad_arguments():
    from honeybadgermpc_amd._capi import HB_ERR_BAD_ARG, ints_to_limbs, load_library, np_ptr

    lib = load_library()
    p = ints_to_limbs([BLS], BLS + 1, 32)
    a = ints_to_limbs([1, 2], BLS, 32)
    out = np.zeros((2, 4), dtype=np.uint64)
    ptrs = (ctypes.c_void_p * 5)(a.ctypes.data, a.ctypes.data, a.ctypes.data, a.ctypes.data, a.ctypes.data)
    assert lib.hb_selftest_ew(np_ptr(p), 4, 6, ptrs, np_ptr(out), 2) == HB_ERR_BAD_ARG       # unknown op
    assert lib.hb_selftest_ew(np_ptr(p), 4, 0x200, ptrs, np_ptr(out), 2) == HB_ERR_BAD_ARG   # unknown flag
    assert lib.hb_selftest_ew(np_ptr(p), 2, MUL, ptrs, np_ptr(out), 2) == HB_ERR_BAD_ARG     # neither 1 nor 4 limbs
    assert lib.hb_selftest_ew(np_ptr(p), 4, MUL, ptrs, np_ptr(out), -1) == HB_ERR_BAD_ARG
    ptrs[1] = None
    assert lib.hb_selftest_ew(np_ptr(p), 4, MUL, ptrs, np_ptr(out), 2) == HB_ERR_BAD_ARG     # a missing operand

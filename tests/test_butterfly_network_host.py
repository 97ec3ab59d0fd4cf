"""CPU-only: the wiring model of honeybadgermpc_amd.butterfly_network against tests/golden/butterfly_network.json (written by
scratch/gen_butterfly_golden.py from the reference's own iterated_butterfly_network, run in the clear), and the per-element
bodies of the butterfly kernels (csrc/hb_bf.hip) run on the host through hb_selftest_bf -- the rows BfMaskRow and BfSwitchRow that the
device runs -- against Python ints.  Exact equality."""
import itertools
import json
import os
import random
import re

import numpy as np
import pytest

from conftest import BLS, REPO
from selftest_cases import run_bf as run

from honeybadgermpc_amd import butterfly_network as bn

PRIMES = [(BLS, 4), (13, 4), (53, 4), ((1 << 256) - 189, 4), ((1 << 255) - 19, 4), (13, 1), ((1 << 64) - 59, 1), (0xFFFFFFFF00000001, 1)]
IDS = ["bls", "13w", "53w", "2^256-189", "2^255-19", "13n", "2^64-59", "goldilocks"]
MASK, SWITCH, INDEX, HALVE = 0, 1, 2, 3


def golden():
    with open(os.path.join(REPO, "tests", "golden", "butterfly_network.json")) as f:
        g = json.load(f)
    assert int(g["modulus"]) == BLS and [c["k"] for c in g["cases"]] == [2, 4, 8, 32]
    return [{"k": c["k"], "inputs": [int(v) for v in c["inputs"]], "signs": c["signs"], "output": [int(v) for v in c["output"]]} for c in g["cases"]]


def mask_ref(p, xs, bits, ps, qs, k, a):
    xi, yi = bn.switch_indices(k, a)
    return [(b - pp) % p for b, pp in zip(bits, ps)] + [(xs[i] - xs[j] - q) % p for i, j, q in zip(xi, yi, qs)]


def switch_ref(p, xs, d, e, ps, qs, pqs, k, a):
    xi, yi = bn.switch_indices(k, a)
    inv2 = pow(2, -1, p)
    out = []
    for j in range(k // 2):
        m = (d[j] * e[j] + d[j] * qs[j] + e[j] * ps[j] + pqs[j]) % p
        x, y = xs[xi[j]], xs[yi[j]]
        out += [(x + y + m) * inv2 % p, (x + y - m) * inv2 % p]
    return out


# ---- the wiring -----------------------------------------------------------------------------------------------------
def test_layers_and_indices_partition_the_inputs():
    assert bn.layers(2) == [0] and bn.layers(8) == [0, 1, 2] * 3 and len(bn.layers(1024)) == 100
    assert bn.switch_indices(8, 0) == ([0, 2, 4, 6], [1, 3, 5, 7])
    assert bn.switch_indices(8, 1) == ([0, 1, 4, 5], [2, 3, 6, 7])
    assert bn.switch_indices(8, 2) == ([0, 1, 2, 3], [4, 5, 6, 7])
    for n in range(1, 11):
        k = 1 << n
        for a in range(n):
            xi, yi = bn.switch_indices(k, a)
            assert sorted(xi + yi) == list(range(k)) and all(y == x + (1 << a) for x, y in zip(xi, yi)) and xi == sorted(xi)
    for bad in (0, 1, 3, 12, -4, 2.0):
        with pytest.raises(ValueError):
            bn.layers(bad)
    for k, a in ((8, 3), (8, -1), (2, 1), (6, 0)):
        with pytest.raises(ValueError):
            bn.switch_indices(k, a)


def test_permutation_reproduces_the_reference():
    for c in golden():
        perm = bn.permutation(c["k"], c["signs"])
        assert sorted(perm) == list(range(c["k"]))
        assert [c["inputs"][i] for i in perm] == c["output"], c["k"]
    k = 8
    straight = [[1] * 4] * 9
    assert sorted(bn.permutation(k, straight)) == list(range(k))
    assert bn.permutation(2, [[1]]) == [0, 1] and bn.permutation(2, [[-1]]) == [1, 0]
    with pytest.raises(ValueError):
        bn.permutation(8, straight[:8])
    with pytest.raises(ValueError):
        bn.permutation(8, [[1, 1, 1, 0]] * 9)
    with pytest.raises(ValueError):
        bn.permutation(8, [[1, 1, 1]] * 9)


@pytest.mark.parametrize("nl", [4, 1])
def test_index_map_on_the_host_every_stride(nl):
    from honeybadgermpc_amd._capi import ints_to_limbs, load_library, np_ptr

    for n in range(1, 11):
        k = 1 << n
        for a in range(n):
            out = np.zeros(k, dtype=np.uint64)
            assert load_library().hb_selftest_bf(np_ptr(ints_to_limbs([13], 14, 8 * nl)), nl, INDEX, None, k, a, np_ptr(out)) == 0
            xi, yi = bn.switch_indices(k, a)
            assert out[0::2].tolist() == xi and out[1::2].tolist() == yi, (k, a)


# ---- the element bodies ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p, nl", PRIMES, ids=IDS)
def test_halving_on_the_host(p, nl):
    rnd = random.Random(p % 1000 + 3 * nl)
    vs = [0, 1, 2, 3, p - 1, p - 2, p - 3, (p - 1) // 2, (p + 1) // 2] + [rnd.randrange(p) for _ in range(200)]
    vs = [v % p for v in vs]
    rc, got = run(p, nl, HALVE, [vs], len(vs), 0, len(vs))
    inv2 = pow(2, -1, p)
    assert rc == 0 and got == [v * inv2 % p for v in vs]
    assert all(2 * h % p == v for h, v in zip(got, vs))


@pytest.mark.parametrize("p, nl", PRIMES, ids=IDS)
def test_mask_elements_on_the_host(p, nl):
    """all corner tuples of {0, 1, p - 1} in (x, y, bit, p, q) and random ones: one switch each, laid out as a layer of stride 1"""
    rnd = random.Random(p % 1000 + 5 * nl)
    ts = [tuple(c) for c in itertools.product([0, 1, p - 1], repeat=5)] + [tuple(rnd.randrange(p) for _ in range(5)) for _ in range(13)]
    assert len(ts) == 256
    k = 2 * len(ts)
    xs = [v for tp in ts for v in tp[:2]]
    bits, ps, qs = ([tp[i] for tp in ts] for i in (2, 3, 4))
    want = mask_ref(p, xs, bits, ps, qs, k, 0)
    rc, got = run(p, nl, MASK, [xs, bits, ps, qs], k, 0, k)
    assert rc == 0 and got == want
    rc, got = run(p, nl, MASK, [xs, None, None, qs], k, 0, k // 2)               # the signs' half opened in advance
    assert rc == 0 and got == want[k // 2:]
    for a in range(1, 9):                                                         # the same values through every other stride
        want = mask_ref(p, xs, bits, ps, qs, k, a)
        rc, got = run(p, nl, MASK, [xs, bits, ps, qs], k, a, k)
        assert rc == 0 and got == want, a


@pytest.mark.parametrize("p, nl", PRIMES, ids=IDS)
def test_switch_elements_on_the_host(p, nl):
    """all 3^7 corner tuples of {0, 1, p - 1} in (x, y, d, e, p, q, pq) -- every operand p - 1 over 2^256 - 189 among them -- and
    random ones"""
    rnd = random.Random(p % 1000 + 7 * nl)
    ts = [tuple(c) for c in itertools.product([0, 1, p - 1], repeat=7)] + [tuple(rnd.randrange(p) for _ in range(7)) for _ in range(4096 - 2187)]
    assert len(ts) == 4096 and (p - 1,) * 7 in ts
    k = 2 * len(ts)
    xs = [v for tp in ts for v in tp[:2]]
    d, e, ps, qs, pqs = ([tp[i] for tp in ts] for i in (2, 3, 4, 5, 6))
    for a in (0, 5, 12):
        rc, got = run(p, nl, SWITCH, [xs, d, e, ps, qs, pqs], k, a, k)
        assert rc == 0 and got == switch_ref(p, xs, d, e, ps, qs, pqs, k, a), a


@pytest.mark.parametrize("p, nl", PRIMES, ids=IDS)
def test_bodies_at_edge_values(p, nl):
    """every operand a value on the edges of the words, the digits and the int8 split, or the Montgomery pre-image of one
    (tests/edge_values.py): each list walks the pool at its own stride; 128 switches"""
    import edge_values

    vs = edge_values.operands(p, nl)
    m, half = len(vs), 128
    k = 2 * half
    xs = [vs[(3 * i + 1) % m] for i in range(k)]
    d, e, ps, qs, pqs = ([vs[(i * s + s) % m] for i in range(half)] for s in (5, 7, 11, 13, 17))
    rc, got = run(p, nl, HALVE, [vs], m, 0, m)
    assert rc == 0 and got == [v * pow(2, -1, p) % p for v in vs]
    for a in (0, 3, 7):
        rc, got = run(p, nl, MASK, [xs, d, ps, qs], k, a, k)
        assert rc == 0 and got == mask_ref(p, xs, d, ps, qs, k, a), a
        rc, got = run(p, nl, SWITCH, [xs, d, e, ps, qs, pqs], k, a, k)
        assert rc == 0 and got == switch_ref(p, xs, d, e, ps, qs, pqs, k, a), a


@pytest.mark.parametrize("p, nl", [(2**256 - 189, 4), (2**64 - 59, 1)], ids=["2^256-189", "2^64-59"])
def test_switch_halves_every_parity_corner(p, nl):
    """cleartext triple (p = q = pq = 0, d = b, e = x - y): the sums x + y +- m that are halved run over 0, 1, 2, p - 1, p - 2
    and their neighbours, odd and even"""
    vals = [0, 1, 2, 3, p - 1, p - 2, p - 3, p - 4, (p - 1) // 2, (p + 1) // 2]
    pairs = [(x, y) for x in vals for y in vals]
    for b in (1, p - 1):
        k = 2
        while k < 2 * len(pairs):
            k *= 2
        full = pairs + [(0, 0)] * (k // 2 - len(pairs))
        xs = [v for pr in full for v in pr]
        zero = [0] * (k // 2)
        e = [(x - y) % p for x, y in full]
        rc, got = run(p, nl, SWITCH, [xs, [b] * (k // 2), e, zero, zero, zero], k, 0, k)
        assert rc == 0
        want = [v for x, y in full for v in ((x, y) if b == 1 else (y, x))]
        assert got == want


def test_whole_network_on_the_host_equals_the_reference():
    """every layer through the mask and switch bodies with cleartext triples: the masked values ARE b and x - y"""
    p = BLS
    for c in golden():
        k, cur = c["k"], c["inputs"]
        zero = [0] * (k // 2)
        for a, row in zip(bn.layers(k), c["signs"]):
            bits = [b % p for b in row]
            rc, masked = run(p, 4, MASK, [cur, bits, zero, zero], k, a, k)
            assert rc == 0 and masked[: k // 2] == bits
            rc, cur = run(p, 4, SWITCH, [cur, masked[: k // 2], masked[k // 2:], zero, zero, zero], k, a, k)
            assert rc == 0
        assert cur == c["output"], k


def test_random_layers_with_real_triples_on_the_host():
    """shares of one party are arbitrary field values: the two passes against Python ints, k up to 1024, every stride"""
    for p, nl in ((BLS, 4), ((1 << 64) - 59, 1)):
        rnd = random.Random(nl)
        for n in (1, 2, 5, 10):
            k = 1 << n
            for a in range(n):
                xs = [rnd.randrange(p) for _ in range(k)]
                bits, ps, qs, pqs, d, e = ([rnd.randrange(p) for _ in range(k // 2)] for _ in range(6))
                rc, got = run(p, nl, MASK, [xs, bits, ps, qs], k, a, k)
                assert rc == 0 and got == mask_ref(p, xs, bits, ps, qs, k, a)
                rc, got = run(p, nl, SWITCH, [xs, d, e, ps, qs, pqs], k, a, k)
                assert rc == 0 and got == switch_ref(p, xs, d, e, ps, qs, pqs, k, a)


# ---- the ABI --------------------------------------------------------------------------------------------------------
def test_abi_names_in_header_and_ctypes_table():
    from honeybadgermpc_amd import _capi

    text = open(os.path.join(REPO, "include", "hbmpc_hip.h")).read()
    for name in ("hb_bf_mask", "hb_bf_switch", "hb_selftest_bf"):
        assert re.search(r"\bint " + name + r"\s*\(", text) and name in _capi.SYMBOLS
    for name, value in (("HB_BF_SELFTEST_MASK", 0), ("HB_BF_SELFTEST_SWITCH", 1), ("HB_BF_SELFTEST_INDEX", 2), ("HB_BF_SELFTEST_HALVE", 3)):
        assert re.search(r"#define " + name + r" " + str(value) + r"\b", text) and getattr(_capi, name) == value


def test_selftest_rejects_bad_arguments():
    xs, h = [1, 2, 3, 4], [1, 2]
    for nl in (4, 1):
        assert run(13, nl, SWITCH, [xs, h, h, h, h, h], 4, 0, 4)[0] == 0
        assert run(13, nl, SWITCH, [xs, h, h, h, h, h], 4, 2, 4)[0] == 2          # log2_stride == log2(k)
        assert run(13, nl, SWITCH, [xs, h, h, h, h, h], 4, -1, 4)[0] == 2
        assert run(13, nl, SWITCH, [xs, h, h, h, h, h], 3, 0, 4)[0] == 2          # k not a power of two
        assert run(13, nl, SWITCH, [xs, h, h, h, h, h], 1, 0, 4)[0] == 2
        assert run(13, nl, SWITCH, [xs, h, h, h, h, None], 4, 0, 4)[0] == 2       # a missing operand
        assert run(13, nl, MASK, [xs, h, None, h], 4, 0, 4)[0] == 2               # signs without p
        assert run(13, nl, MASK, [None, h, h, h], 4, 0, 4)[0] == 2
        assert run(13, nl, 4, [xs, h, h, h, h, h], 4, 0, 4)[0] == 2               # unknown `what`
        assert run(13, nl, HALVE, [xs], -1, 0, 4)[0] == 2
        assert run(13, nl, HALVE, [[]], 0, 0, 0)[0] == 0
    assert run(13, 2, SWITCH, [xs, h, h, h, h, h], 4, 0, 4)[0] == 2               # neither 1 nor 4 limbs

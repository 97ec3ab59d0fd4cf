"""k_mm8f's division by den_l on the matrix cores as a big-integer model (tests/fs_mscale_model.py): every column, word and quotient bound
asserted inside the model, and the result compared with y / den_l mod p, at 1 / den of real arrival sets and of the extreme ones.
CPU only."""
import random

import numpy as np
import pytest

import edge_values
import fs_mscale_model as mm

BLS_R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
PRIMES = [BLS_R, (1 << 256) - 189, (1 << 254) + 0x4f]      # (the last is not prime: the arithmetic does not care, and every den here is a unit)
N, D = 64, 22
X = list(range(1, N + 1))


def _arrival_sets():
    """points of the d arrivals: the benchmark's seeded order, two other seeded ones, all adjacent (low and high), 1 and 64 with the rest
    clustered (at either end and in the middle), and the smallest shape the kernel takes (d = 4)"""
    sets = [[X[i] for i in np.random.Generator(np.random.PCG64(2024)).permutation(N).tolist()[:D]]]
    for seed in (7, 99):
        order = list(range(N))
        random.Random(seed).shuffle(order)
        sets.append([X[i] for i in order[:D]])
    sets.append(list(range(1, D + 1)))
    sets.append(list(range(N - D + 1, N + 1)))
    sets.append([1, 64] + list(range(2, D)))
    sets.append([1, 64] + list(range(44, 64)))
    sets.append([1, 64] + list(range(22, 42)))
    sets.append([1, 2, 3, 4])
    sets.append([1, 13, 6, 7])
    return sets


def _weights(p):
    ws = []
    for xs in _arrival_sets():
        ws += [mm.inv_den(p, xs, j) for j in range(len(xs))]
    return sorted(set(ws))


def _patterns(p):
    """y = 0, 1, p - 1; every element whose bytes are all from {00, 7f, 80, ff} in runs (below p); the edge pool"""
    ys = [0, 1, p - 1]
    for a in (0x00, 0x7f, 0x80, 0xff):
        for b in (0x00, 0x7f, 0x80, 0xff):
            for cut in (0, 1, 15, 16, 17, 31):
                ys.append(int.from_bytes(bytes([a] * cut + [b] * (32 - cut)), "little"))
            ys.append(int.from_bytes(bytes([a, b] * 16), "little"))
    ys += edge_values.edge_pool(p, 4)
    return sorted({y for y in ys if y < p})


@pytest.mark.parametrize("p", PRIMES, ids=["bls-r", "2^256-189", "2^254+79"])
def test_tables_fit_and_constants_are_bytes(p):
    for w in _weights(p):
        digits, cinit = mm.term_tables(p, w)
        assert len(digits) == 32 and all(len(d) == 32 and all(-128 <= x <= 127 for x in d) for d in digits)
        assert all(mm.BIAS <= c < mm.BIAS + 256 for c in cinit)
        # every accumulator, at any input: |sum| <= 32 * 128 * 128 = 2^19 below and above the constant
        for c in range(32):
            worst = sum(128 * abs(digits[b][c]) for b in range(32))
            assert worst <= 1 << 19 and cinit[c] - worst > 0 and cinit[c] + worst < 1 << 31


@pytest.mark.parametrize("p", PRIMES, ids=["bls-r", "2^256-189", "2^254+79"])
def test_scaled_element_at_patterns_and_edges(p):
    facts = set()
    ys = _patterns(p)
    for w in _weights(p):
        tab = mm.term_tables(p, w)
        for y in ys:
            r = mm.scale_model(y, p, tab, facts)
            assert r % p == y * w % p and r < 1 << 256
            assert r < (p if p >> 255 else 2 * p)
    assert "exact" in facts


@pytest.mark.parametrize("p", PRIMES, ids=["bls-r", "2^256-189", "2^254+79"])
def test_scaled_element_at_random_inputs(p):
    rng = random.Random(p % 10007)
    ws = _weights(p)
    tabs = {}
    for it in range(4000):
        w = ws[it % len(ws)]
        if w not in tabs:
            tabs[w] = mm.term_tables(p, w)
        y = rng.randrange(p)
        r = mm.scale_model(y, p, tabs[w])
        assert r % p == y * w % p


def test_residues_that_need_the_conditional_subtraction():
    """p = 2^256 - 189: y = v den mod p for small v puts the residue next to 0, where an estimate one short leaves r = v + p >= 2^256"""
    p = (1 << 256) - 189
    facts = set()
    xs = _arrival_sets()[0]
    for j in (0, 5, 21):
        w = mm.inv_den(p, xs, j)
        den = pow(w, -1, p)
        tab = mm.term_tables(p, w)
        for v in list(range(0, 400)) + [p - 1, p - 2, 1 << 200]:
            assert mm.scale_model(v * den % p, p, tab, facts) == v % p
    assert {"exact", "under", "top1"} <= facts

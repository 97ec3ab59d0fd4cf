"""CPU-only: the share bits of the offline phase -- a random residue shared with its bit planes, by rejection of bitwise-shared
candidates.  The model on Python ints and the number of candidates a round draws; the two rows of csrc/hb_offsb.hip run on the host through
hb_selftest_off_share_bits -- the same functions and the same index arithmetic the kernels run -- against Python ints: the leaves against
the affine maps and, folded by the carry tree's operator on ints, against [r >= p] at every edge candidate; the finish against the model
for every kind of index list, with a sentinel behind every output; what is refused.  Exact equality."""
import asyncio
import math
import os
import random
import re

import numpy as np
import pytest

from conftest import BLS, REPO

from honeybadgermpc_amd import offline

GOLDILOCKS = 0xFFFFFFFF00000001
P64 = (1 << 64) - 59
P256 = (1 << 256) - 189
FIELDS = [(BLS, 4), (P256, 4), (P64, 1), (P64, 4), (GOLDILOCKS, 1), (GOLDILOCKS, 4), (13, 4), (13, 1)]
FIELD_IDS = ["bls", "2^256-189", "2^64-59-narrow", "2^64-59-wide", "goldilocks-narrow", "goldilocks-wide", "13-wide", "13-narrow"]
LEAVES, FINISH = 0, 1
SENTINEL = 0xA5A5A5A5A5A5A5A5                   # in every limb behind an output (no vector here takes that value)


def _lib():
    from honeybadgermpc_amd._capi import load_library

    return load_library()


def _limbs(values, p, nl):
    from honeybadgermpc_amd._capi import ints_to_limbs

    return ints_to_limbs(list(values) or [0], p, 8 * nl)


def _ints(arr, nl):
    from honeybadgermpc_amd._capi import limbs_to_ints

    return limbs_to_ints(np.ascontiguousarray(arr).reshape(-1, nl), 8 * nl)


def _raw(value, nl):
    """an integer below 2^(64 nl) as limbs, whatever the modulus"""
    return np.array([(value >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(nl)], dtype=np.uint64)


def _selftest(p, nl, what, bits, L, bound, candidates, index, out0, out1, count, modulus=True):
    ptr = lambda a: None if a is None else a.ctypes.data
    mod = _raw(p, nl)
    return _lib().hb_selftest_off_share_bits(ptr(mod) if modulus else None, nl, what, ptr(bits), L, ptr(bound), candidates, ptr(index), ptr(out0), ptr(out1), count)


def _edge_candidates(p):
    """the candidates at which the comparison can go wrong, and p - 1 with each single bit flipped: every leaf position decides once"""
    L = p.bit_length()
    return [0, 1, p - 2, p - 1, p, p + 1, 1 << (L - 1), (1 << L) - 1] + [(p - 1) ^ (1 << i) for i in range(L)]


def _planes(values, L):
    """[L][count] ints: plane i holds bit i of every value"""
    return [[(v >> i) & 1 for v in values] for i in range(L)]


def _leaves(p, nl, planes, bound=None):
    """the host rows over planes [L][count] of residues -> (g, p) as [L][count] ints, most significant first"""
    L, count = len(planes), len(planes[0])
    flat = _limbs([v for plane in planes for v in plane], p, nl)
    g = np.full((L * count + 1, nl), SENTINEL, dtype=np.uint64)
    q = np.full((L * count + 1, nl), SENTINEL, dtype=np.uint64)
    before = flat.copy()
    assert _selftest(p, nl, LEAVES, flat, L, None if bound is None else _raw(bound, nl), 0, None, g, q, count) == 0
    assert np.array_equal(flat, before) and (g[L * count:] == SENTINEL).all() and (q[L * count:] == SENTINEL).all()
    gi, qi = _ints(g[:L * count], nl), _ints(q[:L * count], nl)
    return [gi[y * count:(y + 1) * count] for y in range(L)], [qi[y * count:(y + 1) * count] for y in range(L)]


def _fold(g, q, p):
    """the g at the root of (g1, p1) o (g2, p2) = (g1 + p1 g2, p1 p2) over the leaves of one candidate, most significant first"""
    G, Q = g[0], q[0]
    for gi, qi in zip(g[1:], q[1:]):
        G, Q = (G + Q * gi) % p, Q * qi % p
    return G


# ---- the model ------------------------------------------------------------------------------------------------------------------
def test_share_bits_model_is_int_arithmetic():
    rnd = random.Random(3)
    for p in (13, GOLDILOCKS, P64, BLS, P256):
        L = p.bit_length()
        for v in _edge_candidates(p) + [rnd.randrange(1 << L) for _ in range(50)]:
            bits = [(v >> i) & 1 for i in range(L)]
            assert offline.share_bits_model(bits, p) == (v, v < p)
        for bad in ([0] * (L - 1), [0] * (L + 1), [2] + [0] * (L - 1), [True] + [0] * (L - 1)):
            with pytest.raises(ValueError):
                offline.share_bits_model(bad, p)


def test_share_bits_candidates():
    """The bound m >= ceil(count / a) is evaluated with a = p / 2^L as Python evaluates it, a double: over 2^64 - 59 and 2^256 - 189 it is
    1.0, and m = count there.  (Evaluated on rationals, count / a exceeds count over every field, so no m could both equal count over
    2^64 - 59 and reach it.)  The rule itself is checked on exact integers: m is the smallest number whose mean m a lies four
    standard deviations above count - 1, the largest number of kept candidates that is too few.  Over the Goldilocks prime, where a
    is 1 - 2^-32 as a double too, that m is count itself, one below ceil(count / a)."""
    for p in (13, BLS, P256, P64):
        L = p.bit_length()
        a = p / 2 ** L
        last = 0
        for count in list(range(0, 70)) + [255, 256, 1000, 1 << 14, 1 << 16, 1 << 20]:
            m = offline.share_bits_candidates(p, count)
            assert isinstance(m, int) and m >= last and m >= count and m >= math.ceil(count / a), (p, count, m)      # monotone; enough on average
            assert m == offline.share_bits_candidates(p, count)                # no state, no floating point: every party gets this integer
            if count:                                                         # the smallest such m, on exact integers
                enough = lambda k: (k * p - (count - 1) * 2 ** L) > 0 and (k * p - (count - 1) * 2 ** L) ** 2 > 16 * k * p * (2 ** L - p)
                assert enough(m) and not enough(m - 1), (p, count, m)
            last = m
    assert offline.share_bits_candidates(BLS, 0) == 0
    for count in (1, 2, 3, 1000, 1 << 14, 1 << 20):
        assert offline.share_bits_candidates(P64, count) == count             # almost nothing is rejected
    assert offline.share_bits_candidates(GOLDILOCKS, 1000) == 1000
    # four standard deviations over BLS12-381: what a round of 2^14 can be expected to keep
    a = BLS / 2 ** 255
    m = offline.share_bits_candidates(BLS, 10000)
    assert abs(m * a - 4 * math.sqrt(m * a * (1 - a)) - 10000) < 1.0 and abs(a - 0.9057) < 1e-4
    for bad in (-1, 1.0, None, True):
        with pytest.raises(ValueError):
            offline.share_bits_candidates(BLS, bad)
    with pytest.raises(ValueError):
        offline.share_bits_candidates(2, 5)


# ---- the leaves -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p, nl", FIELDS, ids=FIELD_IDS)
def test_leaves_are_the_affine_maps(p, nl):
    """on random residues, not only bits: bound bit 0 -> (b, 1 - b), 1 -> (0, b); the default bound is p - 1"""
    L = p.bit_length()
    rnd = random.Random(p % 1009 + nl)
    for count in (1, 65):
        planes = [[(0, 1, p - 1)[(i + y) % 3] if (i + y) % 4 != 3 else rnd.randrange(p) for i in range(count)] for y in range(L)]
        for bound in (None, 0, (1 << L) - 1, rnd.randrange(1 << L)):
            c = p - 1 if bound is None else bound
            g, q = _leaves(p, nl, planes, bound)
            for y in range(L):
                bit = L - 1 - y
                if (c >> bit) & 1:
                    assert g[y] == [0] * count and q[y] == planes[bit], (count, bound, y)
                else:
                    assert g[y] == planes[bit] and q[y] == [(1 - b) % p for b in planes[bit]], (count, bound, y)


@pytest.mark.parametrize("p, nl", FIELDS, ids=FIELD_IDS)
def test_the_tree_over_the_leaves_is_the_verdict(p, nl):
    L = p.bit_length()
    cands = _edge_candidates(p)
    g, q = _leaves(p, nl, _planes(cands, L))
    roots = [_fold([g[y][i] for y in range(L)], [q[y][i] for y in range(L)], p) for i in range(len(cands))]
    assert roots == [int(v >= p) for v in cands]
    # p - 1 with one bit flipped: a 1 turned 0 is below p - 1 and kept, a 0 turned 1 is above and discarded
    for i in range(L):
        assert roots[8 + i] == (0 if ((p - 1) >> i) & 1 else 1), i
    assert [offline.share_bits_model([(v >> i) & 1 for i in range(L)], p)[1] for v in cands] == [not w for w in roots]
    # an explicit bound: [r > bound]
    bound = cands[2] if p > 13 else 5
    g, q = _leaves(p, nl, _planes(cands + [bound, bound + 1, bound - 1], L), bound)
    assert [_fold([g[y][i] for y in range(L)], [q[y][i] for y in range(L)], p) for i in range(len(cands) + 3)] == [int(v > bound) for v in cands + [bound, bound + 1, bound - 1]]


@pytest.mark.parametrize("nl", [4, 1])
def test_every_candidate_of_13(nl):
    p, L = 13, 4
    cands = list(range(16))
    g, q = _leaves(p, nl, _planes(cands, L))
    assert [_fold([g[y][i] for y in range(L)], [q[y][i] for y in range(L)], p) for i in cands] == [0] * 13 + [1] * 3
    index = np.array([v for v in cands if v < p], dtype=np.int64)
    r = np.zeros((13, nl), dtype=np.uint64)
    r_bits = np.zeros((L * 13, nl), dtype=np.uint64)
    assert _selftest(p, nl, FINISH, _limbs([b for plane in _planes(cands, L) for b in plane], p, nl), L, None, 16, index, r, r_bits, 13) == 0
    assert _ints(r, nl) == list(range(13)) and _ints(r_bits, nl) == [b for plane in _planes(range(13), L) for b in plane]


# ---- the finish -------------------------------------------------------------------------------------------------------------------
def _finish(p, nl, planes, index):
    """the host row over planes [L][candidates] -> (r [k], r_bits [L][k]) as ints; sentinels behind both outputs stay"""
    L, cands, k = len(planes), len(planes[0]), len(index)
    flat = _limbs([v for plane in planes for v in plane], p, nl)
    idx = np.array(list(index) or [0], dtype=np.int64)
    r = np.full((k + 1, nl), SENTINEL, dtype=np.uint64)
    r_bits = np.full((L * k + 1, nl), SENTINEL, dtype=np.uint64)
    before, idx_before = flat.copy(), idx.copy()
    assert _selftest(p, nl, FINISH, flat, L, None, cands, idx, r, r_bits, k) == 0
    assert np.array_equal(flat, before) and np.array_equal(idx, idx_before)
    assert (r[k:] == SENTINEL).all() and (r_bits[L * k:] == SENTINEL).all()
    rb = _ints(r_bits[:L * k], nl) if k else []
    return (_ints(r[:k], nl) if k else []), [rb[q * k:(q + 1) * k] for q in range(L)]


@pytest.mark.parametrize("p, nl", FIELDS, ids=FIELD_IDS)
def test_finish_gathers_the_planes_and_composes_r(p, nl):
    L = p.bit_length()
    rnd = random.Random(p % 1013 + nl)
    cands = _edge_candidates(p)[:8] + [rnd.randrange(1 << L) for _ in range(5)]
    n = len(cands)
    bit_planes = _planes(cands, L)
    share_planes = [[rnd.randrange(p) for _ in range(n)] for _ in range(L)]          # a party's planes hold shares: any residues
    lists = {"empty": [], "single": [n - 1], "all": list(range(n)), "reversed": list(range(n))[::-1], "repeated": [3, 3, 0, 3, n - 1, 0],
             "out of range": [2, -1, n, 0, 1 << 40, -(1 << 63), (1 << 63) - 1, n - 1]}
    for name, index in lists.items():
        inside = [0 <= c < n for c in index]
        r, r_bits = _finish(p, nl, bit_planes, index)
        assert r == [offline.share_bits_model([bit_planes[q][c] for q in range(L)], p)[0] % p if ok else 0 for c, ok in zip(index, inside)], name
        assert r_bits == [[bit_planes[q][c] if ok else 0 for c, ok in zip(index, inside)] for q in range(L)], name
        r, r_bits = _finish(p, nl, share_planes, index)
        assert r == [sum(share_planes[q][c] << q for q in range(L)) % p if ok else 0 for c, ok in zip(index, inside)], name
        assert r_bits == [[share_planes[q][c] if ok else 0 for c, ok in zip(index, inside)] for q in range(L)], name


# ---- what is refused ----------------------------------------------------------------------------------------------------------------
def test_selftest_refuses_bad_arguments():
    p, nl, L, count = BLS, 4, 255, 5
    bits = _limbs([1] * (L * count), p, nl)
    g, q = np.zeros((L * count, nl), dtype=np.uint64), np.zeros((L * count, nl), dtype=np.uint64)
    index = np.arange(count, dtype=np.int64)
    r = np.zeros((count, nl), dtype=np.uint64)
    leaves = lambda **kw: _selftest(**{**dict(p=p, nl=nl, what=LEAVES, bits=bits, L=L, bound=None, candidates=0, index=None, out0=g, out1=q, count=count), **kw})
    finish = lambda **kw: _selftest(**{**dict(p=p, nl=nl, what=FINISH, bits=bits, L=L, bound=None, candidates=count, index=index, out0=r, out1=g, count=count), **kw})
    assert leaves() == 0 and finish() == 0
    assert leaves(what=2) == 2 and leaves(what=-1) == 2 and leaves(modulus=False) == 2 and finish(modulus=False) == 2
    assert _lib().hb_selftest_off_share_bits(_raw(p, nl).ctypes.data, 2, LEAVES, bits.ctypes.data, L, None, 0, None, g.ctypes.data, q.ctypes.data, count) == 2
    for bad_L in (254, 256, 0, -1, 64):
        assert leaves(L=bad_L) == 2 and finish(L=bad_L) == 2, bad_L
    assert leaves(count=-1) == 2 and finish(count=-1) == 2 and finish(candidates=-1) == 2
    assert leaves(bits=None) == 2 and leaves(out0=None) == 2 and leaves(out1=None) == 2
    assert finish(bits=None) == 2 and finish(index=None) == 2 and finish(out0=None) == 2 and finish(out1=None) == 2
    # the bound: below 2^L
    assert leaves(bound=_raw((1 << 255) - 1, nl)) == 0 and leaves(bound=_raw(1 << 255, nl)) == 2 and leaves(bound=_raw(1 << 255, nl), count=0) == 2
    assert _selftest(13, 1, LEAVES, _limbs([1] * 4, 13, 1), 4, _raw(16, 1), 0, None, np.zeros((4, 1), np.uint64), np.zeros((4, 1), np.uint64), 1) == 2
    assert _selftest(13, 1, LEAVES, _limbs([1] * 4, 13, 1), 4, _raw(15, 1), 0, None, np.zeros((4, 1), np.uint64), np.zeros((4, 1), np.uint64), 1) == 0
    # outputs are arrays of their own
    assert leaves(out0=bits) == 2 and leaves(out1=bits) == 2 and leaves(out1=g) == 2 and leaves(out1=g[L * count - 1:]) == 2
    assert finish(out0=bits) == 2 and finish(out1=bits) == 2 and finish(out0=g[:count]) == 2 and finish(out0=index.view(np.uint64)) == 2
    assert finish(out1=bits[count * L - 1:]) == 2
    # nothing to do: nothing is read
    assert _selftest(p, nl, LEAVES, None, L, None, 0, None, None, None, 0) == 0 and _selftest(p, nl, FINISH, None, L, None, 0, None, None, None, 0) == 0
    # no candidates at all: every index is outside, every slot zero, bits is not read
    r[:] = 7
    g[:] = 7
    assert finish(bits=None, candidates=0) == 0 and not r.any() and not g[:L * count].any()


def test_protocol_arguments_are_checked_before_the_device():
    class Co:
        ctx, myid, n, t = None, 0, 4, 1

    for bad in (0, -1, 1.0, None, True):
        with pytest.raises(ValueError):
            asyncio.run(offline.generate_share_bits(Co(), bad))
        with pytest.raises(ValueError):
            asyncio.run(offline.generate_share_bits(Co(), 3, chunk=bad))
        with pytest.raises(ValueError):
            asyncio.run(offline.generate_less_than_preprocessing(Co(), bad))
    for mode in (2, -1, None, True):
        with pytest.raises(ValueError):
            asyncio.run(offline.generate_less_than_preprocessing(Co(), 3, mode=mode))


def test_entry_points_are_declared_and_bound():
    from honeybadgermpc_amd import _capi

    text = open(os.path.join(REPO, "include", "hbmpc_hip.h")).read()
    for name in ("hb_off_sb_leaves", "hb_off_sb_finish", "hb_selftest_off_share_bits"):
        assert re.search(r"\bint " + name + r"\s*\(", text) and name in _capi.SYMBOLS
    for name, value in (("HB_OFF_SB_SELFTEST_LEAVES", 0), ("HB_OFF_SB_SELFTEST_FINISH", 1)):
        assert re.search(rf"#define {name} {value}\b", text) and getattr(_capi, name) == value
    for name in ("share_bits_model", "share_bits_candidates", "sb_leaves", "sb_finish", "share_bits_round", "generate_share_bits", "generate_less_than_preprocessing"):
        assert callable(getattr(offline, name))
    assert offline.LessThanPreprocessing._fields == ("r", "r_bits", "triples", "s", "s_bits")

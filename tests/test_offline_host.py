"""CPU-only: the offline phase's kernels (csrc/hb_off.hip) run on the host through hb_selftest_off -- the same HB_HD functions the
kernels call -- against Python ints: a b + c with its aliasings, the fused inverse square root in its three modes against
offline.invsqrt_model, against w^2 x = 1 and against the inverse of the root the Tonelli-Shanks loop of csrc/hb_sqrt.hip gives (restated
here), with zeros and non-residues counted, and the checkers' degree verdict on crafted columns against offline.degree_check_model and
against what the columns were crafted to be.  Exact equality."""
import asyncio
import ctypes
import os
import random
import re

import numpy as np
import pytest

from conftest import BLS, REPO
from selftest_cases import run_off as _call
from selftest_cases import run_off_mul_add as mul_add

from honeybadgermpc_amd import offline

GOLDILOCKS = 0xFFFFFFFF00000001
P64 = (1 << 64) - 59
P256 = (1 << 256) - 189
FIELDS = [(BLS, 4), (P256, 4), (P64, 1), (GOLDILOCKS, 1), (13, 4), (13, 1)]
FIELD_IDS = ["bls", "2^256-189", "2^64-59", "goldilocks", "13-wide", "13-narrow"]
COUNTS = (0, 1, 63, 64, 65, 300)
MUL_ADD, INVSQRT, DEGREE_CHECK = range(3)


def _lib():
    from honeybadgermpc_amd._capi import load_library

    return load_library()


def _limbs(values, p, nl):
    from honeybadgermpc_amd._capi import ints_to_limbs

    return ints_to_limbs(list(values) or [0], p, 8 * nl)


def _ints(arr, nl, count):
    from honeybadgermpc_amd._capi import limbs_to_ints

    return limbs_to_ints(arr[:count], 8 * nl) if count else []


def invsqrt(p, nl, x, u, mode):
    """-> (rc, out, [zeros, non-residues])"""
    count = len(x)
    xa = _limbs(x, p, nl)
    ua = None if u is None else _limbs(u, p, nl)
    status = np.full(2, 77, dtype=np.uint64)
    out = np.full((max(count, 1), nl), 5, dtype=np.uint64)
    rc = _call(p, nl, INVSQRT | (mode << 8), [xa.ctypes.data, None if ua is None else ua.ctypes.data, status.ctypes.data], out.ctypes.data, count)
    return rc, _ints(out, nl, count), [int(v) for v in status]


def degree_check(p, nl, coeffs, n, k, t):
    ca = _limbs(coeffs, p, nl)
    prm = np.array([n, t], dtype=np.uint64)
    out = np.full(3, 99, dtype=np.uint64)
    rc = _call(p, nl, DEGREE_CHECK, [ca.ctypes.data, prm.ctypes.data], out.ctypes.data, k)
    return rc, [int(v) for v in out]


def ts_root(a, p):
    """the loop of csrc/hb_sqrt.hip (k_sqrt) on Python ints: the root for the smallest non-residue z >= 2; None for a non-residue"""
    if a == 0:
        return 0
    if pow(a, (p - 1) // 2, p) != 1:
        return None
    q, s, c = offline._tonelli_constants(p)
    r, t, m = pow(a, (q + 1) // 2, p), pow(a, q, p), s
    while t != 1:
        k, tt = 0, t
        while tt != 1:
            tt, k = tt * tt % p, k + 1
        b = pow(c, 1 << (m - k - 1), p)
        r, c = r * b % p, b * b % p
        t, m = t * c % p, k
    return r


# ---- a b + c ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p, nl", FIELDS, ids=FIELD_IDS)
def test_mul_add_against_python_ints(p, nl):
    rnd = random.Random(p % 1009 + nl)
    corners = [(x, y, z) for x in (0, 1, p - 1) for y in (0, 1, p - 1) for z in (0, 1, p - 1)]
    for count in COUNTS:
        rows = (corners + [(rnd.randrange(p), rnd.randrange(p), rnd.randrange(p)) for _ in range(count)])[:count]
        a, b, c = ([r[i] for r in rows] for i in range(3))
        want = [(x * y + z) % p for x, y, z in rows]
        assert mul_add(p, nl, a, b, c) == (0, want), count
        assert mul_add(p, nl, a, b, c, b_is_a=True) == (0, [(x * x + z) % p for x, z in zip(a, c)]), count
        for alias in range(3):
            assert mul_add(p, nl, a, b, c, out_is=alias) == (0, want), (count, alias)
        assert mul_add(p, nl, a, b, c, b_is_a=True, out_is=0) == (0, [(x * x + z) % p for x, z in zip(a, c)]), count


# ---- the inverse square root ----------------------------------------------------------------------------------------------------
def test_model_is_the_inverse_of_the_tonelli_shanks_root():
    """on every element of small fields, and where p - 1 has a large power of two: the model's w is 1 / ts_root(x)"""
    for p in (13, 17, 53, 97, 257, 7681):
        for x in range(p):
            w, status = offline.invsqrt_model(x, p)
            r = ts_root(x, p)
            assert status == (1 if x == 0 else (2 if r is None else 0))
            assert w == (0 if status else pow(r, -1, p)) and (status or w * w * x % p == 1)
    rnd = random.Random(3)
    for p in (BLS, GOLDILOCKS, P64, P256, (1 << 255) - 19):
        for _ in range(40):
            x = rnd.randrange(1, p)
            w, status = offline.invsqrt_model(x, p)
            r = ts_root(x, p)
            assert (status, w) == ((2, 0) if r is None else (0, pow(r, -1, p)))


def _invsqrt_inputs(p, count, rnd):
    """squares of corner and random values, every 2-power order of x^q where s is large, and zeros and non-residues at the first, the last
    and the wave-edge positions"""
    q, s, g = offline._tonelli_constants(p)                      # g = z^q generates the 2-Sylow subgroup
    nonres = [v for v in range(2, 200) if pow(v, (p - 1) // 2, p) == p - 1][:4] or [2]
    xs = [v * v % p for v in (1, p - 1, 2, p - 2, (p - 1) // 2, (p + 1) // 2)]
    if s >= 8:
        xs += [pow(g, 1 << j, p) for j in range(1, s + 1)]       # x^q of order 2^(s-j): every length of the correction
        xs += [pow(g, 1 << j, p) * pow(rnd.randrange(2, p), 2 << s, p) % p for j in range(1, s)]       # ... times an odd-order square
    xs += [pow(rnd.randrange(1, p), 2, p) for _ in range(count)]
    xs = xs[:count]
    for pos, v in ((0, 0), (64, 0), (62, 0), (count - 1, nonres[0]), (63, nonres[-1]), (65, nonres[1 % len(nonres)])):
        if 0 <= pos < count and (count > 2 or pos == 0):
            xs[pos] = v % p
    return xs


@pytest.mark.parametrize("p, nl", FIELDS, ids=FIELD_IDS)
def test_invsqrt_scale_against_the_model(p, nl):
    rnd = random.Random(p % 1013 + nl)
    half = (p + 1) // 2
    for count in COUNTS:
        for trial in range(2 if count in (1, 300) else 1):
            x = _invsqrt_inputs(p, count, rnd) if trial == 0 else [pow(rnd.randrange(1, p), 2, p) for _ in range(count)]
            u = [rnd.choice((0, 1, p - 1, rnd.randrange(p))) for _ in range(count)]
            model = [offline.invsqrt_model(v, p) for v in x]
            want_status = [sum(st == 1 for _, st in model), sum(st == 2 for _, st in model)]
            if trial == 0 and count >= 63:
                assert want_status[0] >= 1 and want_status[1] >= 1
            rc, w, status = invsqrt(p, nl, x, None, 0)
            assert rc == 0 and status == want_status and w == [m[0] for m in model], count
            for v, got, (_, st) in zip(x, w, model):
                root = ts_root(v, p)
                if st:
                    assert got == 0 and (v == 0 or root is None)
                else:
                    assert got * got * v % p == 1 and got * root % p == 1, v
            rc, pm1, status = invsqrt(p, nl, x, u, offline.PM1)
            assert rc == 0 and status == want_status and pm1 == [0 if st else a * m % p for a, (m, st) in zip(u, model)], count
            rc, b01, status = invsqrt(p, nl, x, u, offline.ZERO_ONE)
            assert rc == 0 and status == want_status and b01 == [0 if st else (a * m + 1) * half % p for a, (m, st) in zip(u, model)], count


@pytest.mark.parametrize("p, nl", [(BLS, 4), (GOLDILOCKS, 1)], ids=["bls", "goldilocks"])
def test_invsqrt_every_loop_length_makes_bits(p, nl):
    """u a root of x = g^(2^j) up to sign: u w is +-1 and (u w + 1) / 2 is 0 or 1, for x^q of every 2-power order from 2^(s-1) down to 1"""
    q, s, g = offline._tonelli_constants(p)
    assert s == 32
    x = [pow(g, 1 << j, p) for j in range(1, s + 1)]
    assert sorted({next(k for k in range(s + 1) if pow(pow(v, q, p), 1 << k, p) == 1) for v in x}) == list(range(s))
    roots = [ts_root(v, p) for v in x]
    u = [r if i % 2 else p - r for i, r in enumerate(roots)]
    rc, pm1, status = invsqrt(p, nl, x, u, offline.PM1)
    assert rc == 0 and status == [0, 0] and pm1 == [1 if i % 2 else p - 1 for i in range(s)]
    rc, b01, status = invsqrt(p, nl, x, u, offline.ZERO_ONE)
    assert rc == 0 and status == [0, 0] and b01 == [i % 2 for i in range(s)]


# ---- the checkers' verdict --------------------------------------------------------------------------------------------------------
KINDS = ("exact", "lead_zero", "stray_top", "only_top", "stray_next", "const_top_limb", "zero")


def crafted_block(p, n, k, t, rnd):
    """[n][2k] coefficients, column j of kind KINDS[j % 7] -> (flat list, kinds).  2t < n - 1 at the shapes used, so a stray top
    coefficient spoils both sharings."""
    assert 2 * t < n - 1
    L = p.bit_length()
    cols = [[0] * n for _ in range(2 * k)]
    kinds = [KINDS[j % len(KINDS)] for j in range(k)]
    for j, kind in enumerate(kinds):
        secret = rnd.randrange(1 << (L - 3))
        for col, deg in ((j, t), (k + j, 2 * t)):
            poly = [secret] + [rnd.randrange(p) for _ in range(deg - 1)] + [rnd.randrange(1, p)] + [0] * (n - 1 - deg)
            if kind == "lead_zero":
                poly[deg] = 0
            elif kind == "stray_top":
                poly[n - 1] = 1
            elif kind == "only_top":
                poly = [0] * (n - 1) + [rnd.randrange(1, p)]
            elif kind == "stray_next":
                poly[deg + 1] = p - 1
            elif kind == "zero":
                poly = [0] * n
            cols[col] = poly
        if kind == "const_top_limb":
            cols[k + j][0] = secret + (1 << (L - 2))              # below p, and equal to the other constant in every limb but the top one
    return [cols[c][e] for e in range(n) for c in range(2 * k)], kinds


@pytest.mark.parametrize("p, nl", [(BLS, 4), (P256, 4), (P64, 1), (GOLDILOCKS, 1), (13, 4)], ids=["bls", "2^256-189", "2^64-59", "goldilocks", "13"])
@pytest.mark.parametrize("n, t", [(4, 1), (7, 2), (16, 5)])
def test_degree_check_on_crafted_columns(p, nl, n, t):
    rnd = random.Random(n * 31 + p % 1019)
    for k in (1, 64, 65):
        coeffs, kinds = crafted_block(p, n, k, t, rnd)
        bad_degree = sum(kind in ("lead_zero", "stray_top", "only_top", "stray_next", "zero") for kind in kinds)
        want = [bad_degree, bad_degree, sum(kind == "const_top_limb" for kind in kinds)]      # "only_top", "zero": both constants are 0
        assert offline.degree_check_model(coeffs, n, k, t) == want, k
        assert degree_check(p, nl, coeffs, n, k, t) == (0, want), k
    # one sharing alone at fault: the t-sharing's stray coefficient sits at 2t, where the other's leading one is
    coeffs, _ = crafted_block(p, n, 1, t, rnd)
    coeffs[2 * t * 2] = 5
    assert offline.degree_check_model(coeffs, n, 1, t) == [1, 0, 0] and degree_check(p, nl, coeffs, n, 1, t) == (0, [1, 0, 0])
    # nothing to check, and what is refused
    assert degree_check(p, nl, [], n, 0, t) == (0, [0, 0, 0])
    assert degree_check(p, nl, [0] * (2 * n), n, 1, n)[0] == 2 and degree_check(p, nl, [0] * (2 * n), n, 1, (n + 1) // 2)[0] == 2


def test_selftest_refuses_bad_arguments():
    p, nl = BLS, 4
    one = _limbs([1], p, nl)
    out = np.zeros((1, nl), dtype=np.uint64)
    assert _call(p, nl, 3, [one.ctypes.data] * 3, out.ctypes.data, 1) == 2                       # unknown selector
    assert _call(p, nl, INVSQRT | (2 << 8), [one.ctypes.data, None, None], out.ctypes.data, 1) == 2      # unknown mode
    assert _call(p, nl, MUL_ADD | (1 << 8), [one.ctypes.data] * 3, out.ctypes.data, 1) == 2      # a mode where none belongs
    assert _call(p, nl, MUL_ADD, [one.ctypes.data, None, one.ctypes.data], out.ctypes.data, 1) == 2
    assert _call(p, nl, MUL_ADD, [one.ctypes.data] * 3, None, 1) == 2 and _call(p, nl, MUL_ADD, [one.ctypes.data] * 3, out.ctypes.data, -1) == 2
    assert _call(p, nl, INVSQRT, [None, None, None], out.ctypes.data, 1) == 2
    ops = (ctypes.c_void_p * 3)(*[one.ctypes.data] * 3)
    assert _lib().hb_selftest_off(_limbs([p], p + 1, nl).ctypes.data, 2, MUL_ADD, ops, out.ctypes.data, 1) == 2      # neither width
    assert _lib().hb_selftest_off(None, nl, MUL_ADD, ops, out.ctypes.data, 1) == 2
    assert _call(p, nl, MUL_ADD, [None, None, None], None, 0) == 0


def test_protocol_arguments_are_checked_before_the_device():
    class Co:
        ctx, myid = None, 0

        def __init__(self, n, t):
            self.n, self.t = n, t

    for n, t, k in ((4, 0, 1), (3, 1, 1), (6, 2, 1), (4, 1, 0), (4, 1, -1), (4, 1, 1.0)):
        with pytest.raises(ValueError):
            asyncio.run(offline.randousha(Co(n, t), k))
    for k in (0, -3, None):
        with pytest.raises(ValueError):
            asyncio.run(offline.generate_triples(Co(4, 1), k))
        with pytest.raises(ValueError):
            asyncio.run(offline.generate_bits(Co(4, 1), k))
    for enc in (2, -1, None, True):
        with pytest.raises(ValueError):
            asyncio.run(offline.generate_bits(Co(4, 1), 1, encoding=enc))


def test_entry_points_are_declared_and_bound():
    from honeybadgermpc_amd import _capi

    text = open(os.path.join(REPO, "include", "hbmpc_hip.h")).read()
    for name in ("hb_off_mul_add", "hb_off_invsqrt_scale", "hb_off_degree_check", "hb_selftest_off"):
        assert re.search(r"\bint " + name + r"\s*\(", text) and name in _capi.SYMBOLS
    for name, value in (("HB_OFF_PM1", 0), ("HB_OFF_01", 1), ("HB_OFF_SELFTEST_MUL_ADD", 0), ("HB_OFF_SELFTEST_INVSQRT", 1), ("HB_OFF_SELFTEST_DEGREE_CHECK", 2)):
        assert re.search(rf"#define {name} {value}\b", text) and getattr(_capi, name) == value
    assert (offline.PM1, offline.ZERO_ONE) == (_capi.HB_OFF_PM1, _capi.HB_OFF_01)
    for name in ("mul_add", "invsqrt_scale", "degree_check", "invsqrt_model", "degree_check_model", "randousha", "generate_triples", "generate_bits"):
        assert callable(getattr(offline, name))

"""CPU-only: the shared powers and cubes of the offline phase.  The doubling levels (offline.power_levels) and their model on Python ints;
the two rows of csrc/hb_offpow.hip run on the host through hb_selftest_off_powers -- the same functions and the same index arithmetic the
kernels run -- against Python ints in both layouts, with a sentinel in every cell a level must not touch; the whole chain among n parties
on dealt sharings, opened by interpolation on ints; what is refused; and the protocol's argument checks.  Exact equality."""
import asyncio
import os
import random
import re

import numpy as np
import pytest

from conftest import BLS, REPO
from offline_support import _check_sharings, _coefficients, _deal

from honeybadgermpc_amd import offline

GOLDILOCKS = 0xFFFFFFFF00000001
P64 = (1 << 64) - 59
P256 = (1 << 256) - 189
FIELDS = [(BLS, 4), (P256, 4), (P64, 1), (GOLDILOCKS, 1), (13, 4), (13, 1)]
FIELD_IDS = ["bls", "2^256-189", "2^64-59", "goldilocks", "13-wide", "13-narrow"]
COUNTS = (0, 1, 63, 64, 65, 300)
KS = (2, 3, 5, 8, 9)
LAYOUTS = ("item", "power")
MASK, FINISH = 0, 1
SENTINEL = 0xA5A5A5A5A5A5A5A5                   # in every limb of a cell that holds no power yet (no vector here takes that value)


def _lib():
    from honeybadgermpc_amd._capi import load_library

    return load_library()


def _limbs(values, p, nl):
    from honeybadgermpc_amd._capi import ints_to_limbs

    return ints_to_limbs(list(values) or [0], p, 8 * nl)


def _ints(arr, nl):
    from honeybadgermpc_amd._capi import limbs_to_ints

    return limbs_to_ints(np.ascontiguousarray(arr).reshape(-1, nl), 8 * nl)


def _modulus(p, nl):
    from honeybadgermpc_amd._capi import ints_to_limbs

    return ints_to_limbs([p], p + 1, 8 * nl)


def _strides(layout, count, k):
    return (k, 1) if layout == "item" else (1, count)


def _selftest(p, nl, what, powers, strides, x, r, m, w, out, count, modulus=True):
    ptr = lambda a: None if a is None else a.ctypes.data
    mod = _modulus(p, nl)
    return _lib().hb_selftest_off_powers(ptr(mod) if modulus else None, nl, what, ptr(powers), strides[0], strides[1], ptr(x), ptr(r), m, w, ptr(out), count)


class Powers:
    """the powers array of `count` items in one layout as host limbs, with cell access by (item, 0-based power)"""

    def __init__(self, p, nl, count, k, layout):
        self.p, self.nl, self.count, self.k, self.layout = p, nl, count, k, layout
        shape = (max(count, 1), k, nl) if layout == "item" else (k, max(count, 1), nl)
        self.a = np.full(shape, SENTINEL, dtype=np.uint64)
        self.strides = _strides(layout, max(count, 1) if layout == "power" else count, k)

    def column(self, q):
        return self.a[:, q] if self.layout == "item" else self.a[q]

    def set_column(self, q, values):
        if self.count:
            self.column(q)[:self.count] = _limbs(values, self.p, self.nl)

    def get_column(self, q):
        return _ints(self.column(q)[:self.count], self.nl) if self.count else []


def _values(p, count, rnd, salt):
    """count residues: 0, 1 and p - 1 in rotating places, the rest random"""
    corners = (0, 1, p - 1)
    return [corners[(i + salt) % 3] if (i + salt) % 4 != 3 else rnd.randrange(p) for i in range(count)]


# ---- the levels -----------------------------------------------------------------------------------------------------------------
def test_power_levels_make_every_exponent_once():
    for k in list(range(1, 71)) + [255, 256, 257, 1024]:
        levels = offline.power_levels(k)
        have, made = {1}, []
        for m, w in levels:
            assert 1 <= w <= m and m in have
            for j in range(w):
                assert j + 1 in have                                       # both factors exist when the level runs
            new = [m + 1 + j for j in range(w)]
            made += new
            have |= set(new)
        assert made == list(range(2, k + 1)), k                          # each exactly once, in increasing order
        assert len(levels) == (k - 1).bit_length() and sum(w for _, w in levels) == k - 1, k      # (k - 1).bit_length() = ceil(log2 k)
    assert offline.power_levels(1) == [] and offline.power_levels(3) == [(1, 1), (2, 1)]
    assert offline.power_levels(9) == [(1, 1), (2, 2), (4, 4), (8, 1)]
    for bad in (0, -1, 1.0, None, True):
        with pytest.raises(ValueError):
            offline.power_levels(bad)


def test_powers_model_is_pow():
    rnd = random.Random(5)
    for p in (13, P64, BLS, P256):
        for b in (0, 1, p - 1, rnd.randrange(p), rnd.randrange(p) + p):
            for k in (1, 2, 3, 5, 8, 9, 33, 70):
                assert offline.powers_model(b, k, p) == [pow(b, e, p) for e in range(1, k + 1)]


# ---- the two rows against Python ints ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("p, nl", FIELDS, ids=FIELD_IDS)
def test_mask_and_finish_against_python_ints(p, nl, layout):
    rnd = random.Random(p % 1009 + nl + len(layout))
    for count in COUNTS:
        for k in KS:
            for m, w in offline.power_levels(k):
                P = Powers(p, nl, count, k, layout)
                cols = [_values(p, count, rnd, q) for q in range(m)]
                for q in range(m):
                    P.set_column(q, cols[q])
                before = P.a.copy()
                total = count * w
                # mask: out[c w + j] = P[c][m] P[c][j+1] + r2t[c w + j]; the powers are only read
                r2t = _values(p, total, rnd, 1)
                r2t_a = _limbs(r2t, p, nl)
                out = np.full((max(total, 1), nl), SENTINEL, dtype=np.uint64)
                assert _selftest(p, nl, MASK, P.a, P.strides, None, r2t_a, m, w, out, count) == 0, (count, k, m, w)
                want = [(cols[m - 1][c] * cols[j][c] + r2t[c * w + j]) % p for c in range(count) for j in range(w)]
                assert _ints(out[:total], nl) == want if total else True, (count, k, m, w)
                assert np.array_equal(P.a, before) and (out[total:] == SENTINEL).all()
                # finish: P[c][m+1+j] = opened[c w + j] - rt[c w + j]; columns m .. m+w-1 alone change
                opened, rt = _values(p, total, rnd, 2), _values(p, total, rnd, 0)
                if total > 3:
                    opened[3], rt[3] = rt[3], rt[3]                        # a difference of zero
                assert _selftest(p, nl, FINISH, P.a, P.strides, _limbs(opened, p, nl), _limbs(rt, p, nl), m, w, None, count) == 0
                for q in range(k):
                    if m <= q < m + w:
                        assert P.get_column(q) == [(opened[c * w + q - m] - rt[c * w + q - m]) % p for c in range(count)], (count, k, m, w, q)
                        if count:
                            assert (P.column(q)[:count] != before_col(before, layout, q)[:count]).any()
                    else:
                        assert np.array_equal(P.column(q), before_col(before, layout, q)), (count, k, m, w, q)


def before_col(a, layout, q):
    return a[:, q] if layout == "item" else a[q]


# ---- the chain among n parties, on ints -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n, t", [(4, 1), (7, 2)])
@pytest.mark.parametrize("k", [2, 3, 5, 9])
def test_the_chain_makes_sharings_of_the_powers(n, t, k, layout):
    p, nl, count = BLS, 4, 3
    rnd = random.Random(100 * n + k)
    b = [0, p - 1, rnd.randrange(2, p)] if k == 5 else [rnd.randrange(p) for _ in range(count)]
    parties = [Powers(p, nl, count, k, layout) for _ in range(n)]
    shares_b = [_deal(v, t, n, p, rnd) for v in b]                             # [item][party]
    for i, P in enumerate(parties):
        P.set_column(0, [shares_b[c][i] for c in range(count)])
    for m, w in offline.power_levels(k):
        total = count * w
        secrets = [rnd.randrange(p) for _ in range(total)]
        r_t = [_deal(s, t, n, p, rnd) for s in secrets]                        # [element][party]
        r_2t = [_deal(s, 2 * t, n, p, rnd) for s in secrets]
        masked = []
        for i, P in enumerate(parties):
            out = np.zeros((total, nl), dtype=np.uint64)
            assert _selftest(p, nl, MASK, P.a, P.strides, None, _limbs([r[i] for r in r_2t], p, nl), m, w, out, count) == 0
            masked.append(_ints(out, nl))
        opened = []
        for e in range(total):                                                 # the open at degree 2t
            coeffs = _coefficients([masked[i][e] for i in range(n)], p)
            assert not any(coeffs[2 * t + 1:])
            opened.append(coeffs[0])
        assert opened == [(pow(b[e // w], m, p) * pow(b[e // w], e % w + 1, p) + secrets[e]) % p for e in range(total)]
        for i, P in enumerate(parties):
            assert _selftest(p, nl, FINISH, P.a, P.strides, _limbs(opened, p, nl), _limbs([r[i] for r in r_t], p, nl), m, w, None, count) == 0
    for e in range(k):
        constants = _check_sharings(p, n, t, [P.get_column(e) for P in parties])
        assert constants == [pow(v, e + 1, p) for v in b], e
    assert [offline.powers_model(v, k, p) for v in b] == [[pow(v, e + 1, p) for e in range(k)] for v in b]


# ---- what is refused ----------------------------------------------------------------------------------------------------------------
def test_selftest_refuses_bad_arguments():
    p, nl, count, k = BLS, 4, 5, 4
    P = Powers(p, nl, count, k, "item")
    for q in range(2):
        P.set_column(q, [q + 2] * count)
    r = _limbs([1] * (2 * count), p, nl)
    x = _limbs([2] * (2 * count), p, nl)
    out = np.zeros((2 * count, nl), dtype=np.uint64)
    ok = lambda **kw: _selftest(**{**dict(p=p, nl=nl, what=MASK, powers=P.a, strides=(k, 1), x=None, r=r, m=2, w=2, out=out, count=count), **kw})
    assert ok() == 0 and ok(what=FINISH, x=x, out=None) == 0
    assert ok(what=2) == 2 and ok(what=-1) == 2                                # unknown selector
    assert _lib().hb_selftest_off_powers(_modulus(p, nl).ctypes.data, 2, MASK, P.a.ctypes.data, k, 1, None, r.ctypes.data, 2, 2, out.ctypes.data, count) == 2
    assert ok(modulus=False) == 2                                              # null modulus
    assert ok(m=1, w=2) == 2 and ok(m=0, w=0) == 2 and ok(m=2, w=0) == 2       # w > m, m < 1, w < 1
    assert ok(count=-1) == 2
    # strides under which two cells of the count x (m + w) block are one element
    for strides in ((3, 1), (1, 1), (1, 4), (2, 2), (6, 4), (0, 1), (4, 0), (-4, 1), (4, -1)):
        assert ok(strides=strides) == 2, strides
    assert ok(strides=(1, 5)) == 0 and ok(strides=(5, 3), m=1, w=1, count=3) == 0       # 0 3 | 5 8 | 10 13: apart, though the rows interleave
    # null operands where there is work
    assert ok(powers=None) == 2 and ok(r=None) == 2 and ok(out=None) == 2
    assert ok(what=FINISH, x=None, out=None) == 2 and ok(what=FINISH, x=x, r=None, out=None) == 2
    # nothing to do: nothing is read
    assert _selftest(p, nl, MASK, None, (k, 1), None, None, 2, 2, None, 0) == 0 and _selftest(p, nl, FINISH, None, (k, 1), None, None, 2, 2, None, 0) == 0
    # the masked output over the powers or over its mask; the finish's inputs over the columns it writes
    flat = P.a.reshape(-1, nl)
    assert ok(out=flat) == 2 and ok(out=r) == 2 and ok(out=flat[count * k - 1:]) == 2
    assert ok(what=FINISH, x=flat[2:], out=None) == 2 and ok(what=FINISH, x=x, r=flat[2:], out=None) == 2
    assert ok(what=FINISH, x=flat[:2], m=2, w=2, count=1, out=None) == 0        # columns 0 and 1 are not written


def test_protocol_arguments_are_checked_before_the_device():
    class Co:
        ctx, myid, n, t = None, 0, 4, 1

    for bad in (0, -1, 1.0, None, True):
        with pytest.raises(ValueError):
            asyncio.run(offline.generate_powers(Co(), bad, 3))
        with pytest.raises(ValueError):
            asyncio.run(offline.generate_powers(Co(), 3, bad))
        with pytest.raises(ValueError):
            asyncio.run(offline.generate_cubes(Co(), bad, 3))
        with pytest.raises(ValueError):
            asyncio.run(offline.generate_cubes(Co(), 3, bad))
    for layout in ("items", "", None, 0):
        with pytest.raises(ValueError):
            asyncio.run(offline.generate_powers(Co(), 3, 3, layout=layout))


def test_entry_points_are_declared_and_bound():
    from honeybadgermpc_amd import _capi

    text = open(os.path.join(REPO, "include", "hbmpc_hip.h")).read()
    for name in ("hb_off_pow_mask", "hb_off_pow_finish", "hb_selftest_off_powers"):
        assert re.search(r"\bint " + name + r"\s*\(", text) and name in _capi.SYMBOLS
    for name, value in (("HB_OFF_POWERS_SELFTEST_MASK", 0), ("HB_OFF_POWERS_SELFTEST_FINISH", 1)):
        assert re.search(rf"#define {name} {value}\b", text) and getattr(_capi, name) == value
    for name in ("generate_powers", "generate_cubes", "power_levels", "powers_model", "pow_mask", "pow_finish"):
        assert callable(getattr(offline, name))

"""CPU-only: honeybadgermpc_amd.progs.fixedpoint_log -- log_model against an integer enclosure of the logarithm within the DERIVED bound
(every operand at the small shapes, the worst-case r1), the coefficients against an independent recomputation, the counts against their
formulas, the steps of csrc/hb_fxlog.hip through hb_selftest_fxlog (the rows the device runs, behind the step functions the entry
points run) against Python ints, and what the steps refuse."""
import random
from fractions import Fraction
from math import isqrt

import pytest

import bitdec_cases as bc
import log_cases as lc
from conftest import BLS
from log_cases import DEGREES, E, FINISH, FIRST, LEVEL, POLY_MASK, ok, run_log

from honeybadgermpc_amd.progs import bit_decomposition as bd
from honeybadgermpc_amd.progs import fixedpoint_division as fd
from honeybadgermpc_amd.progs import fixedpoint_log as fl

P64 = bc.P64
FIELDS = [(BLS, 4), (P64, 1)]
FIELD_IDS = ["bls", "2^64-59"]
BASES = (2, E, 10)


# ---- the model against the enclosure ------------------------------------------------------------------------------------------
def _worst(p, k, f, base, xs):
    """the largest distance of log_model from the enclosure over xs and the two extreme r1 sets, with the bound"""
    bound = fl.log_error_bound(k, f, None, base)
    limits = fl.log_shifts(k, f, None, base)
    worst = Fraction(0)
    for x in xs:
        enc = lc.log_enclosure(x, f, base)
        for r1s in lc.r1_extremes(limits):
            got = lc.centered(fl.log_model(x, p, k, f, r1s, base), p)
            worst = max(worst, lc.distance(got, enc))
            assert lc.distance(got, enc) <= bound, (k, f, base, x, got, float(enc[0]), float(bound))
    return worst, bound


@pytest.mark.parametrize("base", BASES, ids=["2", "e", "10"])
@pytest.mark.parametrize("k, f", [(8, 4), (16, 8)])
def test_model_within_the_bound_for_every_operand(k, f, base):
    worst, bound = _worst(BLS, k, f, base, range(1, 1 << (k - 1)))
    print(f"(k, f) = ({k}, {f}), base {base}: worst {float(worst):.4f} ulps, bound {float(bound):.4f}")
    assert worst > Fraction(1, 2)                                       # the bound is not vacuous: the roundings are really there


@pytest.mark.parametrize("base", BASES, ids=["2", "e", "10"])
@pytest.mark.parametrize("k, f", [(64, 32), (64, 62)])
def test_model_within_the_bound_at_the_wide_shapes(k, f, base):
    rnd = random.Random(1000 * k + f)
    xs = lc.structured(rnd, k, f, 14) + [rnd.randrange(1, 1 << (k - 1)) for _ in range(1000)]
    assert len(xs) > 2000
    worst, bound = _worst(BLS, k, f, base, xs)
    print(f"(k, f) = ({k}, {f}), base {base}: worst {float(worst):.4f} ulps, bound {float(bound):.4f}")


def test_exact_values_and_zero():
    for k, f in [(8, 4), (16, 8), (64, 32)]:
        limits = fl.log_shifts(k, f)
        for r1s in lc.r1_extremes(limits):
            assert fl.log_model(0, BLS, k, f, r1s) == 0                    # nothing raises, nothing wraps
            assert lc.centered(fl.log_model(1 << f, BLS, k, f, r1s), BLS) in (-1, 0, 1)
    assert lc.log_enclosure(1 << 8, 8) == (0, Fraction(1, 1 << 72))                 # 2 f + 64 digits, in ulps of 2^-f
    lo, hi = lc.log_enclosure(1 << 10, 8)
    assert lo <= 2 << 8 <= hi and hi - lo <= Fraction(1, 1 << 70)
    lo, hi = lc.log_enclosure(1000 << 8, 8, 10)
    assert lo <= 3 << 8 <= hi and hi - lo <= Fraction(1, 1 << 60)
    with pytest.raises(ValueError):
        fl.log_model(1 << 7, BLS, 8, 4, [0] * len(fl.log_shifts(8, 4)))
    with pytest.raises(ValueError):
        fl.log_model(1, BLS, 8, 4, [0])
    for bad in (lambda: fl.log_degree(8, 3), lambda: fl.log_degree(8, 7), lambda: fl.log_weights(8, 4, 1), lambda: fl.log_weights(8, 4, 2.5),
                lambda: fl.log_coefficients(8, 4, 2, 1), lambda: fl.log_layout(8, 4, 8, None, True), lambda: fl.log_error_bound(300, 200)):
        with pytest.raises(ValueError):
            bad()


# ---- the coefficients ---------------------------------------------------------------------------------------------------------
def _ln_series(y, terms):
    """ln(y) for a rational 1/2 < y < 2 by ln(1 + u) = sum (-1)^(n+1) u^n / n; another route than the module's atanh"""
    u = Fraction(y) - 1
    return sum((-1) ** (n + 1) * u ** n / n for n in range(1, terms))


def _independent(k, f, base, d):
    """the coefficients by another route: q from isqrt at 320 bits, the Chebyshev polynomials from cos(n theta) = Re (T + i sqrt(1 - T^2))^n
    expanded by the binomial theorem, ln 2 = sum 1 / (n 2^n), ln(3/4) and ln(6 q) by the series of ln(1 + u)"""
    from math import comb

    prec = 320
    q = 3 - Fraction(isqrt(8 << (2 * prec)), 1 << prec)
    a = [Fraction(0)] * (d + 1)
    for n in range(1, d + 1):
        cn = -2 * (-q) ** n / n
        # T_n(T) = sum_{m} C(n, 2m) T^(n-2m) (T^2 - 1)^m
        for m in range(n // 2 + 1):
            for i in range(m + 1):
                a[n - 2 * m + 2 * i] += cn * comb(n, 2 * m) * comb(m, i) * (-1) ** (m - i)
    ln2 = sum(Fraction(1, n << n) for n in range(1, 400))
    a[0] += _ln_series(Fraction(3, 4), 260) - _ln_series(Fraction((6 * q).numerator >> 200, (6 * q).denominator >> 200), 80)
    lnb = {2: ln2, E: Fraction(1), 10: 3 * ln2 + _ln_series(Fraction(10, 8), 200)}[base]
    return [c / lnb * (1 << (f + fl.GUARD_BITS)) for c in a]


def test_coefficients_and_degree():
    for k, f in [(8, 4), (16, 8), (32, 16), (64, 32), (64, 62)]:
        for base in BASES:
            d = fl.log_degree(k, f, base)
            scale = Fraction(1 << f) / {2: Fraction(6931471805, 10 ** 10), E: 1, 10: Fraction(23025850930, 10 ** 10)}[base]
            assert fl.series_tail(d) * scale <= Fraction(1, 4) * (1 + Fraction(1, 10 ** 8))
            assert d == 2 or fl.series_tail(d - 1) * scale > Fraction(1, 4) * (1 + Fraction(1, 10 ** 8)), (k, f, base)      # one degree fewer breaks it
            coef = fl.log_coefficients(k, f, base)
            want = _independent(k, f, base, d)
            assert len(coef) == d + 1
            for c, w in zip(coef, want):
                assert abs(c - w) <= Fraction(1, 2) + Fraction(1, 1 << 40), (k, f, base)
            assert all(abs(coef[j + 1]) < abs(coef[j]) for j in range(1, d) if abs(coef[j]) > 8)           # they decay: no cancellation
            first, second = fl.log_weights(k, f, base)
            assert second == [1 << (k - 1)] * (k - 1) and len(first) == k - 1
            if base == 2:
                assert first == [(i + 1 - f) * (1 << f) for i in range(k - 1)]
            else:
                for i, w in enumerate(first):
                    enc = lc.log_enclosure(1 << (i + 1), f, base)        # (i + 1 - f) 2^f / log2(base) = log_base(2^(i+1) / 2^f) 2^f
                    assert lc.distance(w, enc) <= Fraction(1, 2) + Fraction(1, 1 << 40)
    assert fl.log_degree(64, 32) in range(10, 15) and fl.log_error_bound(64, 32) < 3


def test_layout_and_counts():
    for k, f, kappa in [(8, 4, 8), (16, 8, 8), (32, 16, 16), (64, 32, 32), (64, 62, 32)]:
        for base in BASES:
            for d in (None, 2, 3, 5, 8, 13):
                lay = fl.log_layout(k, f, kappa, d, base)
                dd, width, n = lay["degree"], lay["width"], k - 1
                assert dd == (d or fl.log_degree(k, f, base)) and lay["levels"] == lc.levels(dd) == (dd - 1).bit_length()
                assert width == fl.log_width(k, f, d, base) >= 2 * k
                shifts = fl.log_shifts(k, f, d, base)
                assert shifts == [n] * (dd - 1) + [n + fl.GUARD_BITS] and max(shifts) < width
                assert lay["n_planes"] == fl.log_planes(k, f, kappa, d, base) == k + kappa + dd * (width + kappa)
                assert lay["n_triples"] == fl.log_triples(k, f, d, base) == bd.bit_triples(n) + fd.preor_triples(n) + 1 + (dd - 1)
                assert lay["opens"] == fl.log_opens(k, f, d, base) == bd.bit_opens(n) + fd.preor_levels(n) + 1 + 2 * lc.levels(dd) + 1
                for ranges, total in ((lay["planes"], lay["n_planes"]), (lay["triples"], lay["n_triples"])):
                    spans = sorted(ranges.values())
                    assert spans[0][0] == 0 and spans[-1][1] == total and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
                assert sum(len(lc.level_powers(l, dd)) for l in range(1, lay["levels"] + 1)) == dd - 1
                assert len(lc.truncation_planes(lay, kappa)) == len(shifts)
    assert fl.log_width(64, 32) == 128 and fl.log_width(8, 4) == 16


# ---- the self-test rows against Python ints -------------------------------------------------------------------------------------
def _vals(rnd, p, n):
    return [rnd.randrange(p) for _ in range(n)]


def _shifts(p):
    return (1, 8, 61) + ((64, 127, 140) if p >> 64 else ())


@pytest.mark.parametrize("p, nl", FIELDS, ids=FIELD_IDS)
def test_first_and_finish_rows(p, nl):
    rnd = random.Random(p % 1009)
    for count in (0, 1, 257):
        opened = _vals(rnd, p, 2 * count)
        ta, tb, tab, ybig, na, nb, s, ipart = (_vals(rnd, p, count) for _ in range(8))
        masked, powers = ok(run_log(p, nl, FIRST, [opened, ta, tb, tab, ybig, na, nb], [], [2, 1], count))
        want_masked, want_t = lc.first_on_ints(p, opened, ta, tb, tab, ybig, na, nb, count)
        assert masked == want_masked and powers == want_t, count
        for m in _shifts(p):
            out, = ok(run_log(p, nl, FINISH, [opened[:count], s, [pow(2, -m, p)], ipart], [m], [1], count))
            assert out == lc.finish_on_ints(p, opened[:count], s, m, ipart), (m, count)


@pytest.mark.parametrize("p, nl", FIELDS, ids=FIELD_IDS)
def test_level_rows_at_every_level(p, nl):
    rnd = random.Random(p % 1013)
    for count in (0, 1, 257):
        for d in DEGREES:
            for level in range(1, lc.levels(d)):
                done, nxt = len(lc.level_powers(level, d)), len(lc.level_powers(level + 1, d))
                for m in _shifts(p) if (d, count) in ((13, 1), (5, 257)) else (8,):
                    opened, s = _vals(rnd, p, done * count), _vals(rnd, p, done * count)
                    ta, tb, powers = _vals(rnd, p, nxt * count), _vals(rnd, p, nxt * count), _vals(rnd, p, d * count)
                    masked, new = ok(run_log(p, nl, LEVEL, [opened, s, [pow(2, -m, p)], ta, tb], [level, d, m], [2 * nxt, powers], count))
                    want_masked, want_powers = lc.level_on_ints(p, level, d, opened, s, m, ta, tb, powers, count)
                    assert masked == want_masked and new == want_powers, (d, level, m, count)
                    half = 1 << (level - 1)
                    assert new[:half * count] == powers[:half * count] and new[(half + done) * count:] == powers[(half + done) * count:]


@pytest.mark.parametrize("p, nl", FIELDS, ids=FIELD_IDS)
def test_poly_mask_rows(p, nl):
    rnd = random.Random(p % 1019)
    kappa = 8
    for count in (0, 1, 257):
        for d in DEGREES:
            done = len(lc.level_powers(lc.levels(d), d))
            for m_in in _shifts(p) if (d, count) in ((13, 1), (3, 257)) else (8,):
                m_out = m_in if m_in + 5 + kappa + 1 <= p.bit_length() - 1 else 8          # the mask must fit below the modulus
                width = m_out + 5
                opened, s = _vals(rnd, p, done * count), _vals(rnd, p, done * count)
                powers, ybig, coef = _vals(rnd, p, d * count), _vals(rnd, p, count), _vals(rnd, p, d + 1)
                bits = [rnd.getrandbits(1) for _ in range((width + kappa) * count)]
                masked, kept = ok(run_log(p, nl, POLY_MASK, [opened, s, [pow(2, -m_in, p)], powers, ybig, coef, bits], [d, m_in, width, m_out, kappa], [1, 1], count))
                want = lc.poly_mask_on_ints(p, d, opened, s, m_in, powers, ybig, coef, bits, width, m_out, kappa, count)
                assert (masked, kept) == want, (d, m_in, count)


def test_refusals_in_the_self_test():
    p, nl, count, d, m, kappa, width = P64, 1, 3, 5, 8, 8, 20
    rnd = random.Random(5)
    v = lambda rows: _vals(rnd, p, rows * count)
    inv = [pow(2, -m, p)]
    first = [v(2), v(1), v(1), v(1), v(1), v(1), v(1)]
    level = [v(1), v(1), inv, v(2), v(2)]                                 # level 1 of d = 5: one power done, two products next
    poly = [v(1), v(1), inv, v(d), v(1), _vals(rnd, p, d + 1), [0, 1] * ((width + kappa) * count // 2)]
    fin = [v(1), v(1), inv, v(1)]
    assert run_log(p, nl, FIRST, first, [], [2, 1], count)[0] == 0
    assert run_log(p, nl, LEVEL, level, [1, d, m], [4, v(d)], count)[0] == 0
    assert run_log(p, nl, POLY_MASK, poly, [d, m, width, m, kappa], [1, 1], count)[0] == 0
    assert run_log(p, nl, FINISH, fin, [m], [1], count)[0] == 0
    from honeybadgermpc_amd._capi import HB_ERR_BAD_ARG as bad
    # null pointers
    for i in range(7):
        assert run_log(p, nl, FIRST, first[:i] + [None] + first[i + 1:], [], [2, 1], count)[0] == bad
    assert run_log(p, nl, FIRST, first, [], [2, None], count)[0] == bad and run_log(p, nl, FIRST, first, [], [None, 1], count)[0] == bad
    for i in range(5):
        assert run_log(p, nl, LEVEL, level[:i] + [None] + level[i + 1:], [1, d, m], [4, v(d)], count)[0] == bad
    for i in range(7):
        assert run_log(p, nl, POLY_MASK, poly[:i] + [None] + poly[i + 1:], [d, m, width, m, kappa], [1, 1], count)[0] == bad
    for i in range(4):
        assert run_log(p, nl, FINISH, fin[:i] + [None] + fin[i + 1:], [m], [1], count)[0] == bad
    # d < 2, d too large, a level out of range, shifts and widths the modulus has no room for, a constant not below the modulus
    for prm in ([1, 1, m], [1, 65, m], [0, d, m], [3, d, m], [-1, d, m], [1, 2, m], [1, d, 0], [1, d, 63]):
        assert run_log(p, nl, LEVEL, level, prm, [4, v(d)], count)[0] == bad, prm
    for prm in ([1, m, width, m, kappa], [65, m, width, m, kappa], [d, 0, width, m, kappa], [d, m, width, width, kappa], [d, m, 60, m, kappa], [d, m, width, m, -1]):
        assert run_log(p, nl, POLY_MASK, poly, prm, [1, 1], count)[0] == bad, prm
    assert run_log(p, nl, FINISH, fin, [0], [1], count)[0] == bad and run_log(p, nl, FINISH, fin, [63], [1], count)[0] == bad
    assert run_log(p, nl, 4, fin, [m], [1], count)[0] == bad and run_log(p, nl, FIRST, first, [], [2, 1], -1)[0] == bad


def test_outputs_laid_over_inputs_are_refused():
    """through ctypes, where two arguments can be one buffer"""
    import ctypes

    import numpy as np

    from honeybadgermpc_amd._capi import HB_ERR_BAD_ARG, ints_to_limbs, load_library, np_ptr

    lib = load_library()
    p, nl, count, d, m, kappa, width = P64, 1, 4, 5, 8, 8, 20
    rnd = random.Random(6)
    buf = lambda rows: np.array(ints_to_limbs(_vals(rnd, p, rows * count), p, 8))
    inv = np.array(ints_to_limbs([pow(2, -m, p)], p, 8))
    pl = np_ptr(ints_to_limbs([p], p + 1, 8))

    def call(what, ops, params, outs):
        ptrs = (ctypes.c_void_p * 8)(*([a.ctypes.data for a in ops] + [None] * (8 - len(ops))))
        optrs = (ctypes.c_void_p * 2)(*([a.ctypes.data for a in outs] + [None] * (2 - len(outs))))
        prm = (ctypes.c_int64 * 5)(*(list(params) + [0] * (5 - len(params))))
        return lib.hb_selftest_fxlog(pl, nl, what, ptrs, prm, optrs, count)

    first = [buf(2)] + [buf(1) for _ in range(6)]
    masked, powers = buf(4), buf(d)
    assert call(FIRST, first, [], [masked, powers]) == 0
    for i in range(7):
        assert call(FIRST, first, [], [first[i], powers]) == HB_ERR_BAD_ARG and call(FIRST, first, [], [masked, first[i]]) == HB_ERR_BAD_ARG
    assert call(FIRST, first, [], [masked, masked[count:]]) == HB_ERR_BAD_ARG
    level = [buf(1), buf(1), inv, buf(2), buf(2)]
    assert call(LEVEL, level, [1, d, m], [masked, powers]) == 0
    for i in (0, 1, 3, 4):
        assert call(LEVEL, level, [1, d, m], [level[i], powers]) == HB_ERR_BAD_ARG and call(LEVEL, level, [1, d, m], [masked, level[i]]) == HB_ERR_BAD_ARG
    assert call(LEVEL, level, [1, d, m], [powers, powers]) == HB_ERR_BAD_ARG
    poly = [buf(1), buf(1), inv, powers, buf(1), buf(2)[:d + 1], buf(width + kappa)]
    kept = buf(1)
    assert call(POLY_MASK, poly, [d, m, width, m, kappa], [masked, kept]) == 0
    for i in (0, 1, 3, 4, 5, 6):
        assert call(POLY_MASK, poly, [d, m, width, m, kappa], [poly[i], kept]) == HB_ERR_BAD_ARG, i
        assert call(POLY_MASK, poly, [d, m, width, m, kappa], [masked, poly[i]]) == HB_ERR_BAD_ARG, i
    assert call(POLY_MASK, poly, [d, m, width, m, kappa], [kept, kept]) == HB_ERR_BAD_ARG
    fin = [buf(1), buf(1), inv, buf(1)]
    assert call(FINISH, fin, [m], [kept]) == 0
    for i in (0, 1, 3):
        assert call(FINISH, fin, [m], [fin[i]]) == HB_ERR_BAD_ARG

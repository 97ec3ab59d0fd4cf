"""CPU-only: honeybadgermpc_amd.progs.fixedpoint_atan -- atan2_model against an integer enclosure of atan2 within the DERIVED bound (every
pair at (8, 4), in radians and in turns; a structured set at the wide shapes; the two extreme r1 sets), the exact values on the axes, the
coefficients and the degree against an independent recomputation, the counts against their formulas, the steps of csrc/hb_fxatan.hip
through hb_selftest_fxatan (the rows the device runs, behind the step functions the entry points run) against Python ints, and what
the steps refuse."""
import random
from fractions import Fraction
from math import comb, isqrt

import pytest

import atan_cases as ac
import bitdec_cases as bc
from atan_cases import ABS, ASSEMBLE, DEGREES, FINISH, FIRST, LEVEL, POLY_MASK, SELECT, SELECT_MASK, SIGN_MASK, ok, run_atan
from conftest import BLS

from honeybadgermpc_amd.progs import fixedpoint as fx
from honeybadgermpc_amd.progs import fixedpoint_atan as fa
from honeybadgermpc_amd.progs import fixedpoint_division as fd

P64 = bc.P64
FIELDS = [(BLS, 4), (P64, 1)]
FIELD_IDS = ["bls", "2^64-59"]


# ---- the model against the enclosure ------------------------------------------------------------------------------------------
def _worst(p, k, f, turns, pairs):
    """the largest distance of atan2_model from the enclosure over the pairs and the two extreme r1 sets, with the bound"""
    bound = fa.atan_error_bound(k, f, turns)
    limits = fa.atan_shifts(k, f, turns)
    worst = Fraction(0)
    for y, x in pairs:
        enc = ac.atan2_enclosure(y, x, f, turns)
        for r1s in ac.r1_extremes(limits):
            got = ac.centered(fa.atan2_model(y, x, p, k, f, r1s, turns), p)
            dist = ac.distance(got, enc)
            worst = max(worst, dist)
            assert dist <= bound, (k, f, turns, y, x, got, float(enc[0]), float(bound))
    return worst, bound


@pytest.mark.parametrize("turns", [False, True], ids=["radians", "turns"])
def test_model_within_the_bound_for_every_pair(turns):
    k, f = 8, 4
    lim = 1 << (k - 1)
    worst, bound = _worst(BLS, k, f, turns, [(y, x) for y in range(-lim + 1, lim) for x in range(-lim + 1, lim)])
    print(f"(k, f) = ({k}, {f}), turns = {turns}: worst {float(worst):.4f} ulps, bound {float(bound):.4f}")
    assert worst > Fraction(1, 2)                                       # the bound is not vacuous: the roundings are really there


@pytest.mark.parametrize("turns", [False, True], ids=["radians", "turns"])
@pytest.mark.parametrize("k, f", ac.SHAPES)
def test_model_within_the_bound_on_the_structured_set(k, f, turns):
    rnd = random.Random(1000 * k + f + turns)
    pairs = ac.structured(rnd, k, f, 3000)
    assert len(pairs) > 3000 and (0, 0) in pairs
    worst, bound = _worst(BLS, k, f, turns, pairs)
    print(f"(k, f) = ({k}, {f}), turns = {turns}: worst {float(worst):.4f} ulps, bound {float(bound):.4f}")


def test_the_enclosure_itself():
    """against values known exactly, and against the float atan2 where a float can tell"""
    import math

    for f in (4, 8, 32):
        for turns, full in ((False, None), (True, 1 << f)):
            lo, hi = ac.atan2_enclosure(1, 1, f, turns)
            assert hi - lo < Fraction(1, 1 << 60)
            if turns:
                assert lo <= Fraction(full, 8) <= hi
                assert all(a <= w <= b for (a, b), w in ((ac.atan2_enclosure(0, -5, f, True), Fraction(full, 2)), (ac.atan2_enclosure(-3, 0, f, True), Fraction(-full, 4)),
                                                           (ac.atan2_enclosure(-7, -7, f, True), Fraction(-3 * full, 8)), (ac.atan2_enclosure(7, -7, f, True), Fraction(3 * full, 8))))
    assert ac.atan2_enclosure(0, 0, 8) == (0, 0) and 0 <= ac.atan2_enclosure(0, 9, 8)[0] <= ac.atan2_enclosure(0, 9, 8)[1] < Fraction(1, 1 << 60)
    rnd = random.Random(3)
    for _ in range(300):
        y, x = rnd.randrange(-1000, 1000), rnd.randrange(-1000, 1000)
        lo, hi = ac.atan2_enclosure(y, x, 16)
        assert abs(float(lo) - math.atan2(y, x) * 65536) < 1e-6 and lo <= hi, (y, x)
        lo, hi = ac.atan2_enclosure(y, x, 16, True)
        assert abs(float(lo) - math.atan2(y, x) / (2 * math.pi) * 65536) < 1e-6 and lo <= hi, (y, x)


def test_exact_values_on_the_axes():
    for k, f in [(8, 4), (16, 8), (64, 32), (64, 61)]:
        top = (1 << (k - 1)) - 1
        for turns in (False, True):
            big, half = fa.atan_constants(f, turns)
            if turns:
                assert (big, half) == (1 << (f - 1), 1 << (f - 2))
            else:
                assert ac.distance(big, ac.atan2_enclosure(0, -1, f)) <= Fraction(1, 2) and ac.distance(half, ac.atan2_enclosure(1, 0, f)) <= Fraction(1, 2)
            for r1s in ac.r1_extremes(fa.atan_shifts(k, f, turns)):
                model = lambda y, x: ac.centered(fa.atan2_model(y, x, BLS, k, f, r1s, turns), BLS)
                for mag in (1, 1 << f, top):
                    assert model(0, 0) == 0 and model(0, mag) == 0               # nothing raises, nothing wraps
                    assert model(0, -mag) == big                                # y = 0, x < 0: +pi, as math.atan2
                    assert model(mag, 0) == half and model(-mag, 0) == -half
    for bad in (lambda: fa.atan2_model(1 << 7, 1, BLS, 8, 4, [0] * len(fa.atan_shifts(8, 4))), lambda: fa.atan2_model(1, -(1 << 7), BLS, 8, 4, [0] * len(fa.atan_shifts(8, 4))),
                lambda: fa.atan2_model(1, 1, BLS, 8, 4, [0]), lambda: fa.atan2_model(1, 1, BLS, 8, 4, [1 << 20] * len(fa.atan_shifts(8, 4))),
                lambda: fa.atan_degree(8, 3), lambda: fa.atan_degree(8, 6), lambda: fa.atan_degree(8, 7), lambda: fa.atan_coefficients(8, 4, False, 4),
                lambda: fa.atan_coefficients(8, 4, False, 1), lambda: fa.atan_layout(8, 4, True), lambda: fa.atan_error_bound(300, 200), lambda: fa.series_tail(4),
                lambda: fa.atan2_model(1, 1, 1 << 20, 16, 8, [0] * len(fa.atan_shifts(16, 8)))):
        with pytest.raises(ValueError):
            bad()


# ---- the coefficients ---------------------------------------------------------------------------------------------------------
def _independent(f, turns, d):
    """the coefficients by another route: r from isqrt at 320 bits, the Chebyshev polynomials from cos(n theta) = Re (T + i sqrt(1 - T^2))^n
    expanded by the binomial theorem, pi from the test's own Machin sum"""
    prec = 320
    r = Fraction(isqrt(2 << (2 * prec)), 1 << prec) - 1
    a = [Fraction(0)] * (d + 1)
    for n in range(1, d + 1, 2):
        cn = 2 * (-1) ** (n // 2) * r ** n / n
        for m in range(n // 2 + 1):                                     # T_n(T) = sum_m C(n, 2m) T^(n-2m) (T^2 - 1)^m
            for i in range(m + 1):
                a[n - 2 * m + 2 * i] += cn * comb(n, 2 * m) * comb(m, i) * (-1) ** (m - i)
    assert not any(a[0::2])
    unit = Fraction(1 << 400, 2 * ac._pi_units(400)[0]) if turns else 1
    return [c * unit * (1 << (f + fa.GUARD_BITS)) for c in a[1::2]]


def test_coefficients_and_degree():
    r_hi = Fraction(41421356238, 10 ** 11)                              # a little above sqrt 2 - 1
    for k, f in [(8, 4), (16, 8), (32, 16), (64, 32), (64, 61)]:
        for turns in (False, True):
            d = fa.atan_degree(k, f, turns)
            scale = Fraction(1 << f) * (Fraction(10 ** 10, 62831853071) if turns else 1)
            tail = lambda deg: 2 * r_hi ** (deg + 2) / ((deg + 2) * (1 - r_hi ** 2)) * scale
            assert d & 1 and d >= 3 and fa.series_tail(d) <= tail(d) and tail(d) <= Fraction(1, 4) * (1 + Fraction(1, 10 ** 8))
            assert d == 3 or tail(d - 2) > Fraction(1, 4) * (1 + Fraction(1, 10 ** 8)), (k, f, turns)      # one degree fewer breaks the rule
            coef = fa.atan_coefficients(k, f, turns)
            want = _independent(f, turns, d)
            assert len(coef) == (d + 1) // 2 == len(want)
            for c, w in zip(coef, want):
                assert abs(c - w) <= Fraction(1, 2) + Fraction(1, 1 << 40), (k, f, turns)
            assert all(abs(c) < 1 << (f + fa.GUARD_BITS) for c in coef)                                     # below 1 in magnitude: no cancellation
            assert all(c > 0 if j % 2 == 0 else c < 0 for j, c in enumerate(coef) if abs(c) > 8)
    assert [fa.atan_degree(64, 32), fa.atan_degree(64, 32, True), fa.atan_degree(16, 8), fa.atan_degree(8, 4)] == [23, 21, 5, 3]
    assert ac.total_products(23) == 15 and ac.levels(23) == 4 and [ac.level_products(l, 23) for l in range(5)] == [1, 2, 3, 5, 4]
    # the series really is atan: the polynomial at degree 23 against the enclosure at a few arguments, well inside the tail
    mono = fa._monomials(23, False)
    for num in (0, 1, 5, 9, 16):
        val = sum(c * Fraction(num, 16) ** (2 * j + 1) for j, c in enumerate(mono))
        lo, hi = ac.atan2_enclosure(num, 16, 40)
        assert abs(val * (1 << 40) - lo) <= fa.series_tail(23) * (1 << 40) + 1, num


def test_the_bound_and_its_terms():
    for k, f in [(8, 4), (16, 8), (64, 32), (64, 61)]:
        delta = fa.quotient_error_bound(k, f)
        assert 2 < delta <= fd.div_error_bound(k, f, None)                 # derived at |Q| <= 1: never above the worst case
        for turns in (False, True):
            bound = fa.atan_error_bound(k, f, turns)
            assert isinstance(bound, Fraction) and bound > (1 if turns else 2) + fa.series_tail(fa.atan_degree(k, f, turns)) * (1 << f) * (Fraction(1, 7) if turns else 1)
            assert bound < delta + 8
    assert fa.quotient_error_bound(64, 32) < fd.div_error_bound(64, 32, None)
    # the quotient really stays within delta of the exact one, at the small shape, for every pair and both extreme r1 sets
    k, f, p = 8, 4, BLS
    theta, width = fd.goldschmidt_iterations(k, f), fd.div_width(k, f)
    limits = fa._div_shifts(k, f)
    delta = fa.quotient_error_bound(k, f)
    worst = Fraction(0)
    for den in range(1, 1 << (k - 1)):
        for num in range(den + 1):
            for r1s in ac.r1_extremes(limits):
                q = ac.centered(fd._div_residues(num, den, p, k, f, r1s, theta, False, width), p)
                worst = max(worst, abs(q - Fraction(num << f, den)))
                assert q >= 0
    print(f"quotient at (8, 4): worst {float(worst):.4f} ulps, delta {float(delta):.4f}")
    assert worst <= delta


@pytest.mark.parametrize("k, f", ac.SHAPES)
def test_the_quotient_stays_within_delta_at_the_wide_shapes(k, f):
    """quotient_error_bound restates fixedpoint_division's recurrence: held here against div's own residues on the structured magnitudes
    and seeded ones, both extreme r1 sets"""
    p, rnd = BLS, random.Random(7 * k + f)
    theta, width, limits, delta = fd.goldschmidt_iterations(k, f), fd.div_width(k, f), fa._div_shifts(k, f), fa.quotient_error_bound(k, f)
    mags = {(min(abs(y), abs(x)), max(abs(y), abs(x))) for y, x in ac.structured(rnd, k, f, 1500)}
    worst = Fraction(0)
    for num, den in sorted(mags):
        if den:
            for r1s in ac.r1_extremes(limits):
                q = ac.centered(fd._div_residues(num, den, p, k, f, r1s, theta, False, width), p)
                worst = max(worst, abs(q - Fraction(num << f, den)))
                assert q >= 0
    print(f"quotient at ({k}, {f}): worst {float(worst):.4f} ulps over {len(mags)} pairs, delta {float(delta):.4f}")
    assert worst <= delta


def test_layout_and_counts():
    for k, f, kappa in [(8, 4, 8), (16, 8, 8), (32, 16, 16), (64, 32, 32), (64, 61, 32)]:
        for turns in (False, True):
            for d in (None,) + DEGREES:
                lay = fa.atan_layout(k, f, kappa, turns, d)
                dd, width, n = lay["degree"], lay["width"], k - 1
                dlay = fd.div_layout(k, f, kappa, None, False)
                assert dd == (d or fa.atan_degree(k, f, turns)) and lay["levels"] == ac.levels(dd) and lay["div"] == dlay
                assert lay["products"] == [ac.level_products(l, dd) for l in range(ac.levels(dd) + 1)]
                assert width == fa.atan_width(k, f, turns, d) >= 2 * k
                shifts = fa.atan_shifts(k, f, turns, d)
                products = ac.total_products(dd)
                theta = fd.goldschmidt_iterations(k, f)
                assert shifts == [2 * (n - f), f] + [2 * f] * (2 * theta - 1) + [n] * products + [n + fa.GUARD_BITS] and max(shifts[-products - 1:]) < width
                assert lay["n_planes"] == fa.atan_planes(k, f, kappa, turns, d) == 3 * (k + kappa) + dlay["n_planes"] + (products + 1) * (width + kappa)
                assert lay["n_triples"] == fa.atan_triples(k, f, turns, d) == 3 * fx.carry_triples(n) + 3 + 2 + dlay["n_triples"] + products + 1 + 1
                assert lay["opens"] == fa.atan_opens(k, f, turns, d) == fa.atan2_opens(k, f, turns, d)
                assert lay["opens"] == 2 * (1 + fx.carry_levels(n)) + 2 + fd.div_opens(k, f, None, False) + 2 * (ac.levels(dd) + 1) + 1 + 1
                for ranges, total in ((lay["planes"], lay["n_planes"]), (lay["triples"], lay["n_triples"])):
                    spans = sorted(ranges.values())
                    assert spans[0][0] == 0 and spans[-1][1] == total and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
                assert len(ac.truncation_planes(lay, kappa)) == len(shifts)
                # an odd polynomial's ladder: (d + 1) / 2 - 1 odd powers, u, and a square a level but the last
                assert products == (dd - 1) // 2 + 1 + max(ac.levels(dd) - 1, 0)
    assert fa.atan_width(64, 32) == 128 and fa.atan_layout(64, 32, 32)["products"] == [1, 2, 3, 5, 4]
    # every power is formed from two that exist by then: the wiring, walked
    for d in range(3, 64, 2):
        have_t, have_u = {0}, {0}
        for level in range(1, ac.levels(d) + 1):
            for j in ac.level_odd(level, d):
                assert j - (1 << (level - 1)) in have_t and level - 1 in have_u
            have_t |= set(ac.level_odd(level, d))
            if ac.level_square(level, d):
                have_u.add(level)
        assert have_t == set(range((d + 1) // 2))


# ---- the self-test rows against Python ints -------------------------------------------------------------------------------------
def _vals(rnd, p, n):
    """uniform residues with the edge operands 0 and p - 1 among the first"""
    out = [rnd.randrange(p) for _ in range(n)]
    for i, v in zip(range(0, n, 3), (0, p - 1, p - 1, 0)):
        out[i] = v
    return out


def _shifts(p):
    return (1, 8, 61) + ((64, 127, 140) if p >> 64 else ())


COUNTS = (0, 1, 5, 257)


@pytest.mark.parametrize("p, nl", FIELDS, ids=FIELD_IDS)
def test_mask_select_and_finish_rows(p, nl):
    rnd = random.Random(p % 1009)
    for count in COUNTS:
        v = lambda rows: _vals(rnd, p, rows * count)
        s, x, y, ta, tb = v(2), v(1), v(1), v(3), v(3)
        masked, = ok(run_atan(p, nl, SIGN_MASK, [s, x, y, ta, tb], [], [6], count))
        assert masked == ac.sign_mask_on_ints(p, s, x, y, ta, tb, count), count
        c, w, sx, ta, tb = v(1), v(1), v(1), v(2), v(2)
        masked, = ok(run_atan(p, nl, SELECT_MASK, [c, w, sx, ta, tb], [], [4], count))
        assert masked == ac.select_mask_on_ints(p, c, w, sx, ta, tb, count), count
        opened, ta, tb, tab, ax, ay = v(4), v(2), v(2), v(2), v(1), v(1)
        out, = ok(run_atan(p, nl, SELECT, [opened, ta, tb, tab, ax, ay], [], [3], count))
        assert out == ac.select_on_ints(p, opened, ta, tb, tab, ax, ay, count), count
        opened, ta, tb, tab, cst = v(2), v(1), v(1), v(1), v(1)
        out, = ok(run_atan(p, nl, FINISH, [opened, ta, tb, tab, cst], [], [1], count))
        assert out == ac.finish_on_ints(p, opened, ta, tb, tab, cst, count), count
        for shift in (0, 1, 3, 31, 60) + ((200, 255) if p >> 64 else ()):
            q, sy, e1, ta, tb = v(1), v(1), v(1), v(2), v(2)
            masked, powers = ok(run_atan(p, nl, FIRST, [q, sy, e1, ta, tb], [shift], [4, 1], count))
            assert (masked, powers) == ac.first_on_ints(p, q, shift, sy, e1, ta, tb, count), (shift, count)


@pytest.mark.parametrize("p, nl", FIELDS, ids=FIELD_IDS)
def test_abs_and_assemble_rows(p, nl):
    rnd = random.Random(p % 1021)
    for count in COUNTS:
        v = lambda rows: _vals(rnd, p, rows * count)
        for k, kappa in [(8, 8), (16, 8), (30, 30)] + ([(64, 32), (128, 100)] if p >> 64 else []):
            opened, ta, tb, tab, x, y = v(6), v(3), v(3), v(3), v(1), v(1)
            bits = [rnd.getrandbits(1) for _ in range((k + kappa) * count)]
            masked, kept = ok(run_atan(p, nl, ABS, [opened, ta, tb, tab, x, y, bits], [k, kappa], [1, 5], count))
            assert (masked, kept) == ac.abs_on_ints(p, opened, ta, tb, tab, x, y, bits, k, kappa, count), (k, count)
            if count:                                                   # the mask is the one hb_fxp_mask writes for w: the comparison can take it
                w = kept[3 * count:4 * count]
                assert (masked, kept[4 * count:]) == bc.run_fxp_mask(p, nl, w, bits, k, k - 1, kappa, count)
        for m in _shifts(p):
            opened, s, eopened, ea, eb, eab, sy, g, ta, tb = v(1), v(1), v(2), v(1), v(1), v(1), v(1), v(1), v(1), v(1)
            consts = _vals(rnd, p, 2)
            got = ok(run_atan(p, nl, ASSEMBLE, [opened, s, [pow(2, -m, p)], eopened, ea, eb, eab, sy, g, consts, ta, tb], [m], [2, 1], count))
            assert tuple(got) == ac.assemble_on_ints(p, opened, s, m, eopened, ea, eb, eab, sy, g, consts, ta, tb, count), (m, count)


@pytest.mark.parametrize("p, nl", FIELDS, ids=FIELD_IDS)
def test_level_rows_at_every_level(p, nl):
    rnd = random.Random(p % 1013)
    for count in COUNTS:
        for d in DEGREES:
            rows = (d + 1) // 2
            for level in range(ac.levels(d)):
                done, nxt = ac.level_products(level, d), ac.level_products(level + 1, d)
                for m in _shifts(p) if (d, count) in ((13, 1), (23, 5), (5, 257)) else (8,):
                    opened, s = _vals(rnd, p, done * count), _vals(rnd, p, done * count)
                    ta, tb, powers = _vals(rnd, p, nxt * count), _vals(rnd, p, nxt * count), _vals(rnd, p, rows * count)
                    masked, new = ok(run_atan(p, nl, LEVEL, [opened, s, [pow(2, -m, p)], ta, tb], [level, d, m], [2 * nxt, powers], count))
                    want_masked, want_powers = ac.level_on_ints(p, level, d, opened, s, m, ta, tb, powers, count)
                    assert masked == want_masked and new == want_powers, (d, level, m, count)
                    half = 1 << (level - 1) if level else 0
                    odd = done - 1                                      # the square is never stored
                    assert new[:half * count] == powers[:half * count] and new[(half + odd) * count:] == powers[(half + odd) * count:]


@pytest.mark.parametrize("p, nl", FIELDS, ids=FIELD_IDS)
def test_poly_mask_rows(p, nl):
    rnd = random.Random(p % 1019)
    kappa = 8
    for count in COUNTS:
        for d in DEGREES:
            rows, done = (d + 1) // 2, ac.level_products(ac.levels(d), d)
            for m_in in _shifts(p) if (d, count) in ((13, 1), (3, 257), (23, 5)) else (8,):
                m_out = m_in if m_in + 5 + kappa + 1 <= p.bit_length() - 1 else 8          # the mask must fit below the modulus
                width = m_out + 5
                opened, s = _vals(rnd, p, done * count), _vals(rnd, p, done * count)
                powers, coef = _vals(rnd, p, rows * count), _vals(rnd, p, rows)
                bits = [rnd.getrandbits(1) for _ in range((width + kappa) * count)]
                masked, kept = ok(run_atan(p, nl, POLY_MASK, [opened, s, [pow(2, -m_in, p)], powers, coef, bits], [d, m_in, width, m_out, kappa], [1, 1], count))
                want = ac.poly_mask_on_ints(p, d, opened, s, m_in, powers, coef, bits, width, m_out, kappa, count)
                assert (masked, kept) == want, (d, m_in, count)


@pytest.mark.parametrize("p, nl", FIELDS, ids=FIELD_IDS)
def test_the_rows_chained_give_the_model(p, nl):
    """ONE holder (degree-0 shares) walks the ladder and the assembly through the self-test rows with products_trunc's job done on ints:
    the result is atan2_model's for the same r1"""
    k, f, kappa = 16, 8, 8
    rnd = random.Random(p % 1031)
    for turns in (False, True):
        lay = fa.atan_layout(k, f, kappa, turns)
        d, width, n = lay["degree"], lay["width"], k - 1
        assert width + kappa + 1 <= p.bit_length() - 1                     # both fields hold the shape
        pairs = ac.e2e_pairs(rnd, k, f, 16)
        count = len(pairs)
        limits = fa.atan_shifts(k, f, turns, d)
        n_div = len(fa._div_shifts(k, f))
        r1s = [[rnd.randrange(1 << m) for m in limits] for _ in range(count)]
        theta, dwidth = fd.goldschmidt_iterations(k, f), fd.div_width(k, f)
        trip = lambda rows: (lambda a, b: (a, b, [u * v % p for u, v in zip(a, b)]))(_vals(rnd, p, rows * count), _vals(rnd, p, rows * count))
        res = lambda vs: [v % p for v in vs]
        ys, xs = res(y for y, _ in pairs), res(x for _, x in pairs)
        s = [int(x < 0) for _, x in pairs] + [int(y < 0) for y, _ in pairs]
        ta, tb, tab = trip(3)
        masked, = ok(run_atan(p, nl, SIGN_MASK, [s, xs, ys, ta, tb], [], [6], count))
        bits = [rnd.getrandbits(1) for _ in range((k + kappa) * count)]
        _, kept = ok(run_atan(p, nl, ABS, [masked, ta, tb, tab, xs, ys, bits], [k, kappa], [1, 5], count))
        assert kept[:2 * count] == [abs(x) for _, x in pairs] + [abs(y) for y, _ in pairs]
        c = [int(abs(x) < abs(y)) for y, x in pairs]
        ta, tb, tab = trip(2)
        masked, = ok(run_atan(p, nl, SELECT_MASK, [c, kept[3 * count:4 * count], s[:count], ta, tb], [], [4], count))
        nde, = ok(run_atan(p, nl, SELECT, [masked, ta, tb, tab, kept[:count], kept[count:2 * count]], [], [3], count))
        assert nde[:2 * count] == [min(abs(x), abs(y)) for y, x in pairs] + [max(abs(x), abs(y)) for y, x in pairs]
        q = [fd._div_residues(nde[i], nde[count + i], p, k, f, r1s[i][:n_div], theta, False, dwidth) for i in range(count)]
        ta, tb, tab = trip(2)
        masked, t = ok(run_atan(p, nl, FIRST, [q, s[count:], nde[2 * count:], ta, tb], [n - f], [4, 1], count))
        e_opened, e_trip = masked[2 * count:], tuple(v[count:] for v in (ta, tb, tab))
        powers = t + [0] * ((d - 1) // 2 * count)
        at = n_div
        sv = opened = None
        for level in range(lay["levels"] + 1):
            c_level = lay["products"][level]
            prods = [bc.beaver(masked[2 * r * count + i], masked[(2 * r + 1) * count + i], ta[r * count + i], tb[r * count + i], tab[r * count + i], p)
                     for r in range(c_level) for i in range(count)]
            r1 = [r1s[i][at + r] for r in range(c_level) for i in range(count)]
            sv = [(v + r) % p for v, r in zip(prods, r1)]
            opened = [(v + (1 << (width - 1)) + r) % p for v, r in zip(prods, r1)]          # r2 = 0
            at += c_level
            if level < lay["levels"]:
                ta, tb, tab = trip(lay["products"][level + 1])
                masked, powers = ok(run_atan(p, nl, LEVEL, [opened, sv, [pow(2, -n, p)], ta, tb], [level, d, n], [2 * lay["products"][level + 1], powers], count))
        m_out = n + fa.GUARD_BITS
        coef = [v % p for v in fa.atan_coefficients(k, f, turns)]
        planes = [(r1s[i][at] >> r) & 1 if r < m_out else 0 for r in range(width + kappa) for i in range(count)]
        masked, sv = ok(run_atan(p, nl, POLY_MASK, [opened, sv, [pow(2, -n, p)], powers, coef, planes], [d, n, width, m_out, kappa], [1, 1], count))
        ta, tb, tab = trip(1)
        consts = list(fa.assemble_constants(p, f, turns))
        masked, cst = ok(run_atan(p, nl, ASSEMBLE, [masked, sv, [pow(2, -m_out, p)], e_opened, e_trip[0], e_trip[1], e_trip[2], s[count:], kept[2 * count:3 * count], consts, ta, tb],
                                  [m_out], [2, 1], count))
        out, = ok(run_atan(p, nl, FINISH, [masked, ta, tb, tab, cst], [], [1], count))
        assert out == [fa.atan2_model(y, x, p, k, f, r1s[i], turns) for i, (y, x) in enumerate(pairs)], turns


def test_refusals_in_the_self_test():
    from honeybadgermpc_amd._capi import HB_ERR_BAD_ARG as bad

    p, nl, count, d, m, kappa, width, k = P64, 1, 3, 5, 8, 8, 20, 16
    rnd = random.Random(5)
    v = lambda rows: _vals(rnd, p, rows * count)
    inv = [pow(2, -m, p)]
    steps = {
        SIGN_MASK: ([v(2), v(1), v(1), v(3), v(3)], [], [6]),
        ABS: ([v(6), v(3), v(3), v(3), v(1), v(1), [0, 1] * ((k + kappa) * count // 2)], [k, kappa], [1, 5]),
        SELECT_MASK: ([v(1), v(1), v(1), v(2), v(2)], [], [4]),
        SELECT: ([v(4), v(2), v(2), v(2), v(1), v(1)], [], [3]),
        FIRST: ([v(1), v(1), v(1), v(2), v(2)], [3], [4, 1]),
        LEVEL: ([v(2), v(2), inv, v(1), v(1)], [1, d, m], [2, 3]),      # level 1 of d = 5: t^3 and u^2 done, one product next
        POLY_MASK: ([v(1), v(1), inv, v(3), _vals(rnd, p, 3), [0, 1] * ((width + kappa) * count // 2)], [d, m, width, m, kappa], [1, 1]),
        ASSEMBLE: ([v(1), v(1), inv, v(2), v(1), v(1), v(1), v(1), v(1), _vals(rnd, p, 2), v(1), v(1)], [m], [2, 1]),
        FINISH: ([v(2), v(1), v(1), v(1), v(1)], [], [1]),
    }
    for what, (ops, prm, outs) in steps.items():
        assert run_atan(p, nl, what, ops, prm, outs, count)[0] == 0, what
        for i in range(len(ops)):                                       # null pointers
            assert run_atan(p, nl, what, ops[:i] + [None] + ops[i + 1:], prm, outs, count)[0] == bad, (what, i)
        for i in range(len(outs)):
            assert run_atan(p, nl, what, ops, prm, outs[:i] + [None] + outs[i + 1:], count)[0] == bad, (what, i)
        assert run_atan(p, nl, what, ops, prm, outs, -1)[0] == bad
    ops, _, outs = steps[LEVEL]
    for prm in ([1, 1, m], [1, 65, m], [1, 4, m], [0, 2, m], [2, d, m], [-1, d, m], [1, d, 0], [1, d, 63]):
        assert run_atan(p, nl, LEVEL, ops, prm, outs, count)[0] == bad, prm
    ops, _, outs = steps[POLY_MASK]
    for prm in ([1, m, width, m, kappa], [65, m, width, m, kappa], [6, m, width, m, kappa], [d, 0, width, m, kappa], [d, m, width, width, kappa], [d, m, 60, m, kappa],
                [d, m, width, m, -1]):
        assert run_atan(p, nl, POLY_MASK, ops, prm, outs, count)[0] == bad, prm
    ops, _, outs = steps[ABS]
    for prm in ([1, kappa], [k, -1], [60, kappa], [k, 60]):
        assert run_atan(p, nl, ABS, ops, prm, outs, count)[0] == bad, prm
    ops, _, outs = steps[FIRST]
    assert run_atan(p, nl, FIRST, ops, [-1], outs, count)[0] == bad and run_atan(p, nl, FIRST, ops, [256], outs, count)[0] == bad
    ops, _, outs = steps[ASSEMBLE]
    assert run_atan(p, nl, ASSEMBLE, ops, [0], outs, count)[0] == bad and run_atan(p, nl, ASSEMBLE, ops, [63], outs, count)[0] == bad
    assert run_atan(p, nl, 9, ops, [m], outs, count)[0] == bad and run_atan(p, nl, -1, ops, [m], outs, count)[0] == bad


def test_outputs_laid_over_inputs_are_refused():
    """through ctypes, where two arguments can be one buffer"""
    import ctypes

    import numpy as np

    from honeybadgermpc_amd._capi import HB_ERR_BAD_ARG, ints_to_limbs, load_library, np_ptr

    lib = load_library()
    p, nl, count, d, m, kappa, width, k = P64, 1, 4, 5, 8, 8, 20, 16
    rnd = random.Random(6)
    buf = lambda rows: np.array(ints_to_limbs([rnd.randrange(p) for _ in range(rows * count)], p, 8))
    inv = np.array(ints_to_limbs([pow(2, -m, p)], p, 8))
    two = np.array(ints_to_limbs([5, 7], p, 8))
    pl = np_ptr(ints_to_limbs([p], p + 1, 8))

    def call(what, ops, params, outs):
        ptrs = (ctypes.c_void_p * ac.SLOTS)(*([a.ctypes.data for a in ops] + [None] * (ac.SLOTS - len(ops))))
        optrs = (ctypes.c_void_p * 2)(*([a.ctypes.data for a in outs] + [None] * (2 - len(outs))))
        prm = (ctypes.c_int64 * 5)(*(list(params) + [0] * (5 - len(params))))
        return lib.hb_selftest_fxatan(pl, nl, what, ptrs, prm, optrs, count)

    # (operands, the operands that live in host memory as constants, params, outputs)
    steps = {
        SIGN_MASK: ([buf(2), buf(1), buf(1), buf(3), buf(3)], (), [], [buf(6)]),
        ABS: ([buf(6), buf(3), buf(3), buf(3), buf(1), buf(1), buf(k + kappa)], (), [k, kappa], [buf(1), buf(5)]),
        SELECT_MASK: ([buf(1), buf(1), buf(1), buf(2), buf(2)], (), [], [buf(4)]),
        SELECT: ([buf(4), buf(2), buf(2), buf(2), buf(1), buf(1)], (), [], [buf(3)]),
        FIRST: ([buf(1), buf(1), buf(1), buf(2), buf(2)], (), [3], [buf(4), buf(3)]),
        LEVEL: ([buf(2), buf(2), inv, buf(1), buf(1)], (2,), [1, d, m], [buf(2), buf(3)]),
        POLY_MASK: ([buf(1), buf(1), inv, buf(3), buf(1)[:3], buf(width + kappa)], (2,), [d, m, width, m, kappa], [buf(1), buf(1)]),
        ASSEMBLE: ([buf(1), buf(1), inv, buf(2), buf(1), buf(1), buf(1), buf(1), buf(1), two, buf(1), buf(1)], (2, 9), [m], [buf(2), buf(1)]),
        FINISH: ([buf(2), buf(1), buf(1), buf(1), buf(1)], (), [], [buf(1)]),
    }
    for what, (ops, consts, prm, outs) in steps.items():
        assert call(what, ops, prm, outs) == 0, what
        for i, op in enumerate(ops):
            if i in consts:
                continue
            for o in range(len(outs)):
                laid = list(outs)
                laid[o] = op
                assert call(what, ops, prm, laid) == HB_ERR_BAD_ARG, (what, i, o)
        if len(outs) == 2:
            assert call(what, ops, prm, [outs[0], outs[0]]) == HB_ERR_BAD_ARG, what
            big = outs[0] if len(outs[0]) >= len(outs[1]) else outs[1]
            assert call(what, ops, prm, [big, big[len(big) - 1:]] if big is outs[0] else [big[len(big) - 1:], big]) == HB_ERR_BAD_ARG, what
    # the polynomial's coefficients are read too: an output laid over them is refused
    ops, _, prm, outs = steps[POLY_MASK]
    assert call(POLY_MASK, ops, prm, [ops[4], outs[1]]) == HB_ERR_BAD_ARG and call(POLY_MASK, ops, prm, [outs[0], ops[4]]) == HB_ERR_BAD_ARG


def test_header_capi_and_wiring():
    import os

    from conftest import REPO
    from honeybadgermpc_amd import _capi

    text = open(os.path.join(REPO, "include", "hbmpc_hip.h")).read()
    names = ["hb_fxatan_sign_mask", "hb_fxatan_abs", "hb_fxatan_select_mask", "hb_fxatan_select", "hb_fxatan_first", "hb_fxatan_level", "hb_fxatan_poly_mask",
             "hb_fxatan_assemble", "hb_fxatan_finish", "hb_selftest_fxatan"]
    for name in names:
        assert f"int {name}(" in text and name in _capi.SYMBOLS, name
    for i, name in enumerate(["SIGN_MASK", "ABS", "SELECT_MASK", "SELECT", "FIRST", "LEVEL", "POLY_MASK", "ASSEMBLE", "FINISH"]):
        assert f"#define HB_FXATAN_SELFTEST_{name} {i}\n" in text and getattr(_capi, f"HB_FXATAN_SELFTEST_{name}") == i == getattr(ac, name)
    assert fa.MAX_DEGREE == 63 and "FXATAN_MAX_DEGREE = 63" in open(os.path.join(REPO, "honeybadgermpc_amd", "csrc", "hb_fxatan.hip")).read()
    assert hasattr(fx.FixedPointArray, "atan2") and hasattr(fx.FixedPointArray, "atan")

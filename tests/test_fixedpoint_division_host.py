"""CPU-only: honeybadgermpc_amd.progs.fixedpoint_division -- the prefix OR wiring on Python ints, the bodies of csrc/hb_div.hip through
hb_selftest_div against Python ints and chained into the whole division, the counts against a table worked out by hand, and the
accuracy of div_model against the exact quotient, asserted against the DERIVED bound div_error_bound."""
import itertools
import os
import random
import re
from fractions import Fraction

import pytest

import bitdec_cases as bc
import division_cases as dc
from conftest import BLS, REPO
from division_cases import (FIRST, NORM, NORM_MASK, OR_COMBINE, OR_MASK, PAIR_MASK, PRODUCT_STEP, SIGN, T_GOLD, T_RECIP, T_RESULT, TRUNC, TRUNC_STEP, ok, run_div)

from honeybadgermpc_amd.progs import bit_decomposition as bd
from honeybadgermpc_amd.progs import fixedpoint as fx
from honeybadgermpc_amd.progs import fixedpoint_division as fd


# ---- wiring ---------------------------------------------------------------------------------------------------------------------
def test_preor_counts():
    for n, triples in dc.PREOR_TRIPLES.items():
        levels = fd.preor_levels(n)
        assert levels == (0 if n == 1 else (n - 1).bit_length()) and (1 << levels) >= n > (1 << levels) // 2
        per_level = [fd.preor_level_triples(n, l) for l in range(levels)]
        assert per_level == [sum(1 for j in range(n) if (j >> l) & 1) for l in range(levels)] == [len(fd.preor_nodes(n, l)) for l in range(levels)]
        assert sum(per_level) == fd.preor_triples(n) == triples, n
        with pytest.raises(ValueError):
            fd.preor_level_triples(n, levels)
    for bad in (0, 257, -1, 2.0, True):
        with pytest.raises(ValueError):
            fd.preor_levels(bad)


@pytest.mark.parametrize("from_top", [True, False])
def test_network_is_the_prefix_or(from_top):
    def want(bits):
        n = len(bits)
        return [int(any(bits[i:])) if from_top else int(any(bits[:i + 1])) for i in range(n)]

    for n in range(1, 13):
        for bits in itertools.product((0, 1), repeat=n):
            assert dc.prefix_or_on_ints(fd, bits, from_top) == want(bits), (n, bits)
    rnd = random.Random(7)
    for n in (33, 63, 256):
        words = [0, 1, 1 << (n - 1), (1 << n) - 1] + [rnd.getrandbits(n) >> rnd.randrange(n) for _ in range(40)] + [1 << rnd.randrange(n) for _ in range(20)]
        for w in words:
            bits = [(w >> i) & 1 for i in range(n)]
            assert dc.prefix_or_on_ints(fd, bits, from_top) == want(bits), (n, w)


# ---- the bodies, one at a time ------------------------------------------------------------------------------------------------
def _rand(rnd, p, n):
    return [rnd.choice((0, 1, p - 1, rnd.randrange(p))) if i < 6 else rnd.randrange(p) for i in range(n)]


def _mask_ints(v, rows, e, count, p, width, m):
    """(masked, v + r1) of value v from the planes' values (any residues), as fxp_mask_elem's Horner sums"""
    r = sum(rows[i * count + e] << i for i in range(len(rows) // count))
    r1 = sum(rows[i * count + e] << i for i in range(m))
    return (v + (1 << (width - 1)) + r) % p, (v + r1) % p


@pytest.mark.parametrize("p, nl", bc.HOST_FIELDS, ids=bc.HOST_FIELD_IDS)
def test_each_body_on_arbitrary_residues(p, nl):
    rnd = random.Random(p % 1000)
    count = 9
    # the masked pair of one product
    x, y, ta, tb = (_rand(rnd, p, count) for _ in range(4))
    masked, = ok(run_div(p, nl, PAIR_MASK, [x, y, ta, tb], [], [2], count))
    assert masked == [(v - a) % p for v, a in zip(x, ta)] + [(v - a) % p for v, a in zip(y, tb)]
    # a level of the prefix OR, both directions
    for n in dc.OR_PLANES + (11, 63):
        for from_top in (1, 0):
            at = (lambda r: n - 1 - r) if from_top else (lambda r: r)
            for level in range(fd.preor_levels(n)):
                nodes = fd.preor_nodes(n, level)
                t = len(nodes)
                y0, ta, tb, tab, opened = _rand(rnd, p, n * count), _rand(rnd, p, t * count), _rand(rnd, p, t * count), _rand(rnd, p, t * count), _rand(rnd, p, 2 * t * count)
                masked, = ok(run_div(p, nl, OR_MASK, [y0, ta, tb], [n, level, from_top], [2 * t], count))
                y1, = ok(run_div(p, nl, OR_COMBINE, [opened, ta, tb, tab], [n, level, from_top], [y0], count))
                want = list(y0)
                for i, (j, q) in enumerate(nodes):
                    for e in range(count):
                        yj, yq = y0[at(j) * count + e], y0[at(q) * count + e]
                        assert (masked[2 * i * count + e], masked[(2 * i + 1) * count + e]) == ((yj - ta[i * count + e]) % p, (yq - tb[i * count + e]) % p)
                        want[at(j) * count + e] = (yj + yq - bc.beaver(opened[2 * i * count + e], opened[(2 * i + 1) * count + e], ta[i * count + e], tb[i * count + e],
                                                                      tab[i * count + e], p)) % p
                assert y1 == want, (n, level, from_top)                          # the nodes' new values and every other plane as it was
    # the scale step
    for n in (1, 2, 7, 33):
        for signed in (True, False):
            products = 2 if signed else 1
            x, y, u, ta, tb = _rand(rnd, p, count), _rand(rnd, p, n * count), _rand(rnd, p, count), _rand(rnd, p, products * count), _rand(rnd, p, products * count)
            masked, v = ok(run_div(p, nl, NORM_MASK, [x, y, u if signed else None, ta, tb], [n], [2 * products, 1], count))
            for e in range(count):
                ys = [y[i * count + e] for i in range(n)] + [0]
                assert v[e] == sum((ys[i] - ys[i + 1]) << (n - 1 - i) for i in range(n)) % p
                want = [(x[e] - ta[e]) % p, (v[e] - tb[e]) % p] + ([(u[e] - ta[count + e]) % p, (v[e] - tb[count + e]) % p] if signed else [])
                assert [masked[r * count + e] for r in range(2 * products)] == want
    # products to what the next open needs
    ta, tb, tab, aux, na, nb = (_rand(rnd, p, 2 * count) for _ in range(6))
    opened = _rand(rnd, p, 4 * count)
    prod = [[bc.beaver(opened[2 * r * count + e], opened[(2 * r + 1) * count + e], ta[r * count + e], tb[r * count + e], tab[r * count + e], p) for e in range(count)]
            for r in range(2)]
    cst = rnd.randrange(p)
    out, = ok(run_div(p, nl, PRODUCT_STEP, [opened, ta, tb, tab, aux], [SIGN, 1], [1], count))
    assert out == [(aux[e] - 2 * prod[0][e]) % p for e in range(count)]
    for products in (2, 1):
        vp = [(aux[e] - (2 * prod[1][e] if products == 2 else 0)) % p for e in range(count)]
        out, = ok(run_div(p, nl, PRODUCT_STEP, [opened, ta, tb, tab, aux], [NORM, products], [2], count))
        assert out == prod[0] + vp
        out, = ok(run_div(p, nl, PRODUCT_STEP, [opened, ta, tb, tab, aux, [cst], na, nb], [NORM, products], [2], count))
        assert out == [(cst - 2 * prod[0][e] - na[e]) % p for e in range(count)] + [(vp[e] - nb[e]) % p for e in range(count)]
    bits_p = p.bit_length()
    for width, m, kappa in [(8, 3, 2), (16, 8, 8), (32, 31, 8), (128, 64, 32), (200, 130, 40)]:
        if width + kappa + 1 > bits_p - 1:
            continue
        nbits = width + kappa
        rows = _rand(rnd, p, 2 * nbits * count)                                  # planes of ANY residues: the Horner sums are linear
        out0, out1 = ok(run_div(p, nl, PRODUCT_STEP, [opened, ta, tb, tab, None, [cst], None, None, rows], [FIRST, 2, width, m, kappa], [1, 2], count))
        for e in range(count):
            assert (out0[e], out1[e]) == _mask_ints(prod[1][e], rows[:nbits * count], e, count, p, width, m) and out1[count + e] == (cst - prod[0][e]) % p
        for products in (1, 2):
            out0, out1 = ok(run_div(p, nl, PRODUCT_STEP, [opened, ta, tb, tab, None, None, None, None, rows], [TRUNC, products, width, m, kappa], [products, products], count))
            for r in range(products):
                for e in range(count):
                    assert (out0[r * count + e], out1[r * count + e]) == _mask_ints(prod[r][e], rows[r * nbits * count:(r + 1) * nbits * count], e, count, p, width, m)
    # truncation to what the next open needs
    s, c, xin, e0, e1 = _rand(rnd, p, 2 * count), _rand(rnd, p, 2 * count), _rand(rnd, p, count), _rand(rnd, p, count), _rand(rnd, p, count)
    for m in (1, 2, bits_p - 2) + ((31, 32, 33, 64) if bits_p > 70 else ()):
        inv = pow(2, -m, p)
        t = [[(s[r * count + e] - c[r * count + e] % (1 << m)) * inv % p for e in range(count)] for r in range(2)]
        out, = ok(run_div(p, nl, TRUNC_STEP, [c, s, [inv]], [T_RESULT, 1, 0, m], [1], count))
        assert out == t[0]
        out, = ok(run_div(p, nl, TRUNC_STEP, [c, s, [inv], None, None, e0, e1, ta, tb], [T_RECIP, 1, 2, m], [4], count))
        assert out == [(e0[e] - ta[e]) % p for e in range(count)] + [(t[0][e] - tb[e]) % p for e in range(count)] + \
            [(e1[e] - ta[count + e]) % p for e in range(count)] + [(t[0][e] - tb[count + e]) % p for e in range(count)]
        for rows in (1, 2):
            xs = t[1] if rows == 2 else xin
            for products in (1, 2):
                out, = ok(run_div(p, nl, TRUNC_STEP, [c, s, [inv], [cst], xin if rows == 1 else None, None, None, ta, tb], [T_GOLD, rows, products, m], [2 * products], count))
                want = [(t[0][e] - ta[e]) % p for e in range(count)] + [(cst + xs[e] - tb[e]) % p for e in range(count)]
                if products == 2:
                    want += [(xs[e] - ta[count + e]) % p for e in range(count)] + [(xs[e] - tb[count + e]) % p for e in range(count)]
                assert out == want, (m, rows, products)


CHAIN = [(p, nl, shape) for p, nl in bc.HOST_FIELDS for shape in ((8, 4, 8), (12, 8, 8), (16, 8, 8), (64, 32, 32))
         if fd.div_width(shape[0], shape[1]) + shape[2] + 1 <= p.bit_length() - 1]
CHAIN_IDS = [f"{bc.HOST_FIELD_IDS[bc.HOST_FIELDS.index((p, nl))]}-k{k}-f{f}" for p, nl, (k, f, kappa) in CHAIN]


@pytest.mark.parametrize("signed", [True, False], ids=["signed", "unsigned"])
@pytest.mark.parametrize("p, nl, shape", CHAIN, ids=CHAIN_IDS)
def test_chained_bodies_reproduce_the_models(p, nl, shape, signed):
    k, f, kappa = shape
    assert {q for q, _, _ in CHAIN} == {q for q, _ in bc.HOST_FIELDS if q != 13}      # every field but the 4-bit one admits a shape
    rnd = random.Random(k * 100 + f + signed)
    count = 6 if k == 64 else 14
    a, b = dc.e2e_inputs(rnd, k, f, count, signed)
    for theta in ((None,) if k == 64 else (None, 1)):
        theta = fd.goldschmidt_iterations(k, f) if theta is None else theta
        out, (c, v), r1s = dc.chain_on_host(fd, bd, p, nl, a, b, k, f, kappa, theta, signed, rnd, all_ones=(0, 2 * theta))
        assert [(fd._centered(ci, p), fd._centered(vi, p)) for ci, vi in zip(c, v)] == [fd.norm_model(x, k, signed) for x in b]
        assert out == [fd.div_model(a[e], b[e], p, k, f, [r[e] for r in r1s], theta, signed) for e in range(count)]
        bound = fd.div_error_bound(k, f, theta)
        assert all(abs(fd._centered(o, p) - Fraction(x << f, y)) <= bound for o, x, y in zip(out, a, b))


# ---- counts ---------------------------------------------------------------------------------------------------------------------
def test_counts_reproduce_the_table_and_the_ranges_tile():
    for (k, f, kappa, theta, signed), width, planes, triples, opens in dc.TABLE:
        lay = fd.div_layout(k, f, kappa, theta, signed)
        assert (lay["theta"], lay["width"], lay["n_planes"], lay["n_triples"], lay["opens"]) == (theta, width, planes, triples, opens)
        assert fd.div_planes(k, f, kappa, theta, signed) == planes and fd.div_triples(k, f, theta, signed) == triples and fd.div_opens(k, f, theta, signed) == opens
        want_planes = ([("ltz", k + kappa)] if signed else []) + [("bit_decompose", k + kappa), ("w", width + kappa), ("y0", width + kappa)]
        want_triples = ([("ltz", 2 * k - 3), ("sign", 1)] if signed else []) + [("bit_decompose", bd.bit_triples(k - 1)), ("prefix_or", fd.preor_triples(k - 1)),
                                                                              ("norm", 2 if signed else 1), ("w", 1), ("first", 2)]
        for i in range(1, theta):
            want_planes += [(f"iter{i}.y", width + kappa), (f"iter{i}.x", width + kappa)]
            want_triples.append((f"iter{i}", 2))
        want_planes.append(("last", width + kappa))
        want_triples.append(("last", 1))
        for ranges, want, total in ((lay["planes"], want_planes, planes), (lay["triples"], want_triples, triples)):
            assert list(ranges) == [name for name, _ in want]
            at = 0
            for name, size in want:                                              # no gap, no overlap, in step order
                assert ranges[name] == (at, at + size), name
                at += size
            assert at == total
        assert fd.norm_planes(k, kappa, signed) == lay["planes"]["bit_decompose"][1] and fd.norm_triples(k, signed) == lay["triples"]["norm"][1]
        assert fd.norm_opens(k, signed) == opens - (2 * theta + 4)
    # every extra iteration: 2 triples, 2 opens, 2 (width + kappa) planes
    a, b = fd.div_layout(64, 32, 32, 5), fd.div_layout(64, 32, 32, 6)
    assert (b["n_triples"] - a["n_triples"], b["opens"] - a["opens"], b["n_planes"] - a["n_planes"]) == (2, 2, 2 * (128 + 32))
    assert fd.div_layout(64, 32, 32)["theta"] == fd.goldschmidt_iterations(64, 32) == 7


# ---- bounds and accuracy ------------------------------------------------------------------------------------------------------
def test_bound_functions():
    for k, f in [(8, 4), (12, 8), (16, 8), (24, 12), (32, 16), (64, 32), (16, 14), (6, 4)]:
        eps0 = fd.initial_residual_bound(k, f)
        assert eps0 == Fraction(858, 10000) + Fraction(1, 1 << (k - 1)) + Fraction(1 << (k - 1), 1 << (2 * f)) and eps0 < Fraction(3, 4)
        theta = fd.goldschmidt_iterations(k, f)
        assert (1 << (k - 2)) * eps0 ** (2 ** theta) <= 1 and (theta == 1 or (1 << (k - 2)) * eps0 ** (2 ** (theta - 1)) > 1)
        bounds = [fd.div_error_bound(k, f, t) for t in range(1, theta + 2)]
        assert all(x > y for x, y in zip(bounds, bounds[1:theta])) or theta == 1       # more iterations help until the rounding term takes over
        assert bounds[theta - 1] >= 2 and bounds[theta - 1] < 2 * theta + 4            # the roundings of 2 theta + 1 truncations, and one ulp
        small = fd.goldschmidt_iterations(k, f, divisor_bits=2)
        assert small <= theta and fd.initial_residual_bound(k, f, 2) < eps0
        assert fd.div_error_bound(k, f, small, divisor_bits=2) < fd.div_error_bound(k, f, small) or small == theta
        assert fd.div_width(k, f) >= 2 * k and (k != 2 * f or fd.div_width(k, f) == 2 * k)
    assert fd.goldschmidt_iterations(64, 32) == 7 and fd.goldschmidt_iterations(8, 4) == 3
    assert fd.alpha_prime(8) == int(2.9142 * 128) and fd.alpha_prime(64) == (29142 << 63) // 10000
    for k, f in [(8, 3), (8, 7), (8, 8), (300, 200), (8.0, 4), (True, 1)]:
        with pytest.raises(ValueError):
            fd.initial_residual_bound(k, f)
        with pytest.raises(ValueError):
            fd.div_layout(k, f, 8)
    for call in (lambda: fd.div_error_bound(8, 4, 0), lambda: fd.initial_residual_bound(8, 4, 8), lambda: fd.initial_residual_bound(8, 4, 0),
                 lambda: fd.div_model(1, 1, BLS, 8, 4, [0] * 6), lambda: fd.div_model(1, 1, BLS, 8, 4, [64] + [0] * 6), lambda: fd.div_model(1, 1, 65537, 8, 4, [0] * 7),
                 lambda: fd.norm_model(128, 8), lambda: fd.norm_model(-128, 8)):
        with pytest.raises(ValueError):
            call()


def test_norm_model():
    for k in (4, 8, 13):
        for b in range(-(1 << (k - 1)) + 1, 1 << (k - 1)):
            c, v = fd.norm_model(b, k)
            if b == 0:
                assert (c, v) == (0, 0)
                continue
            assert c == b * v and (1 << (k - 2)) <= c < (1 << (k - 1)) and abs(v) & (abs(v) - 1) == 0 and (v < 0) == (b < 0)
            if b > 0:
                assert fd.norm_model(b, k, signed=False) == (c, v)


def _errors(k, f, pairs, theta, draws, rnd, p=BLS):
    limits = dc.r1_limits(fd, k, f, theta)
    worst = Fraction(0)
    for a, b in pairs:
        for d in range(draws):
            r1s = [(0, (1 << m) - 1)[d] if d < 2 else rnd.randrange(1 << m) for m in limits]
            got = fd._centered(fd.div_model(a, b, p, k, f, r1s, theta), p)
            worst = max(worst, abs(got - Fraction(a << f, b)))
    return worst


def test_accuracy_exhaustive_at_8_4():
    """ALL (a, b) in range, four mask draws a pair (all-zero r1, all-ones r1, two random): the derived bound holds"""
    k, f = 8, 4
    rnd = random.Random(84)
    pairs = [(a, b) for b in range(-127, 128) if b for a in range(-128, 128) if abs(a) << f < abs(b) << (k - 2)]
    assert len(pairs) > 40000
    theta = fd.goldschmidt_iterations(k, f)
    worst = _errors(k, f, pairs, theta, 4, rnd)
    print(f"(8, 4) theta {theta}: worst {float(worst):.3f} ulps, bound {float(fd.div_error_bound(k, f, theta)):.3f}")
    assert worst <= fd.div_error_bound(k, f, theta)


@pytest.mark.parametrize("k, f", [(12, 8), (16, 8), (24, 12), (32, 16), (64, 32)])
def test_accuracy_targeted(k, f):
    rnd = random.Random(k)
    pairs = dc.targeted_pairs(rnd, k, f)
    default = fd.goldschmidt_iterations(k, f)
    for theta in sorted({1, 2, default}):
        worst = _errors(k, f, pairs, theta, 3, rnd)
        print(f"({k}, {f}) theta {theta}: worst {float(worst):.3f} ulps, bound {float(fd.div_error_bound(k, f, theta)):.3f}")
        assert worst <= fd.div_error_bound(k, f, theta)
    # a caller who knows the divisor is small spends fewer rounds under the bound the function states for that range
    bits = 2 * f - k + 3                                                         # 2^(2f-k+2) <= |b| < 2^bits: a = 2^f is admissible (reciprocal)
    small = [(rnd.choice((1, -1)) * min(dc.admissible_a(b, k, f), 1 << f), b) for b in range(1 << (bits - 1), 1 << bits)][:300]
    theta = fd.goldschmidt_iterations(k, f, divisor_bits=bits)
    assert theta <= default and (k != 2 * f or theta < default)
    assert _errors(k, f, small, theta, 3, rnd) <= fd.div_error_bound(k, f, theta, divisor_bits=bits)
    assert fd.div_model(0, 0, BLS, k, f, [0] * (2 * default + 1)) == 0 == fd.div_model(5, 0, BLS, k, f, [1] * (2 * default + 1))      # b = 0: no error, 0


# ---- the ABI ------------------------------------------------------------------------------------------------------------------
def test_abi_names_in_header_and_ctypes_table():
    from honeybadgermpc_amd import _capi

    text = open(os.path.join(REPO, "include", "hbmpc_hip.h")).read()
    for name in ("hb_div_pair_mask", "hb_div_or_mask", "hb_div_or_combine", "hb_div_norm_mask", "hb_div_product_step", "hb_div_trunc_step", "hb_selftest_div"):
        assert name in _capi.SYMBOLS and re.search(r"\b" + name + r"\(", text)
    for name, value in (("HB_DIV_SIGN", SIGN), ("HB_DIV_NORM", NORM), ("HB_DIV_FIRST", FIRST), ("HB_DIV_TRUNC", TRUNC), ("HB_DIV_T_RESULT", T_RESULT),
                        ("HB_DIV_T_RECIP", T_RECIP), ("HB_DIV_T_GOLD", T_GOLD), ("HB_DIV_SELFTEST_OR_MASK", OR_MASK), ("HB_DIV_SELFTEST_OR_COMBINE", OR_COMBINE),
                        ("HB_DIV_SELFTEST_NORM_MASK", NORM_MASK), ("HB_DIV_SELFTEST_PRODUCT_STEP", PRODUCT_STEP), ("HB_DIV_SELFTEST_TRUNC_STEP", TRUNC_STEP),
                        ("HB_DIV_SELFTEST_PAIR_MASK", PAIR_MASK)):
        assert re.search(r"#define " + name + r" " + str(value) + r"\b", text) and getattr(_capi, name) == value
    assert (fd.SIGN, fd.NORM, fd.FIRST, fd.TRUNC, fd.T_RESULT, fd.T_RECIP, fd.T_GOLD) == (SIGN, NORM, FIRST, TRUNC, T_RESULT, T_RECIP, T_GOLD)


def test_selftest_rejects_bad_arguments():
    import ctypes

    import numpy as np

    from honeybadgermpc_amd._capi import HB_ERR_BAD_ARG, ints_to_limbs, load_library, np_ptr

    p, nl, count = BLS, 4, 3
    v = [1, 2, 3]
    two, four = v * 2, v * 4
    planes = [0] * (24 * count)
    bad = [
        (OR_MASK, [v * 5, v, v], [5, 3, 1], [2]),                                # 5 planes have 3 levels
        (OR_MASK, [v * 5, v, v], [5, -1, 1], [2]),
        (OR_MASK, [v, v, v], [1, 0, 1], [2]),                                    # one plane has no level
        (OR_MASK, [v, v, v], [257, 0, 1], [2]),
        (OR_MASK, [v * 5, None, v * 2], [5, 0, 1], [4]),
        (OR_COMBINE, [v * 4, v * 2, v * 2, None], [5, 0, 1], [v * 5]),
        (NORM_MASK, [v, v, None, v, v], [0], [2, 1]),
        (NORM_MASK, [v, v * 2, None, v, None], [2], [2, 1]),
        (NORM_MASK, [v, v * 2, None, v, v], [2], [2, None]),
        (PRODUCT_STEP, [two, v, v, v, v], [9, 1], [1]),                          # no such mode
        (PRODUCT_STEP, [two, v, v, v, v], [SIGN, 2], [1]),
        (PRODUCT_STEP, [two, v, v, v, None], [SIGN, 1], [1]),
        (PRODUCT_STEP, [two, v, v, v, v, [1], v, None], [NORM, 1], [2]),         # nxt_a without nxt_b
        (PRODUCT_STEP, [two, v, v, v, v, None, v, v], [NORM, 1], [2]),           # no constant
        (PRODUCT_STEP, [two, v, v, v, v, [p], v, v], [NORM, 1], [2]),            # a constant that is no residue
        (PRODUCT_STEP, [four, two, two, two, None, [1], None, None, planes], [FIRST, 1, 16, 8, 8], [1, 2]),
        (PRODUCT_STEP, [four, two, two, two, None, [1], None, None, planes], [FIRST, 2, 16, 8, 8], [1, None]),
        (PRODUCT_STEP, [four, two, two, two, None, [1], None, None, None], [FIRST, 2, 16, 8, 8], [1, 2]),
        (PRODUCT_STEP, [two, v, v, v, None, None, None, None, planes], [TRUNC, 1, 16, 16, 8], [1, 1]),       # m < width
        (PRODUCT_STEP, [two, v, v, v, None, None, None, None, planes], [TRUNC, 1, 250, 8, 8], [1, 1]),       # no room below the modulus
        (PRODUCT_STEP, [two, v, v, v, None, None, None, None, planes], [TRUNC, 3, 16, 8, 8], [1, 1]),
        (TRUNC_STEP, [v, v, [1]], [T_RESULT, 1, 0, 0], [1]),
        (TRUNC_STEP, [v, v, [1]], [T_RESULT, 1, 0, 254], [1]),
        (TRUNC_STEP, [v, v, [1]], [T_RESULT, 2, 0, 8], [1]),
        (TRUNC_STEP, [v, v, None], [T_RESULT, 1, 0, 8], [1]),
        (TRUNC_STEP, [v, v, [p]], [T_RESULT, 1, 0, 8], [1]),
        (TRUNC_STEP, [v, v, [1], None, None, v, None, two, two], [T_RECIP, 1, 2, 8], [4]),
        (TRUNC_STEP, [v, v, [1], None, None, v, v, two, two], [T_RECIP, 1, 1, 8], [2]),
        (TRUNC_STEP, [v, v, [1], None, v, None, None, two, two], [T_GOLD, 1, 2, 8], [4]),                    # no alpha
        (TRUNC_STEP, [v, v, [1], [1], None, None, None, two, two], [T_GOLD, 1, 2, 8], [4]),                  # one row needs the kept x
        (TRUNC_STEP, [v, v, [1], [1], v, None, None, two, None], [T_GOLD, 1, 2, 8], [4]),
        (PAIR_MASK, [v, v, v, None], [], [2]),
        (7, [v], [], [1]),
    ]
    for i, (what, operands, params, outs) in enumerate(bad):
        ops = [o if o is None or len(o) != 1 or o[0] < p else None for o in operands]
        if ops != operands:                                                       # a constant at the modulus: hand it over unreduced
            arrays = [None if o is None else ints_to_limbs(list(o), p + 1, 32) for o in operands]
            ptrs = (ctypes.c_void_p * 9)(*([None if a is None else a.ctypes.data for a in arrays] + [None] * (9 - len(arrays))))
            out = np.zeros((16, 4), dtype=np.uint64)
            optrs = (ctypes.c_void_p * 2)(out.ctypes.data, out.ctypes.data)
            prm = (ctypes.c_int64 * 5)(*(list(params) + [0] * (5 - len(params))))
            rc = load_library().hb_selftest_div(np_ptr(ints_to_limbs([p], p + 1, 32)), 4, what, ptrs, prm, optrs, count)
        else:
            rc, _ = run_div(p, nl, what, operands, params, outs, count)
        assert rc == HB_ERR_BAD_ARG, i
    rc, _ = run_div(p, nl, OR_MASK, [None, None, None], [5, 0, 1], [None], 0)     # count == 0: nothing to do, nothing looked at
    assert rc == 0
    rc, _ = run_div(p, nl, TRUNC_STEP, [None, None, [1]], [T_RESULT, 1, 0, 8], [None], 0)
    assert rc == 0
    rc, _ = run_div(p, nl, OR_MASK, [v * 5, v * 2, v * 2], [5, 0, 1], [4], -1)
    assert rc == HB_ERR_BAD_ARG


def test_fixed_point_array_still_refuses_a_shared_divisor_in_div():
    """FixedPointArray.div by a public number stays as it is; the shared divisor has its own methods"""
    import asyncio

    class Ctx:
        n_limbs, modulus = 4, BLS

        def elems(self, t, *a, **kw):
            return t

    class Co:
        ctx = Ctx()

    x = fx.FixedPointArray(Co(), object())
    with pytest.raises(NotImplementedError):
        asyncio.run(x.div(x, None))
    assert callable(x.divide) and callable(x.reciprocal)

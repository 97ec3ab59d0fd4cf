"""CPU-only: honeybadgermpc_amd.progs.fixedpoint_sqrt -- the counts against a table worked out by hand, the weights against their
definition, sqrt_model against floor(sqrt(x 2^f)) and the exact inverse root within the DERIVED bounds, the steps of csrc/hb_fxsqrt.hip
through hb_selftest_fxsqrt (the rows the device runs, behind the step functions the entry points run) against Python ints and chained
into the whole protocol, bit for bit against sqrt_model, and what the steps refuse."""
import ctypes
import os
import random
import re
from fractions import Fraction
from math import isqrt

import numpy as np
import pytest

import bitdec_cases as bc
import sqrt_cases as sc
from conftest import BLS, REPO
from sqrt_cases import BOTH, FIRST, GH, NORM_MASK, OUT, R, RSQRT, SQRT, TRUNC_STEP, ok, run_sqrt

from honeybadgermpc_amd.progs import bit_decomposition as bd
from honeybadgermpc_amd.progs import fixedpoint_division as fd
from honeybadgermpc_amd.progs import fixedpoint_sqrt as fs


# ---- host functions ---------------------------------------------------------------------------------------------------------------
def test_counts_reproduce_the_table_and_the_ranges_tile():
    for (k, f, kappa, theta, what), width, planes, triples, opens in sc.TABLE:
        lay = fs.sqrt_layout(k, f, kappa, theta, what)
        assert (lay["width"], lay["n_planes"], lay["n_triples"], lay["opens"]) == (width, planes, triples, opens), (k, f, theta, what)
        assert (fs.sqrt_width(k, f, theta, what), fs.sqrt_planes(k, f, kappa, theta, what), fs.sqrt_triples(k, f, theta, what), fs.sqrt_opens(k, f, theta, what)) == \
            (width, planes, triples, opens)
        for ranges, total in ((lay["planes"], planes), (lay["triples"], triples)):
            spans = sorted(ranges.values())
            assert spans[0][0] == 0 and spans[-1][1] == total and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        shifts = fs.sqrt_shifts(k, theta, what)
        assert planes == k + kappa + len(shifts) * (width + kappa) and max(shifts) < width
    for (k, f), theta in sc.DEFAULT_THETA.items():
        assert fs.sqrt_iterations(k, f) == theta and fs.sqrt_layout(k, f)["theta"] == theta
    assert fs.sqrt_shifts(8, 2, BOTH) == [7, 19, 14, 14, 7, 8, 8, 10, 10] and fs.sqrt_shifts(8, 1, RSQRT) == [7, 19, 14, 10]
    assert (fs.SQRT, fs.RSQRT, fs.BOTH, fs.GH, fs.R, fs.OUT) == (SQRT, RSQRT, BOTH, GH, R, OUT)


def test_weights_equal_their_definition():
    for k, f in sc.SHAPES + [(64, 62)]:
        root, inverse = fs.sqrt_weights(k, f, BOTH)
        assert root == fs.sqrt_weights(k, f, SQRT) and inverse == fs.sqrt_weights(k, f, RSQRT) and len(root) == len(inverse) == k - 1
        for i in range(k - 1):
            # W = floor(2^(e / 2)) <=> W^2 <= 2^e < (W + 1)^2, e = 2 sh + 2 f +- (i + 1 - f)
            for w, e in ((root[i], 2 * fs.GUARD_BITS + 2 * f + (i + 1 - f)), (inverse[i], 2 * fs.GUARD_BITS + 2 * f - (i + 1 - f))):
                assert e >= 0 and w * w <= 1 << e < (w + 1) * (w + 1), (k, f, i)
                if e % 2 == 0:
                    assert w == 1 << (e // 2)
        assert max(root) < 1 << (fs.GUARD_BITS + (k + 2 * f) // 2 + 1)          # the result's bits and the guard bits
    for bad in (lambda: fs.sqrt_weights(8, 3), lambda: fs.sqrt_weights(8, 7), lambda: fs.sqrt_weights(8, 4, 0), lambda: fs.sqrt_weights(8, 4, 4),
                lambda: fs.sqrt_weights(300, 200), lambda: fs.sqrt_error_bound(8, 4, 0), lambda: fs.sqrt_layout(8, 4, 8, None, True)):
        with pytest.raises(ValueError):
            bad()


def test_bound_functions():
    for k, f in sc.SHAPES + [(64, 62)]:
        e0 = fs.initial_root_error(k, f)
        assert isinstance(e0, Fraction) and Fraction(267, 10000) < e0 < Fraction(27, 1000)
        # the line against C^(-1/2) on a grid of the mantissas, in exact arithmetic: (A - B C - e0)^2 C <= 1 <= (A - B C + e0)^2 C
        n = k - 1
        A, B = Fraction(fs.a_prime(k), 1 << (n + fs.Y0_SHIFT)), Fraction(fs.Y0_SLOPE, 1 << fs.Y0_SHIFT)
        grid = 1 << min(n - 1, 10)
        for step in range(grid + 1):
            C = Fraction(1, 2) + Fraction(step, 2 * grid)
            y0 = A - B * C
            assert (y0 - e0) ** 2 * C <= 1 <= (y0 + e0) ** 2 * C, (k, step)
        theta = fs.sqrt_iterations(k, f)
        root, inverse = fs.sqrt_error_bound(k, f, None, BOTH)
        assert (root, inverse) == (fs.sqrt_error_bound(k, f, theta, SQRT), fs.sqrt_error_bound(k, f, theta, RSQRT)) and isinstance(root, Fraction)
        assert 2 < root < 7 and 1 < inverse < 4                                 # below the division's 11.8 at (64, 32): roundings add, none is amplified
        assert fs.sqrt_error_bound(k, f, theta + 1, RSQRT) > inverse            # the roundings add up with theta once the iteration has converged
    assert fs.sqrt_error_bound(64, 32, 3, SQRT) > 100                           # one iteration short: hundreds of ulps


# ---- the model against the real roots ----------------------------------------------------------------------------------------------
def _errors(k, f, theta, what, xs, r1_sets):
    """-> the largest |model - floor(sqrt(x 2^f))| and |model - 2^(3f/2) / sqrt(x)| (in contract) over xs and the r1 sets"""
    worst = [Fraction(0), Fraction(0)]
    for x in xs:
        for r1s in r1_sets:
            got = fs.sqrt_model(x, BLS, k, f, r1s, theta, what)
            got = got if what == BOTH else (got, got)
            if what & SQRT:
                worst[0] = max(worst[0], Fraction(abs(got[0] - isqrt(x << f))))
            if what & RSQRT:
                if x == 0:
                    assert got[1] == 0
                elif sc.in_rsqrt_contract(x, k, f):
                    worst[1] = max(worst[1], abs(got[1] - sc.exact_rsqrt(x, f)))
    return worst


@pytest.mark.parametrize("k, f", sc.SHAPES, ids=[f"k{k}-f{f}" for k, f in sc.SHAPES])
def test_model_within_the_derived_bounds(k, f):
    rnd = random.Random(k * 100 + f)
    xs = sc.operands(rnd, k, f)
    assert {(x.bit_length() - f) & 1 for x in xs if x} == {0, 1}                # both parities of e + 1 - f
    theta = fs.sqrt_iterations(k, f)
    root, inverse = fs.sqrt_error_bound(k, f, theta, BOTH)
    for what in (BOTH, SQRT, RSQRT):
        worst = _errors(k, f, theta, what, xs, sc.r1_sets(rnd, fs.sqrt_shifts(k, theta, what)))
        print(f"(k, f) = ({k}, {f}), theta = {theta}, what = {what}: worst {float(worst[0]):.3f} of {float(root):.3f}, {float(worst[1]):.3f} of {float(inverse):.3f} ulps")
        assert worst[0] <= root and worst[1] <= inverse, (what, worst)
    assert fs.sqrt_model(0, BLS, k, f, [0] * len(fs.sqrt_shifts(k, theta, BOTH)), theta, BOTH) == (0, 0)


def test_exhaustive_at_8_4():
    k, f = 8, 4
    for theta in (1, 2):
        root, inverse = fs.sqrt_error_bound(k, f, theta, BOTH)
        limits = fs.sqrt_shifts(k, theta, BOTH)
        worst = _errors(k, f, theta, BOTH, range(1 << (k - 1)), [[0] * len(limits), [(1 << m) - 1 for m in limits]])
        assert worst[0] <= root and worst[1] <= inverse, (theta, worst)


def test_one_iteration_fewer_violates_the_bound_at_64_32():
    """the default is no higher than it has to be: at theta = sqrt_iterations - 1 a listed operand is off by more than the bound"""
    k, f = 64, 32
    theta = fs.sqrt_iterations(k, f) - 1
    rnd = random.Random(6432)
    limits = fs.sqrt_shifts(k, theta, BOTH)
    worst = _errors(k, f, theta, BOTH, sc.operands(rnd, k, f, extra=0), [[0] * len(limits)])
    root, inverse = fs.sqrt_error_bound(k, f, None, BOTH)
    assert worst[0] > root and worst[1] > inverse, worst


def test_model_refuses():
    k, f = 8, 4
    limits = fs.sqrt_shifts(k, 1, SQRT)
    good = [0] * len(limits)
    assert abs(fs.sqrt_model(16, BLS, k, f, good, 1, SQRT) - 16) <= fs.sqrt_error_bound(k, f, 1, SQRT)        # sqrt(1.0)
    for bad in (lambda: fs.sqrt_model(16, BLS, k, f, good[:-1], 1, SQRT), lambda: fs.sqrt_model(16, BLS, k, f, [1 << limits[0]] + good[1:], 1, SQRT),
                lambda: fs.sqrt_model(16, BLS, k, f, good, 1, BOTH), lambda: fs.sqrt_model(1 << 7, BLS, k, f, good, 1, SQRT),
                lambda: fs.sqrt_model(-1, BLS, k, f, good, 1, SQRT),                # a negative x is outside the contract
                lambda: fs.sqrt_model(16, 257, k, f, good, 1, SQRT),                # a width the modulus has no room for
                lambda: fs.sqrt_model(16, BLS, k, f, good, 0, SQRT), lambda: fs.sqrt_model(16, BLS, k, 3, good, 1, SQRT)):
        with pytest.raises(ValueError):
            bad()


# ---- the steps on the host ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p, nl", bc.HOST_FIELDS, ids=bc.HOST_FIELD_IDS)
def test_each_body_on_arbitrary_residues(p, nl):
    rnd = random.Random(p % 1009)
    count = 5
    vec = lambda rows=1: [rnd.randrange(p) for _ in range(rows * count)]
    row = lambda v, r: v[r * count:(r + 1) * count]
    for n in (1, 2, 3, 7, 8, 15, 22, 63):
        for sets in (1, 2):
            x, y, w, ta, tb = vec(), vec(n), [rnd.randrange(p) for _ in range(sets * n)], vec(), vec()
            if n == 7:
                w[0], w[-1] = p - 1, p - 1
                y[:count] = [p - 1] * count
            masked, kept = ok(run_sqrt(p, nl, NORM_MASK, [x, y, w, ta, tb], [n, sets], [2, 1 + sets], count))
            for e in range(count):
                col = [row(y, i)[e] for i in range(n)] + [0]
                v = sum((col[i] - col[i + 1]) << (n - 1 - i) for i in range(n)) % p
                assert row(kept, 0)[e] == v and (row(masked, 0)[e], row(masked, 1)[e]) == ((x[e] - ta[e]) % p, (v - tb[e]) % p), (n, e)
                for s in range(sets):
                    assert row(kept, 1 + s)[e] == sum(w[s * n + i] * col[i] for i in range(n)) % p, (n, s, e)
    opened, ta, tb, na, nb = vec(2), vec(), vec(), vec(), vec()
    tab = [a * b % p for a, b in zip(ta, tb)]
    for a, b in ((rnd.randrange(p), rnd.randrange(p)), (p - 1, p - 1), (0, 53 % p)):
        masked, h = ok(run_sqrt(p, nl, FIRST, [opened, ta, tb, tab, [a], [b], na, nb], [], [2, 1], count))
        for e in range(count):
            c = bc.beaver(opened[e], opened[count + e], ta[e], tb[e], tab[e], p)
            assert h[e] == (a - b * c) % p and (masked[e], masked[count + e]) == ((c - na[e]) % p, (h[e] - nb[e]) % p)
    bits = p.bit_length()
    for m in sorted({1, 2, min(8, bits - 2), bits - 2}):
        inv = pow(2, -m, p)
        s, c, kept, ta, tb = vec(2), vec(2), vec(2), vec(2), vec(2)
        t = [[(s[r * count + e] - c[r * count + e] % (1 << m)) * inv % p for e in range(count)] for r in range(2)]
        cst = rnd.randrange(p)
        for rows in (1, 2):
            masked, gh = ok(run_sqrt(p, nl, TRUNC_STEP, [c[:rows * count], s[:rows * count], [inv], None, kept[:count] if rows == 1 else None, ta[:count], tb[:count]],
                                     [GH, rows, BOTH, m], [2, 2], count))
            h = t[1] if rows == 2 else kept[:count]
            assert gh == t[0] + h and masked == [(g - a) % p for g, a in zip(t[0], ta)] + [(v - b) % p for v, b in zip(h, tb)], (m, rows)
        r = [(cst - v) % p for v in t[0]]
        for which in (SQRT, RSQRT, BOTH):
            products = 2 if which == BOTH else 1
            masked, = ok(run_sqrt(p, nl, TRUNC_STEP, [c[:count], s[:count], [inv], [cst], kept, ta[:products * count], tb[:products * count]], [R, 1, which, m],
                                  [2 * products], count))
            firsts = [row(kept, 0), row(kept, 1)] if which == BOTH else [row(kept, 0 if which == SQRT else 1)]
            want = []
            for q, first in enumerate(firsts):
                want += [(g - a) % p for g, a in zip(first, row(ta, q))] + [(v - b) % p for v, b in zip(r, row(tb, q))]
            assert masked == want, (m, which)
            masked, = ok(run_sqrt(p, nl, TRUNC_STEP, [c[:products * count], s[:products * count], [inv], None, kept[:products * count], ta[:products * count],
                                                      tb[:products * count]], [OUT, products, which, m], [2 * products], count))
            want = []
            for q in range(products):
                want += [(g - a) % p for g, a in zip(t[q], row(ta, q))] + [(v - b) % p for v, b in zip(row(kept, q), row(tb, q))]
            assert masked == want, (m, which)


CHAIN = [(p, nl, shape) for p, nl in bc.HOST_FIELDS for shape in ((8, 4, 8), (16, 8, 8), (64, 32, 32)) if fs.sqrt_width(*shape[:2], None, BOTH) + shape[2] + 2 <= p.bit_length() - 1]
CHAIN_IDS = [f"{bc.HOST_FIELD_IDS[bc.HOST_FIELDS.index((p, nl))]}-k{k}-f{f}" for p, nl, (k, f, kappa) in CHAIN]


@pytest.mark.parametrize("what", [SQRT, RSQRT, BOTH], ids=["sqrt", "rsqrt", "both"])
@pytest.mark.parametrize("p, nl, shape", CHAIN, ids=CHAIN_IDS)
def test_chained_bodies_reproduce_the_model(p, nl, shape, what):
    """the whole chain through the host bodies equals sqrt_model bit for bit for the r1 it was dealt, all-ones r1 included"""
    assert {q for q, _, _ in CHAIN} == {q for q, _ in bc.HOST_FIELDS if q != 13}
    k, f, kappa = shape
    rnd = random.Random(p % 1013 + k + what)
    theta = fs.sqrt_iterations(k, f)
    count = 6 if k < 64 else 3
    xs = sc.e2e_inputs(rnd, k, f, 10)
    xs = [xs[0], xs[1]] + rnd.sample(xs[2:], count - 2)
    n_trunc = len(fs.sqrt_shifts(k, theta, what))
    outs, r1s = sc.chain_on_host(fs, fd, bd, p, nl, xs, k, f, kappa, theta, what, rnd, all_ones=(0, 1, n_trunc - 1))
    for e, x in enumerate(xs):
        want = fs.sqrt_model(x, p, k, f, [r[e] for r in r1s], theta, what)
        want = want if what == BOTH else (want,)
        assert tuple(o[e] for o in outs) == want, (e, x)
    assert all(o[0] == 0 for o in outs)                                      # x = 0


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_abi_names_in_header_and_ctypes_table():
    from honeybadgermpc_amd import _capi

    text = open(os.path.join(REPO, "include", "hbmpc_hip.h")).read()
    for name in ("hb_fxsqrt_norm_mask", "hb_fxsqrt_first", "hb_fxsqrt_trunc_step", "hb_selftest_fxsqrt"):
        assert name in _capi.SYMBOLS and re.search(r"\b" + name + r"\(", text)
    for name, value in (("HB_FXSQRT_GH", GH), ("HB_FXSQRT_R", R), ("HB_FXSQRT_OUT", OUT), ("HB_FXSQRT_SELFTEST_NORM_MASK", NORM_MASK), ("HB_FXSQRT_SELFTEST_FIRST", FIRST),
                        ("HB_FXSQRT_SELFTEST_TRUNC_STEP", TRUNC_STEP)):
        assert re.search(r"#define " + name + r" " + str(value) + r"\b", text) and getattr(_capi, name) == value


def test_selftest_rejects_bad_arguments_and_overlaps():
    from honeybadgermpc_amd._capi import HB_ERR_BAD_ARG, ints_to_limbs, load_library, np_ptr

    p, nl, count = BLS, 4, 3
    v = [1, 2, 3]
    two = v * 2
    bad = [
        (NORM_MASK, [v, v * 2, v[:2], v, v], [0, 1], [2, 2]),
        (NORM_MASK, [v, v * 2, v[:2], v, v], [257, 1], [2, 2]),
        (NORM_MASK, [v, v * 2, v[:2], v, v], [2, 0], [2, 2]),
        (NORM_MASK, [v, v * 2, v[:2], v, v], [2, 3], [2, 2]),
        (NORM_MASK, [v, v * 2, None, v, v], [2, 1], [2, 2]),
        (NORM_MASK, [v, v * 2, v[:2], v, None], [2, 1], [2, 2]),
        (NORM_MASK, [v, v * 2, v[:2], v, v], [2, 1], [2, None]),
        (FIRST, [two, v, v, v, None, [1], v, v], [], [2, 1]),
        (FIRST, [two, v, v, v, [1], [1], v, None], [], [2, 1]),
        (FIRST, [two, v, v, v, [1], [1], v, v], [], [2, None]),
        (FIRST, [two, v, v, v, [p], [1], v, v], [], [2, 1]),                      # a constant that is no residue
        (FIRST, [two, v, v, v, [1], [p], v, v], [], [2, 1]),
        (TRUNC_STEP, [v, v, [1], None, v, v, v], [3, 1, BOTH, 8], [2, 2]),        # no such mode
        (TRUNC_STEP, [v, v, [1], None, v, v, v], [GH, 3, BOTH, 8], [2, 2]),
        (TRUNC_STEP, [v, v, [1], None, v, v, v], [GH, 1, SQRT, 8], [2, 2]),
        (TRUNC_STEP, [v, v, [1], None, None, v, v], [GH, 1, BOTH, 8], [2, 2]),    # one row needs the kept h
        (TRUNC_STEP, [v, v, [1], None, v, v, v], [GH, 1, BOTH, 8], [2, None]),
        (TRUNC_STEP, [v, v, [1], None, v, v, v], [GH, 1, BOTH, 0], [2, 2]),
        (TRUNC_STEP, [v, v, [1], None, v, v, v], [GH, 1, BOTH, 254], [2, 2]),     # m outside 0 < m <= bits(p) - 2
        (TRUNC_STEP, [v, v, None, None, v, v, v], [GH, 1, BOTH, 8], [2, 2]),
        (TRUNC_STEP, [v, v, [p], None, v, v, v], [GH, 1, BOTH, 8], [2, 2]),
        (TRUNC_STEP, [v, v, [1], None, two, v, v], [R, 1, SQRT, 8], [2]),         # no constant
        (TRUNC_STEP, [v, v, [1], [p], two, v, v], [R, 1, SQRT, 8], [2]),
        (TRUNC_STEP, [two, two, [1], [1], two, v, v], [R, 2, SQRT, 8], [2]),
        (TRUNC_STEP, [v, v, [1], [1], two, v, v], [R, 1, 0, 8], [2]),
        (TRUNC_STEP, [v, v, [1], [1], two, v, v], [R, 1, 4, 8], [2]),
        (TRUNC_STEP, [v, v, [1], [1], None, v, v], [R, 1, SQRT, 8], [2]),
        (TRUNC_STEP, [v, v, [1], None, v, v, v], [OUT, 1, BOTH, 8], [2]),         # BOTH is two rows
        (TRUNC_STEP, [two, two, [1], None, two, two, two], [OUT, 2, RSQRT, 8], [4]),
        (TRUNC_STEP, [v, v, [1], None, None, v, v], [OUT, 1, SQRT, 8], [2]),
        (5, [v], [], [1]),
    ]
    lib = load_library()
    modulus = np_ptr(ints_to_limbs([p], p + 1, 32))
    for i, (what, operands, params, outs) in enumerate(bad):
        if any(o is not None and len(o) == 1 and o[0] >= p for o in operands):    # a constant at the modulus: hand it over unreduced
            arrays = [None if o is None else ints_to_limbs(list(o), p + 1, 32) for o in operands]
            ptrs = (ctypes.c_void_p * 8)(*([None if a is None else a.ctypes.data for a in arrays] + [None] * (8 - len(arrays))))
            out = np.zeros((32, 4), dtype=np.uint64)
            optrs = (ctypes.c_void_p * 2)(out.ctypes.data, out[16:].ctypes.data)
            prm = (ctypes.c_int64 * 4)(*(list(params) + [0] * (4 - len(params))))
            rc = lib.hb_selftest_fxsqrt(modulus, 4, what, ptrs, prm, optrs, count)
        else:
            rc, _ = run_sqrt(p, nl, what, operands, params, outs, count)
        assert rc == HB_ERR_BAD_ARG, i
    rc, _ = run_sqrt(p, nl, NORM_MASK, [None, None, v[:2], None, None], [2, 1], [None, None], 0)     # count == 0: nothing to do
    assert rc == 0
    rc, _ = run_sqrt(p, nl, TRUNC_STEP, [None, None, [1], None, None, None, None], [GH, 1, BOTH, 8], [None, None], 0)
    assert rc == 0
    rc, _ = run_sqrt(p, nl, FIRST, [two, v, v, v, [1], [1], v, v], [], [2, 1], -1)
    assert rc == HB_ERR_BAD_ARG

    # an output laid over an input, or over the other output, is refused as the entry points refuse it: every operand in ONE buffer
    eb = 8 * nl * count                                                           # bytes a row
    buf = np.zeros((64 * count, nl), dtype=np.uint64)
    at = lambda r: buf.ctypes.data + r * eb
    one = ints_to_limbs([1], p, 32)

    def call(what, params, ops, outs):
        ptrs = (ctypes.c_void_p * 8)(*(list(ops) + [None] * (8 - len(ops))))
        optrs = (ctypes.c_void_p * 2)(*(list(outs) + [None] * (2 - len(outs))))
        return lib.hb_selftest_fxsqrt(modulus, nl, what, ptrs, (ctypes.c_int64 * 4)(*(list(params) + [0] * (4 - len(params)))), optrs, count)

    c1 = one.ctypes.data
    # NORM_MASK, n = 2, sets = 2: x 0, y 1..2, weights 3, ta 4, tb 5; masked 10..11, kept 12..14
    ops = [at(0), at(1), at(3), at(4), at(5)]
    assert call(NORM_MASK, [2, 2], ops, [at(10), at(12)]) == 0
    for outs in ([at(0), at(12)], [at(2) - eb // 2, at(12)], [at(4), at(12)], [at(10), at(5)], [at(10), at(11)], [at(10), at(8)], [at(12), at(12)], [at(3), at(12)],
                 [at(10), at(1)]):
        assert call(NORM_MASK, [2, 2], ops, outs) == HB_ERR_BAD_ARG, outs
    # FIRST: opened 0..1, ta 2, tb 3, tab 4, nxt 5, 6; masked 10..11, h 12
    ops = [at(0), at(2), at(3), at(4), c1, c1, at(5), at(6)]
    assert call(FIRST, [], ops, [at(10), at(12)]) == 0
    for outs in ([at(1), at(12)], [at(10), at(11)], [at(10), at(6)], [at(6), at(12)], [at(10), at(4)], [at(9), at(10)]):
        assert call(FIRST, [], ops, outs) == HB_ERR_BAD_ARG, outs
    # TRUNC_STEP: opened 0..1, s 2..3, kept 4..5, ta 6..7, tb 8..9; masked 10..13, kept_out 14..15
    ops = [at(0), at(2), c1, c1, at(4), at(6), at(8)]
    for mode, rows, which, outs_ok, bad_outs in ((GH, 1, BOTH, [at(10), at(14)], ([at(0), at(14)], [at(10), at(11)], [at(10), at(4)], [at(3) - eb, at(14)], [at(7) - eb, at(14)])),
                                                 (GH, 2, BOTH, [at(10), at(14)], ([at(1), at(14)], [at(10), at(3)])),
                                                 (R, 1, BOTH, [at(10), None], ([at(5), None], [at(9), None], [at(7) - 3 * eb, None])),
                                                 (OUT, 2, BOTH, [at(10), None], ([at(1), None], [at(5), None], [at(3), None]))):
        assert call(TRUNC_STEP, [mode, rows, which, 8], ops, outs_ok) == 0, mode
        for outs in bad_outs:
            assert call(TRUNC_STEP, [mode, rows, which, 8], ops, outs) == HB_ERR_BAD_ARG, (mode, outs)
    assert call(TRUNC_STEP, [GH, 2, BOTH, 8], ops, [at(10), at(4)]) == 0             # two rows: the kept h is not looked at


def test_protocol_refuses_before_anything_is_opened():
    """the checks of the coroutines that need no device: a width the modulus has no room for, a bad k / f / theta / kappa"""
    for k, f, kappa, theta, what in ((8, 3, 8, None, SQRT), (8, 7, 8, None, SQRT), (8, 4, 8, 0, SQRT), (8, 4, 8, None, 5), (8, 4, 1.5, None, SQRT)):
        with pytest.raises(ValueError):
            fs.sqrt_layout(k, f, kappa, theta, what)
    from honeybadgermpc_amd.progs.fixedpoint import check_params

    with pytest.raises(ValueError):                                              # (64, 32, 32) over a 64-bit field: 140 + 32 + 1 bits do not fit
        check_params(bc.P64, fs.sqrt_width(64, 32), 63, 32)

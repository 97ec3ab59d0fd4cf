"""CPU-only: honeybadgermpc_amd.progs.fixedpoint_exp -- the counts and the tiling of the layout ranges against a table worked out by hand,
the tables against their definition, exp2_model and exp_model against integer enclosures of the exact values within the DERIVED bounds
(every in-contract input at (8, 4) and (16, 8), both extremes of every rounding), the steps of csrc/hb_fxexp.hip through
hb_selftest_fxexp (the rows the device runs, behind the step functions the entry points run) against Python ints and chained into the
whole protocol, bit for bit against the models, and what the steps refuse."""
import ctypes
import os
import random
import re
from fractions import Fraction

import numpy as np
import pytest

import bitdec_cases as bc
import exp_cases as ec
from conftest import BLS, REPO
from exp_cases import EXTRA, FINISH_LOOKUP_MASK, PRODUCTS_TRUNC, TREE_STEP, ok, run_exp

from honeybadgermpc_amd.progs import bit_decomposition as bd
from honeybadgermpc_amd.progs import demux as dx
from honeybadgermpc_amd.progs import fixedpoint_exp as fe

WORST = {}                                                        # (what, k, f, g) -> the largest error seen, in ulps (printed with -s)


# ---- host functions ---------------------------------------------------------------------------------------------------------------
def test_counts_reproduce_the_table_and_the_ranges_tile():
    for (k, f, kappa, g), groups, tree, planes, triples, opens, rows in ec.TABLE:
        lay = fe.exp2_layout(k, f, kappa, g)
        assert (lay["groups"], lay["tree"], lay["n_planes"], lay["n_triples"], lay["opens"]) == (groups, tree, planes, triples, opens), (k, f, g)
        assert lay["demux_rows"] == rows == fe.exp2_demux_rows(k, f, g)
        assert (fe.exp2_groups(k, f, g), fe.exp2_planes(k, f, kappa, g), fe.exp2_triples(k, f, g), fe.exp2_opens(k, f, g)) == (groups, planes, triples, opens)
        assert lay["width"] == fe.exp2_width(k) == 2 * (k + 2) + 2 and lay["bits"] == k and lay["g"] == g
        assert (lay["demux_opened"], lay["demux_products"]) == (sum(o for lv in rows for _, o, _ in lv), sum(q for lv in rows for _, _, q in lv))
        for ranges, total in ((lay["planes"], planes), (lay["triples"], triples)):
            spans = sorted(ranges.values())
            assert spans[0][0] == 0 and spans[-1][1] == total and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        assert fe.exp2_shifts(k, f, g) == [k + 2] * len(groups) and planes == k + 1 + kappa + len(groups) * (lay["width"] + kappa)
        widths = [w for _, w in groups] + [(k - 3).bit_length() + 1]
        assert sum(w for _, w in groups) == f and max(w for _, w in groups) <= g and max(widths[:-1]) - min(widths[:-1]) <= 1
        assert fe.exp2_group_bits(k, f) == list(range(f, f + widths[-1] - 1)) + [k - 1]
    for (k, f, kappa, g), planes, triples, opens in ec.EXP_TABLE:
        lay = fe.exp_layout(k, f, kappa, g)
        assert (lay["n_planes"], lay["n_triples"], lay["opens"], lay["bits"]) == (planes, triples, opens, k + 1)
        assert (fe.exp_planes(k, f, kappa, g), fe.exp_triples(k, f, g), fe.exp_opens(k, f, g)) == (planes, triples, opens)
        assert lay["planes"]["exponent"] == (0, lay["width"] + kappa) and fe.exp2_group_bits(k, f, k + 1)[-1] == k
    # the trade g makes can be counted: at (64, 32) g = 8 has the fewest opens, g = 4 two more for about a quarter of the demultiplexer triples
    a, b = fe.exp2_layout(64, 32, 32, 8), fe.exp2_layout(64, 32, 32, 4)
    assert (a["opens"], b["opens"], a["demux_products"], b["demux_products"]) == (17, 19, 4 * 304 + 164, 8 * 24 + 164)
    assert fe.default_group_width(64, 32) == 8 and fe.exp2_layout(64, 32)["g"] == 8
    assert all(fe.exp2_opens(64, 32, g) >= 17 for g in range(1, 13)) and all(fe.exp2_opens(64, 32, g) > 17 for g in range(1, 8))


def test_tables_equal_their_definition():
    for (k, f, kappa, g), groups, *_ in ec.TABLE:
        s, mi = k + fe.GUARD_BITS, (k - 3).bit_length()
        tables = fe.exp2_tables(k, f, g)
        assert len(tables) == len(groups) + 1
        for (o, w), table in zip(groups, tables):
            assert len(table) == 1 << w and table[0] == 1 << s
            for j, t in enumerate(table):
                lo, hi = ec.exp2_enclosure(j << o, f)                     # 2^(j 2^(o-f)) 2^(f + EXTRA)
                assert ((2 * t - 1) << (f + EXTRA)) <= (2 * lo) << s and (2 * hi) << s <= ((2 * t + 1) << (f + EXTRA)), (k, f, g, o, j)
                assert t.bit_length() <= s + 1
        assert tables[-1] == [1 << j if j < k - 2 else 0 for j in range(1 << mi)] + [0] * (1 << mi)
    L, fl = fe.exponent_factor(64)
    assert fl == 64 and abs(L * 10 ** 18 - 1442695040888963407 * (1 << 64)) < 10 ** 18 + (1 << 64)   # log2(e) = 1.442695040888963407..., 18 places
    for bad in (lambda: fe.exp2_tables(8, 4, 0), lambda: fe.exp2_tables(8, 4, 13), lambda: fe.exp2_tables(8, 5, 2), lambda: fe.exp2_tables(3, 1, 1),
                lambda: fe.exp2_tables(8, 0, 1), lambda: fe.exp2_groups(8, 4, True), lambda: fe.exp2_layout(8, 4, 1.5, 2), lambda: fe.exp2_layout(300, 32, 32, 8)):
        with pytest.raises(ValueError):
            bad()


def _check(what, model, bound, enclosure, xs, p, k, f, g, limits):
    worst = 0
    for x in xs:
        enc = enclosure(x, f)
        b = bound(x)
        for r1s in ec.r1_extremes(limits):
            got = model(x, p, k, f, r1s, g)
            assert got < 1 << (k - 1)
            err = ec.error_ulps(got, enc)
            assert err <= b * (1 << EXTRA), (what, k, f, g, x, float(Fraction(err, 1 << EXTRA)), float(b))
            worst = max(worst, err)
    WORST[(what, k, f, g)] = float(Fraction(worst, 1 << EXTRA))
    print(f"{what} ({k}, {f}, g = {g}): largest error {WORST[(what, k, f, g)]:.4f} ulps over {len(xs)} inputs")


@pytest.mark.parametrize("k, f, g", [(8, 4, 2), (8, 4, None), (16, 8, 3), (16, 8, None)], ids=["k8-f4-g2", "k8-f4", "k16-f8-g3", "k16-f8"])
def test_exp2_model_within_the_bound_for_every_input(k, f, g):
    """EVERY in-contract x, every truncation at r1 = 0 and again at the all-ones r1"""
    bound = fe.exp2_error_bound(k, f, g)
    assert isinstance(bound, Fraction) and 1 < bound < 2
    xs = [x for x in range(-(1 << (k - 1)), 1 << (k - 1)) if ec.in_exp2_contract(x, k, f)]
    assert len(xs) == (1 << (k - 1)) + ((k - 2 - f) << f)
    _check("exp2", fe.exp2_model, lambda x: bound, ec.exp2_enclosure, xs, BLS, k, f, g, fe.exp2_shifts(k, f, g))
    for x in xs:                                                          # below -f: exactly 0; at -f: one ulp or, rounded up, two
        if x < -(f << f):
            assert fe.exp2_model(x, BLS, k, f, [0] * len(fe.exp2_shifts(k, f, g)), g) == 0


@pytest.mark.parametrize("g", [4, 5, 6, 7, 8, None])
@pytest.mark.parametrize("k, f", [(64, 32), (64, 40)], ids=["k64-f32", "k64-f40"])
def test_exp2_model_within_the_bound_on_seeded_inputs(k, f, g):
    rnd = random.Random(1000 * k + 10 * f + (g or 0))
    xs = ec.operands(fe, rnd, k, f, g, False, 300)
    bound = fe.exp2_error_bound(k, f, g)
    _check("exp2", fe.exp2_model, lambda x: bound, ec.exp2_enclosure, xs, BLS, k, f, g, fe.exp2_shifts(k, f, g))
    z = [0] * len(fe.exp2_shifts(k, f, g))
    assert fe.exp2_model(-(f << f), BLS, k, f, z, g) == 1 and fe.exp2_model(-(f << f) - 1, BLS, k, f, z, g) == 0 and fe.exp2_model(-(1 << (k - 1)), BLS, k, f, z, g) == 0
    assert fe.exp2_model(0, BLS, k, f, z, g) == 1 << f and fe.exp2_model(3 << f, BLS, k, f, z, g) == 8 << f
    # the issue's rough count, (1.5 G - 1) 2^(k-2-s) + 2, measures against the floor; against the exact real it is one less, and the products of the
    # relative errors add next to nothing
    rough = Fraction(3 * len(fe.exp2_groups(k, f, g)) - 2, 2) / (1 << (fe.GUARD_BITS + 2)) + 2
    assert rough - 1 <= bound < rough - 1 + Fraction(1, 1 << 40)


@pytest.mark.parametrize("k, f, g", [(8, 4, 2), (16, 8, 3), (64, 32, 8), (64, 32, 4), (64, 40, None)], ids=["k8-f4", "k16-f8", "k64-f32-g8", "k64-f32-g4", "k64-f40"])
def test_exp_model_within_its_bound(k, f, g):
    rnd = random.Random(77 * k + f)
    if k <= 8:
        xs = [x for x in range(-(1 << (k - 1)), 1 << (k - 1)) if ec.in_exp_contract(x, k, f)]
    else:
        xs = ec.operands(fe, rnd, k, f, g, True, 200)
    limits = [k] + fe.exp2_shifts(k, f, g)
    _check("exp", fe.exp_model, lambda x: fe.exp_error_bound(k, f, x, g), ec.exp_enclosure, xs, BLS, k, f, g, limits)
    # the bound is a function of the magnitude: about ln 2 2^-f of the result where the result is large, a few ulps where it is small
    top = ec.largest_in_contract(k, f, True)
    assert fe.exp_error_bound(k, f, -(1 << (k - 1)), g) < 4 and fe.exp_error_bound(k, f, top, g) > Fraction(1 << (k - 3), 1 << f)
    assert fe.exp_model(0, BLS, k, f, [0] * len(limits), g) == 1 << f


def test_models_refuse():
    z = [0, 0]
    for bad in (lambda: fe.exp2_model(0, BLS, 8, 4, [0], 2), lambda: fe.exp2_model(0, BLS, 8, 4, [0, 1 << 10], 2), lambda: fe.exp2_model(128, BLS, 8, 4, z, 2),
                lambda: fe.exp2_model(-129, BLS, 8, 4, z, 2), lambda: fe.exp2_model(0, BLS, 8, 4, z, 13), lambda: fe.exp2_model(0, 2 ** 31 - 1, 16, 8, [0] * 3, 3),
                lambda: fe.exp_model(0, BLS, 8, 4, z, 2), lambda: fe.exp_model(0, BLS, 8, 4, [1 << 8, 0, 0], 2), lambda: fe.exp_error_bound(8, 4, 128, 2),
                lambda: fe.exp2_error_bound(8, 5, 2)):
        with pytest.raises(ValueError):
            bad()
    assert fe.exp2_model(BLS - 1, BLS, 8, 4, z, 2) == fe.exp2_model(-1, BLS, 8, 4, z, 2)              # a residue or a signed int


# ---- the rows on the host ---------------------------------------------------------------------------------------------------------
def _rows(rnd, p, rows, count):
    return [[rnd.randrange(p) for _ in range(count)] for _ in range(rows)]


@pytest.mark.parametrize("p, nl", bc.HOST_FIELDS, ids=bc.HOST_FIELD_IDS)
def test_each_body_on_arbitrary_residues(p, nl):
    rnd = random.Random(p % 997)
    count = 5
    # finish, lookup and mask: every merge and a group of one bit, one to three groups a launch, tables of arbitrary residues and of short constants
    shapes = ec.MERGES + [(1, 0), (3, 2), (8, 4)]
    for n_groups in (1, 2, 3):
        for trial in range(len(shapes)):
            chosen = [shapes[(trial + i) % len(shapes)] for i in range(n_groups)]
            if sum(1 << (wl + wh) for wl, wh in chosen) > 600 and p >> 64:
                chosen = chosen[:1]
            short = trial & 1
            bits, opened, ta, tab, tables, desc, want = _rows(rnd, p, 3, count), [], [], [], [], [], {}
            pairs, kept_rows = 2, 6
            slots = rnd.sample(range(kept_rows), len(chosen))
            for (wl, wh), slot in zip(chosen, slots):
                entries = 1 << (wl + wh)
                top = min(p, 1 << 67) if short else p
                table = [0 if rnd.random() < 0.3 else rnd.randrange(top) for _ in range(entries)]
                if wh == 0:
                    plane = rnd.randrange(3)
                    desc += [1, 0, plane, 0, len(tables), slot]
                    want[slot] = [(table[0] + (table[1] - table[0]) * b) % p for b in bits[plane]]
                else:
                    o, a, ab = _rows(rnd, p, (1 << wl) + (1 << wh), count), _rows(rnd, p, (1 << wl) + (1 << wh), count), _rows(rnd, p, entries, count)
                    desc += [wl, wh, len(opened), len(tab), len(tables), slot]
                    want[slot] = ec.lookup_on_ints(p, wl, wh, o, a, ab, table, count)
                    opened, ta, tab = opened + o, ta + a, tab + ab
                tables += table
            na, nb = _rows(rnd, p, pairs, count), _rows(rnd, p, pairs, count)
            m0, k0 = _rows(rnd, p, 2 * pairs, count), _rows(rnd, p, kept_rows, count)
            masked, kept = ok(run_exp(p, nl, FINISH_LOOKUP_MASK, [bc.flat(bits), bc.flat(opened) or None, bc.flat(ta) or None, bc.flat(tab) or None, tables, bc.flat(na), bc.flat(nb)],
                                      [len(chosen), pairs, kept_rows] + desc, [bc.flat(m0), bc.flat(k0)], count))
            for slot in range(kept_rows):
                got = kept[slot * count:(slot + 1) * count]
                assert got == (want[slot] if slot in want else k0[slot]), (chosen, slot)
                if slot < 2 * pairs:
                    mk = masked[slot * count:(slot + 1) * count]
                    nxt = (nb if slot & 1 else na)[slot >> 1]
                    assert mk == ([(v - a) % p for v, a in zip(want[slot], nxt)] if slot in want else m0[slot]), (chosen, slot)
    # products to truncation masks: one to five products
    width, kappa = (140, 32) if p >> 64 else (30, 8)
    nbits = width + kappa
    for products in (1, 2, 3, 4, 5) if nbits + 2 <= p.bit_length() else ():          # (p = 13 has no room for a truncation: refused, below)
        for m in (1, 8, width - 1):
            opened, ta, tb, tab = _rows(rnd, p, 2 * products, count), _rows(rnd, p, products, count), _rows(rnd, p, products, count), _rows(rnd, p, products, count)
            planes = _rows(rnd, p, products * nbits, count)
            masked, s = ok(run_exp(p, nl, PRODUCTS_TRUNC, [bc.flat(v) for v in (opened, ta, tb, tab, planes)], [products, width, m, kappa], [products, products], count))
            for r in range(products):
                for e in range(count):
                    v = bc.beaver(opened[2 * r][e], opened[2 * r + 1][e], ta[r][e], tb[r][e], tab[r][e], p)
                    r1 = sum(planes[r * nbits + i][e] << i for i in range(m))
                    assert masked[r * count + e] == (v + (1 << (width - 1)) + sum(planes[r * nbits + i][e] << i for i in range(nbits))) % p and s[r * count + e] == (v + r1) % p
    # the step after an open of masked truncations: one to five rows, a carried factor in and none
    for rows in (1, 2, 3, 4, 5):
        for carried in (False, True):
            for m in (1, 8, 61) + ((64, 127, 140) if p >> 64 else ()):
                if m > p.bit_length() - 2:
                    continue
                opened, s = _rows(rnd, p, rows, count), _rows(rnd, p, rows, count)
                carry = [rnd.randrange(p) for _ in range(count)] if carried else None
                values = rows + carried
                ta, tb = _rows(rnd, p, values // 2, count), _rows(rnd, p, values // 2, count)
                masked, kept = ok(run_exp(p, nl, TREE_STEP, [bc.flat(opened), bc.flat(s), [pow(2, -m, p)], carry, bc.flat(ta) or None, bc.flat(tb) or None], [rows, m],
                                          [2 * (values // 2) or None, 1 if values & 1 else None], count))
                vals = [[(s[j][e] - opened[j][e] % (1 << m)) * pow(2, -m, p) % p for e in range(count)] for j in range(rows)] + ([carry] if carried else [])
                for q in range(values // 2):
                    assert masked[2 * q * count:(2 * q + 1) * count] == [(v - a) % p for v, a in zip(vals[2 * q], ta[q])], (rows, carried, m, q)
                    assert masked[(2 * q + 1) * count:(2 * q + 2) * count] == [(v - a) % p for v, a in zip(vals[2 * q + 1], tb[q])], (rows, carried, m, q)
                if values & 1:
                    assert kept == vals[-1]


CHAIN = [(p, nl, shape) for p, nl in bc.HOST_FIELDS for shape in ((8, 4, 8, 2), (16, 8, 8, 3), (16, 8, 8, 1), (64, 32, 32, 8)) if fe.exp2_width(shape[0]) + shape[2] + 2 <= p.bit_length() - 1]
CHAIN_IDS = [f"{bc.HOST_FIELD_IDS[bc.HOST_FIELDS.index((p, nl))]}-k{k}-f{f}-g{g}" for p, nl, (k, f, kappa, g) in CHAIN]


@pytest.mark.parametrize("natural", [False, True], ids=["exp2", "exp"])
@pytest.mark.parametrize("p, nl, shape", CHAIN, ids=CHAIN_IDS)
def test_chained_rows_reproduce_the_model(p, nl, shape, natural):
    """the whole chain through the host rows equals the model bit for bit for the r1 it was dealt, all-ones r1 included, for both widths"""
    assert {q for q, _, _ in CHAIN} == {q for q, _ in bc.HOST_FIELDS if q != 13}
    k, f, kappa, g = shape
    rnd = random.Random(p % 1013 + k + g + natural)
    count = 6 if k < 64 else 3
    pool = ec.operands(fe, rnd, k, f, g, natural, 4)
    xs = [0, -(f << f) - 1] + rnd.sample(pool, count - 2)
    n_trunc = (1 if natural else 0) + len(fe.exp2_shifts(k, f, g))
    out, r1s = ec.chain_on_host(fe, bd, dx, p, nl, xs, k, f, kappa, g, natural, rnd, all_ones=(0, n_trunc - 1))
    model = fe.exp_model if natural else fe.exp2_model
    for e, x in enumerate(xs):
        assert out[e] == model(x, p, k, f, [r[e] for r in r1s], g), (e, x)
    assert out[1] == 0                                                     # below -f: exactly 0


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_abi_names_in_header_and_ctypes_table():
    from honeybadgermpc_amd import _capi

    text = open(os.path.join(REPO, "include", "hbmpc_hip.h")).read()
    for name in ("hb_fxexp_finish_lookup_mask", "hb_fxexp_products_trunc", "hb_fxexp_tree_step", "hb_selftest_fxexp"):
        assert name in _capi.SYMBOLS and re.search(r"\b" + name + r"\(", text)
    for name, value in (("HB_FXEXP_SELFTEST_FINISH_LOOKUP_MASK", FINISH_LOOKUP_MASK), ("HB_FXEXP_SELFTEST_PRODUCTS_TRUNC", PRODUCTS_TRUNC), ("HB_FXEXP_SELFTEST_TREE_STEP", TREE_STEP)):
        assert re.search(r"#define " + name + r" " + str(value) + r"\b", text) and getattr(_capi, name) == value
    from honeybadgermpc_amd.progs import fixedpoint as fx

    assert callable(fx.FixedPointArray.exp2) and callable(fx.FixedPointArray.exp)


def test_selftest_rejects_bad_arguments_and_overlaps():
    from honeybadgermpc_amd._capi import HB_ERR_BAD_ARG, ints_to_limbs, load_library, np_ptr

    p, nl, count = BLS, 4, 3
    v = [1, 2, 3]
    rows = lambda n: v * n
    grp = [1, 1, 0, 0, 0, 0]                                               # a (1, 1) merge: 4 opened rows, 4 products, 4 entries, slot 0
    flm = [rows(1), rows(4), rows(4), rows(4), [1, 2, 3, 4], rows(1), rows(1)]
    bad = [
        (FINISH_LOOKUP_MASK, flm, [0, 1, 2] + grp, [2, 2]),                                          # no group
        (FINISH_LOOKUP_MASK, flm, [9, 1, 2] + grp, [2, 2]),
        (FINISH_LOOKUP_MASK, flm, [1, 129, 2] + grp, [2, 2]),
        (FINISH_LOOKUP_MASK, flm, [1, 1, 0] + grp, [2, 2]),
        (FINISH_LOOKUP_MASK, flm, [1, 1, 2, 0, 1, 0, 0, 0, 0], [2, 2]),                              # wl = 0
        (FINISH_LOOKUP_MASK, flm, [1, 1, 2, 7, 6, 0, 0, 0, 0], [2, 2]),                              # 13 bits
        (FINISH_LOOKUP_MASK, flm, [1, 1, 2, 2, 0, 0, 0, 0, 0], [2, 2]),                              # wh = 0 goes with wl = 1 alone
        (FINISH_LOOKUP_MASK, flm, [1, 1, 2, 1, 1, -1, 0, 0, 0], [2, 2]),
        (FINISH_LOOKUP_MASK, flm, [1, 1, 2, 1, 1, 0, 0, 0, 2], [2, 2]),                              # a slot at kept_rows
        (FINISH_LOOKUP_MASK, flm, [2, 1, 2] + grp + grp, [2, 2]),                                    # two groups in one slot
        (FINISH_LOOKUP_MASK, [rows(1), None] + flm[2:], [1, 1, 2] + grp, [2, 2]),
        (FINISH_LOOKUP_MASK, flm[:4] + [None] + flm[5:], [1, 1, 2] + grp, [2, 2]),
        (FINISH_LOOKUP_MASK, flm[:5] + [None, rows(1)], [1, 1, 2] + grp, [2, 2]),                    # slot 0 is masked: it needs the next triple
        (FINISH_LOOKUP_MASK, flm, [1, 1, 2] + grp, [2, None]),
        (FINISH_LOOKUP_MASK, flm, [1, 1, 2] + grp, [None, 2]),
        (FINISH_LOOKUP_MASK, [None] + flm[1:], [1, 1, 2, 1, 0, 0, 0, 0, 0], [2, 2]),                 # a group of one bit needs its plane
        (PRODUCTS_TRUNC, [rows(2), v, v, v, rows(40)], [0, 30, 8, 10], [1, 1]),
        (PRODUCTS_TRUNC, [rows(2), v, v, v, rows(40)], [129, 30, 8, 10], [1, 1]),
        (PRODUCTS_TRUNC, [rows(2), v, v, v, rows(40)], [1, 30, 0, 10], [1, 1]),
        (PRODUCTS_TRUNC, [rows(2), v, v, v, rows(40)], [1, 30, 30, 10], [1, 1]),
        (PRODUCTS_TRUNC, [rows(2), v, v, v, rows(40)], [1, 250, 8, 10], [1, 1]),                     # no room below the modulus
        (PRODUCTS_TRUNC, [rows(2), v, v, v, None], [1, 30, 8, 10], [1, 1]),
        (PRODUCTS_TRUNC, [rows(2), v, v, None, rows(40)], [1, 30, 8, 10], [1, 1]),
        (PRODUCTS_TRUNC, [rows(2), v, v, v, rows(40)], [1, 30, 8, 10], [1, None]),
        (TREE_STEP, [v, v, [1], None, None, None], [0, 8], [None, 1]),
        (TREE_STEP, [v, v, [1], None, None, None], [129, 8], [None, 1]),
        (TREE_STEP, [v, v, [1], None, None, None], [1, 0], [None, 1]),
        (TREE_STEP, [v, v, [1], None, None, None], [1, 254], [None, 1]),
        (TREE_STEP, [v, v, None, None, None, None], [1, 8], [None, 1]),
        (TREE_STEP, [v, v, [p], None, None, None], [1, 8], [None, 1]),                               # 2^(-m) that is no residue
        (TREE_STEP, [v, v, [1], None, None, None], [1, 8], [None, None]),                            # the odd value has nowhere to go
        (TREE_STEP, [v, v, [1], v, None, v], [1, 8], [2, None]),                                     # a pair needs both triple rows
        (TREE_STEP, [v, v, [1], v, v, v], [1, 8], [None, None]),
        (TREE_STEP, [None, v, [1], v, v, v], [1, 8], [2, None]),
        (3, [v], [], [1]),
    ]
    lib = load_library()
    modulus = np_ptr(ints_to_limbs([p], p + 1, 32))
    for i, (what, operands, params, outs) in enumerate(bad):
        if any(o is not None and len(o) == 1 and o[0] >= p for o in operands):    # a constant at the modulus: hand it over unreduced
            arrays = [None if o is None else ints_to_limbs(list(o), p + 1, 32) for o in operands]
            ptrs = (ctypes.c_void_p * 8)(*([None if a is None else a.ctypes.data for a in arrays] + [None] * (8 - len(arrays))))
            out = np.zeros((32, 4), dtype=np.uint64)
            optrs = (ctypes.c_void_p * 2)(out.ctypes.data, out[16:].ctypes.data)
            prm = (ctypes.c_int64 * 51)(*(list(params) + [0] * (51 - len(params))))
            rc = lib.hb_selftest_fxexp(modulus, 4, what, ptrs, prm, optrs, count)
        else:
            rc, _ = run_exp(p, nl, what, operands, params, outs, count)
        assert rc == HB_ERR_BAD_ARG, i
    assert run_exp(p, nl, FINISH_LOOKUP_MASK, [None, None, None, None, [1, 2, 3, 4], None, None], [1, 1, 2] + grp, [None, None], 0)[0] == 0       # count == 0: nothing to do
    assert run_exp(p, nl, PRODUCTS_TRUNC, [None] * 5, [1, 30, 8, 10], [None, None], 0)[0] == 0
    assert run_exp(p, nl, TREE_STEP, [None, None, [1], None, None, None], [1, 8], [None, None], 0)[0] == 0
    assert run_exp(p, nl, TREE_STEP, [v, v, [1], None, None, None], [1, 8], [None, 1], -1)[0] == HB_ERR_BAD_ARG

    # an output laid over an input, or over the other output, is refused as the entry points refuse it: every operand in ONE buffer
    eb = 8 * nl * count                                                           # bytes a row
    buf = np.zeros((96 * count, nl), dtype=np.uint64)
    at = lambda r: buf.ctypes.data + r * eb
    one = ints_to_limbs([1], p, 32)
    tables = ints_to_limbs([1, 2, 3, 4, 5, 6], p, 32)

    def call(what, params, ops, outs):
        ptrs = (ctypes.c_void_p * 8)(*(list(ops) + [None] * (8 - len(ops))))
        optrs = (ctypes.c_void_p * 2)(*(list(outs) + [None] * (2 - len(outs))))
        return lib.hb_selftest_fxexp(modulus, nl, what, ptrs, (ctypes.c_int64 * 51)(*(list(params) + [0] * (51 - len(params)))), optrs, count)

    # FINISH_LOOKUP_MASK, a (1, 1) merge in slot 1 and a bit in slot 0, one pair: bits 0, opened 1..4, ta 5..8, tab 9..12, nxt 13, 14; masked 20..21, kept 22..23
    ops = [at(0), at(1), at(5), at(9), tables.ctypes.data, at(13), at(14)]
    prm = [2, 1, 2, 1, 1, 0, 0, 0, 1, 1, 0, 0, 0, 4, 0]
    assert call(FINISH_LOOKUP_MASK, prm, ops, [at(20), at(22)]) == 0
    for outs in ([at(0), at(22)], [at(4), at(22)], [at(8), at(22)], [at(12), at(22)], [at(13), at(22)], [at(20), at(14)], [at(20), at(21)], [at(21), at(22)], [at(20), at(0)],
                 [at(20), at(11)], [at(22), at(22)], [at(20), tables.ctypes.data]):
        assert call(FINISH_LOOKUP_MASK, prm, ops, outs) == HB_ERR_BAD_ARG, outs
    # PRODUCTS_TRUNC, two products, width 30, kappa 10: opened 0..3, ta 4..5, tb 6..7, tab 8..9, bits 10..89; masked 90..91, s 92..93
    ops = [at(0), at(4), at(6), at(8), at(10)]
    assert call(PRODUCTS_TRUNC, [2, 30, 8, 10], ops, [at(90), at(92)]) == 0
    for outs in ([at(3), at(92)], [at(5), at(92)], [at(90), at(7)], [at(90), at(9)], [at(89), at(92)], [at(90), at(91)], [at(90), at(50)], [at(92), at(92)]):
        assert call(PRODUCTS_TRUNC, [2, 30, 8, 10], ops, outs) == HB_ERR_BAD_ARG, outs
    # TREE_STEP, three rows and a carry: opened 0..2, s 3..5, carry 6, ta 7..8, tb 9..10; masked 20..23 (three rows, no carry: masked 20..21, kept 24)
    ops = [at(0), at(3), one.ctypes.data, at(6), at(7), at(9)]
    assert call(TREE_STEP, [3, 8], ops, [at(20), None]) == 0
    for outs in ([at(2), None], [at(5), None], [at(6), None], [at(8), None], [at(10), None], [at(1), None]):
        assert call(TREE_STEP, [3, 8], ops, outs) == HB_ERR_BAD_ARG, outs
    ops = [at(0), at(3), one.ctypes.data, None, at(7), at(9)]
    assert call(TREE_STEP, [3, 8], ops, [at(20), at(24)]) == 0
    for outs in ([at(20), at(21)], [at(20), at(2)], [at(20), at(7)], [at(24), at(24)]):
        assert call(TREE_STEP, [3, 8], ops, outs) == HB_ERR_BAD_ARG, outs


def test_protocol_refuses_before_anything_is_opened():
    """the checks of the coroutines that need no device: g out of 1 .. 12, an integer group of more than 12 bits, a width that does not
    fit the modulus, a bad k / f / kappa"""
    for k, f, kappa, g in ((8, 4, 8, 0), (8, 4, 8, 13), (8, 5, 8, 2), (8, 0, 8, 1), (3, 1, 8, 1), (8, 4, 1.5, 2), (300, 32, 32, 8)):
        with pytest.raises(ValueError):
            fe.exp2_layout(k, f, kappa, g)
        with pytest.raises(ValueError):
            fe.exp_layout(k, f, kappa, g)
    with pytest.raises(ValueError):                                              # mi + 1 > 12 needs k - 3 >= 2^11, far past the planes a decomposition takes
        fe._check_kf(2 ** 11 + 3, 32)

    class Ctx:
        modulus = bc.P64

    with pytest.raises(ValueError):                                              # (64, 32, 32) over a 64-bit field: 134 + 32 + 1 bits do not fit
        fe._check_protocol(Ctx, fe.exp2_layout(64, 32, 32, 8), 64, 32, 32, False)
    fe._check_protocol(Ctx, fe.exp2_layout(16, 8, 8, 3), 16, 8, 8, False)
    fe._check_protocol(Ctx, fe.exp_layout(16, 8, 8, 3), 16, 8, 8, True)

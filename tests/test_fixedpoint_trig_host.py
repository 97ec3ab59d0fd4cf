"""CPU-only: honeybadgermpc_amd.progs.fixedpoint_trig -- the tables against an enclosure of their own (half-angle roots and angle addition,
not the series that built them), the counts against formulas worked out by hand, sincos_turns_model and sincos_model inside
trig_error_bound (EVERY signed input at (8, 4) and (16, 8), both extremes of every truncation: every integer part occurs, so this is
the periodicity test too), the guards minimal by their rules, the steps of csrc/hb_fxtrig.hip through hb_selftest_fxtrig (the rows the
device runs, behind the step functions the entry points run) against Python ints, every lane split the same bits, chained into the
whole protocol bit-equal to the models, and the refusals."""
import ctypes
import os
import random
import re
from fractions import Fraction

import numpy as np
import pytest

import bitdec_cases as bc
import trig_cases as tc
from conftest import BLS, REPO
from honeybadgermpc_amd.progs import bit_decomposition as bd
from honeybadgermpc_amd.progs import demux as dx
from honeybadgermpc_amd.progs import fixedpoint_trig as ft
from trig_cases import BOTH, COS, CPRODUCTS_TRUNC, FINISH_LOOKUP_MASK, SIN, TREE_STEP, ok, run_trig


# ---- tables, counts, constants ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k, f, g, radians", [(8, 4, 2, False), (8, 4, 1, False), (8, 4, 4, False), (16, 8, 3, False), (16, 8, 4, True), (64, 32, 8, False), (64, 40, 6, False),
                                              (64, 32, 8, True)])
def test_tables_are_the_exact_roundings(k, f, g, radians):
    fbits = f + ft.TURN_GUARD if radians else f
    groups, tables = ft.trig_groups(k, f, g, radians), ft.trig_tables(k, f, g, radians)
    s = fbits + ft.TRIG_GUARD if len(groups) > 1 else f
    assert len(tables) == len(groups) and sum(w for _, w in groups) == fbits and max(w for _, w in groups) - min(w for _, w in groups) <= 1
    half = 1 << (tc._P - s - 1)
    for (o, w), (ctab, stab) in zip(groups, tables):
        assert len(ctab) == len(stab) == 1 << w
        for j in range(1 << w):
            for entry, (lo, hi) in zip((ctab[j], stab[j]), tc.cis_enclosure(j << o, fbits)):
                assert hi - lo < 1 << 40 and max(abs((entry << (tc._P - s)) - lo), abs((entry << (tc._P - s)) - hi)) <= half + (hi - lo), (o, j)
    # the top group's entries are signed; every lower group's are not once the top group has two bits or more
    top_c, top_s = tables[-1]
    if groups[-1][1] >= 2:
        assert min(top_c) == -(1 << s) and max(top_c) == 1 << s and min(top_s) == -(1 << s) and max(top_s) == 1 << s
        assert all(v >= 0 for ctab, stab in tables[:-1] for v in ctab + stab)
    assert all(ctab[0] == 1 << s and stab[0] == 0 for ctab, stab in tables)


def test_counts_against_the_hand_table():
    for (k, f, kappa, g, radians, want), groups, tree, planes, triples, opens, rows in tc.TABLE:
        lay = ft.trig_layout(k, f, kappa, g, radians, want)
        fbits = f + 3 if radians else f
        assert lay["groups"] == groups == ft.trig_groups(k, f, g, radians) and lay["tree"] == tree and lay["ft"] == fbits
        assert lay["n_planes"] == planes == ft.trig_planes(k, f, kappa, g, radians, want)
        assert lay["n_triples"] == bd.bit_triples(fbits) + triples == ft.trig_triples(k, f, g, radians, want)
        assert lay["opens"] == bd.bit_opens(fbits) + opens == ft.trig_opens(k, f, g, radians)
        assert lay["demux_rows"] == rows == ft.trig_demux_rows(k, f, g, radians)
        assert lay["demux_opened"] == sum(o for lv in rows for _, o, _ in lv) and lay["demux_products"] == sum(q for lv in rows for _, _, q in lv)
        for ranges, total in ((lay["planes"], lay["n_planes"]), (lay["triples"], lay["n_triples"])):          # contiguous, in step order, from row 0
            spans = sorted(ranges.values())
            assert spans[0][0] == 0 and spans[-1][1] == total and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            names = [n for n, _ in sorted(ranges.items(), key=lambda kv: kv[1])]
            assert names == (["turns"] if radians and ranges is lay["planes"] else []) + ["bit_decompose"] + [f"tree{i}" for i in range(len(tree))]
        assert len(ft.trig_shifts(k, f, g, radians, want)) == (1 if radians else 0) + sum(n * (2 if md == BOTH else 1) for n, md in zip(lay["tree"], lay["modes"]))
    # want of one component: the last level's other truncation goes, and for the cosine the triple that feeds the sine alone
    both, one, sine = ft.trig_layout(64, 32, 32, 8), ft.trig_layout(64, 32, 32, 8, want=("cos",)), ft.trig_layout(64, 32, 32, 8, want=("sin",))
    assert both["n_planes"] - one["n_planes"] == both["width"] + 32 and both["n_triples"] - one["n_triples"] == 1 and both["opens"] == one["opens"]
    assert sine["n_planes"] == one["n_planes"] and sine["n_triples"] == both["n_triples"] and sine["opens"] == both["opens"]
    assert ft.trig_layout(64, 32, 32, 8, want=("cos", "sin")) == both
    # the default g: the smallest among those with the fewest opens
    for k, f, radians in ((8, 4, False), (16, 8, False), (64, 32, False), (64, 32, True), (64, 40, False)):
        fbits = f + 3 if radians else f
        best = min((ft.trig_opens(k, f, g, radians), g) for g in range(1, min(fbits, 12) + 1))
        assert ft.default_group_width(k, f, radians) == best[1]


def test_guards_are_minimal_by_their_rules():
    assert ft._guard_rule(ft.TRIG_GUARD) and not ft._guard_rule(ft.TRIG_GUARD - 1)
    assert ft._turn_rule(ft.TURN_GUARD, ft.FL_EXTRA) and not ft._turn_rule(ft.TURN_GUARD, ft.FL_EXTRA - 1)
    assert not any(ft._turn_rule(ft.TURN_GUARD - 1, extra) for extra in range(0, 200))                        # no fl rescues a smaller turn guard
    for k in (8, 16, 64):
        L, fl, m = ft.turn_factor(k)
        assert (fl, m) == (k + ft.FL_EXTRA, k + ft.FL_EXTRA - ft.TURN_GUARD)
        assert abs(2 * L * tc._PI - (1 << (fl + tc._P))) <= tc._PI + (1 << 20)                                # |L - 2^fl / (2 pi)| <= 1/2, by the tests' own pi
    # the bounds the rules give: about 1.25 ulps for turns and 2.25 for radians at 16 factors, less with fewer, 1/2 with one group
    assert Fraction(124, 100) < ft.trig_error_bound(64, 32, 2) < Fraction(125, 100)
    assert Fraction(1) < ft.trig_error_bound(64, 32, 8) < ft.trig_error_bound(64, 32, 4) < ft.trig_error_bound(64, 32, 2)
    assert Fraction(2) < ft.trig_error_bound(64, 29, 2, True) <= Fraction(225, 100) and ft.trig_error_bound(8, 4, 4) == Fraction(1, 2)
    assert ft.trig_error_bound(64, 32, 8, True) - ft.trig_error_bound(64, 32, 8) < 1


# ---- the models -------------------------------------------------------------------------------------------------------------------
def _check(model, enclosure, bound, xs, p, k, f, g, limits, want=("sin", "cos")):
    worst = 0
    for x in xs:
        enc = enclosure(x, f)
        for r1s in tc.r1_extremes(limits):
            got = model(x, p, k, f, r1s, g, want)
            for name, v in zip(want, got):
                err = tc.error_ulps(tc.centered(v, p), enc[name])
                worst = max(worst, err)
                assert err <= bound * (1 << tc.EXTRA), (x, name, r1s[0], tc.centered(v, p), float(Fraction(err, 1 << tc.EXTRA)))
            if len(got) == 2:                                                   # sin^2 + cos^2 within what the bound implies: 2 B sqrt(2) 2^f + 2 B^2
                sv, cv = (tc.centered(v, p) for v in got) if want[0] == "sin" else (tc.centered(v, p) for v in got[::-1])
                assert abs(sv * sv + cv * cv - (1 << (2 * f))) <= 2 * bound * Fraction(17, 12) * (1 << f) + 2 * bound * bound, x
    return Fraction(worst, 1 << tc.EXTRA)


@pytest.mark.parametrize("k, f, g", [(8, 4, 1), (8, 4, 2), (8, 4, 3), (8, 4, 4), (16, 8, 3), (16, 8, 8)], ids=lambda v: str(v))
def test_turns_model_within_the_bound_for_every_input(k, f, g):
    xs = range(-(1 << (k - 1)), 1 << (k - 1))
    bound = ft.trig_error_bound(k, f, g)
    worst = _check(ft.sincos_turns_model, tc.turns_enclosure, bound, xs, BLS, k, f, g, ft.trig_shifts(k, f, g))
    assert worst > bound / 4                                                    # the bound is no idle one
    z = [0] * len(ft.trig_shifts(k, f, g))
    for turn in range(-(1 << (k - 1 - f)), 1 << (k - 1 - f)):                   # exact at the quarter turns, whatever the integer part
        for quarter, (sv, cv) in enumerate([(0, 1), (1, 0), (0, -1), (-1, 0)]):
            got = ft.sincos_turns_model((turn << f) + (quarter << f >> 2), BLS, k, f, z, g)
            assert [tc.centered(v, BLS) for v in got] == [sv << f, cv << f]


@pytest.mark.parametrize("g", [4, 6, 8, 11, None])
@pytest.mark.parametrize("k, f", [(64, 32), (64, 40)], ids=["k64-f32", "k64-f40"])
def test_turns_model_within_the_bound_on_seeded_inputs(k, f, g):
    rnd = random.Random(1000 * k + 10 * f + (g or 0))
    xs = tc.operands(rnd, k, f, 150)
    _check(ft.sincos_turns_model, tc.turns_enclosure, ft.trig_error_bound(k, f, g), xs, BLS, k, f, g, ft.trig_shifts(k, f, g))
    for want in (("cos",), ("sin",), ("cos", "sin")):                            # one component: the same value for the same r1 of its truncations
        limits = ft.trig_shifts(k, f, g, want=want)
        assert len(limits) == len(ft.trig_shifts(k, f, g)) - (2 - len(want))
        for x in xs[:40]:
            r1s = [rnd.randrange(1 << m) for m in ft.trig_shifts(k, f, g)]
            sv, cv = ft.sincos_turns_model(x, BLS, k, f, r1s, g)
            part = r1s[:-2] + ([r1s[-2]] if want == ("cos",) else [r1s[-1]] if want == ("sin",) else r1s[-2:])
            assert ft.sincos_turns_model(x, BLS, k, f, part, g, want) == tuple(cv if n == "cos" else sv for n in want)


@pytest.mark.parametrize("k, f, g", [(8, 4, 2), (8, 4, 7), (16, 8, 3), (64, 32, 8), (64, 32, 4), (64, 40, None)], ids=lambda v: str(v))
def test_radian_model_within_its_bound(k, f, g):
    rnd = random.Random(77 * k + f)
    xs = range(-(1 << (k - 1)), 1 << (k - 1)) if k <= 16 else tc.operands(rnd, k, f, 150) + [round(q * 3.141592653589793 * 2 ** (f - 1)) + d for q in range(-8, 9) for d in (-1, 0, 1)]
    bound = ft.trig_error_bound(k, f, g, True)
    worst = _check(ft.sincos_model, tc.radians_enclosure, bound, xs, BLS, k, f, g, ft.trig_shifts(k, f, g, True))
    assert worst > bound / 4
    z = [0] * len(ft.trig_shifts(k, f, g, True))
    assert [tc.centered(v, BLS) for v in ft.sincos_model(0, BLS, k, f, z, g)] == [0, 1 << f]


def test_models_and_layouts_refuse():
    z = [0, 0]
    for bad in (lambda: ft.sincos_turns_model(0, BLS, 8, 4, [0], 2), lambda: ft.sincos_turns_model(0, BLS, 8, 4, [0, 1 << 18], 2), lambda: ft.sincos_turns_model(128, BLS, 8, 4, z, 2),
                lambda: ft.sincos_turns_model(-129, BLS, 8, 4, z, 2), lambda: ft.sincos_turns_model(0, BLS, 8, 4, z, 13), lambda: ft.sincos_turns_model(0, BLS, 8, 4, z, 0),
                lambda: ft.sincos_turns_model(0, 2 ** 31 - 1, 16, 8, [0] * 4, 3), lambda: ft.sincos_model(0, BLS, 8, 4, z, 2), lambda: ft.sincos_model(0, BLS, 8, 4, [1 << 8, 0, 0], 2),
                lambda: ft.sincos_turns_model(0, BLS, 8, 4, z, 2, ("tan",)), lambda: ft.sincos_turns_model(0, BLS, 8, 4, z, 2, ()), lambda: ft.sincos_turns_model(0, BLS, 8, 4, z, 2, ("sin", "sin")),
                lambda: ft.trig_error_bound(8, 8, 2), lambda: ft.trig_error_bound(8, 0, 2), lambda: ft.trig_layout(300, 270, 32, 8), lambda: ft.trig_layout(8, 4, 1.5, 2),
                lambda: ft.trig_layout(1, 1, 8, 1), lambda: ft.trig_groups(8, 4, 13)):
        with pytest.raises(ValueError):
            bad()
    assert ft.sincos_turns_model(BLS - 1, BLS, 8, 4, z, 2) == ft.sincos_turns_model(-1, BLS, 8, 4, z, 2)       # a residue or a signed int

    # what the modulus or the 256-bit truncation width has no room for
    ft._check_room(bc.P64, ft.trig_layout(16, 8, 8, 3), 16, 8, 8, False)
    ft._check_room(bc.P64, ft.trig_layout(16, 8, 8, 3, True), 16, 8, 8, True)
    for p, shape, radians in ((bc.P64, (64, 32, 32, 8), False), (bc.P64, (28, 8, 8, 4), True), (BLS, (120, 110, 32, 8), False), (bc.P64, (32, 31, 8, 31), False), (bc.P64, (60, 8, 8, 8), False)):
        k, f, kappa, g = shape
        with pytest.raises(ValueError):
            ft._check_room(p, ft.trig_layout(k, f, kappa, min(g, 12), radians), k, f, kappa, radians)


# ---- the rows on the host ---------------------------------------------------------------------------------------------------------
def _rows(rnd, p, rows, count):
    return [[rnd.randrange(p) for _ in range(count)] for _ in range(rows)]


def _signed_table(rnd, p, entries, kind):
    """kind 0: arbitrary residues; 1: short entries of both signs with zeros among them (the protocol's); 2: everything within a few digits of p"""
    top = min(p // 2, 1 << 67)
    if kind == 0:
        return [rnd.randrange(p) for _ in range(entries)]
    return [0 if rnd.random() < 0.2 else rnd.choice((-1, 1)) * rnd.randrange(1, top + 1) for _ in range(entries)] if kind == 1 else [-rnd.randrange(1, top + 1) for _ in range(entries)]


def _lookup_case(rnd, p, chosen, count, kind, pairs, kept_slots, mode):
    bits, opened, ta, tab, tables, desc, want = _rows(rnd, p, 3, count), [], [], [], [], [], {}
    slots = rnd.sample(range(kept_slots), len(chosen))
    for (wl, wh), slot in zip(chosen, slots):
        entries = 1 << (wl + wh)
        ctab, stab = _signed_table(rnd, p, entries, kind), _signed_table(rnd, p, entries, kind)
        if wh == 0:
            plane = rnd.randrange(3)
            desc += [1, 0, plane, 0, len(tables), slot]
            want[slot] = tuple([(t[0] + (t[1] - t[0]) * b) % p for b in bits[plane]] for t in (ctab, stab))
        else:
            o, a, ab = _rows(rnd, p, (1 << wl) + (1 << wh), count), _rows(rnd, p, (1 << wl) + (1 << wh), count), _rows(rnd, p, entries, count)
            desc += [wl, wh, len(opened), len(tab), len(tables), slot]
            want[slot] = tuple(tc.lookup_on_ints(p, wl, wh, o, a, ab, t, count) for t in (ctab, stab))
            opened, ta, tab = opened + o, ta + a, tab + ab
        tables += [t % p for t in ctab + stab]
    tp = tc.triples_of(mode)
    na, nb = _rows(rnd, p, tp * pairs, count), _rows(rnd, p, tp * pairs, count)
    m0, k0 = _rows(rnd, p, 2 * tp * pairs, count), _rows(rnd, p, 2 * kept_slots, count)
    ops = [bc.flat(bits), bc.flat(opened) or None, bc.flat(ta) or None, bc.flat(tab) or None, tables, bc.flat(na), bc.flat(nb)]
    return ops, desc, want, (na, nb), (m0, k0)


def _check_lookup(p, nl, rnd, chosen, count, kind, mode, splits):
    pairs, kept_slots = 2, 5
    ops, desc, want, (na, nb), (m0, k0) = _lookup_case(rnd, p, chosen, count, kind, pairs, kept_slots, mode)
    tp, first = tc.triples_of(mode), None
    for split in splits:
        masked, kept = ok(run_trig(p, nl, FINISH_LOOKUP_MASK, ops, [len(chosen), pairs, kept_slots, mode, split] + desc, [bc.flat(m0), bc.flat(k0)], count))
        if first is not None:
            assert (masked, kept) == first, (chosen, split)                     # every lane split: the same bits
            continue
        first = (masked, kept)
        row = lambda arr, r: arr[r * count:(r + 1) * count]
        for slot in range(kept_slots):
            if slot not in want:
                assert row(kept, 2 * slot) == k0[2 * slot] and row(kept, 2 * slot + 1) == k0[2 * slot + 1]
                continue
            re, im = want[slot]
            assert row(kept, 2 * slot) == re and row(kept, 2 * slot + 1) == im, (chosen, slot, kind)
            if slot < 2 * pairs:
                q, side = slot >> 1, slot & 1
                for t in range(tp):
                    vals = [tc.operand_values(re[e], im[e], mode, side, p)[t] for e in range(count)]
                    assert row(masked, 2 * (tp * q + t) + side) == [(v - a) % p for v, a in zip(vals, (nb if side else na)[tp * q + t])], (chosen, slot, t, mode)
        named = {2 * (tp * (s >> 1) + t) + (s & 1) for s in want if s < 2 * pairs for t in range(tp)}
        assert all(row(masked, r) == m0[r] for r in range(2 * tp * pairs) if r not in named)         # rows that no group names are left alone


@pytest.mark.parametrize("p, nl", bc.HOST_FIELDS, ids=bc.HOST_FIELD_IDS)
def test_finish_lookup_mask_row_on_signed_tables_for_every_split(p, nl):
    rnd = random.Random(p % 997)
    shapes = tc.MERGES + [(1, 0), (3, 2), (6, 4)]
    for n_groups in (1, 2, 3):
        for trial, _ in enumerate(shapes):
            chosen = [shapes[(trial + i) % len(shapes)] for i in range(n_groups)]
            if sum(1 << (wl + wh) for wl, wh in chosen) > 600:
                chosen = chosen[:1]
            big = sum(1 << (wl + wh) for wl, wh in chosen) > 64
            _check_lookup(p, nl, rnd, chosen, 1 if big and p >> 64 else 5, trial % 3, (trial + n_groups) % 3, tc.SPLITS if n_groups == 1 or not big else (1, 4))
    for count, chosen, kind in ((0, [(2, 2)], 1), (1, [(4, 4)], 1), (257, [(2, 2), (1, 0)], 1), (257, [(4, 3)], 2)):
        if count == 0:
            ops, desc, _, _, _ = _lookup_case(rnd, p, chosen, 1, kind, 2, 5, BOTH)
            assert run_trig(p, nl, FINISH_LOOKUP_MASK, [None] * 4 + [ops[4], None, None], [1, 2, 5, BOTH, 4] + desc, [None, None], 0)[0] == 0
        else:
            _check_lookup(p, nl, rnd, chosen, count, kind, BOTH, (1, 2, 16) if count == 257 else tc.SPLITS)


@pytest.mark.parametrize("p, nl", bc.HOST_FIELDS, ids=bc.HOST_FIELD_IDS)
def test_cproducts_trunc_and_tree_step_rows(p, nl):
    rnd = random.Random(p % 991)
    width, kappa = (140, 32) if p >> 64 else (30, 8)
    nbits = width + kappa
    inv = lambda m: pow(2, -m, p)
    for count in (0, 1, 5, 257):
        for mode in (BOTH, COS, SIN):
            tp, comps = tc.triples_of(mode), tc.comps_of(mode)
            # complex products to truncation masks: one to five products (p = 13 has no room for a truncation: refused, below)
            for products in ((1, 2, 3, 4, 5) if count == 5 else (1, 3)) if nbits + 2 <= p.bit_length() else ():
                for m in (1, 8, width - 1) if count == 5 else (8,):
                    opened, ta, tb, tab = _rows(rnd, p, 2 * tp * products, count), _rows(rnd, p, tp * products, count), _rows(rnd, p, tp * products, count), _rows(rnd, p, tp * products, count)
                    planes = _rows(rnd, p, comps * products * nbits, count)
                    masked, s = ok(run_trig(p, nl, CPRODUCTS_TRUNC, [bc.flat(v) for v in (opened, ta, tb, tab, planes)], [products, mode, width, m, kappa],
                                            [comps * products, comps * products], count))
                    for q in range(products):
                        for e in range(count):
                            prods = [bc.beaver(opened[2 * r][e], opened[2 * r + 1][e], ta[r][e], tb[r][e], tab[r][e], p) for r in range(tp * q, tp * q + tp)]
                            for c, v in enumerate(tc.components(prods, mode, p)):
                                row = comps * q + c
                                r1 = sum(planes[row * nbits + i][e] << i for i in range(m))
                                assert masked[row * count + e] == (v + (1 << (width - 1)) + sum(planes[row * nbits + i][e] << i for i in range(nbits))) % p, (mode, q, c)
                                assert s[row * count + e] == (v + r1) % p
            # the step after an open of masked truncations: one to five complex values, a carried one in and none; the next level in `mode`
            for cvalues in ((1, 2, 3, 4, 5) if count == 5 else (2, 3)):
                for carried in (False, True):
                    for m in ((1, 8, 61) + ((64, 127, 140) if p >> 64 else ())) if count == 5 else (8,):
                        if m > p.bit_length() - 2:
                            continue
                        rows = 2 * cvalues
                        opened, s = _rows(rnd, p, rows, count), _rows(rnd, p, rows, count)
                        carry = _rows(rnd, p, 2, count) if carried else None
                        values = cvalues + carried
                        pairs = values // 2
                        ta, tb = _rows(rnd, p, tp * pairs, count), _rows(rnd, p, tp * pairs, count)
                        masked, kept = ok(run_trig(p, nl, TREE_STEP, [bc.flat(opened), bc.flat(s), [inv(m)], bc.flat(carry) if carried else None, bc.flat(ta) or None, bc.flat(tb) or None],
                                                   [rows, 0, m, mode], [2 * tp * pairs or None, 2 if values & 1 else None], count))
                        t = [[(s[j][e] - opened[j][e] % (1 << m)) * inv(m) % p for e in range(count)] for j in range(rows)]
                        vals = [(t[2 * u], t[2 * u + 1]) for u in range(cvalues)] + ([(carry[0], carry[1])] if carried else [])
                        for u in range(2 * pairs):
                            q, side = u >> 1, u & 1
                            for k3 in range(tp):
                                want = [(tc.operand_values(vals[u][0][e], vals[u][1][e], mode, side, p)[k3] - (tb if side else ta)[tp * q + k3][e]) % p for e in range(count)]
                                r = 2 * (tp * q + k3) + side
                                assert masked[r * count:(r + 1) * count] == want, (cvalues, carried, m, mode, u, k3)
                        if values & 1:
                            assert kept == vals[-1][0] + vals[-1][1]
        # final: the results, one or two rows
        for rows in (1, 2):
            m = min(9, p.bit_length() - 2)
            opened, s = _rows(rnd, p, rows, count), _rows(rnd, p, rows, count)
            _, kept = ok(run_trig(p, nl, TREE_STEP, [bc.flat(opened), bc.flat(s), [inv(m)], None, None, None], [rows, 1, m, 0], [None, rows], count))
            assert kept == [(s[j][e] - opened[j][e] % (1 << m)) * inv(m) % p for j in range(rows) for e in range(count)]


CHAIN_SHAPES = [((8, 4, 8, 4), False), ((8, 4, 8, 2), False), ((8, 4, 8, 1), False), ((16, 8, 8, 3), False), ((16, 8, 8, 3), True), ((64, 32, 32, 8), False), ((64, 32, 32, 8), True)]
CHAIN = [(p, nl, shape, radians) for p, nl in bc.HOST_FIELDS for shape, radians in CHAIN_SHAPES if p != 13 and
         max(2 * shape[0] + 1 if radians else 0, ft.trig_width(shape[0], shape[1], radians)) + shape[2] + 2 <= p.bit_length() - 1]
CHAIN_IDS = [f"{bc.HOST_FIELD_IDS[bc.HOST_FIELDS.index((p, nl))]}-k{k}-f{f}-g{g}-{'radians' if radians else 'turns'}" for p, nl, (k, f, kappa, g), radians in CHAIN]


@pytest.mark.parametrize("p, nl, shape, radians", CHAIN, ids=CHAIN_IDS)
def test_chained_rows_reproduce_the_model(p, nl, shape, radians):
    """the whole chain through the host rows equals the model bit for bit for the r1 it was dealt, all-ones r1 included, for both widths,
    each `want` and two lane splits"""
    assert {q for q, _, _, _ in CHAIN} == {q for q, _ in bc.HOST_FIELDS if q != 13}
    k, f, kappa, g = shape
    rnd = random.Random(p % 1013 + k + g + radians)
    count = 6 if k < 64 else 3
    xs = [0, -(1 << (k - 1))] + rnd.sample(tc.operands(rnd, k, f, 4), count - 2)
    model = ft.sincos_model if radians else ft.sincos_turns_model
    for want, split in zip(tc.WANTS if k < 64 else tc.WANTS[:2], (1, 4, 2, 16)):
        n_trunc = len(ft.trig_shifts(k, f, g, radians, want))
        out, r1s = tc.chain_on_host(ft, bd, dx, p, nl, xs, k, f, kappa, g, radians, want, rnd, split=split, all_ones=(0, n_trunc - 1))
        assert len(r1s) == n_trunc
        for e, x in enumerate(xs):
            assert tuple(out[n][e] for n in want) == model(x, p, k, f, [r[e] for r in r1s], g, want), (want, e, x)


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_abi_names_in_header_and_ctypes_table():
    from honeybadgermpc_amd import _capi

    text = open(os.path.join(REPO, "include", "hbmpc_hip.h")).read()
    for name in ("hb_fxtrig_finish_lookup_mask", "hb_fxtrig_cproducts_trunc", "hb_fxtrig_tree_step", "hb_selftest_fxtrig"):
        assert name in _capi.SYMBOLS and re.search(r"\b" + name + r"\(", text)
    for name, value in (("HB_FXTRIG_SELFTEST_FINISH_LOOKUP_MASK", FINISH_LOOKUP_MASK), ("HB_FXTRIG_SELFTEST_CPRODUCTS_TRUNC", CPRODUCTS_TRUNC), ("HB_FXTRIG_SELFTEST_TREE_STEP", TREE_STEP)):
        assert re.search(r"#define " + name + r" " + str(value) + r"\b", text) and getattr(_capi, name) == value
    assert (ft.MODE_BOTH, ft.MODE_COS, ft.MODE_SIN) == (BOTH, COS, SIN) and ft.SPLITS == tc.SPLITS and ft.lookup_split(1) in ft.SPLITS and ft.lookup_split(1 << 20) in ft.SPLITS
    from honeybadgermpc_amd.progs import fixedpoint as fx

    assert all(callable(getattr(fx.FixedPointArray, n)) for n in ("sincos", "sin", "cos", "sincos_turns"))


def test_selftest_rejects_bad_arguments_and_overlaps():
    from honeybadgermpc_amd._capi import HB_ERR_BAD_ARG, ints_to_limbs, load_library, np_ptr

    p, nl, count = BLS, 4, 3
    v = [1, 2, 3]
    rows = lambda n: v * n
    grp = [1, 1, 0, 0, 0, 0]                                               # a (1, 1) merge: 4 opened rows, 4 products, 8 entries, slot 0
    flm = [rows(1), rows(4), rows(4), rows(4), list(range(1, 9)), rows(3), rows(3)]
    cpt = [rows(6), rows(3), rows(3), rows(3), rows(80)]
    bad = [
        (FINISH_LOOKUP_MASK, flm, [0, 1, 2, 0, 1] + grp, [6, 4]),                                    # no group
        (FINISH_LOOKUP_MASK, flm, [9, 1, 2, 0, 1] + grp, [6, 4]),
        (FINISH_LOOKUP_MASK, flm, [1, 65, 2, 0, 1] + grp, [6, 4]),
        (FINISH_LOOKUP_MASK, flm, [1, 1, 0, 0, 1] + grp, [6, 4]),
        (FINISH_LOOKUP_MASK, flm, [1, 1, 2, 3, 1] + grp, [6, 4]),                                    # no such mode
        (FINISH_LOOKUP_MASK, flm, [1, 1, 2, -1, 1] + grp, [6, 4]),
        (FINISH_LOOKUP_MASK, flm, [1, 1, 2, 0, 0] + grp, [6, 4]),                                    # splits: 1, 2, 4, 8, 16
        (FINISH_LOOKUP_MASK, flm, [1, 1, 2, 0, 3] + grp, [6, 4]),
        (FINISH_LOOKUP_MASK, flm, [1, 1, 2, 0, 32] + grp, [6, 4]),
        (FINISH_LOOKUP_MASK, flm, [1, 1, 2, 0, 1, 0, 1, 0, 0, 0, 0], [6, 4]),                        # wl = 0
        (FINISH_LOOKUP_MASK, flm, [1, 1, 2, 0, 1, 7, 6, 0, 0, 0, 0], [6, 4]),                        # 13 bits
        (FINISH_LOOKUP_MASK, flm, [1, 1, 2, 0, 1, 2, 0, 0, 0, 0, 0], [6, 4]),                        # wh = 0 goes with wl = 1 alone
        (FINISH_LOOKUP_MASK, flm, [1, 1, 2, 0, 1, 1, 1, -1, 0, 0, 0], [6, 4]),
        (FINISH_LOOKUP_MASK, flm, [1, 1, 2, 0, 1, 1, 1, 0, 0, 0, 2], [6, 4]),                        # a slot at kept_slots
        (FINISH_LOOKUP_MASK, flm, [2, 1, 2, 0, 1] + grp + grp, [6, 4]),                              # two groups in one slot
        (FINISH_LOOKUP_MASK, [rows(1), None] + flm[2:], [1, 1, 2, 0, 1] + grp, [6, 4]),
        (FINISH_LOOKUP_MASK, flm[:4] + [None] + flm[5:], [1, 1, 2, 0, 1] + grp, [6, 4]),
        (FINISH_LOOKUP_MASK, flm[:5] + [None, rows(3)], [1, 1, 2, 0, 1] + grp, [6, 4]),              # slot 0 is masked: it needs the next triples
        (FINISH_LOOKUP_MASK, flm, [1, 1, 2, 0, 1] + grp, [6, None]),
        (FINISH_LOOKUP_MASK, flm, [1, 1, 2, 0, 1] + grp, [None, 4]),
        (FINISH_LOOKUP_MASK, [None] + flm[1:], [1, 1, 2, 0, 1, 1, 0, 0, 0, 0, 0], [6, 4]),           # a group of one bit needs its plane
        (CPRODUCTS_TRUNC, cpt, [0, 0, 30, 8, 10], [2, 2]),
        (CPRODUCTS_TRUNC, cpt, [65, 0, 30, 8, 10], [2, 2]),
        (CPRODUCTS_TRUNC, cpt, [1, 3, 30, 8, 10], [2, 2]),
        (CPRODUCTS_TRUNC, cpt, [1, 0, 30, 0, 10], [2, 2]),
        (CPRODUCTS_TRUNC, cpt, [1, 0, 30, 30, 10], [2, 2]),
        (CPRODUCTS_TRUNC, cpt, [1, 0, 250, 8, 10], [2, 2]),                                          # no room below the modulus
        (CPRODUCTS_TRUNC, cpt[:4] + [None], [1, 0, 30, 8, 10], [2, 2]),
        (CPRODUCTS_TRUNC, cpt[:3] + [None, rows(80)], [1, 0, 30, 8, 10], [2, 2]),
        (CPRODUCTS_TRUNC, cpt, [1, 0, 30, 8, 10], [2, None]),
        (TREE_STEP, [rows(2), rows(2), [1], None, None, None], [0, 0, 8, 0], [None, 2]),
        (TREE_STEP, [rows(2), rows(2), [1], None, None, None], [130, 0, 8, 0], [None, 2]),
        (TREE_STEP, [rows(3), rows(3), [1], None, None, None], [3, 0, 8, 0], [None, 2]),             # two rows a complex value
        (TREE_STEP, [rows(2), rows(2), [1], None, None, None], [2, 0, 0, 0], [None, 2]),
        (TREE_STEP, [rows(2), rows(2), [1], None, None, None], [2, 0, 254, 0], [None, 2]),
        (TREE_STEP, [rows(2), rows(2), [1], None, None, None], [2, 0, 8, 3], [None, 2]),
        (TREE_STEP, [rows(2), rows(2), [1], None, None, None], [2, 2, 8, 0], [None, 2]),
        (TREE_STEP, [rows(2), rows(2), [1], rows(2), None, None], [2, 1, 8, 0], [None, 2]),          # a final step carries nothing
        (TREE_STEP, [rows(2), rows(2), None, None, None, None], [2, 0, 8, 0], [None, 2]),
        (TREE_STEP, [rows(2), rows(2), [p], None, None, None], [2, 0, 8, 0], [None, 2]),             # 2^(-m) that is no residue
        (TREE_STEP, [rows(2), rows(2), [1], None, None, None], [2, 0, 8, 0], [None, None]),          # the odd value has nowhere to go
        (TREE_STEP, [rows(2), rows(2), [1], None, None, None], [2, 1, 8, 0], [None, None]),
        (TREE_STEP, [rows(2), rows(2), [1], rows(2), None, rows(3)], [2, 0, 8, 0], [6, None]),       # a pair needs both triples' rows
        (TREE_STEP, [rows(2), rows(2), [1], rows(2), rows(3), rows(3)], [2, 0, 8, 0], [None, None]),
        (TREE_STEP, [None, rows(2), [1], rows(2), rows(3), rows(3)], [2, 0, 8, 0], [6, None]),
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
            prm = (ctypes.c_int64 * 53)(*(list(params) + [0] * (53 - len(params))))
            rc = lib.hb_selftest_fxtrig(modulus, 4, what, ptrs, prm, optrs, count)
        else:
            rc, _ = run_trig(p, nl, what, operands, params, outs, count)
        assert rc == HB_ERR_BAD_ARG, i
    assert ok(run_trig(p, nl, FINISH_LOOKUP_MASK, flm, [1, 1, 2, 0, 1] + grp, [6, 4], count))                                                    # the good forms of the calls above
    assert ok(run_trig(p, nl, CPRODUCTS_TRUNC, cpt, [1, 0, 30, 8, 10], [2, 2], count))
    assert ok(run_trig(p, nl, TREE_STEP, [rows(2), rows(2), [1], rows(2), rows(3), rows(3)], [2, 0, 8, 0], [6, None], count))
    assert run_trig(p, nl, CPRODUCTS_TRUNC, [None] * 5, [1, 0, 30, 8, 10], [None, None], 0)[0] == 0                                               # count == 0: nothing to do
    assert run_trig(p, nl, TREE_STEP, [None, None, [1], None, None, None], [2, 0, 8, 0], [None, None], 0)[0] == 0
    assert run_trig(p, nl, TREE_STEP, [rows(2), rows(2), [1], None, None, None], [2, 0, 8, 0], [None, 2], -1)[0] == HB_ERR_BAD_ARG

    # an output laid over an input, or over the other output, is refused as the entry points refuse it: every operand in ONE buffer
    eb = 8 * nl * count                                                           # bytes a row
    buf = np.zeros((140 * count, nl), dtype=np.uint64)
    at = lambda r: buf.ctypes.data + r * eb
    one = ints_to_limbs([1], p, 32)
    tables = ints_to_limbs(list(range(1, 13)), p, 32)

    def call(what, params, ops, outs):
        ptrs = (ctypes.c_void_p * 8)(*(list(ops) + [None] * (8 - len(ops))))
        optrs = (ctypes.c_void_p * 2)(*(list(outs) + [None] * (2 - len(outs))))
        return lib.hb_selftest_fxtrig(modulus, nl, what, ptrs, (ctypes.c_int64 * 53)(*(list(params) + [0] * (53 - len(params)))), optrs, count)

    # FINISH_LOOKUP_MASK, a (1, 1) merge in slot 1 and a bit in slot 0, one pair in mode 0: bits 0, opened 1..4, ta 5..8, tab 9..12, nxt 13..15, 16..18; masked 20..25, kept 26..29
    ops = [at(0), at(1), at(5), at(9), tables.ctypes.data, at(13), at(16)]
    prm = [2, 1, 2, 0, 2, 1, 1, 0, 0, 0, 1, 1, 0, 0, 0, 8, 0]
    assert call(FINISH_LOOKUP_MASK, prm, ops, [at(20), at(26)]) == 0
    for outs in ([at(0), at(26)], [at(4), at(26)], [at(8), at(26)], [at(12), at(26)], [at(15), at(26)], [at(20), at(18)], [at(20), at(25)], [at(23), at(26)], [at(20), at(0)],
                 [at(20), at(11)], [at(26), at(26)], [at(20), tables.ctypes.data], [at(17), at(26)]):
        assert call(FINISH_LOOKUP_MASK, prm, ops, outs) == HB_ERR_BAD_ARG, outs
    # CPRODUCTS_TRUNC, two products in mode 0, width 20, kappa 10: opened 0..11, ta 12..17, tb 18..23, tab 24..29, bits 30..149 -- in a buffer of their own
    big = np.zeros((160 * count, nl), dtype=np.uint64)
    bt = lambda r: big.ctypes.data + r * eb
    ops = [bt(0), bt(12), bt(18), bt(24), bt(30)]
    assert call(CPRODUCTS_TRUNC, [2, 0, 20, 8, 10], ops, [bt(150), bt(154)]) == 0
    for outs in ([bt(8), bt(154)], [bt(17), bt(154)], [bt(150), bt(21)], [bt(150), bt(29)], [bt(149), bt(154)], [bt(150), bt(153)], [bt(150), bt(90)], [bt(154), bt(154)]):
        assert call(CPRODUCTS_TRUNC, [2, 0, 20, 8, 10], ops, outs) == HB_ERR_BAD_ARG, outs
    # TREE_STEP, two complex values and a carry into mode 0: opened 0..3, s 4..7, carry 8..9, ta 10..12, tb 13..15; masked 20..25, kept 26..27
    ops = [at(0), at(4), one.ctypes.data, at(8), at(10), at(13)]
    assert call(TREE_STEP, [4, 0, 8, 0], ops, [at(20), at(26)]) == 0
    for outs in ([at(3), at(26)], [at(7), at(26)], [at(9), at(26)], [at(12), at(26)], [at(15), at(26)], [at(20), at(25)], [at(20), at(9)], [at(26), at(26)], [at(20), at(1)]):
        assert call(TREE_STEP, [4, 0, 8, 0], ops, outs) == HB_ERR_BAD_ARG, outs
    assert call(TREE_STEP, [4, 1, 8, 0], [at(0), at(4), one.ctypes.data], [None, at(26)]) == 0                 # final: four rows of results
    for outs in ([None, at(3)], [None, at(5)]):
        assert call(TREE_STEP, [4, 1, 8, 0], [at(0), at(4), one.ctypes.data], outs) == HB_ERR_BAD_ARG, outs

"""CPU-only: honeybadgermpc_amd.progs.demux -- the wiring against the counts of the issue's table, the plan evaluated on Python ints
against demux_model, and the rows of csrc/hb_demux.hip run on the host through hb_selftest_demux -- the same HB_HD functions and the
same addressing the kernels run -- against Python ints: body by body on arbitrary residues, chained on cleartext bits with zero and
with random masks, and chained on dealt Shamir shares with the open done by host interpolation.  Exact equality: the result does not
depend on the masks."""
import ctypes
import random

import numpy as np
import pytest

import bitdec_cases as bc
import demux_cases as dc
from demux_cases import FINISH, LEAVES, MASK, bits_of, run_demux

from honeybadgermpc_amd.progs import demux as dx

CHAIN_MS = (1, 2, 3, 5, 6)


# ---- the wiring ----------------------------------------------------------------------------------------------------------------
def test_counts_reproduce_the_table():
    for m, levels, opened, products in dc.TABLE:
        assert dx.demux_levels(m) == levels, m
        assert [dx.demux_opened(m, l) for l in range(levels)] == opened, m
        assert [dx.demux_products(m, l) for l in range(levels)] == products, m
        assert dx.demux_triples(m) == (sum(opened), sum(products)) and dx.demux_group_rows(m) == sum(products), m
    assert dx.demux_triples(10) == (328, 1332) and dx.MAX_BITS == 12
    # the bit-by-bit chain the issue compares with: m - 1 rounds, 2 (2^m - 2) elements opened, 2^m - 2 products
    assert (10 - 1, 2 * (2 ** 10 - 2), 2 ** 10 - 2) == (9, 2044, 1022)


def test_plan():
    assert dx.demux_plan(1) == []
    assert dx.demux_plan(2) == [dx.DemuxLevel([(0, 1, 1)], None, [(0, 1)], 0)]
    assert dx.demux_plan(3) == [dx.DemuxLevel([(0, 1, 1)], (2, 1), [(0, 1)], 0), dx.DemuxLevel([(0, 2, 1)], None, [(0, 2)], 4)]
    assert dx.demux_plan(5) == [dx.DemuxLevel([(0, 1, 1), (2, 1, 1)], (4, 1), [(0, 1), (2, 3)], 0),
                                dx.DemuxLevel([(0, 2, 2)], (4, 1), [(0, 4)], 8),
                                dx.DemuxLevel([(0, 4, 1)], None, [(8, 4)], 24)]
    ten = dx.demux_plan(10)
    assert [lv.merges for lv in ten] == [[(0, 1, 1), (2, 1, 1), (4, 1, 1), (6, 1, 1), (8, 1, 1)], [(0, 2, 2), (4, 2, 2)], [(0, 4, 4)], [(0, 8, 2)]]
    assert [lv.carried for lv in ten] == [None, (8, 2), (8, 2), None]
    assert ten[3].sources == [(52, 16)] and [lv.out_row for lv in ten] == [0, 20, 52, 308]      # the carried group stayed in level 0's rows
    for m in range(1, dx.MAX_BITS + 1):
        plan = dx.demux_plan(m)
        assert len(plan) == dx.demux_levels(m) == (0 if m == 1 else (m - 1).bit_length()), m
        groups = [(i, 1) for i in range(m)]                             # (bit offset, width), from the least significant
        for l, lv in enumerate(plan):
            assert len(lv.merges) == len(groups) // 2 <= dx.MAX_BITS // 2 and (lv.carried is not None) == bool(len(groups) & 1), (m, l)
            for k, (bit, wl, wh) in enumerate(lv.merges):
                assert (bit, wl) == groups[2 * k] and (bit + wl, wh) == groups[2 * k + 1], (m, l, k)
            if lv.carried:
                assert lv.carried == groups[-1], (m, l)
            groups = [(bit, wl + wh) for bit, wl, wh in lv.merges] + ([lv.carried] if lv.carried else [])
            # the tab numbering of the level is a bijection onto range(demux_products)
            assert sorted(dc.tab_rows(lv).values()) == list(range(dx.demux_products(m, l))), (m, l)
        assert groups == [(0, m)], m


def test_refusals():
    for call in (lambda: dx.demux_levels(0), lambda: dx.demux_levels(13), lambda: dx.demux_plan(13), lambda: dx.demux_plan(True), lambda: dx.demux_plan(2.0),
                 lambda: dx.demux_opened(5, 3), lambda: dx.demux_opened(5, -1), lambda: dx.demux_products(1, 0), lambda: dx.demux_products(4, 2),
                 lambda: dx.demux_opened(4, True), lambda: dx.demux_triples(0), lambda: dx.demux_group_rows(13), lambda: dx.demux_model(4, 2),
                 lambda: dx.demux_model(-1, 2), lambda: dx.demux_model(0, 13), lambda: dx.demux_model(1.0, 2), lambda: dx.histogram_model([8], 3),
                 lambda: dx.lookup_model(0, [[1]] * 5, 2, 13)):
        with pytest.raises(ValueError):
            call()


def indices_for(m):
    if m <= 6:
        return list(range(1 << m))
    top, rnd = 1 << m, random.Random(m)
    return [0, 1, top - 1, top - 2] + [rnd.randrange(top) for _ in range(12)]


@pytest.mark.parametrize("m", range(1, dx.MAX_BITS + 1))
def test_plan_on_ints_is_the_model(m):
    for s in indices_for(m):
        want = dx.demux_model(s, m)
        assert sum(want) == 1 and want[s] == 1 and len(want) == 1 << m
        assert dc.plan_on_ints(dx, bits_of(s, m), m) == want, (m, s)


def test_companion_models():
    p = 97
    table = [[3, 200], [5, 6], [7, 8]]
    assert [dx.lookup_model(s, table, 2, p) for s in range(4)] == [[3, 6], [5, 6], [7, 8], [0, 0]]
    assert dx.histogram_model([0, 3, 3, 1, 3], 2) == [1, 1, 0, 3]
    assert dx.aggregate_model([0, 3, 3, 1], [[1, 2], [90, 4], [10, 6], [7, 8]], 2, p) == [[1, 2], [7, 8], [0, 0], [3, 10]]


# ---- the kernels' rows -------------------------------------------------------------------------------------------------------
def draw(rnd, p, n):
    return [rnd.choice([0, 1, p - 1, rnd.randrange(p), rnd.randrange(p)]) for _ in range(n)]


@pytest.mark.parametrize("p, nl", dc.HOST_FIELDS, ids=dc.FIELD_IDS)
def test_each_body_on_arbitrary_residues(p, nl):
    """the planes hold SHARES: any residues in every slot, the corners 0 and p - 1 among them"""
    rnd = random.Random(p % 1000 + 3)
    for m in (1, 2, 3, 4, 5, 6, 10):
        for count in (0, 1, 3):
            bits = [draw(rnd, p, count) for _ in range(m)]
            if m == 3:
                bits = [[p - 1] * count for _ in range(m)]
            if m == 1:
                rc, (out,) = run_demux(p, nl, LEAVES, [bits[0]], [1, 0], [2], count)
                assert rc == 0 and out == [(1 - b) % p for b in bits[0]] + bits[0], count
                continue
            rows = dx.demux_group_rows(m)
            groups = [draw(rnd, p, count) for _ in range(rows)]
            for level, lv in enumerate(dx.demux_plan(m)):
                n_open, n_prod = dx.demux_opened(m, level), dx.demux_products(m, level)
                ta, tab, opened = ([draw(rnd, p, count) for _ in range(r)] for r in (n_open, n_prod, n_open))
                rc, (masked,) = run_demux(p, nl, MASK, [bc.flat(bits), bc.flat(groups), bc.flat(ta)], [m, level], [n_open], count)
                assert rc == 0
                src = []
                for k, (_, wl, wh) in enumerate(lv.merges):
                    src += [[dc.factor(lv.sources, k, False, wl, [b[e] for b in bits], [g[e] for g in groups], p)[lo] for e in range(count)] for lo in range(1 << wl)]
                    src += [[dc.factor(lv.sources, k, True, wh, [b[e] for b in bits], [g[e] for g in groups], p)[hi] for e in range(count)] for hi in range(1 << wh)]
                assert len(src) == n_open
                assert masked == bc.flat([[(x - a) % p for x, a in zip(xs, as_)] for xs, as_ in zip(src, ta)]), (m, level, count)
                rc, (after,) = run_demux(p, nl, FINISH, [bc.flat(opened), bc.flat(ta), bc.flat(tab)], [m, level], [bc.flat(groups)], count)
                assert rc == 0
                want, off = [list(g) for g in groups], 0
                tab_rows = dc.tab_rows(lv)
                for k, (_, wl, wh) in enumerate(lv.merges):
                    for hi in range(1 << wh):
                        for lo in range(1 << wl):
                            r = tab_rows[(k, hi, lo)]
                            want[lv.out_row + r] = [bc.beaver(opened[off + lo][e], opened[off + (1 << wl) + hi][e], ta[off + lo][e], ta[off + (1 << wl) + hi][e],
                                                              tab[r][e], p) for e in range(count)]
                    off += (1 << wl) + (1 << wh)
                assert after == bc.flat(want), (m, level, count)       # and every row of another level is as it was
                groups = want


@pytest.mark.parametrize("p, nl", dc.HOST_FIELDS, ids=dc.FIELD_IDS)
@pytest.mark.parametrize("masks", ["zero", "random"])
def test_chain_on_cleartext_bits(p, nl, masks):
    rnd = random.Random(5)
    for m in CHAIN_MS:
        idx = list(range(1 << m)) if m <= 3 else [0, 1, (1 << m) - 1, (1 << m) - 2] + [rnd.randrange(1 << m) for _ in range(5)]
        for count in (0, 1, 3):
            for first in range(0, len(idx), 3) if count == 3 else (0,):
                ss = (idx[first:first + count] + [0, 0])[:count]
                planes = bc.flat([[bits_of(s, m)[i] for s in ss] for i in range(m)])

                def triples(level):
                    ta, tab = dc.level_triples(dx, m, level, count, p, rnd, zero=masks == "zero")
                    return [(bc.flat(ta), bc.flat(tab))]

                (out,) = dc.chain(dx, p, nl, 0, [planes], m, count, triples)
                assert out == bc.flat([[dx.demux_model(s, m)[j] for s in ss] for j in range(1 << m)]), (m, count, ss)


@pytest.mark.parametrize("p, nl", dc.HOST_FIELDS, ids=dc.FIELD_IDS)
def test_chain_on_shamir_shares(p, nl):
    """n = 4, t = 1: every party runs the rows on its shares, the open is interpolation on the host; every output plane reconstructs to
    the one-hot vector, from the first t + 1 parties and from the last"""
    n, t = 4, 1
    rnd = random.Random(9)
    for m in CHAIN_MS:
        for count in (0, 1, 3):
            ss = [rnd.randrange(1 << m) for _ in range(count)]
            if count == 3:
                ss[0], ss[1] = (1 << m) - 1, 0
            dealt = bc.deal(rnd, p, n, t, [bits_of(s, m)[i] for i in range(m) for s in ss])

            def triples(level):
                ta, tab = dc.level_triples(dx, m, level, count, p, rnd)
                a, ab = bc.deal(rnd, p, n, t, bc.flat(ta)), bc.deal(rnd, p, n, t, bc.flat(tab))
                return list(zip(a, ab))

            outs = dc.chain(dx, p, nl, t, dealt, m, count, triples)
            want = bc.flat([[dx.demux_model(s, m)[j] for s in ss] for j in range(1 << m)])
            if count:
                assert bc.reconstruct(p, t, outs) == want and bc.reconstruct(p, t, outs, first=2) == want, (m, count, ss)
            else:
                assert outs == [[]] * n


def test_refused_arguments_return_the_error_code():
    from honeybadgermpc_amd._capi import ints_to_limbs, load_library, np_ptr

    p, nl, count = dc.P64, 1, 3
    z = [0] * (64 * count)
    assert run_demux(p, nl, MASK, [z, z, z], [3, 0], [4], count)[0] == 0
    for params in ([0, 0], [13, 0], [3, 2], [3, -1], [1, 0], [1 << 40, 0]):
        assert run_demux(p, nl, MASK, [z, z, z], params, [4], count)[0] == dc.BAD_ARG, params
        assert run_demux(p, nl, FINISH, [z, z, z], params, [z], count)[0] == dc.BAD_ARG, params
    assert run_demux(p, nl, 3, [z, z, z], [3, 0], [4], count)[0] == dc.BAD_ARG
    assert run_demux(p, nl, MASK, [z, z, z], [3, 0], [4], -1)[0] == dc.BAD_ARG
    assert run_demux(p, nl, LEAVES, [z], [1, 0], [2], -1)[0] == dc.BAD_ARG
    # null operands where there is work; level 0 reads no stored group, level 1 of m = 3 does
    assert run_demux(p, nl, MASK, [z, None, z], [3, 0], [4], count)[0] == 0
    assert run_demux(p, nl, MASK, [z, None, z], [3, 1], [6], count)[0] == dc.BAD_ARG
    assert run_demux(p, nl, MASK, [None, z, z], [3, 0], [4], count)[0] == dc.BAD_ARG
    assert run_demux(p, nl, MASK, [z, z, None], [3, 0], [4], count)[0] == dc.BAD_ARG
    assert run_demux(p, nl, MASK, [z, z, z], [3, 0], [None], count)[0] == dc.BAD_ARG
    assert run_demux(p, nl, FINISH, [None, z, z], [3, 0], [z], count)[0] == dc.BAD_ARG
    assert run_demux(p, nl, FINISH, [z, z, None], [3, 0], [z], count)[0] == dc.BAD_ARG
    assert run_demux(p, nl, LEAVES, [None], [1, 0], [2], count)[0] == dc.BAD_ARG
    assert run_demux(p, nl, MASK, [None, None, None], [3, 0], [None], 0)[0] == 0         # nothing to do: nothing is looked at
    # an output lying over an input
    lib = load_library()
    buf = np.zeros((64 * count, nl), dtype=np.uint64)
    other = np.zeros((64 * count, nl), dtype=np.uint64)
    prm = (ctypes.c_int64 * 2)(3, 0)
    pl = np_ptr(ints_to_limbs([p], p + 1, 8 * nl))
    for what, ops in ((MASK, [other, other, buf]), (MASK, [buf, other, other]), (FINISH, [buf, other, other]), (FINISH, [other, other, buf]), (LEAVES, [buf])):
        ptrs = (ctypes.c_void_p * 8)(*([o.ctypes.data for o in ops] + [None] * (8 - len(ops))))
        outs = (ctypes.c_void_p * 2)(buf.ctypes.data + 8 * nl, None)
        assert lib.hb_selftest_demux(pl, nl, what, ptrs, prm, outs, count) == dc.BAD_ARG, what
    assert lib.hb_selftest_demux(pl, 2, MASK, ptrs, prm, outs, count) == dc.BAD_ARG

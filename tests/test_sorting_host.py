"""CPU-only: honeybadgermpc_amd.progs.sorting -- the merge-exchange network (closed index form against the filtered enumeration,
matchings, the zero-one principle, the counts), the host model, the plan's layout, and the three rows of csrc/hb_sort.hip run on
the host by hb_selftest_sort against Python-int formulas, over buffers of exactly the documented sizes."""
import itertools
import random

import numpy as np
import pytest

import sort_cases as sc
from conftest import BLS

P64 = (1 << 64) - 59
SIZES = list(range(0, 40)) + [63, 64, 65, 100, 257, 1000]


def _enumerate(n):
    """the layers of Algorithm M as filtered enumerations: [(p, r, d, [(i, i + d)])]"""
    out = []
    if n < 2:
        return out
    t = (n - 1).bit_length()
    p = 1 << (t - 1)
    while p:
        q, r, d = 1 << (t - 1), 0, p
        while True:
            out.append((p, r, d, [(i, i + d) for i in range(max(n - d, 0)) if i & p == r]))
            if q == p:
                break
            d, q, r = q - p, q >> 1, p
        p >>= 1
    return out


def test_closed_form_equals_the_filtered_enumeration_and_layers_are_matchings():
    from honeybadgermpc_amd.progs import sorting as so

    for n in SIZES:
        want = [(p.bit_length() - 1, r, d, pairs) for p, r, d, pairs in _enumerate(n) if pairs]
        got, pairs = so.layers(n), so.comparators(n)
        assert [(a, r, d) for a, r, d, _ in got] == [(a, r, d) for a, r, d, _ in want], n
        assert [cnt for *_, cnt in got] == [len(w[3]) for w in want], n
        assert pairs == [w[3] for w in want], n
        for layer in pairs:
            rows = [i for pair in layer for i in pair]
            assert len(set(rows)) == len(rows) and all(0 <= lo < hi < n for lo, hi in layer), n
    assert so.layers(0) == so.layers(1) == [] and so.comparators(1) == []
    for bad in (-1, 2.0, True, None):
        with pytest.raises(ValueError):
            so.layers(bad)


def test_zero_one_principle_exhaustively():
    from honeybadgermpc_amd.progs import sorting as so

    for n in range(0, 13):
        pairs = so.comparators(n)
        for bits in itertools.product((0, 1), repeat=n):
            v = list(bits)
            for layer in pairs:
                for lo, hi in layer:
                    if v[lo] >= v[hi]:
                        v[lo], v[hi] = v[hi], v[lo]
            assert v == sorted(bits), (n, bits)


def test_layer_and_comparator_counts():
    from honeybadgermpc_amd.progs import sorting as so

    for j in range(1, 11):
        ls = so.layers(1 << j)
        assert len(ls) == j * (j + 1) // 2 and sum(c for *_, c in ls) == (j * j - j + 4) * (1 << j) // 4 - 1, j
    for n, n_layers, n_cmp in ((5, 6, 9), (13, 10, 48), (1000, 55, 23499), (1024, 55, 24063)):
        ls = so.layers(n)
        assert (len(ls), sum(c for *_, c in ls)) == (n_layers, n_cmp), n


def test_sort_model():
    from honeybadgermpc_amd.progs import sorting as so

    rnd = random.Random(5)
    k = 10
    lim = 1 << (k - 2)
    for n in (0, 1, 2, 3, 5, 13, 64, 257):
        for batch in (1, 3):
            keys = [rnd.choice([-lim, lim - 1, 0, 0, 1]) if rnd.random() < 0.4 else rnd.randrange(-lim, lim) for _ in range(batch * n)]
            tags = list(range(batch * n))
            out = so.sort_model([keys, tags, [7 * t for t in tags]], n, k)
            for b in range(batch):
                sl = slice(b * n, (b + 1) * n)
                assert out[0][sl] == sorted(keys[sl]), (n, batch)
                assert sorted(zip(out[0][sl], out[1][sl], out[2][sl])) == sorted((keys[i], i, 7 * i) for i in range(b * n, (b + 1) * n))
    # ties swap: equal keys exchange their payloads
    assert so.sort_model([[4, 4], [0, 1]], 2, k) == [[4, 4], [1, 0]]
    assert so.sort_model([[3, 4], [0, 1]], 2, k) == [[3, 4], [0, 1]]
    for bad in ([lim], [-lim - 1], [0.5], [True]):
        with pytest.raises(ValueError):
            so.sort_model([bad + [0]], 2, k)
    so.sort_model([[lim - 1, -lim]], 2, k)
    for call in (lambda: so.sort_model([], 2, k), lambda: so.sort_model([[1, 2], [1]], 2, k), lambda: so.sort_model([[1, 2, 3]], 2, k), lambda: so.sort_model([[1]], 1, 1)):
        with pytest.raises(ValueError):
            call()


def test_sort_plan_totals_views_and_arguments():
    from honeybadgermpc_amd.progs import fixedpoint as fx
    from honeybadgermpc_amd.progs import sorting as so

    for n, batch, width, k, kappa in ((13, 3, 3, 8, 8), (5, 1, 1, 64, 32), (8, 2, 2, 8, 8), (2, 1, 1, 2, 0), (1, 2, 1, 8, 8), (0, 1, 2, 8, 8), (1000, 2, 4, 16, 16)):
        plan = so.SortPlan(n, batch, width, k, kappa)
        assert plan.layers == so.layers(n) and plan.n_layers == len(plan.layers)
        assert plan.slots == [batch * c for *_, c in plan.layers] and plan.total_slots == sum(plan.slots)
        assert plan.opens == sum(2 + fx.carry_levels(k - 1) for _ in plan.layers)
        assert (plan.bit_rows, plan.carry_rows, plan.swap_rows) == (k + kappa, 2 * k - 3, width)
        for kind, rows in (("bits", k + kappa), ("carry", fx.carry_triples(k - 1)), ("swap", width)):
            assert plan.rows(kind) == rows and plan.size(kind) == sum(rows * s for s in plan.slots)
            buf = np.arange(plan.size(kind) * 2, dtype=np.int64).reshape(plan.size(kind), 2)
            at = 0
            for l in range(plan.n_layers):
                v = plan.views(buf, kind, l)
                assert v.shape == (rows, plan.slots[l], 2) and plan.offset(kind, l) == at
                assert np.shares_memory(v, buf) and np.array_equal(v.reshape(-1, 2), buf[at:at + rows * plan.slots[l]])
                at += rows * plan.slots[l]
            assert at == plan.size(kind)                      # the blocks tile the buffer
            if plan.n_layers:
                for bad in (buf[:-1], buf.reshape(-1), np.zeros((plan.size(kind) + 1, 2), dtype=np.int64)):
                    with pytest.raises(ValueError):
                        plan.views(bad, kind, 0)
                with pytest.raises(ValueError):
                    plan.views(buf, kind, plan.n_layers)
            with pytest.raises(ValueError):
                plan.views(buf, "triples", 0)
    for args in ((-1, 1, 1, 8, 8), (5, 0, 1, 8, 8), (5, 1, 0, 8, 8), (5, 1, 257, 8, 8), (5, 1, 1, 1, 8), (5, 1, 1, 8, -1), (5.0, 1, 1, 8, 8), (5, 1, 1, 8, None),
                 ((1 << 31) + 1, 1, 1, 8, 8), (1 << 20, (1 << 20) + 1, 1, 8, 8)):
        with pytest.raises(ValueError):
            so.SortPlan(*args)
    assert so.SortPlan(5, 1, 256, 8, 8).swap_rows == 256


def _case(p, nl, n, batch, width, layer, k, kappa, seed):
    """the three rows of one layer against the formulas; operands are uniform residues (the rows are polynomial identities in them)"""
    rnd = random.Random(seed)
    slots, plane = batch * layer[3], batch * n
    table = [[rnd.randrange(p) for _ in range(plane)] for _ in range(width)]
    bits = [[rnd.randrange(p) for _ in range(slots)] for _ in range(k + kappa)]
    rc, (masked, r1) = sc.run_sort(p, nl, sc.CMP_MASK, [sc.flat(table), sc.flat(bits)], n, batch, width, layer, k, kappa, [slots, slots])
    assert rc == 0 and (masked, r1) == sc.cmp_mask_model(p, table, bits, n, batch, layer, k, kappa), (n, batch, width, layer)
    c, carry = ([rnd.randrange(p) for _ in range(slots)] for _ in range(2))
    if slots:
        c[0] = p - 1
    tp, tq, tpq = ([[rnd.randrange(p) for _ in range(slots)] for _ in range(width)] for _ in range(3))
    inv = [pow(2, -(k - 1), p)]
    rc, (out,) = sc.run_sort(p, nl, sc.SWAP_MASK, [sc.flat(table), c, r1, carry, sc.flat(tp), sc.flat(tq), inv], n, batch, width, layer, k, kappa, [2 * width * slots])
    assert rc == 0 and out == sc.flat(sc.swap_mask_model(p, table, c, r1, carry, tp, tq, n, batch, layer, k)), (n, batch, width, layer)
    opened = [[rnd.randrange(p) for _ in range(slots)] for _ in range(2 * width)]
    rc, (new,) = sc.run_sort(p, nl, sc.SWAP_FINISH, [sc.flat(opened), sc.flat(tp), sc.flat(tq), sc.flat(tpq)], n, batch, width, layer, k, kappa, [sc.flat(table)])
    want = sc.swap_finish_model(p, table, opened, tp, tq, tpq, n, batch, layer)
    assert rc == 0 and new == sc.flat(want), (n, batch, width, layer)
    touched = {row for s in range(slots) for row in sc.slot_rows(s, n, layer)}
    assert len(touched) == 2 * slots                                               # a matching, across the arrays too
    for w in range(width):
        assert all(new[w * plane + i] == table[w][i] for i in range(plane) if i not in touched)
    return table, tp, tq, c, r1, carry, out


@pytest.mark.parametrize("p, nl", [(BLS, 4), (P64, 1)], ids=["bls", "2^64-59"])
def test_selftest_rows_against_python_ints(p, nl):
    from honeybadgermpc_amd.progs import sorting as so

    k, kappa = 8, 8
    layers13 = so.layers(13)
    assert {(a, bool(r)) for a, r, _, _ in layers13} >= {(0, False), (0, True), (1, False), (1, True), (3, False)} and len({c for *_, c in layers13}) > 3
    assert any(c & (c - 1) for *_, c in layers13)                                  # counts that are no power of two
    seed = 0
    for batch, width in ((1, 1), (3, 3), (1, 3), (3, 1)):
        for layer in layers13:
            _case(p, nl, 13, batch, width, layer, k, kappa, seed)
            seed += 1
    _case(p, nl, 16, 2, 2, (3, 8, 8, 0), k, kappa, 90)                             # a = 3, r = p: the last layer group of n = 16 has none (cnt 0)
    _case(p, nl, 32, 1, 2, (3, 8, 8, 8), k, kappa, 91)                             # a = 3, r = p
    _case(p, nl, 2, 1, 1, (0, 0, 1, 1), k, kappa, 92)                              # one slot
    _case(p, nl, 2, 1, 3, (0, 0, 1, 0), k, kappa, 93)                              # no slot
    _case(p, nl, 13, 3, 1, (1, 2, 2, 0), k, kappa, 94)
    if nl == 4:
        _case(p, nl, 5, 2, 2, so.layers(5)[2], 64, 32, 95)


@pytest.mark.parametrize("p, nl", [(BLS, 4), (P64, 1)], ids=["bls", "2^64-59"])
def test_swap_mask_decides_the_swap_of_real_comparisons(p, nl):
    """with the comparison's true c, r1 and carry: u opens to [key_lo >= key_hi] -- ties included -- for keys at both ends of the range"""
    k, kappa, n, batch, width = 8, 8, 2, 6, 2
    layer = (0, 0, 1, 1)
    lim = 1 << (k - 2)
    pairs = [(-lim, lim - 1), (lim - 1, -lim), (5, 5), (-lim, -lim), (0, 1), (3, -2)]
    rnd = random.Random(11)
    keys = [v % p for pair in pairs for v in pair]
    table = [keys, [rnd.randrange(p) for _ in keys]]
    bit_rows = [[rnd.getrandbits(1) for _ in range(batch)] for _ in range(k + kappa)]
    rc, (masked, r1) = sc.run_sort(p, nl, sc.CMP_MASK, [sc.flat(table), sc.flat(bit_rows)], n, batch, width, layer, k, kappa, [batch, batch])
    assert rc == 0
    carry = [int(masked[s] % (1 << (k - 1)) >= r1[s]) for s in range(batch)]        # the carry of c2 + (2^m - 1 - r1) + 1
    zero = [[0] * batch] * width
    rc, (out,) = sc.run_sort(p, nl, sc.SWAP_MASK, [sc.flat(table), masked, r1, carry, sc.flat(zero), sc.flat(zero), [pow(2, -(k - 1), p)]], n, batch, width, layer, k,
                             kappa, [2 * width * batch])
    assert rc == 0
    rows = sc.unflat(out, 2 * width)
    assert rows[0] == rows[2] == [int(lo >= hi) for lo, hi in pairs]
    assert rows[1] == [(lo - hi) % p for lo, hi in pairs]


def test_selftest_refuses_bad_layers_and_parameters():
    p, nl, k, kappa = BLS, 4, 8, 8
    table, bits = [0] * 13, [0] * (16 * 6)
    for layer in ((0, 0, 2, 1), (1, 2, 4, 1), (1, 1, 2, 1), (0, 0, 1, 7), (0, 0, 13, 0), (0, 0, 0, 1), (31, 0, 1, 1), (-1, 0, 1, 1), (0, 0, 1, -1), (2, 4, 4, 5)):
        rc, _ = sc.run_sort(p, nl, sc.CMP_MASK, [table, bits], 13, 1, 1, layer, k, kappa, [6, 6])
        assert rc == 2, layer
    for n, batch in ((1, 1), (13, 0), ((1 << 31) + 1, 1)):
        assert sc.run_sort(p, nl, sc.CMP_MASK, [table, bits], n, batch, 1, (0, 0, 1, 0), k, kappa, [6, 6])[0] == 2
    good = (0, 0, 1, 6)
    assert sc.run_sort(p, nl, sc.CMP_MASK, [table, bits], 13, 1, 1, good, k, kappa, [6, 6])[0] == 0
    assert sc.run_sort(p, nl, sc.CMP_MASK, [table, bits], 13, 1, 1, good, 1, kappa, [6, 6])[0] == 2
    assert sc.run_sort(p, nl, sc.CMP_MASK, [table, bits], 13, 1, 1, good, 200, 60, [6, 6])[0] == 2          # k + kappa + 1 would wrap
    assert sc.run_sort(p, nl, sc.CMP_MASK, [table, None], 13, 1, 1, good, k, kappa, [6, 6])[0] == 2
    assert sc.run_sort(p, nl, 3, [table, bits], 13, 1, 1, good, k, kappa, [6, 6])[0] == 2
    six = [0] * 6
    ops = [table, six, six, six, six, six, [pow(2, -7, p)]]
    assert sc.run_sort(p, nl, sc.SWAP_MASK, ops, 13, 1, 1, good, k, kappa, [12])[0] == 0
    assert sc.run_sort(p, nl, sc.SWAP_MASK, ops, 13, 1, 0, good, k, kappa, [12])[0] == 2
    assert sc.run_sort(p, nl, sc.SWAP_MASK, ops, 13, 1, 257, good, k, kappa, [12])[0] == 2
    assert sc.run_sort(p, nl, sc.SWAP_MASK, ops[:6] + [None], 13, 1, 1, good, k, kappa, [12])[0] == 2
    assert sc.run_sort(p, nl, sc.SWAP_FINISH, [six + six, six, six, six], 13, 1, 0, good, k, kappa, [table])[0] == 2

"""CPU-only: the less-than half of honeybadgermpc_amd.share_comparison -- the host model against tests/golden/less_than.json (written by
scratch/gen_less_than_golden.py from the reference's own LessThan mixin driven over cleartext shares with recorded draws) and against
[a < b] itself, and the steps of csrc/hb_lt.hip run on the host through hb_selftest_lt -- the same rows, arithmetic and addressing,
that the kernel runs -- against Python ints, singly and chained into the whole protocol with the tree's operator folded in Python.
Exact equality."""
import json
import os
import random
import re

import pytest

from conftest import BLS, REPO
from selftest_cases import run_lt as run

from honeybadgermpc_amd import share_comparison as sc

GOLDILOCKS = 0xFFFFFFFF00000001
P64 = (1 << 64) - 59
P256 = (1 << 256) - 189
FIELDS = [(BLS, 4), (P256, 4), (P64, 1), (GOLDILOCKS, 1)]
FIELD_IDS = ["bls", "2^256-189", "2^64-59", "goldilocks"]
MASK, LEAVES, XOR_MASK, DMASK, MID, XOR_FINISH = range(6)
COUNTS = (0, 1, 257)
MODES = (sc.DIRECT, sc.REFERENCE)


def golden():
    with open(os.path.join(REPO, "tests", "golden", "less_than.json")) as f:
        return json.load(f)


def beaver(d, e, a, b, ab, p):
    return (d * e + d * b + e * a + ab) % p


def bit_planes(values, L):
    """[plane][element], least significant first, flat"""
    return [(v >> i) & 1 for i in range(L) for v in values]


def fold(g, q, p):
    """the root's g of the tree's operator over planes [node][element], most significant first, adjacent pairs level by level"""
    while len(g) > 1:
        ng, nq = [], []
        for j in range(len(g) // 2):
            ng.append([(g1 + p1 * g2) % p for g1, p1, g2 in zip(g[2 * j], q[2 * j], g[2 * j + 1])])
            nq.append([p1 * p2 % p for p1, p2 in zip(q[2 * j], q[2 * j + 1])])
        if len(g) & 1:
            ng.append(g[-1])
            nq.append(q[-1])
        g, q = ng, nq
    return g[0]


def d0_select(d, s1, s2, sp, L, p):
    """share_comparison.py:186-199 with [s_1], [s_2], [s_1 s_2] any residues"""
    d0 = d & 1
    x1, x2, x12 = d0 ^ (d < (1 << (L - 1))), d0 ^ (d < (1 << (L - 2))), d0 ^ (d < ((1 << (L - 1)) + (1 << (L - 2))))
    return ((1 - s1 - s2 + sp) * d0 + (s2 - sp) * x2 + (s1 - sp) * x1 + sp * x12) % p


def edge_pairs(p):
    """(c, r): c on the corners and with single bits at the words' edges; r equal to c, beside it, and differing in bit 0 or the top bit only"""
    L = p.bit_length()
    cs = [0, 1, p - 1, (1 << (L - 1)) - 1] + [1 << k for k in (31, 32, 63, 64) if k < L and (1 << k) < p] + [(1 << k) - 1 for k in (32, 64) if k < L]
    pairs = []
    for c in cs:
        for r in (c, c + 1, c - 1, c ^ 1, c ^ (1 << (L - 1))):
            if 0 <= r < p:
                pairs.append((c, r))
    return pairs


def edge_masks(p):
    L = p.bit_length()
    lo, hi = 1 << (L - 2), 1 << (L - 1)
    return [v for v in (lo - 1, lo, hi - 1, hi, lo + hi - 1, lo + hi, p - 1, 0) if v < p]


# ---- the host model against the reference and against the comparison itself -----------------------------------------------
def test_model_reproduces_the_reference_runs():
    g = golden()
    assert int(g["modulus"]) == BLS and len(g["cases"]) >= 40
    half = (BLS - 1) // 2
    kinds = set()
    for c in g["cases"]:
        a, b, r, s = (int(c[k]) for k in "abrs")
        assert a < half and b < half
        ref = sc.less_than_model(a, b, r, s, BLS, sc.REFERENCE)
        assert (ref["c"], ref["d"], ref["out"]) == (int(c["c"]), int(c["d"]), int(c["out"])), c
        assert ref["out"] == (1 if a < b else 0) == sc.less_than_model(a, b, r, s, BLS, sc.DIRECT)["out"] == sc.less_than_model(a, b, r, None, BLS)["out"]
        kinds.add("eq" if a == b else ("+1" if b == a + 1 else ("-1" if b == a - 1 else ("<" if a < b else ">"))))
        kinds |= {k for k, hit in (("a0", a == 0), ("btop", b == (BLS - 3) // 2)) if hit}
    assert kinds == {"eq", "+1", "-1", "<", ">", "a0", "btop"}


@pytest.mark.parametrize("p, nl", FIELDS, ids=FIELD_IDS)
def test_model_is_the_comparison_on_valid_inputs(p, nl):
    rnd = random.Random(p % 1033)
    half = (p - 1) // 2
    for i in range(3000):
        a = rnd.randrange(half)
        b = a if i % 6 == 0 else (min(a + 1, half - 1) if i % 6 == 1 else rnd.randrange(half))
        r, s = rnd.randrange(p), rnd.randrange(p)
        want = 1 if a < b else 0
        ref, direct = sc.less_than_model(a, b, r, s, p, sc.REFERENCE), sc.less_than_model(a, b, r, s, p, sc.DIRECT)
        assert ref["out"] == want == direct["out"], (a, b, r, s)
        assert direct["w"] == (1 if r > direct["c"] else 0) == ref["x"] & 1 and ref["c"] == direct["c"] == (2 * (a - b) + r) % p


def test_counts_and_parameter_checks():
    assert [sc.less_than_triples(L) for L in (255, 256, 64)] == [508, 510, 126]
    assert [sc.less_than_triples(L, sc.REFERENCE) for L in (255, 256, 64)] == [510, 512, 128]
    assert [sc.less_than_opens(L) for L in (255, 256, 257, 64, 65, 2, 3)] == [10, 10, 11, 8, 9, 3, 4]
    assert [sc.less_than_opens(L, sc.REFERENCE) for L in (255, 256, 64)] == [11, 11, 9]
    assert sc.less_than_opens(BLS.bit_length()) == 10 and sc.less_than_opens(P64.bit_length(), sc.REFERENCE) == 9
    for bad in (1, 0, -1, 2.0, True, None):
        with pytest.raises(ValueError):
            sc.less_than_triples(bad)
        with pytest.raises(ValueError):
            sc.less_than_opens(bad)
    for bad in (2, -1, None, True):
        with pytest.raises(ValueError):
            sc.less_than_triples(255, bad)
        with pytest.raises(ValueError):
            sc.less_than_opens(255, bad)
        with pytest.raises(ValueError):
            sc.less_than_model(1, 2, 3, 4, BLS, bad)

    class Co:                                                            # the mode is checked before anything touches the device
        ctx = None

    import asyncio

    for kw in ({"mode": sc.REFERENCE}, {"mode": sc.REFERENCE, "s": 1}, {"mode": sc.REFERENCE, "s_bits": 1}, {"mode": 2}):
        with pytest.raises(ValueError):
            asyncio.run(sc.less_than(Co(), None, None, None, None, None, **kw))


# ---- the kernels' bodies on the host -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("p, nl", FIELDS, ids=FIELD_IDS)
def test_selftest_bodies_against_python_ints(p, nl):
    """every operand any residue (a share of a bit is one), the corners in front"""
    rnd = random.Random(p % 1039)
    L = p.bit_length()
    for count in COUNTS:
        draw = lambda k=count: [rnd.choice((0, 1, p - 1, rnd.randrange(p))) for _ in range(k)]    # noqa: E731
        a, b, r = draw(), draw(), draw()
        for bb in (b, None):
            rc, (got,) = run(p, nl, MASK, [a, bb, r], 0, [1], count)
            assert rc == 0 and got == [(2 * (x - (y if bb else 0)) + z) % p for x, y, z in zip(a, b, r)], (count, bb is None)
        c = ([v for v, _ in edge_pairs(p)] + [rnd.randrange(p) for _ in range(count)])[:count]
        planes = draw(L * count)
        for mode in MODES:
            rc, (g, q) = run(p, nl, LEAVES, [c, planes], mode, [L, L], count)
            want_g, want_q = [], []
            for j in range(L):
                i = L - 1 - j
                for e in range(count):
                    rb, cb = planes[i * count + e], (c[e] >> i) & 1
                    want_g.append(0 if cb else rb)
                    if mode == sc.DIRECT:
                        want_q.append(rb if cb else (1 - rb) % p)
                    else:
                        want_q.append((2 - rb) % p if cb else (1 + rb) % p)
            assert rc == 0 and g == want_g and q == want_q, (count, mode)
        r0, w, pa, qa, pb, qb = (draw() for _ in range(6))
        want_u = [(1 - y) % p if x & 1 else y for x, y in zip(c, r0)]
        rc, (u, m) = run(p, nl, XOR_MASK, [c, r0, w, pa, qa], 0, [1, 2], count)
        assert rc == 0 and u == want_u and m == [(x - y) % p for x, y in zip(want_u, pa)] + [(x - y) % p for x, y in zip(w, qa)], count
        x, s, s_planes = draw(), draw(), draw(L * count)
        s0, s1, s2 = s_planes[:count], s_planes[(L - 1) * count:], s_planes[(L - 2) * count:(L - 1) * count]
        rc, (u, m) = run(p, nl, DMASK, [c, r0, x, s, s_planes, pa, qa, pb, qb], 0, [1, 5], count)
        want = [[(y + z) % p for y, z in zip(s, x)]] + [[(y - z) % p for y, z in zip(v, t)] for v, t in ((want_u, pa), (s0, qa), (s1, pb), (s2, qb))]
        assert rc == 0 and u == want_u and m == [v for row in want for v in row], count
        opened, pqa, pqb, pc, qc = draw(5 * count), draw(), draw(), draw(), draw()
        opened[:count] = (edge_masks(p) + opened[:count])[:count]                            # d on both sides of the three thresholds
        o = [opened[k * count:(k + 1) * count] for k in range(5)]
        rc, (v, d0, m) = run(p, nl, MID, [opened, want_u, s_planes, pa, qa, pqa, pb, qb, pqb, pc, qc], 0, [1, 1, 2], count)
        us0 = [beaver(o[1][e], o[2][e], pa[e], qa[e], pqa[e], p) for e in range(count)]
        sp = [beaver(o[3][e], o[4][e], pb[e], qb[e], pqb[e], p) for e in range(count)]
        want_v = [(want_u[e] + s0[e] - 2 * us0[e]) % p for e in range(count)]
        want_d0 = [d0_select(o[0][e], s1[e], s2[e], sp[e], L, p) for e in range(count)]
        assert rc == 0 and v == want_v and d0 == want_d0 and m == [(y - z) % p for y, z in zip(want_v, pc)] + [(y - z) % p for y, z in zip(want_d0, qc)], count
        op2, tpq = draw(2 * count), draw()
        rc, (out,) = run(p, nl, XOR_FINISH, [op2, want_v, want_d0, pc, qc, tpq], 0, [1], count)
        assert rc == 0 and out == [(want_v[e] + want_d0[e] - 2 * beaver(op2[e], op2[count + e], pc[e], qc[e], tpq[e], p)) % p for e in range(count)], count
    # the largest operands everywhere
    big = [p - 1]
    rc, (v, d0, m) = run(p, nl, MID, [big * 5, big, big * L] + [big] * 8, 0, [1, 1, 2], 1)
    bb = beaver(*big * 5, p)
    assert rc == 0 and v == [(2 * (p - 1) - 2 * bb) % p] and d0 == [d0_select(p - 1, p - 1, p - 1, bb, L, p)]
    # what is checked: L, the mode, the selector, NULL operands, a negative count
    assert run(p, nl, LEAVES, [big, big * L], 0, [L, L], 1, L=L - 1)[0] == 2 and run(p, nl, LEAVES, [big, big * L], 2, [L, L], 1)[0] == 2
    assert run(p, nl, DMASK, [big] * 4 + [big * L] + [big] * 4, 0, [1, 5], 1, L=L + 1)[0] == 2
    assert run(p, nl, MID, [big * 5, big, big * L] + [big] * 8, 0, [1, 1, 2], 1, L=0)[0] == 2
    assert run(p, nl, 6, [big] * 6, 0, [1], 1)[0] == 2 and run(p, nl, MASK, [big, None, None], 0, [1], 1)[0] == 2 and run(p, nl, MASK, [big] * 3, 0, [1], -1)[0] == 2


def chain(p, nl, mode, cases, rnd):
    """the bodies chained into the whole protocol for one party holding the values themselves (a share of degree 0), the tree's
    operator folded in Python: -> [{"c", "x" | "w", "d", "out"}] as less_than_model returns them.  cases: (a, b, r, s)."""
    L, n = p.bit_length(), len(cases)
    a, b, r, s = ([c[k] for c in cases] for k in range(4))
    draw = lambda: [rnd.randrange(p) for _ in range(n)]    # noqa: E731
    rc, (c,) = run(p, nl, MASK, [a, b, r], 0, [1], n)
    assert rc == 0
    r_planes = bit_planes(r, L)
    rc, (g, q) = run(p, nl, LEAVES, [c, r_planes], mode, [L, L], n)
    assert rc == 0
    root = fold([g[j * n:(j + 1) * n] for j in range(L)], [q[j * n:(j + 1) * n] for j in range(L)], p)
    ta, tb, tc = ((x, y, [v * w % p for v, w in zip(x, y)]) for x, y in ((draw(), draw()) for _ in range(3)))
    if mode == sc.DIRECT:
        rc, (u, m) = run(p, nl, XOR_MASK, [c, r_planes[:n], root, ta[0], ta[1]], 0, [1, 2], n)
        assert rc == 0
        rc, (out,) = run(p, nl, XOR_FINISH, [m, u, root, *ta], 0, [1], n)
        assert rc == 0
        return [{"c": c[e], "w": root[e], "out": out[e]} for e in range(n)]
    s_planes = bit_planes(s, L)
    rc, (u, m) = run(p, nl, DMASK, [c, r_planes[:n], root, s, s_planes, ta[0], ta[1], tb[0], tb[1]], 0, [1, 5], n)
    assert rc == 0
    rc, (v, d0, m2) = run(p, nl, MID, [m, u, s_planes, *ta, *tb, tc[0], tc[1]], 0, [1, 1, 2], n)
    assert rc == 0
    rc, (out,) = run(p, nl, XOR_FINISH, [m2, v, d0, *tc], 0, [1], n)
    assert rc == 0
    return [{"c": c[e], "x": root[e], "d": m[e], "out": out[e]} for e in range(n)]


@pytest.mark.parametrize("p, nl", FIELDS, ids=FIELD_IDS)
def test_chained_bodies_and_folded_leaves_equal_the_model(p, nl):
    """the leaves folded by the tree's operator give the model's x and w, and the steps around the tree the model's c, d and result:
    at the edge values of c and r (any pair is reached by a = (c - r) / 2, b = 0), with s and d = s + x on both sides of 2^(L-2),
    2^(L-1) and their sum, s = p - 1 and s = 0, and on valid pairs"""
    rnd = random.Random(p % 1049)
    L, half, inv2 = p.bit_length(), (p - 1) // 2, pow(2, -1, p)
    cases = []
    masks = edge_masks(p)
    for k, (c, r) in enumerate(edge_pairs(p)):
        a = (c - r) * inv2 % p
        x = sc.less_than_model(a, 0, r, 0, p, sc.REFERENCE)["x"]
        t = masks[k % len(masks)]
        cases += [(a, 0, r, t), (a, 0, r, (t - x) % p)]                    # s at a threshold, d at a threshold
    for i in range(24):
        a = rnd.randrange(half)
        cases.append((a, a if i % 4 == 0 else rnd.randrange(half), rnd.randrange(p), rnd.choice(masks[:6] + [0, rnd.randrange(p)])))    # not p - 1: s + x would wrap
    seen_d = set()
    for mode in MODES:
        got = chain(p, nl, mode, cases, rnd)
        for (a, b, r, s), res in zip(cases, got):
            assert res == sc.less_than_model(a, b, r, s, p, mode), (mode, a, b, r, s)
            if mode == sc.REFERENCE:
                seen_d.add(res["d"])
        for (a, b, r, s), res in zip(cases[-24:], got[-24:]):
            assert res["out"] == (1 if a < b else 0)
    lo, hi = 1 << (L - 2), 1 << (L - 1)
    assert {v for v in (lo - 1, lo, hi - 1, hi, lo + hi - 1, lo + hi) if v < p} <= seen_d


def test_entry_points_are_declared_and_bound():
    from honeybadgermpc_amd import _capi
    from honeybadgermpc_amd.progs import fixedpoint

    text = open(os.path.join(REPO, "include", "hbmpc_hip.h")).read()
    for name in ("hb_lt_mask", "hb_lt_leaves", "hb_lt_xor_mask", "hb_lt_dmask", "hb_lt_mid", "hb_lt_xor_finish", "hb_selftest_lt"):
        assert re.search(r"\bint " + name + r"\s*\(", text) and name in _capi.SYMBOLS
    assert (_capi.HB_LT_DIRECT, _capi.HB_LT_REFERENCE) == (0, 1) == (sc.DIRECT, sc.REFERENCE)
    for name, value in (("HB_LT_DIRECT", 0), ("HB_LT_REFERENCE", 1), ("HB_LT_SELFTEST_MASK", 0), ("HB_LT_SELFTEST_XOR_FINISH", 5)):
        assert re.search(rf"#define {name} {value}\b", text) and getattr(_capi, name) == value
    for name in ("lt_mask", "lt_leaves", "lt_xor_mask", "lt_dmask", "lt_mid", "lt_xor_finish", "less_than", "less_than_model"):
        assert callable(getattr(sc, name))
    assert sc.carry_tree is fixedpoint.carry_tree

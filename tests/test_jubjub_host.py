"""CPU-only: the host model honeybadgermpc_amd.elliptic_curve against tests/golden/jubjub.json (written by scratch/gen_jubjub_golden.py
from the reference's own Jubjub, Point and mimc_plain), and the Jubjub steps (csrc/hb_jj.hip) run on the host through hb_selftest_jj
-- the same rows, arithmetic and addressing, that the kernel runs -- against the golden file, the host model and Python ints.
Exact equality."""
import itertools
import json
import os
import random
import re

import pytest

from conftest import BLS, REPO
from selftest_cases import run_jj as run

from honeybadgermpc_amd.elliptic_curve import Ideal, Jubjub, Point, Subgroup
from honeybadgermpc_amd.progs.mimc import mimc_plain

PRIMES = [(BLS, 4), (13, 4), (53, 4), ((1 << 256) - 189, 4), ((1 << 255) - 19, 4), (13, 1), ((1 << 64) - 59, 1), (0xFFFFFFFF00000001, 1)]
IDS = ["bls", "13w", "53w", "2^256-189", "2^255-19", "13n", "2^64-59", "goldilocks"]
P64 = (1 << 64) - 59
SCALAR_MUL, DOUBLE_TABLE, MASK, STAGE1, STAGE2, STAGE3, SCALE = range(7)
N_BCAST, P_BCAST = 1, 2
R_J = 6554484396890773809930967563523245729705921265872317281365359162392183254199


def golden():
    with open(os.path.join(REPO, "tests", "golden", "jubjub.json")) as f:
        g = json.load(f)
    assert int(g["modulus"]) == BLS and len(g["adds"]) >= 60 and len(g["muls"]) == 16 and len(g["encrypts"]) == 4
    return g


def _xy(v):
    return int(v[0]), int(v[1])


# ---- Python-int models of the stages ------------------------------------------------------------------------------------------
def beaver(p, d, e, tp, tq, tpq):
    return (d * e + d * tq + e * tp + tpq) % p


def mask_ref(p, x1, y1, x2, y2, tp, tq):
    return [(x1 - tp[0]) % p, (x2 - tq[0]) % p, (y1 - tp[1]) % p, (y2 - tq[1]) % p, (x1 - tp[2]) % p, (y2 - tq[2]) % p, (y1 - tp[3]) % p, (x2 - tq[3]) % p]


def stage1_ref(p, A, tp, tq, tpq, rx, ry):
    xp, yp, a, b = (beaver(p, A[2 * k], A[2 * k + 1], tp[k], tq[k], tpq[k]) for k in range(4))
    return [(xp - tp[4]) % p, (yp - tq[4]) % p, (a + b - tp[5]) % p, (rx - tq[5]) % p, (yp + xp - tp[6]) % p, (ry - tq[6]) % p]


def stage2_ref(p, B, tp, tq, tpq, rx, ry, d):
    w, u, v = (beaver(p, B[2 * (k - 4)], B[2 * (k - 4) + 1], tp[k], tq[k], tpq[k]) for k in (4, 5, 6))
    return [u, v, (1 + d * w - tp[7]) % p, (rx - tq[7]) % p, (1 - d * w - tp[8]) % p, (ry - tq[8]) % p]


def stage3_ref(p, C, tp, tq, tpq):
    return [beaver(p, C[0], C[1], tp[7], tq[7], tpq[7]), beaver(p, C[2], C[3], tp[8], tq[8], tpq[8])]


def cols(rows):
    """[row][i] -> [i][row]"""
    return [list(c) for c in zip(*rows)]


def flat(rows):
    return [v for row in rows for v in row]


# ---- the host model ---------------------------------------------------------------------------------------------------
def test_host_model_equals_the_reference():
    g = golden()
    curve = Jubjub()
    assert (curve.p, curve.a, curve.d) == (BLS, int(g["a"]), int(g["d"])) and curve.a == BLS - 1 and curve.is_complete() and curve.is_smooth()
    assert curve == Jubjub(-1, -(10240 * pow(10241, -1, BLS))) and curve != Jubjub(-1, 2, P64) and Subgroup.BLS12_381 == BLS
    gp = Point(*_xy(g["GP"]))
    assert (gp.x, int(g["r_J"])) == (5, R_J)
    pts = set()
    for c in g["adds"]:
        P, Q, S = (Point(*_xy(c[k])) for k in ("P", "Q", "sum"))
        assert P + Q == S and Q + P == S and P - (-Q) == S
        pts |= {(P.x, P.y), (Q.x, Q.y)}
        if P == Q:
            assert P.double() == S
    assert {(0, 1), (0, BLS - 1), (gp.x, gp.y), (BLS - 5, gp.y)} <= pts and len(pts) >= 11
    assert any(c["P"] == c["Q"] for c in g["adds"]) and sum(_xy(c["sum"]) == (0, 1) for c in g["adds"]) >= 7
    ns = set()
    for c in g["muls"]:
        n, P, out = int(c["n"]), Point(*_xy(c["P"])), Point(*_xy(c["out"]))
        assert P * n == out and n * P == out
        ns.add(n)
    assert {1, 2, 3, 8 * R_J - 1, 8 * R_J, 8 * R_J + 1, BLS - 1, -5} <= ns and sum(n.bit_length() >= 254 for n in ns) >= 9
    assert gp * (8 * R_J) == Point(0, 1) and gp * R_J != Point(0, 1)
    for c in g["encrypts"]:
        a, pub = int(c["a"]), Point(*_xy(c["pub"]))
        assert gp * int(c["priv"]) == pub and a * gp == Point(*_xy(c["a_"]))
        k = (a * pub).x
        assert k == int(c["k"]) and [(mimc_plain(i, k) + int(m)) % BLS for i, m in enumerate(c["ms"])] == [int(v) for v in c["cs"]]


def test_host_model_behaviour():
    gp = Point(5, 6846412461894745224441235558443359243034138132682534265960483512729196124138)
    curve = gp.curve
    with pytest.raises(Exception, match="not on the given curve"):
        Point(5, 7)
    with pytest.raises(Exception, match="not of type Jubjub"):
        Point(0, 1, curve="jubjub")
    with pytest.raises(Exception, match="isn't an int"):
        gp * 2.0
    with pytest.raises(Exception, match="not smooth"):
        Jubjub(3, 3)
    with pytest.raises(Exception, match="different curves"):
        gp + Point(0, 1, Jubjub(-1, 2, P64))
    ideal = gp * 0
    assert type(ideal) is Ideal and ideal == Ideal(curve) and ideal != gp and gp != ideal and -ideal is ideal and ideal * 7 is ideal
    assert gp + ideal == gp and ideal + gp == gp and (-gp).x == BLS - 5 and (-gp).y == gp.y
    assert gp * -3 == -(gp * 3) == (-gp) * 3 and gp * 3 == gp + gp + gp and gp.double() == gp * 2 and gp - gp == Point(0, 1)
    assert (gp[0], gp[1]) == (gp.x, gp.y) and Point(gp.x + BLS, gp.y) == gp and str(ideal) == "Ideal"
    assert curve.contains_point(gp) and str(curve) == repr(curve)
    # the 64-bit field carries a curve: p = 1 mod 4 makes -1 a square, 2 is a non-square
    small = Jubjub(-1, 2, P64)
    assert small.is_complete() and P64 % 4 == 1 and not Jubjub(-1, 4, P64).is_complete()
    q = narrow_point(random.Random(1), small)
    assert q * 5 == q + q + q + q + q and q * (P64 - 1) + q == q * P64


def narrow_point(rnd, curve):
    """a random point of a curve with a = -1: y^2 = (1 + x^2) / (1 - d x^2), p = 1 mod 4 or 3 mod 4 alike by trying"""
    p = curve.p
    assert curve.a == p - 1
    while True:
        x = rnd.randrange(p)
        den = (1 - curve.d * x * x) % p
        if den == 0:
            continue
        y2 = (1 + x * x) * pow(den, -1, p) % p
        if pow(y2, (p - 1) // 2, p) != 1:
            continue
        y = sqrt_mod(y2, p)
        return Point(x, y, curve)


def sqrt_mod(v, p):
    """Tonelli-Shanks"""
    q, s = p - 1, 0
    while q % 2 == 0:
        q, s = q // 2, s + 1
    z = 2
    while pow(z, (p - 1) // 2, p) != p - 1:
        z += 1
    m, c, t, r = s, pow(z, q, p), pow(v, q, p), pow(v, (q + 1) // 2, p)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2, i = t2 * t2 % p, i + 1
        b = pow(c, 1 << (m - i - 1), p)
        m, c, t, r = i, b * b % p, t * b * b % p, r * b % p
    assert r * r % p == v
    return r


# ---- the cleartext bodies ----------------------------------------------------------------------------------------------
def test_scalar_mul_body_equals_the_golden_file():
    g = golden()
    a, d = int(g["a"]), int(g["d"])
    ns, xs, ys, want = [], [], [], []
    for c in g["muls"]:
        n, (x, y) = int(c["n"]), _xy(c["P"])
        if n < 0:                                            # the body takes canonical scalars: n P = (-n) (-P)
            n, x = -n, -x % BLS
        ns.append(n), xs.append(x), ys.append(y), want.append(_xy(c["out"]))
    count = len(ns)
    rc, (ox, oy) = run(BLS, 4, SCALAR_MUL, [ns, xs, ys], count, 2, a=a, d=d)
    assert rc == 0 and list(zip(ox, oy)) == want
    # one scalar for all, one point for all, both; n = 0 leaves the neutral element
    gp = _xy(g["GP"])
    fixed = [(int(c["n"]), _xy(c["out"])) for c in g["muls"] if _xy(c["P"]) == gp and int(c["n"]) > 0]
    rc, (ox, oy) = run(BLS, 4, SCALAR_MUL, [[n for n, _ in fixed], [gp[0]], [gp[1]]], len(fixed), 2, a=a, d=d, flags=P_BCAST)
    assert rc == 0 and list(zip(ox, oy)) == [o for _, o in fixed]
    n = ns[-1]
    rc, (ox, oy) = run(BLS, 4, SCALAR_MUL, [[n], xs, ys], count, 2, a=a, d=d, flags=N_BCAST)
    assert rc == 0 and [Point(x, y) for x, y in zip(ox, oy)] == [Point(x, y) * n for x, y in zip(xs, ys)]
    rc, (ox, oy) = run(BLS, 4, SCALAR_MUL, [[0], [gp[0]], [gp[1]]], 3, 2, a=a, d=d, flags=N_BCAST | P_BCAST)
    assert rc == 0 and list(zip(ox, oy)) == [(0, 1)] * 3


def test_scalar_mul_and_double_table_bodies_on_the_narrow_curve():
    curve = Jubjub(-1, 2, P64)
    rnd = random.Random(64)
    pts = [narrow_point(rnd, curve) for _ in range(6)] + [Point(0, 1, curve), Point(0, P64 - 1, curve)]
    ns = [0, 1, 2, P64 - 1, P64 - 2, (1 << 63), rnd.randrange(P64), rnd.randrange(P64)]
    xs, ys = [q.x for q in pts], [q.y for q in pts]
    rc, (ox, oy) = run(P64, 1, SCALAR_MUL, [ns, xs, ys], len(ns), 2, a=curve.a, d=curve.d)
    want = [q * n if n else Point(0, 1, curve) for q, n in zip(pts, ns)]
    assert rc == 0 and list(zip(ox, oy)) == [(w.x, w.y) for w in want]
    K = 9
    rc, rows = run(P64, 1, DOUBLE_TABLE, [xs, ys], len(pts), 3 * K, a=curve.a, arg=K)
    assert rc == 0
    for j in range(K):
        for i, q in enumerate(pts):
            zi = pow(rows[2 * K + j][i], -1, P64)
            w = q * (1 << j)
            assert (rows[j][i] * zi % P64, rows[K + j][i] * zi % P64) == (w.x, w.y), (j, i)


def test_double_table_body_equals_the_host_model():
    g = golden()
    a = int(g["a"])
    pts = [Point(*_xy(c["P"])) for c in g["muls"][-8:]] + [Point(0, 1), Point(0, -1)]
    xs, ys = [q.x for q in pts], [q.y for q in pts]
    K, n = 33, len(pts)
    rc, rows = run(BLS, 4, DOUBLE_TABLE, [xs, ys], n, 3 * K, a=a, arg=K)
    assert rc == 0
    cur = list(pts)
    for j in range(K):
        for i in range(n):
            zi = pow(rows[2 * K + j][i], -1, BLS)
            assert (rows[j][i] * zi % BLS, rows[K + j][i] * zi % BLS) == (cur[i].x, cur[i].y), (j, i)
        cur = [q.double() for q in cur]


# ---- the addition of shared points, in the clear -----------------------------------------------------------------------------
def chain(p, nl, d, x1, y1, x2, y2, rnd, stride_extra=0):
    """the four stages chained with shares dealt at n = 1 (the share IS the value, so what a stage writes is what the next one reads
    as opened), random triples and random non-zero rs -> (x3, y3) lists"""
    m = len(x1)
    stride = m + stride_extra
    tp = [[rnd.randrange(p) for _ in range(stride)] for _ in range(9)]
    tq = [[rnd.randrange(p) for _ in range(stride)] for _ in range(9)]
    tpq = [[a * b % p for a, b in zip(ra, rb)] for ra, rb in zip(tp, tq)]
    rx, ry = ([rnd.randrange(1, p) for _ in range(m)] for _ in range(2))
    P, Q, PQ = flat(tp), flat(tq), flat(tpq)
    rc, A = run(p, nl, MASK, [x1, y1, x2, y2, P, Q], m, 8, arg=stride)
    assert rc == 0
    rc, B = run(p, nl, STAGE1, [flat(A), P, Q, PQ, rx, ry], m, 6, arg=stride)
    assert rc == 0
    rc, uvC = run(p, nl, STAGE2, [flat(B), P, Q, PQ, rx, ry], m, 6, d=d, arg=stride)
    assert rc == 0
    uv, C = uvC[:2], uvC[2:]
    rc, D = run(p, nl, STAGE3, [flat(C), P, Q, PQ], m, 2, arg=stride)
    assert rc == 0
    # each sig is its denominator times r
    for i in range(m):
        w = d * x1[i] * x2[i] * y1[i] * y2[i]
        assert D[0][i] == (1 + w) * rx[i] % p and D[1][i] == (1 - w) * ry[i] % p
    inv = [[pow(v, -1, p) for v in row] for row in D]
    rc, out = run(p, nl, SCALE, [flat(inv), flat(uv)], m, 2)
    assert rc == 0
    return out


@pytest.mark.parametrize("stride_extra", [0, 5], ids=["dense", "strided"])
def test_stage_bodies_reproduce_every_golden_add(stride_extra):
    g = golden()
    d = int(g["d"])
    x1, y1, x2, y2, want = [], [], [], [], []
    for c in g["adds"]:
        (a, b), (e, f) = _xy(c["P"]), _xy(c["Q"])
        x1.append(a), y1.append(b), x2.append(e), y2.append(f), want.append(_xy(c["sum"]))
    x3, y3 = chain(BLS, 4, d, x1, y1, x2, y2, random.Random(7 + stride_extra), stride_extra)
    assert list(zip(x3, y3)) == want


def test_stage_bodies_on_the_narrow_curve():
    curve = Jubjub(-1, 2, P64)
    rnd = random.Random(65)
    pts = [narrow_point(rnd, curve) for _ in range(12)] + [Point(0, 1, curve), Point(0, P64 - 1, curve)]
    pairs = [(a, b) for a in pts for b in pts][:120] + [(q, -q) for q in pts]
    x3, y3 = chain(P64, 1, curve.d, [a.x for a, _ in pairs], [a.y for a, _ in pairs], [b.x for _, b in pairs], [b.y for _, b in pairs], rnd, 3)
    assert list(zip(x3, y3)) == [((a + b).x, (a + b).y) for a, b in pairs]


@pytest.mark.parametrize("p, nl", PRIMES, ids=IDS)
def test_stage_bodies_every_corner(p, nl):
    """Field arithmetic only: no curve is needed.  A stage has up to 28 operands, so not all 3^28 corner tuples of {0, 1, p - 1} can be
    run; what can go wrong sits in a Beaver step (the one lazy sum) and in the additions around it.  So: 243 elements in which the
    five operands (opened d, opened e, p, q, pq) of EVERY Beaver step of a stage run through all 3^5 corner tuples -- step k in an
    order of its own, so the steps' results meet in varying combinations -- while every other operand cycles through the corners;
    then every operand 0, every operand 1, every operand p - 1 (over 2^256 - 189 the largest case); then random elements.  d takes the
    corners and a random value."""
    rnd = random.Random(p % 1000 + 19 * nl)
    corners = [0, 1, p - 1]
    tuples = list(itertools.product(corners, repeat=5))
    n_rand = 64
    m = len(tuples) + 3 + n_rand
    stride = m + 2

    def column(kind, step=0, slot=0):
        """operand values for the m elements; kind "step": slot `slot` of the corner tuple for Beaver step `step`, else cycling corners"""
        if kind == "step":
            order = tuples[step * 37 % 243:] + tuples[:step * 37 % 243]
            head = [tp[slot] for tp in order]
        else:
            head = [corners[(i + step) % 3] for i in range(243)]
        return head + [0, 1, p - 1] + [rnd.randrange(p) for _ in range(n_rand)]

    def triples(steps):
        """-> (tp, tq, tpq) [9][stride]: rows of the Beaver steps in `steps` carry corner tuples (slots 2, 3, 4), the others cycle"""
        out = []
        for slot in (2, 3, 4):
            out.append([column("step", k, slot) if k in steps else column("cycle", k + slot) for k in range(9)])
        return [[row + [rnd.randrange(p), 7 % p] for row in comp] for comp in out]

    # mask
    x1, y1, x2, y2 = (column("cycle", s) for s in range(4))
    tp, tq, tpq = triples(())
    rc, A = run(p, nl, MASK, [x1, y1, x2, y2, flat(tp), flat(tq)], m, 8, arg=stride)
    assert rc == 0
    for i in range(m):
        assert [row[i] for row in A] == mask_ref(p, x1[i], y1[i], x2[i], y2[i], [r[i] for r in tp], [r[i] for r in tq]), i
    # stage 1: Beaver steps 0..3 read rows (2k, 2k + 1) of A
    tp, tq, tpq = triples((0, 1, 2, 3))
    A = [column("step", k, s) for k in range(4) for s in (0, 1)]
    rx, ry = column("cycle", 1), column("cycle", 2)
    rc, B = run(p, nl, STAGE1, [flat(A), flat(tp), flat(tq), flat(tpq), rx, ry], m, 6, arg=stride)
    assert rc == 0
    for i in range(m):
        assert [row[i] for row in B] == stage1_ref(p, [r[i] for r in A], [r[i] for r in tp], [r[i] for r in tq], [r[i] for r in tpq], rx[i], ry[i]), i
    # stage 2: Beaver steps 4..6 read rows (0, 1), (2, 3), (4, 5) of B
    tp, tq, tpq = triples((4, 5, 6))
    B = [column("step", k, s) for k in (4, 5, 6) for s in (0, 1)]
    for d in (0, 1, p - 1, rnd.randrange(p)):
        rc, uvC = run(p, nl, STAGE2, [flat(B), flat(tp), flat(tq), flat(tpq), rx, ry], m, 6, d=d, arg=stride)
        assert rc == 0
        for i in range(m):
            assert [row[i] for row in uvC] == stage2_ref(p, [r[i] for r in B], [r[i] for r in tp], [r[i] for r in tq], [r[i] for r in tpq], rx[i], ry[i], d), (d, i)
    # stage 3: Beaver steps 7, 8 read rows (0, 1), (2, 3) of C
    tp, tq, tpq = triples((7, 8))
    C = [column("step", k, s) for k in (7, 8) for s in (0, 1)]
    rc, D = run(p, nl, STAGE3, [flat(C), flat(tp), flat(tq), flat(tpq)], m, 2, arg=stride)
    assert rc == 0
    for i in range(m):
        assert [row[i] for row in D] == stage3_ref(p, [r[i] for r in C], [r[i] for r in tp], [r[i] for r in tq], [r[i] for r in tpq]), i
    # the scaling: all nine corner pairs and random ones, in both rows
    pairs = list(itertools.product(corners, repeat=2)) + [(rnd.randrange(p), rnd.randrange(p)) for _ in range(23)]
    inv = [[a for a, _ in pairs], [b for _, b in pairs]]
    uv = [[b for _, b in pairs], [a for a, _ in reversed(pairs)]]
    rc, out = run(p, nl, SCALE, [flat(inv), flat(uv)], len(pairs), 2)
    assert rc == 0 and out == [[a * b % p for a, b in zip(ri, ru)] for ri, ru in zip(inv, uv)]


@pytest.mark.parametrize("p, nl", PRIMES, ids=IDS)
def test_stage_bodies_at_edge_values(p, nl):
    """every operand of every stage a value on the edges of the words, the digits and the int8 split, or the Montgomery pre-image of one
    (tests/edge_values.py): each operand row walks the list at a stride of its own, so the Beaver steps meet them in varying pairs"""
    import edge_values

    vs = edge_values.operands(p, nl)
    m = len(vs)
    strides = iter(range(1, 200, 2))
    walk = lambda: (lambda s: [vs[(i * s + s) % m] for i in range(m)])(next(strides))    # noqa: E731
    x1, y1, x2, y2, rx, ry = (walk() for _ in range(6))
    tp, tq, tpq = ([walk() for _ in range(9)] for _ in range(3))
    at = lambda rows, i: [r[i] for r in rows]    # noqa: E731
    rc, A = run(p, nl, MASK, [x1, y1, x2, y2, flat(tp), flat(tq)], m, 8, arg=m)
    assert rc == 0 and cols(A) == [mask_ref(p, x1[i], y1[i], x2[i], y2[i], at(tp, i), at(tq, i)) for i in range(m)]
    A = [walk() for _ in range(8)]
    rc, B = run(p, nl, STAGE1, [flat(A), flat(tp), flat(tq), flat(tpq), rx, ry], m, 6, arg=m)
    assert rc == 0 and cols(B) == [stage1_ref(p, at(A, i), at(tp, i), at(tq, i), at(tpq, i), rx[i], ry[i]) for i in range(m)]
    B = [walk() for _ in range(6)]
    for d in (p - 1, vs[m // 2]):
        rc, uvC = run(p, nl, STAGE2, [flat(B), flat(tp), flat(tq), flat(tpq), rx, ry], m, 6, d=d, arg=m)
        assert rc == 0 and cols(uvC) == [stage2_ref(p, at(B, i), at(tp, i), at(tq, i), at(tpq, i), rx[i], ry[i], d) for i in range(m)], d
    C = [walk() for _ in range(4)]
    rc, D = run(p, nl, STAGE3, [flat(C), flat(tp), flat(tq), flat(tpq)], m, 2, arg=m)
    assert rc == 0 and cols(D) == [stage3_ref(p, at(C, i), at(tp, i), at(tq, i), at(tpq, i)) for i in range(m)]
    inv, uv = [walk(), walk()], [walk(), walk()]
    rc, out = run(p, nl, SCALE, [flat(inv), flat(uv)], m, 2)
    assert rc == 0 and out == [[a * b % p for a, b in zip(ri, ru)] for ri, ru in zip(inv, uv)]


def test_stage_bodies_largest_case():
    p = (1 << 256) - 189
    m = 4
    top = [p - 1] * m
    t9 = [p - 1] * (9 * m)
    rc, A = run(p, 4, MASK, [top, top, top, top, t9, t9], m, 8, arg=m)
    assert rc == 0 and A == [[0] * m] * 8
    rc, B = run(p, 4, STAGE1, [[p - 1] * (8 * m), t9, t9, t9, top, top], m, 6, arg=m)
    assert rc == 0 and cols(B) == [stage1_ref(p, [p - 1] * 8, [p - 1] * 9, [p - 1] * 9, [p - 1] * 9, p - 1, p - 1)] * m
    rc, uvC = run(p, 4, STAGE2, [[p - 1] * (6 * m), t9, t9, t9, top, top], m, 6, d=p - 1, arg=m)
    assert rc == 0 and cols(uvC) == [stage2_ref(p, [p - 1] * 6, [p - 1] * 9, [p - 1] * 9, [p - 1] * 9, p - 1, p - 1, p - 1)] * m
    rc, D = run(p, 4, STAGE3, [[p - 1] * (4 * m), t9, t9, t9], m, 2, arg=m)
    assert rc == 0 and cols(D) == [stage3_ref(p, [p - 1] * 4, [p - 1] * 9, [p - 1] * 9, [p - 1] * 9)] * m


# ---- the ABI and the argument checks that need no device -------------------------------------------------------------------
def test_abi_names_in_header_and_ctypes_table():
    from honeybadgermpc_amd import _capi

    text = open(os.path.join(REPO, "include", "hbmpc_hip.h")).read()
    for name in ("hb_jj_scalar_mul", "hb_jj_double_table", "hb_jj_add_mask", "hb_jj_add_stage1", "hb_jj_add_stage2", "hb_jj_add_stage3", "hb_jj_add_finish",
                 "hb_selftest_jj"):
        assert re.search(r"\bint " + name + r"\s*\(", text) and name in _capi.SYMBOLS
    for name, value in (("HB_JJ_SCALAR_BROADCAST", 1), ("HB_JJ_POINT_BROADCAST", 2), ("HB_JJ_SELFTEST_SCALAR_MUL", 0), ("HB_JJ_SELFTEST_DOUBLE_TABLE", 1),
                        ("HB_JJ_SELFTEST_MASK", 2), ("HB_JJ_SELFTEST_STAGE1", 3), ("HB_JJ_SELFTEST_STAGE2", 4), ("HB_JJ_SELFTEST_STAGE3", 5),
                        ("HB_JJ_SELFTEST_SCALE", 6)):
        assert re.search(r"#define " + name + r" " + str(value) + r"\b", text) and getattr(_capi, name) == value
    assert "progs/jubjub.py:87-113" in text and "elliptic_curve.py" in text
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert "hb_jj_scalar_mul" in doc and "hb_jj_add_finish" in doc


def test_selftest_rejects_bad_arguments():
    v = [1, 2, 3]
    nine = v * 9
    for nl in (4, 1):
        assert run(13, nl, SCALAR_MUL, [v, v, v], 3, 2, a=12, d=2)[0] == 0
        assert run(13, nl, SCALAR_MUL, [v, v, v], 3, 2, a=12)[0] == 2                      # no d
        assert run(13, nl, SCALAR_MUL, [v, v, v], 3, 2, d=2)[0] == 2                       # no a
        assert run(13, nl, SCALAR_MUL, [v, v, v], 3, 2, a=13, d=2)[0] == 2                 # a not below the modulus
        assert run(13, nl, SCALAR_MUL, [v, v, v], 3, 2, a=12, d=2, flags=4)[0] == 2        # an unknown flag
        assert run(13, nl, SCALAR_MUL, [v, None, v], 3, 2, a=12, d=2)[0] == 2              # a missing operand
        assert run(13, nl, SCALAR_MUL, [v, v, v], -1, 2, a=12, d=2)[0] == 2
        assert run(13, nl, DOUBLE_TABLE, [v, v], 3, 6, a=12, arg=2)[0] == 0
        assert run(13, nl, DOUBLE_TABLE, [v, v], 3, 6, a=12, arg=0)[0] == 2                # no rows
        assert run(13, nl, DOUBLE_TABLE, [v, v], 3, 6, arg=2)[0] == 2
        assert run(13, nl, MASK, [v, v, v, v, nine, nine], 3, 8, arg=3)[0] == 0
        assert run(13, nl, MASK, [v, v, v, v, nine, nine], 3, 8, arg=2)[0] == 2            # a row stride below the count
        assert run(13, nl, MASK, [v, v, v, None, nine, nine], 3, 8, arg=3)[0] == 2
        assert run(13, nl, STAGE2, [v * 6, nine, nine, nine, v, v], 3, 6, d=2, arg=3)[0] == 0
        assert run(13, nl, STAGE2, [v * 6, nine, nine, nine, v, v], 3, 6, arg=3)[0] == 2   # no d
        assert run(13, nl, STAGE2, [v * 6, nine, nine, nine, v, v], 3, 6, d=14, arg=3)[0] == 2
        assert run(13, nl, STAGE3, [v * 4, nine, nine, nine], 3, 2, arg=3, flags=1)[0] == 2
        assert run(13, nl, STAGE3, [v * 4, nine, nine, None], 3, 2, arg=3)[0] == 2
        assert run(13, nl, 7, [v, v, v], 3, 2, a=12, d=2)[0] == 2                          # unknown `what`
        assert run(13, nl, SCALE, [[], []], 0, 2)[0] == 0
    assert run(13, 2, SCALE, [v * 2, v * 2], 3, 2)[0] == 2                                 # neither 1 nor 4 limbs


def test_argument_checks_of_the_python_layer_that_need_no_device():
    from honeybadgermpc_amd.progs import jubjub, mimc_jubjub_pkc

    assert [jubjub.shared_mul_pairs(n) for n in (1, 2, 3, 4, 5, 7, 8, -6, 255)] == [0, 1, 2, 2, 3, 4, 3, 3, 14]
    with pytest.raises(ValueError):
        jubjub.shared_mul_pairs(0)
    for bad in (1.0, True, "3"):
        with pytest.raises(TypeError):
            jubjub.shared_mul_pairs(bad)
    assert mimc_jubjub_pkc.GP == Point(*_xy(golden()["GP"])) and mimc_jubjub_pkc.GP.curve == Jubjub()

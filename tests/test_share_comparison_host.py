"""CPU-only: honeybadgermpc_amd.share_comparison -- the host functions and host models against tests/golden/share_comparison.json
(written by scratch/gen_share_comparison_golden.py from the reference's own Equality mixin: legendre_mod_p, and _gen_test_bit /
gen_test_bit / _prog driven over cleartext shares with recorded draws), the two finishing maps, and the steps of csrc/hb_eq.hip
run on the host through hb_selftest_eq -- the same rows, arithmetic and addressing, that the kernel runs -- against Python ints.
Exact equality."""
import itertools
import json
import os
import random
import re

import pytest

from conftest import BLS, REPO
from selftest_cases import run_eq as run

from honeybadgermpc_amd import share_comparison as sc

GOLDILOCKS = 0xFFFFFFFF00000001
P64 = (1 << 64) - 59
P256 = (1 << 256) - 189
FIELDS = [(BLS, 4), (P256, 4), (P64, 1), (GOLDILOCKS, 1)]
FIELD_IDS = ["bls", "2^256-189", "2^64-59", "goldilocks"]
LEGENDRE, MASK1, MID, CSHARE, FINISH = range(5)
COUNTS = (0, 1, 257)


def golden():
    with open(os.path.join(REPO, "tests", "golden", "share_comparison.json")) as f:
        return json.load(f)


def beaver(d, e, a, b, ab, p):
    return (d * e + d * b + e * a + ab) % p


# ---- the host functions against the reference ------------------------------------------------------------------------------
def test_legendre_equals_the_reference():
    g = golden()
    assert int(g["modulus"]) == BLS and g["nr"] == 5 == sc.smallest_nonresidue(BLS)
    assert len(g["legendre"]) >= 40 and {c["out"] for c in g["legendre"]} == {-1, 0, 1}
    for c in g["legendre"]:
        assert sc.legendre_mod_p(int(c["a"]), BLS) == c["out"], c
    by_value = {int(c["a"]): c["out"] for c in g["legendre"]}
    assert (by_value[0], by_value[1], by_value[BLS - 1], by_value[5], by_value[25]) == (0, 1, 1, -1, 1)


def test_reference_mode_equals_the_reference_coroutines():
    g = golden()
    assert len(g["test_bit"]) >= 16
    seen = set()
    for c in g["test_bit"]:
        diff, b = int(c["diff"]), c["b"]
        got_c, factor = sc.test_bit_model(diff, b, int(c["r"]), int(c["rp"]), BLS, 5, sc.REFERENCE)
        assert (got_c, factor) == (int(c["c"]), int(c["out"])), c
        seen.add((diff == 0, b))
        if diff == 0:                                                    # the quirk: b = 0 gives -2 where the protocol wants 1
            assert factor == (1 if b else BLS - 2)
        else:
            assert factor in (0, 1, 3, BLS - 2)
    assert seen == set(itertools.product((True, False), (0, 1)))
    assert sorted({c["kappa"] for c in g["equal"]}) == [1, 2, 3, 5, 32]
    for c in g["equal"]:
        kappa, x, y = c["kappa"], int(c["x"]), int(c["y"])
        bits, rs, rps = [int(b) for b in c["bits"]], [int(v) for v in c["rs"]], [int(v) for v in c["rps"]]
        assert len(bits) == len(rs) == len(rps) == kappa
        assert [sc.test_bit_model((x - y) % BLS, b, r, rp, BLS, 5, sc.REFERENCE)[0] for b, r, rp in zip(bits, rs, rps)] == [int(v) for v in c["cs"]]
        assert sc.equal_model((x - y) % BLS, bits, rs, rps, BLS, 5, sc.REFERENCE) == int(c["out"]), c
        if x == y:
            assert int(c["out"]) == pow(-2, bits.count(0), BLS)            # nonzero, not 1: the reference's own test asserts truthiness only
            assert sc.equal_model(0, bits, rs, rps, BLS, 5, sc.BIT) == 1


@pytest.mark.parametrize("p, nl", FIELDS, ids=FIELD_IDS)
def test_bit_mode_gives_exactly_one_or_zero(p, nl):
    rnd = random.Random(p % 1013)
    nr = sc.smallest_nonresidue(p)
    assert nr == {BLS: 5, P64: 2}.get(p, nr)
    seen = set()
    while len(seen) < 6:                                                 # diff = 0 fixes L by b: two combinations there, four with diff != 0
        zero, b = rnd.getrandbits(1), rnd.getrandbits(1)
        diff, r, rp = (0 if zero else rnd.randrange(1, p)), rnd.randrange(1, p), rnd.randrange(1, p)
        c, factor = sc.test_bit_model(diff, b, r, rp, p, nr, sc.BIT)
        leg = sc.legendre_mod_p(c, p)
        if leg == 0:
            continue
        seen.add((bool(zero), b, leg))
        # s = 2 b - 1 agrees with L when diff = 0: _b rp^2 is a square exactly when b = 1
        assert factor == (1 if leg == 2 * b - 1 else 0), (diff, b, leg)
        if zero:
            assert leg == 2 * b - 1 and factor == 1
        ref = sc.test_bit_model(diff, b, r, rp, p, nr, sc.REFERENCE)[1]
        assert ref == leg * (nr - (nr - 1) * b + leg) * pow(2, -1, p) % p
    assert len({(z, b) for z, b, _ in seen if z}) == 2 and len({k for k in seen if not k[0]}) == 4
    # the map itself at all eight (diff == 0, b, L): it does not look at diff, and (b, L) -> 1 exactly when L = 2 b - 1
    for zero, b, leg in itertools.product((True, False), (0, 1), (1, -1)):
        assert ((1 - leg) * pow(2, -1, p) + leg * b) % p == (1 if leg == 2 * b - 1 else 0)
    assert sc.test_bit_model(0, 1, 5, 0, p, nr, sc.BIT) == (0, None) and sc.equal_model(0, [1, 1], [3, 5], [7, 0], p, nr) is None


def test_parameter_checks_and_counts():
    for p in (BLS, P256, P64, GOLDILOCKS):
        nr = sc.smallest_nonresidue(p)
        sc.check_nonresidue(p, nr)
        for bad in (1, 4, nr * nr, 0, p, 2.0, True):
            with pytest.raises(ValueError):
                sc.check_nonresidue(p, bad)
    with pytest.raises(ValueError):
        sc.check_nonresidue(BLS, 2)                                          # 2 is a square modulo the BLS12-381 scalar field's prime
    assert [sc.equality_triples(k) for k in (1, 2, 3, 5, 32)] == [3, 7, 11, 19, 127]
    assert [sc.equality_opens(k) for k in (1, 2, 3, 4, 5, 8, 9, 32, 33)] == [3, 4, 5, 5, 6, 6, 7, 8, 9]
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            sc.equality_triples(bad)
        with pytest.raises(ValueError):
            sc.equality_opens(bad)
    for bad in (2, -1, None, True):
        with pytest.raises(ValueError):
            sc.test_bit_model(1, 1, 1, 1, BLS, 5, bad)
    with pytest.raises(ValueError):
        sc.test_bit_model(1, 2, 1, 1, BLS, 5)


# ---- the kernels' bodies on the host -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("p, nl", FIELDS, ids=FIELD_IDS)
def test_selftest_legendre(p, nl):
    rnd = random.Random(p % 1019)
    nr = sc.smallest_nonresidue(p)
    for count in COUNTS:
        a = ([0, 1, p - 1, nr, nr * nr % p, 2, 3, p - 2] + [rnd.randrange(p) for _ in range(count)])[:count] if count > 1 else [rnd.randrange(1, p)] * count
        rc, (got,) = run(p, nl, LEGENDRE, [a], 0, 0, ["i8"], count)
        assert rc == 0 and got == [sc.legendre_mod_p(v, p) for v in a], count
    rc, (got,) = run(p, nl, LEGENDRE, [[0, 1, p - 1]], 0, 0, ["i8"], 3)
    assert got == [0, 1, sc.legendre_mod_p(p - 1, p)]


@pytest.mark.parametrize("p, nl", FIELDS, ids=FIELD_IDS)
def test_selftest_mask1_mid_cshare(p, nl):
    rnd = random.Random(p % 1021)
    nr = sc.smallest_nonresidue(p)
    for count, rows in itertools.product(COUNTS, (1, 3)):
        n = rows * count
        draw = lambda k: [rnd.choice((0, 1, p - 1, rnd.randrange(p))) for _ in range(k)]    # noqa: E731
        x, y = draw(count), draw(count)
        r, rp, pa, qa, pb, qb = (draw(n) for _ in range(6))
        for yy in (y, None):
            diff = [(a - (b if yy else 0)) % p for a, b in zip(x, y)]
            rc, (got,) = run(p, nl, MASK1, [x, yy, r, rp, pa, qa, pb, qb], rows, 0, [4 * rows], count)
            want = [(diff[i % count] - pa[i]) % p for i in range(n)] + [(r[i] - qa[i]) % p for i in range(n)] + [(rp[i] - pb[i]) % p for i in range(n)] + \
                   [(rp[i] - qb[i]) % p for i in range(n)]
            assert rc == 0 and got == want, (count, rows, yy is None)
        opened, pqa, pqb, bits, pc, qc, pqc = draw(4 * n), draw(n), draw(n), [rnd.getrandbits(1) for _ in range(n)], draw(n), draw(n), draw(n)
        if n:
            bits[0] = rnd.randrange(p)                                      # a share of a bit is any residue
        rc, (m2, dr) = run(p, nl, MID, [opened, pa, qa, pqa, pb, qb, pqb, bits, pc, qc, [nr]], rows, 0, [2 * rows, rows], count)
        o = [opened[k * n:(k + 1) * n] for k in range(4)]
        want_dr = [beaver(o[0][i], o[1][i], pa[i], qa[i], pqa[i], p) for i in range(n)]
        rp2 = [beaver(o[2][i], o[3][i], pb[i], qb[i], pqb[i], p) for i in range(n)]
        assert rc == 0 and dr == want_dr and m2 == [(nr - (nr - 1) * bits[i] - pc[i]) % p for i in range(n)] + [(rp2[i] - qc[i]) % p for i in range(n)], (count, rows)
        opened2 = draw(2 * n)
        rc, (c,) = run(p, nl, CSHARE, [opened2, want_dr, pc, qc, pqc], rows, 0, [rows], count)
        assert rc == 0 and c == [(want_dr[i] + beaver(opened2[i], opened2[n + i], pc[i], qc[i], pqc[i], p)) % p for i in range(n)], (count, rows)
    # the largest operands everywhere
    big = [p - 1]
    rc, (m2, dr) = run(p, nl, MID, [big * 4] + [big] * 9 + [[nr]], 1, 0, [2, 1], 1)
    assert rc == 0 and dr == [beaver(*big * 5, p)] and m2 == [(nr - (nr - 1) * (p - 1) - (p - 1)) % p, (beaver(*big * 5, p) + 1) % p]
    for bad in ([0], [1]):
        assert run(p, nl, MID, [big * 4] + [big] * 9 + [bad], 1, 0, [2, 1], 1)[0] == 2
    assert run(p, nl, MASK1, [big] * 8, 0, 0, [4], 1)[0] == 2 and run(p, nl, 9, [big], 1, 0, [1], 1)[0] == 2


@pytest.mark.parametrize("p, nl", FIELDS, ids=FIELD_IDS)
def test_selftest_bodies_at_edge_values(p, nl):
    """the Legendre symbol of, and the masking / Beaver bodies over, values on the edges of the words, the digits and the int8 split and
    their Montgomery pre-images (tests/edge_values.py): each list walks the pool at its own stride"""
    import edge_values

    vs = edge_values.operands(p, nl)
    n = len(vs)
    nr = sc.smallest_nonresidue(p)
    rc, (got,) = run(p, nl, LEGENDRE, [vs], 0, 0, ["i8"], n)
    assert rc == 0 and got == [sc.legendre_mod_p(v, p) for v in vs]
    walk = lambda s, k=n: [vs[(i * s + s) % n] for i in range(k)]    # noqa: E731
    x, y, r, rp, pa, qa, pb, qb = (walk(s) for s in (1, 3, 5, 7, 11, 13, 17, 19))
    rc, (got,) = run(p, nl, MASK1, [x, y, r, rp, pa, qa, pb, qb], 1, 0, [4], n)
    assert rc == 0 and got == [(a - b - c) % p for a, b, c in zip(x, y, pa)] + [(a - b) % p for a, b in zip(r, qa)] + \
        [(a - b) % p for a, b in zip(rp, pb)] + [(a - b) % p for a, b in zip(rp, qb)]
    opened, pqa, pqb, bits, pc, qc, pqc = walk(23, 4 * n), walk(29), walk(31), walk(37), walk(41), walk(43), walk(47)
    rc, (m2, dr) = run(p, nl, MID, [opened, pa, qa, pqa, pb, qb, pqb, bits, pc, qc, [nr]], 1, 0, [2, 1], n)
    o = [opened[k * n:(k + 1) * n] for k in range(4)]
    want_dr = [beaver(o[0][i], o[1][i], pa[i], qa[i], pqa[i], p) for i in range(n)]
    rp2 = [beaver(o[2][i], o[3][i], pb[i], qb[i], pqb[i], p) for i in range(n)]
    assert rc == 0 and dr == want_dr and m2 == [(nr - (nr - 1) * bits[i] - pc[i]) % p for i in range(n)] + [(rp2[i] - qc[i]) % p for i in range(n)]
    opened2 = walk(53, 2 * n)
    rc, (c,) = run(p, nl, CSHARE, [opened2, want_dr, pc, qc, pqc], 1, 0, [1], n)
    assert rc == 0 and c == [(want_dr[i] + beaver(opened2[i], opened2[n + i], pc[i], qc[i], pqc[i], p)) % p for i in range(n)]


@pytest.mark.parametrize("p, nl", FIELDS, ids=FIELD_IDS)
def test_selftest_finish_both_modes(p, nl):
    rnd = random.Random(p % 1031)
    nr = sc.smallest_nonresidue(p)
    inv2 = pow(2, -1, p)
    for count, rows, mode in itertools.product(COUNTS, (1, 3), (sc.BIT, sc.REFERENCE)):
        n = rows * count
        c = [rnd.randrange(1, p) for _ in range(n)]
        bits = [rnd.choice((0, 1, rnd.randrange(p))) for _ in range(n)]
        want_zero = [0] * rows
        if count > 1:
            c[:3] = [0, 1, p - 1]                                           # the corners, in row 0
            want_zero[0] = 1
            if rows > 1:
                c[2 * count + 5] = 0
                want_zero[2] = 1
        rc, (got, zero_rows) = run(p, nl, FINISH, [c, bits, [nr]], rows, mode, [rows, "zr"], count)
        want = []
        for v, b in zip(c, bits):
            leg = sc.legendre_mod_p(v, p)
            if leg == 0:
                want.append(0)
            elif mode == sc.BIT:
                want.append(((1 - leg) * inv2 + leg * b) % p)
            else:
                want.append((leg * (nr + leg) * inv2 - leg * (nr - 1) * inv2 * b) % p)
        assert rc == 0 and got == want and zero_rows == want_zero, (count, rows, mode)
    # exact bits in, the models out
    for b, zero in itertools.product((0, 1), (True, False)):
        diff, r, rp = (0 if zero else rnd.randrange(1, p)), rnd.randrange(1, p), rnd.randrange(1, p)
        for mode in (sc.BIT, sc.REFERENCE):
            c, factor = sc.test_bit_model(diff, b, r, rp, p, nr, mode)
            rc, (got, zr) = run(p, nl, FINISH, [[c], [b], [nr]], 1, mode, [1, "zr"], 1)
            assert rc == 0 and got == [factor] and zr == [0]
    rc, (got, zr) = run(p, nl, FINISH, [[1], [1], None], 1, sc.BIT, [1, "zr"], 1)      # BIT does not read nr
    assert rc == 0 and got == [1]
    assert run(p, nl, FINISH, [[1], [1], None], 1, sc.REFERENCE, [1, "zr"], 1)[0] == 2 and run(p, nl, FINISH, [[1], [1], [nr]], 1, 2, [1, "zr"], 1)[0] == 2


def test_entry_points_are_declared_and_bound():
    from honeybadgermpc_amd import _capi
    from honeybadgermpc_amd.exceptions import HoneyBadgerMPCError, PreprocessingExhausted

    text = open(os.path.join(REPO, "include", "hbmpc_hip.h")).read()
    for name in ("hb_legendre", "hb_eq_mask1", "hb_eq_mid", "hb_eq_cshare", "hb_eq_finish", "hb_selftest_eq"):
        assert re.search(r"\bint " + name + r"\s*\(", text) and name in _capi.SYMBOLS
    assert (_capi.HB_EQ_BIT, _capi.HB_EQ_REFERENCE) == (0, 1) == (sc.BIT, sc.REFERENCE)
    for name, value in (("HB_EQ_BIT", 0), ("HB_EQ_REFERENCE", 1), ("HB_EQ_SELFTEST_FINISH", 4)):
        assert re.search(rf"#define {name} {value}\b", text)
    assert issubclass(PreprocessingExhausted, HoneyBadgerMPCError) and sc.KAPPA == 32

"""CPU-only: the host model of honeybadgermpc_amd.progs.mimc against tests/golden/mimc.json (written by scratch/gen_mimc_golden.py
from the reference's own mimc_plain and ROUND), and the per-element bodies of the MiMC kernels (csrc/hb_mimc.hip) run on the host
through hb_selftest_mimc -- the body k_mimc_plain calls and the rows MimcRoundRow and MimcFirstRow that the device runs -- against Python ints.
Exact equality."""
import itertools
import json
import os
import random
import re

import pytest

from conftest import BLS, REPO
from selftest_cases import run_mimc as run

from honeybadgermpc_amd.progs import mimc

PRIMES = [(BLS, 4), (13, 4), (53, 4), ((1 << 256) - 189, 4), ((1 << 255) - 19, 4), (13, 1), ((1 << 64) - 59, 1), (0xFFFFFFFF00000001, 1)]
IDS = ["bls", "13w", "53w", "2^256-189", "2^255-19", "13n", "2^64-59", "goldilocks"]
PLAIN, ROUND, FIRST = 0, 1, 2
SUB, PAIR = 1, 2


def golden():
    with open(os.path.join(REPO, "tests", "golden", "mimc.json")) as f:
        g = json.load(f)
    assert int(g["modulus"]) == BLS and len(g["cases"]) >= 40
    return g["ROUND"], [(int(c["x"]), int(c["k"]), int(c["out"])) for c in g["cases"]]


def round_ref(p, y, r, r2, r3, key, ctr, r_next):
    x3 = (y ** 3 + 3 * y * y * r + 3 * y * r2 + r3) % p
    return (x3 + key) % p if r_next is None else (x3 + key + ctr + 1 - r_next) % p


# ---- the host model ---------------------------------------------------------------------------------------------------
def test_host_model_equals_the_reference():
    rounds, cases = golden()
    assert rounds == 161 == mimc.ROUND == mimc.rounds_for(BLS)
    corners = {0, 1, 2, BLS - 2, BLS - 1}
    assert {(x, k) for x, k, _ in cases} >= set(itertools.product(corners, repeat=2))
    for x, k, out in cases:
        assert mimc.mimc_plain(x, k) == out == mimc.mimc_plain(x, k, BLS, 161)
    assert mimc.mimc_plain(0, 15) == 19122928589704245340849002450804166427984131042532676177178399305556307915117
    assert mimc.mimc_plain(3, 5, 13, 2) == (pow(pow(3 + 5, 3, 13) + 5 + 1, 3, 13) + 5) % 13


def test_rounds_for():
    assert [mimc.rounds_for(p) for p in (2, 3, 4, 9, 10, 13, 27, 28)] == [1, 1, 2, 2, 3, 3, 3, 4]
    assert mimc.rounds_for((1 << 64) - 59) == 41 and mimc.rounds_for((1 << 256) - 189) == 162
    for p, _ in PRIMES:
        r = mimc.rounds_for(p)
        assert 3 ** r >= p > 3 ** (r - 1)
    for bad in (1, 0, -5, 2.5, "13"):
        with pytest.raises(ValueError):
            mimc.rounds_for(bad)
    for bad in (0, -1, 1.0, True, 1 << 31):
        with pytest.raises(ValueError):
            mimc.mimc_plain(1, 2, 13, bad)


# ---- the cleartext body -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, PAIR], ids=["one", "pair"])
def test_plain_body_equals_the_golden_file(flags):
    rounds, cases = golden()
    xs, ks, outs = ([c[i] for c in cases] for i in range(3))
    rc, got = run(BLS, 4, PLAIN, [xs, ks, None], len(xs), arg=rounds, flags=flags)
    assert rc == 0 and got == outs
    for x, k, out in cases[:6] + cases[-3:]:                         # a key for all, and the counter x + i from start = x
        rc, got = run(BLS, 4, PLAIN, [[x] * 3, [k], None], 3, arg=rounds, bcast=1, flags=flags)
        assert rc == 0 and got == [out] * 3
        rc, got = run(BLS, 4, PLAIN, [None, [k], None], 1, arg=rounds, start=x, bcast=1, flags=flags)
        assert rc == 0 and got == [out]


@pytest.mark.parametrize("p, nl", PRIMES, ids=IDS)
def test_plain_body_equals_python_ints(p, nl):
    rnd = random.Random(p % 1000 + 11 * nl)
    corners = [0, 1, 2, p - 2, p - 1]
    pairs = list(itertools.product(corners, repeat=2)) + [(rnd.randrange(p), rnd.randrange(p)) for _ in range(12)]
    xs, ks = [x for x, _ in pairs], [k for _, k in pairs]
    ms = [rnd.choice([0, 1, p - 1, rnd.randrange(p)]) for _ in pairs]
    n = len(pairs)
    assert (p - 1, p - 1) in pairs
    for rounds in sorted({1, 2, 7, mimc.rounds_for(p)}):
        f = [mimc.mimc_plain(x, k, p, rounds) for x, k in pairs]
        for flags in (0, PAIR):
            rc, got = run(p, nl, PLAIN, [xs, ks, None], n, arg=rounds, flags=flags)
            assert rc == 0 and got == f, (rounds, flags)
            rc, got = run(p, nl, PLAIN, [xs, ks, ms], n, arg=rounds, flags=flags)
            assert rc == 0 and got == [(m + v) % p for m, v in zip(ms, f)], (rounds, flags)
            rc, got = run(p, nl, PLAIN, [xs, ks, ms], n, arg=rounds, flags=flags | SUB)
            assert rc == 0 and got == [(m - v) % p for m, v in zip(ms, f)], (rounds, flags)
            for key in (0, 1, p - 1, ks[-1]):                            # one key for all
                rc, got = run(p, nl, PLAIN, [xs, [key], None], n, arg=rounds, bcast=1, flags=flags)
                assert rc == 0 and got == [mimc.mimc_plain(x, key, p, rounds) for x in xs], (rounds, flags, key)
            # counters: from 0, from a start whose start + i wraps past p, with a key for all and a key per element
            for start in (0, p - 3, rnd.randrange(p)):
                want = [mimc.mimc_plain((start + i) % p, ks[i], p, rounds) for i in range(n)]
                rc, got = run(p, nl, PLAIN, [None, ks, None], n, arg=rounds, start=start, flags=flags)
                assert rc == 0 and got == want, (rounds, flags, start)
                rc, got = run(p, nl, PLAIN, [None, ks, ms], n, arg=rounds, start=start, flags=flags | SUB)
                assert rc == 0 and got == [(m - v) % p for m, v in zip(ms, want)], (rounds, flags, start)
                rc, got = run(p, nl, PLAIN, [None, [ks[3]], ms], n, arg=rounds, start=start, bcast=1, flags=flags)
                assert rc == 0 and got == [(m + mimc.mimc_plain((start + i) % p, ks[3], p, rounds)) % p for i, m in enumerate(ms)]
    rc, got = run(p, nl, PLAIN, [None, [5 % p], None], 0, arg=1, bcast=1)
    assert rc == 0 and got == []


# ---- the round and first-mask bodies ------------------------------------------------------------------------------------
@pytest.mark.parametrize("p, nl", PRIMES, ids=IDS)
def test_round_body_every_corner(p, nl):
    """all 3^6 corner tuples of {0, 1, p - 1} in (y, r, r2, r3, r_next, key) -- every operand p - 1 over 2^256 - 189 among them --
    and random ones, at the first round, the one before the last and the last of 161, in both modes, with a key per element and a
    key for all"""
    rnd = random.Random(p % 1000 + 13 * nl)
    ts = [tuple(c) for c in itertools.product([0, 1, p - 1], repeat=6)] + [tuple(rnd.randrange(p) for _ in range(6)) for _ in range(1024 - 729)]
    assert len(ts) == 1024 and (p - 1,) * 6 in ts
    y, r, r2, r3, rn, key = ([tp[i] for tp in ts] for i in range(6))
    for ctr in (0, 159, 160):
        rc, got = run(p, nl, ROUND, [y, r, r2, r3, key, rn], len(ts), arg=ctr)
        assert rc == 0 and got == [round_ref(p, *tp[:4], tp[5], ctr, tp[4]) for tp in ts], ctr
        rc, got = run(p, nl, ROUND, [y, r, r2, r3, key, None], len(ts), arg=ctr)
        assert rc == 0 and got == [round_ref(p, *tp[:4], tp[5], ctr, None) for tp in ts], ctr
        for k1 in (0, p - 1, key[-1]):
            rc, got = run(p, nl, ROUND, [y, r, r2, r3, [k1], rn], len(ts), arg=ctr, bcast=1)
            assert rc == 0 and got == [round_ref(p, *tp[:4], k1, ctr, tp[4]) for tp in ts], (ctr, k1)
            rc, got = run(p, nl, ROUND, [y, r, r2, r3, [k1], None], len(ts), arg=ctr, bcast=1)
            assert rc == 0 and got == [round_ref(p, *tp[:4], k1, ctr, None) for tp in ts], (ctr, k1)
    # a round counter far above a small modulus
    ctr = (1 << 62) + 12345
    rc, got = run(p, nl, ROUND, [y, r, r2, r3, key, rn], len(ts), arg=ctr)
    assert rc == 0 and got == [round_ref(p, *tp[:4], tp[5], ctr, tp[4]) for tp in ts]


@pytest.mark.parametrize("p, nl", PRIMES, ids=IDS)
def test_bodies_at_edge_values(p, nl):
    """every operand a value on the edges of the words, the digits and the int8 split, or the Montgomery pre-image of one
    (tests/edge_values.py): each list walks the pool at its own stride"""
    import edge_values

    vs = edge_values.operands(p, nl)
    m = len(vs)
    y, r, r2, r3, key, rn = ([vs[(i * s + s) % m] for i in range(m)] for s in (1, 3, 5, 7, 11, 13))
    for ctr in (0, 160):
        rc, got = run(p, nl, ROUND, [y, r, r2, r3, key, rn], m, arg=ctr)
        assert rc == 0 and got == [round_ref(p, *tp[:4], tp[4], ctr, tp[5]) for tp in zip(y, r, r2, r3, key, rn)], ctr
        rc, got = run(p, nl, ROUND, [y, r, r2, r3, key, None], m, arg=ctr)
        assert rc == 0 and got == [round_ref(p, *tp[:4], tp[4], ctr, None) for tp in zip(y, r, r2, r3, key)], ctr
    rounds = mimc.rounds_for(p)
    for flags in (0, PAIR):
        rc, got = run(p, nl, PLAIN, [y, key, None], m, arg=rounds, flags=flags)
        assert rc == 0 and got == [mimc.mimc_plain(x, k, p, rounds) for x, k in zip(y, key)], flags
    rc, got = run(p, nl, FIRST, [y, key, r], m)
    assert rc == 0 and got == [(a + b - c) % p for a, b, c in zip(y, key, r)]


def test_round_body_largest_case():
    p = (1 << 256) - 189
    m = [p - 1] * 4
    for ctr in (0, 159, 160):
        for rn in (m, None):
            rc, got = run(p, 4, ROUND, [m, m, m, m, m, rn], 4, arg=ctr)
            assert rc == 0 and got == [round_ref(p, p - 1, p - 1, p - 1, p - 1, p - 1, ctr, None if rn is None else p - 1)] * 4
    rc, got = run(p, 4, PLAIN, [m, m, m], 4, arg=162)
    assert rc == 0 and got == [(p - 1 + mimc.mimc_plain(p - 1, p - 1, p, 162)) % p] * 4


@pytest.mark.parametrize("p, nl", PRIMES, ids=IDS)
def test_first_mask_body(p, nl):
    rnd = random.Random(p % 1000 + 17 * nl)
    ts = [tuple(c) for c in itertools.product([0, 1, p - 1], repeat=3)] + [tuple(rnd.randrange(p) for _ in range(3)) for _ in range(37)]
    x, key, r0 = ([tp[i] for tp in ts] for i in range(3))
    n = len(ts)
    rc, got = run(p, nl, FIRST, [x, key, r0], n)
    assert rc == 0 and got == [(a + b - c) % p for a, b, c in ts]
    rc, got = run(p, nl, FIRST, [x, [key[-1]], r0], n, bcast=1)
    assert rc == 0 and got == [(a + key[-1] - c) % p for a, _, c in ts]
    for start in (0, p - 5, rnd.randrange(p)):
        rc, got = run(p, nl, FIRST, [None, key, r0], n, start=start)
        assert rc == 0 and got == [(start + i + b - c) % p for i, (_, b, c) in enumerate(ts)], start


def test_chained_bodies_give_the_cipher():
    """first mask, then 161 rounds with cubes of random r: the "opened" value of a round is what the round before wrote (x - r in
    the clear).  A shared x under a key for all, a key per element, and counters under a key per element."""
    rounds, cases = golden()
    p = BLS
    rnd = random.Random(161)
    xs, ks, outs = ([c[i] for c in cases] for i in range(3))
    n = len(cases)
    r = [[rnd.randrange(p) for _ in range(n)] for _ in range(rounds)]
    r2 = [[v * v % p for v in row] for row in r]
    r3 = [[v * v * v % p for v in row] for row in r]

    def chain(x_op, key_op, bcast, start=None):
        rc, cur = run(p, 4, FIRST, [x_op, key_op, r[0]], n, start=start, bcast=bcast)
        assert rc == 0
        for c in range(rounds):
            rc, cur = run(p, 4, ROUND, [cur, r[c], r2[c], r3[c], key_op, r[c + 1] if c + 1 < rounds else None], n, arg=c, bcast=bcast)
            assert rc == 0
        return cur

    assert chain(xs, ks, 0) == outs
    assert chain(xs, [ks[-1]], 1) == [mimc.mimc_plain(x, ks[-1]) for x in xs]
    x0 = cases[-1][0]
    got = chain(None, ks, 0, start=x0)
    assert got == [mimc.mimc_plain(x0 + i, k) for i, k in enumerate(ks)]
    assert chain([x0] * n, [cases[-1][1]], 1)[0] == cases[-1][2]


# ---- the ABI ----------------------------------------------------------------------------------------------------------
def test_abi_names_in_header_and_ctypes_table():
    from honeybadgermpc_amd import _capi

    text = open(os.path.join(REPO, "include", "hbmpc_hip.h")).read()
    for name in ("hb_mimc_plain", "hb_mimc_first", "hb_mimc_round", "hb_selftest_mimc"):
        assert re.search(r"\bint " + name + r"\s*\(", text) and name in _capi.SYMBOLS
    for name, value in (("HB_MIMC_SUB", 1), ("HB_MIMC_PAIR", 2), ("HB_MIMC_SELFTEST_PLAIN", 0), ("HB_MIMC_SELFTEST_ROUND", 1), ("HB_MIMC_SELFTEST_FIRST", 2)):
        assert re.search(r"#define " + name + r" " + str(value) + r"\b", text) and getattr(_capi, name) == value
    assert "progs/mimc.py:10-15" in text and ":25-30" in text and ":46-55" in text


def test_selftest_rejects_bad_arguments():
    v = [1, 2, 3]
    for nl in (4, 1):
        assert run(13, nl, PLAIN, [v, v, None], 3, arg=3)[0] == 0
        assert run(13, nl, PLAIN, [v, v, None], 3, arg=0)[0] == 2                 # rounds < 1
        assert run(13, nl, PLAIN, [v, v, None], 3, arg=-4)[0] == 2
        assert run(13, nl, PLAIN, [v, v, None], -1, arg=3)[0] == 2                # a negative count
        assert run(13, nl, PLAIN, [v, None, None], 3, arg=3)[0] == 2              # no key
        assert run(13, nl, PLAIN, [v, v, None], 3, arg=3, flags=SUB)[0] == 2      # addend - F without an addend
        assert run(13, nl, PLAIN, [v, v, v], 3, arg=3, flags=4)[0] == 2           # an unknown flag
        assert run(13, nl, PLAIN, [None, v, None], 3, arg=3, start=13)[0] == 2    # start not below the modulus
        assert run(13, nl, PLAIN, [None, v, None], 3, arg=3, start=12)[0] == 0
        assert run(13, nl, ROUND, [v, v, v, v, v, v], 3, arg=0)[0] == 0
        assert run(13, nl, ROUND, [v, v, v, v, v, v], 3, arg=-1)[0] == 2          # a negative round counter
        assert run(13, nl, ROUND, [v, v, v, v, v, v], -1, arg=0)[0] == 2
        for i in range(5):
            ops = [v] * 6
            ops[i] = None
            assert run(13, nl, ROUND, ops, 3, arg=0)[0] == 2                      # a missing operand
        assert run(13, nl, FIRST, [v, v, v], 3)[0] == 0
        assert run(13, nl, FIRST, [v, v, None], 3)[0] == 2
        assert run(13, nl, FIRST, [v, None, v], 3)[0] == 2
        assert run(13, nl, FIRST, [None, v, v], 3, start=14)[0] == 2
        assert run(13, nl, 3, [v, v, v], 3, arg=1)[0] == 2                        # unknown `what`
        assert run(13, nl, ROUND, [[], [], [], [], [], []], 0, arg=0)[0] == 0
    assert run(13, 2, PLAIN, [v, v, None], 3, arg=3)[0] == 2                      # neither 1 nor 4 limbs

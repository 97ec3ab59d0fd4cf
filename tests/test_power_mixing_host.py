"""CPU-only: the bodies of the power-mixing kernels (csrc/hb_pm.hip) run on the host through hb_selftest_pm -- the same HB_HD
functions the kernels call, walked tile by tile and lane by lane -- against Python ints and the binomial formula

    [a^m] = sum_{j <= m} C(m, j) c^(m-j) [b^j],   [b^0] = 1

applied to arbitrary "share" values (the map is linear in them), and Newton's identities of power_mixing.py.  Exact equality."""
import math
import os
import random
import re

import numpy as np
import pytest

from conftest import BLS, REPO

from honeybadgermpc_amd.power_mixing import newton_coefficients, transform_order

PRIMES = [(BLS, 4), (13, 4), (53, 4), ((1 << 256) - 189, 4), ((1 << 255) - 19, 4), (13, 1), ((1 << 64) - 59, 1), (0xFFFFFFFF00000001, 1)]
IDS = ["bls", "13w", "53w", "2^256-189", "2^255-19", "13n", "2^64-59", "goldilocks"]
KS = [1, 2, 3, 8, 33, 64]
SUMS, POWERS, TABLES, MAC, CONV = 0, 1, 2, 3, 4
# products between two reductions in the lazy accumulation of hb_pm.hip (PmAcc<NL>::L = 4 Lazy<NL>::GROUP): L p <= 2^(29 NL)
ACC_LEN = {4: 28, 1: 84}


def run(p, nl, what, cs, powers, k, group=1, rows=None):
    """hb_selftest_pm over lists of ints -> (rc, flat list of ints)"""
    from honeybadgermpc_amd._capi import ints_to_limbs, limbs_to_ints, load_library, np_ptr

    lib = load_library()
    nb = 8 * nl
    m = len(powers)
    flat = [x for row in powers for x in row]
    c_arr = ints_to_limbs(list(cs) or [0], p, nb)
    p_arr = ints_to_limbs(flat or [0], p, nb)
    n_out = {SUMS: k, POWERS: m * k, TABLES: 2 * m * (k + 1), MAC: k}[what] if rows is None else rows
    out = np.zeros((max(n_out, 1), nl), dtype=np.uint64)
    rc = lib.hb_selftest_pm(np_ptr(ints_to_limbs([p], p + 1, nb)), nl, what, np_ptr(c_arr), np_ptr(p_arr), m, k, group, np_ptr(out))
    return rc, limbs_to_ints(out[:n_out], nb)


def binomial_powers(p, c, shares, k):
    """[a^m], m = 1 .. k, from c and the values standing for [b^1] .. [b^k]"""
    b = [1] + list(shares)
    return [sum(math.comb(m, j) * pow(c, m - j, p) * b[j] for j in range(m + 1)) % p for m in range(1, k + 1)]


def draw(p, rnd):
    return rnd.choice([0, 1, p - 1, rnd.randrange(p), rnd.randrange(p), rnd.randrange(p)])


@pytest.mark.parametrize("p, nl", PRIMES, ids=IDS)
def test_direct_path_against_the_binomial_formula(p, nl):
    rnd = random.Random(p % 1000 + 3 * nl)
    for k in [k for k in KS if k < p]:
        for m in sorted({1, 2, k, k + 3}):
            cs = [draw(p, rnd) for _ in range(m)]
            powers = [[draw(p, rnd) for _ in range(k)] for _ in range(m)]
            if m >= 2:
                cs[0] = 0                                     # c = 0: a = b, the powers pass through unchanged
                cs[1] = p - 1
                powers[1] = [p - 1] * k
            want = [binomial_powers(p, c, row, k) for c, row in zip(cs, powers)]
            if cs[0] == 0:
                assert want[0] == [x % p for x in powers[0]]
            rc, got = run(p, nl, POWERS, cs, powers, k)
            assert rc == 0 and got == [x for row in want for x in row], (k, m)
            sums = [sum(row[i] for row in want) % p for i in range(k)]
            for group in sorted({1, 2, m}):
                rc, got = run(p, nl, SUMS, cs, powers, k, group=group)
                assert rc == 0 and got == sums, (k, m, group)


@pytest.mark.parametrize("p, nl", PRIMES, ids=IDS)
def test_true_powers_give_true_powers(p, nl):
    """shares that ARE b^j (one party, degree 0): the outputs are a^m"""
    rnd = random.Random(p % 1000 + 5 * nl)
    k = max(k for k in KS if k < p)
    msgs = [rnd.randrange(p) for _ in range(5)]
    bs = [rnd.randrange(p) for _ in range(5)]
    rc, got = run(p, nl, POWERS, [(a - b) % p for a, b in zip(msgs, bs)], [[pow(b, j, p) for j in range(1, k + 1)] for b in bs], k)
    assert rc == 0 and got == [pow(a, m, p) for a in msgs for m in range(1, k + 1)]


@pytest.mark.parametrize("p, nl", PRIMES, ids=IDS)
def test_tables_on_the_host(p, nl):
    rnd = random.Random(p % 1000 + 7 * nl)
    k = max(k for k in KS if k < p)
    cs = [0, 1, p - 1, rnd.randrange(p)]
    powers = [[draw(p, rnd) for _ in range(k)] for _ in cs]
    rc, got = run(p, nl, TABLES, cs, powers, k)
    assert rc == 0
    inv_fact = [pow(math.factorial(j) % p, -1, p) for j in range(k + 1)]
    u = [[1] + [row[j - 1] * inv_fact[j] % p for j in range(1, k + 1)] for row in powers]
    v = [[pow(c, i, p) * inv_fact[i] % p for i in range(k + 1)] for c in cs]
    assert got == [x for row in u for x in row] + [x for row in v for x in row]


@pytest.mark.parametrize("p, nl", PRIMES, ids=IDS)
def test_every_operand_p_minus_1_at_the_accumulation_bound(p, nl):
    """The lazy accumulation takes ACC_LEN products between two reductions (hb_pm.hip's header proves L p <= 2^(29 NL)): the
    largest value its columns and REDC ever see is every operand p - 1 over a whole window -- here at exactly that length,
    one below, one above and several windows, for the multiply-accumulate pass and for the direct path's windows."""
    acc = ACC_LEN[nl]
    for m in (acc - 1, acc, acc + 1, 3 * acc):
        rows = [[p - 1] * 5 for _ in range(m)]
        for group in (m, acc, 7):
            rc, got = run(p, nl, MAC, [x for r in rows for x in r], rows, 5, group=group)
            assert rc == 0 and got == [m % p] * 5, (m, group)
    # the direct kernel's staging and windows over tables that are p - 1 throughout: output m sums m + 1 products (p - 1)^2 = 1,
    # so the outputs around m + 1 = acc, 2 acc, ... sit exactly at whole windows; k = 300 also crosses into a second tile
    for k in (acc - 1, acc, acc + 1, 3 * acc, 300):
        for clients in (1, 3):
            rows = [[p - 1] * (k + 1) for _ in range(clients)]
            rc, got = run(p, nl, CONV, [x for r in rows for x in r], rows, k, group=clients, rows=k)
            assert rc == 0 and got == [clients * (m + 1) % p for m in range(1, k + 1)], (k, clients)


@pytest.mark.parametrize("p, nl", PRIMES, ids=IDS)
def test_mac_pass_random(p, nl):
    rnd = random.Random(p % 1000 + 9 * nl)
    for m, n, group in ((1, 3, 1), (5, 8, 2), (100, 4, 33), (200, 2, 200)):
        u = [[draw(p, rnd) for _ in range(n)] for _ in range(m)]
        v = [[draw(p, rnd) for _ in range(n)] for _ in range(m)]
        rc, got = run(p, nl, MAC, [x for r in u for x in r], v, n, group=group)
        assert rc == 0 and got == [sum(u[c][f] * v[c][f] for c in range(m)) % p for f in range(n)]


@pytest.mark.parametrize("p, nl", PRIMES, ids=IDS)
def test_mac_pass_at_edge_values(p, nl):
    """the multiply-accumulate pass over values on the edges of the words, the digits and the int8 split, and their Montgomery pre-images
    (tests/edge_values.py): every ordered pair meets once across the rows, in windows of one, of the accumulation bound and of all rows"""
    import edge_values

    vs = edge_values.operands(p, nl)
    m = len(vs)
    u = [[vs[(c + f) % m] for f in range(m)] for c in range(m)]
    v = [[vs[(3 * c + 2 * f + 1) % m] for f in range(m)] for c in range(m)]
    want = [sum(u[c][f] * v[c][f] for c in range(m)) % p for f in range(m)]
    for group in (1, ACC_LEN[nl], m):
        rc, got = run(p, nl, MAC, [x for r in u for x in r], v, m, group=group)
        assert rc == 0 and got == want, group


def test_argument_checks_on_the_host():
    for nl in (4, 1):
        assert run(13, nl, SUMS, [1], [[1] * 13], 13)[0] == 2          # k >= p: HB_ERR_BAD_ARG
        assert run(13, nl, POWERS, [1], [[1] * 14], 14)[0] == 2
        assert run(13, nl, SUMS, [1], [[1] * 12], 12)[0] == 0
        assert run(13, nl, SUMS, [1], [[]], 0, rows=1)[0] == 2         # k <= 0
        assert run(13, nl, 7, [1], [[1]], 1, rows=1)[0] == 2           # unknown `what`
    rc, got = run(BLS, 4, SUMS, [], [], 5)                            # no clients: zeros
    assert rc == 0 and got == [0] * 5


def test_transform_order():
    assert [transform_order(k) for k in (1, 2, 3, 4, 63, 64, 1000, 1024, 2048)] == [4, 8, 8, 16, 128, 256, 2048, 4096, 8192]


@pytest.mark.parametrize("p", [BLS, (1 << 64) - 59, 53], ids=["bls", "2^64-59", "53"])
def test_newton_coefficients(p):
    rnd = random.Random(p % 1000)
    for k in (1, 2, 7, 40):
        if k >= p:
            continue
        msgs = [rnd.randrange(p) for _ in range(k)]
        sums = [sum(pow(a, m, p) for a in msgs) % p for m in range(1, k + 1)]
        coeffs = newton_coefficients(sums, p)
        assert len(coeffs) == k + 1 and coeffs[k] == 1 and all(0 <= c < p for c in coeffs)

        def at(x):
            return sum(c * pow(x, i, p) for i, c in enumerate(coeffs)) % p

        assert all(at(a) == 0 for a in msgs)
        others = [x for x in (rnd.randrange(p) for _ in range(100)) if x not in msgs]
        assert others and all(at(x) != 0 for x in others)
    assert newton_coefficients([5], p) == [(-5) % p, 1]
    with pytest.raises(ValueError):
        newton_coefficients([], p)
    with pytest.raises(ValueError):
        newton_coefficients([1] * 13, 13)


def test_abi_names_in_header_and_ctypes_table():
    from honeybadgermpc_amd import _capi

    text = open(os.path.join(REPO, "include", "hbmpc_hip.h")).read()
    for name in ("hb_pm_power_sums", "hb_pm_powers", "hb_selftest_pm"):
        assert re.search(r"\bint " + name + r"\s*\(", text) and name in _capi.SYMBOLS
    for name, value in (("HB_PM_AUTO", 0), ("HB_PM_DIRECT", 1), ("HB_PM_NTT", 2)):
        assert re.search(r"#define " + name + r" " + str(value) + r"\b", text) and getattr(_capi, name) == value
    assert "hb_debug_pm_slab_bytes" in _capi.DEBUG_SYMBOLS

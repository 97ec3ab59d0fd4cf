"""CPU-only: honeybadgermpc_amd.progs.fixedpoint -- the host functions and host models against tests/golden/fixedpoint.json (written by
scratch/gen_fixedpoint_golden.py from the reference's own progs/fixedpoint.py: its pure functions, and its trunc_pr / div2m / trunc
coroutines driven over cleartext shares with recorded bits), the algebraic identities of the models over four fields, and the
per-element bodies of csrc/hb_fxp.hip run on the host through hb_selftest_fxp -- the same HB_HD functions the kernels call -- against
Python ints, the carry tree level by level among them.  Exact equality."""
import ctypes
import itertools
import json
import os
import random
import re

import numpy as np
import pytest

from conftest import BLS, REPO

from honeybadgermpc_amd.progs import fixedpoint as fx

GOLDILOCKS = 0xFFFFFFFF00000001
P64 = (1 << 64) - 59
P256 = (1 << 256) - 189
FIELDS = [(BLS, 4), (P256, 4), (P64, 1), (GOLDILOCKS, 1)]
FIELD_IDS = ["bls", "2^256-189", "2^64-59", "goldilocks"]
MASK, TRUNC_PR, LEAVES, CARRY_MASK, CARRY_COMBINE, FINISH = range(6)


def shapes_for(p):
    """(k, m, kappa) of the issue: the wide sets on the 32-byte fields, the narrow ones on the 64-bit primes"""
    return [(64, 32, 32), (128, 32, 32), (64, 63, 32)] if p >> 64 else [(16, 8, 16), (32, 8, 16), (16, 15, 16)]


def golden():
    with open(os.path.join(REPO, "tests", "golden", "fixedpoint.json")) as f:
        return json.load(f)


def run(p, nl, what, operands, params, out_rows, count):
    """hb_selftest_fxp over lists of ints (None: a NULL operand; arrays of several rows are flat, row-major) -> (rc, [out lists])"""
    from honeybadgermpc_amd._capi import ints_to_limbs, limbs_to_ints, load_library, np_ptr

    lib = load_library()
    nb = 8 * nl
    arrays = [None if o is None else ints_to_limbs(list(o) or [0], p, nb) for o in operands]
    ptrs = (ctypes.c_void_p * 6)(*([None if x is None else x.ctypes.data for x in arrays] + [None] * (6 - len(arrays))))
    outs = [None if r is None else np.zeros((max(r * count, 1), nl), dtype=np.uint64) for r in out_rows]
    optrs = (ctypes.c_void_p * 2)(*([None if o is None else o.ctypes.data for o in outs] + [None] * (2 - len(outs))))
    prm = (ctypes.c_int64 * 5)(*(list(params) + [0] * (5 - len(params))))
    rc = lib.hb_selftest_fxp(np_ptr(ints_to_limbs([p], p + 1, nb)), nl, what, ptrs, prm, optrs, count)
    return rc, [None if o is None else limbs_to_ints(o[:r * count], nb) for o, r in zip(outs, out_rows)]


def masks(bits, m):
    """(r1, r2) from a list of bits, least significant first"""
    return sum(b << i for i, b in enumerate(bits[:m])), sum(b << i for i, b in enumerate(bits[m:]))


def signed_draws(rnd, k):
    top = 1 << (k - 1)
    return [0, 1, -1, top - 1, -(top - 1), -top] + [rnd.randrange(-top, top) for _ in range(6)]


# ---- the host functions against the reference ------------------------------------------------------------------------------
def test_pure_functions_equal_the_reference():
    g = golden()
    assert (g["F"], g["KAPPA"], g["K"]) == (fx.F, fx.KAPPA, fx.K) == (32, 32, 64) and int(g["modulus"]) == BLS
    assert len(g["to_fixed"]) >= 50 and len(g["binary"]) >= 50 and len(g["from_fixed"]) >= 50
    for c in g["to_fixed"]:
        x = float.fromhex(c["x"]) if "x" in c["x"] or "p" in c["x"] else int(c["x"])
        assert fx.to_fixed_point_repr(x, c["f"]) == int(c["out"]), c
    assert fx.to_fixed_point_repr(-3.8) == int(-3.8 * 2 ** 32) and fx.to_fixed_point_repr(-2.0 ** -33) == 0        # towards zero
    for c in g["binary"]:
        assert "".join(map(str, fx.binary_repr(int(c["x"]), c["k"]))) == c["out"], c
    with pytest.raises(TypeError):
        fx.binary_repr(2.0, 8)
    for c in g["from_fixed"]:
        assert fx.from_fixed_point_repr(int(c["v"]), BLS, c["k"], c["f"], c["signed"]) == float.fromhex(c["out"]), c


def test_host_models_equal_the_reference_coroutines():
    g = golden()
    for name, model in (("trunc_pr", fx.trunc_pr_model), ("div2m", fx.div2m_model), ("trunc", fx.trunc_model)):
        assert len(g[name]) >= 20
        for c in g[name]:
            k, m, x = c["k"], c["m"], int(c["x"])
            bits = [int(b) for b in c["bits"]]
            assert len(bits) == k + g["KAPPA"]
            r1, r2 = masks(bits, m)
            assert model(x % BLS, r1, r2, BLS, k, m) == int(c["out"]), (name, c)


@pytest.mark.parametrize("p, nl", FIELDS, ids=FIELD_IDS)
def test_host_model_identities(p, nl):
    rnd = random.Random(p % 1009)
    for k, m, kappa in shapes_for(p):
        fx.check_params(p, k, m, kappa, full=True)
        for x in signed_draws(rnd, k):
            for mode in ("random", "random", "zero", "one"):
                n = k + kappa
                bits = [rnd.getrandbits(1) for _ in range(n)] if mode == "random" else [0 if mode == "zero" else 1] * n
                r1, r2 = masks(bits, m)
                xr = x % p
                assert fx.div2m_model(xr, r1, r2, p, k, m, kappa) == x % (1 << m), (k, m, x)
                assert fx.trunc_model(xr, r1, r2, p, k, m, kappa) == (x >> m) % p, (k, m, x)
                assert fx.trunc_pr_model(xr, r1, r2, p, k, m, kappa) == ((x >> m) + (1 if (x % (1 << m)) + r1 >= 1 << m else 0)) % p, (k, m, x)
                if m == k - 1:
                    assert fx.ltz_model(xr, r1, r2, p, k, kappa) == (1 if x < 0 else 0), (k, x)
        r1, r2 = masks([rnd.getrandbits(1) for _ in range(k + kappa)], k - 1)
        for x in signed_draws(rnd, k):
            assert fx.ltz_model(x % p, r1, r2, p, k, kappa) == (1 if x < 0 else 0)


def test_parameter_checks_and_tree_counts():
    for p, k, m, kappa in ((BLS, 64, 0, 32), (BLS, 64, 64, 32), (BLS, 64, 65, 32), (BLS, 64, -1, 32), (BLS, 222, 32, 32), (BLS, 64, 32, 190), (P64, 32, 8, 31),
                           (P64, 64, 32, 32), (GOLDILOCKS, 47, 8, 16), (BLS, 64, 32, -1), (BLS, 64.0, 32, 32), (BLS, 64, True, 32)):
        with pytest.raises(ValueError):
            fx.check_params(p, k, m, kappa)
    fx.check_params(BLS, 221, 32, 32)            # 221 + 32 + 1 = 254 = 255 - 1
    fx.check_params(P64, 46, 8, 16)              # 46 + 16 + 1 = 63
    fx.check_params(GOLDILOCKS, 46, 8, 16)
    fx.check_params(BLS, 128, 32, 32)            # what mul asks for: trunc_pr(., 2 K, F)
    with pytest.raises(ValueError):
        fx.trunc_pr_model(1, 0, 0, P64, 64, 32)
    assert [fx.carry_levels(m) for m in (1, 2, 3, 4, 7, 8, 31, 63, 64, 100)] == [1, 2, 2, 3, 3, 4, 5, 6, 7, 7]
    assert all(fx.carry_triples(m) == 2 * m - 1 <= 2 * m for m in range(1, 130))
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError):
            fx.carry_levels(bad)
        with pytest.raises(ValueError):
            fx.carry_triples(bad)


def test_argument_checks_raise_before_anything_is_called_in_c():
    """a context whose library refuses every call: the parameter checks of the tensor level and of the coroutines come first"""
    import asyncio

    class NoLib:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was called")

    class Ctx:
        modulus, n_limbs, lib = BLS, 4, NoLib()

        def elems(self, *a, **k):
            raise AssertionError("an operand was looked at")

    class Co:
        ctx, batches = Ctx(), 0

    ctx, co = Ctx(), Co()
    for call in (lambda: fx.random2m(ctx, None, 64, 64, 32), lambda: fx.trunc_mask(ctx, None, None, 64, 0, 32), lambda: fx.trunc_mask(ctx, None, None, 200, 32, 54),
                 lambda: fx.trunc_pr_finish(ctx, None, None, None, 0), lambda: fx.trunc_pr_finish(ctx, None, None, None, 254), lambda: fx.ltl_leaves(ctx, None, None, 254),
                 lambda: fx.div2m_finish(ctx, None, None, None, None, 0), lambda: fx.div2m_finish(ctx, None, None, None, None, 8, mode=3)):
        with pytest.raises(ValueError):
            call()
    for coro in (lambda: fx.trunc_pr(co, None, None, 64, 64), lambda: fx.div2m(co, None, None, None, 64, 0), lambda: fx.trunc(co, None, None, None, 222, 32),
                 lambda: fx.ltz(co, None, None, None, k=222), lambda: fx.lt(co, None, None, None, None, k=1), lambda: fx.mul(co, None, None, None, None, f=32, k=111)):
        with pytest.raises(ValueError):
            asyncio.run(coro())


# ---- the kernels' bodies -----------------------------------------------------------------------------------------------------
def draw(rnd, p, n):
    return [rnd.choice([0, 1, p - 1, rnd.randrange(p), rnd.randrange(p)]) for _ in range(n)]


@pytest.mark.parametrize("p, nl", FIELDS, ids=FIELD_IDS)
def test_mask_body(p, nl):
    """the planes hold SHARES, any residues: x + 2^(k-1) + sum 2^i b_i and r1, r2 for corner and random residues in every slot"""
    rnd = random.Random(p % 1000 + 3)
    extra = [(130, 65, 32), (200, 127, 32), (65, 64, 0), (64, 29, 32), (70, 58, 7)] if nl == 4 else [(20, 3, 10), (30, 29, 0), (2, 1, 0)]
    for k, m, kappa in shapes_for(p) + extra:
        n, count = k + kappa, 7
        planes = [draw(rnd, p, count) for _ in range(n)]
        for corner in (0, 1, p - 1):
            planes[rnd.randrange(n)] = [corner] * count
        if k == 64 and m == 63:
            planes = [[p - 1] * count for _ in range(n)]
        xs = [0, 1, p - 1] + draw(rnd, p, count - 3)
        flat = [v for row in planes for v in row]
        r1 = [sum(planes[i][e] << i for i in range(m)) % p for e in range(count)]
        r2 = [sum(planes[m + i][e] << i for i in range(n - m)) % p for e in range(count)]
        rc, (masked, got_r1) = run(p, nl, MASK, [xs, flat], [k, m, kappa], [1, 1], count)
        assert rc == 0 and got_r1 == r1 and masked == [(x + (1 << (k - 1)) + a + (b << m)) % p for x, a, b in zip(xs, r1, r2)], (k, m, kappa)
        rc, (got_r2, got_r1) = run(p, nl, MASK, [None, flat], [k, m, kappa], [1, 1], count)
        assert rc == 0 and got_r1 == r1 and got_r2 == r2, (k, m, kappa)


@pytest.mark.parametrize("p, nl", FIELDS, ids=FIELD_IDS)
def test_mask_trunc_and_finish_bodies_at_edge_values(p, nl):
    """the planes, x, c, r1 and the carry values on the edges of the words, the digits and the int8 split, or Montgomery pre-images of
    such (tests/edge_values.py): each plane and operand walks the list at a stride of its own"""
    import edge_values

    vs = edge_values.operands(p, nl)
    count = len(vs)
    walk = lambda s: [vs[(i * s + s) % count] for i in range(count)]    # noqa: E731
    for k, m, kappa in shapes_for(p):
        n = k + kappa
        planes = [walk(2 * j + 1) for j in range(n)]
        xs = walk(2 * n + 1)
        r1 = [sum(planes[i][e] << i for i in range(m)) % p for e in range(count)]
        r2 = [sum(planes[m + i][e] << i for i in range(n - m)) % p for e in range(count)]
        rc, (masked, got_r1) = run(p, nl, MASK, [xs, [v for row in planes for v in row]], [k, m, kappa], [1, 1], count)
        assert rc == 0 and got_r1 == r1 and masked == [(x + (1 << (k - 1)) + a + (b << m)) % p for x, a, b in zip(xs, r1, r2)], (k, m, kappa)
    x, c, r1, carry = walk(3), walk(5), walk(7), walk(11)
    for m in (1, 29, 32, 58) + ((64, 128, 253) if nl == 4 else ()):
        inv = pow(2, -m, p)
        rc, (got,) = run(p, nl, TRUNC_PR, [x, c, r1, [inv]], [0, m], [1], count)
        assert rc == 0 and got == [(a - b % (1 << m) + d) * inv % p for a, b, d in zip(x, c, r1)], m
        for mode in (fx.MOD, fx.TRUNC, fx.NEG_TRUNC):
            a2 = [(b % (1 << m) - d + (1 << m) * (1 - e)) % p for b, d, e in zip(c, r1, carry)]
            want = a2 if mode == fx.MOD else [(a - v) * inv * (1 if mode == fx.TRUNC else -1) % p for a, v in zip(x, a2)]
            rc, (got,) = run(p, nl, FINISH, [None if mode == fx.MOD else x, c, r1, carry, [inv]], [0, m, 0, mode], [1], count)
            assert rc == 0 and got == want, (m, mode)


@pytest.mark.parametrize("p, nl", FIELDS, ids=FIELD_IDS)
def test_trunc_pr_leaf_and_finish_bodies(p, nl):
    rnd = random.Random(p % 1000 + 5)
    ms = [1, 8, 15, 29, 31, 32, 33, 58, 62] + ([63, 64, 65, 100, 127, 128, 129, 191, 193, 253] if nl == 4 else [])
    corners = [tuple(c) for c in itertools.product([0, 1, p - 1], repeat=4)]
    for m in ms:
        ts = corners + [tuple(rnd.randrange(p) for _ in range(4)) for _ in range(20)]
        x, c, r1, carry = ([t[i] for t in ts] for i in range(4))
        c[-1], c[-2] = (1 << m) - 1, 1 << m
        n, inv = len(ts), pow(2, -m, p)
        rc, (got,) = run(p, nl, TRUNC_PR, [x, c, r1, [inv]], [0, m], [1], n)
        assert rc == 0 and got == [(a - b % (1 << m) + d) * inv % p for a, b, d in zip(x, c, r1)], m
        for mode in (fx.MOD, fx.TRUNC, fx.NEG_TRUNC):
            a2 = [(b % (1 << m) - d + (1 << m) * (1 - e)) % p for b, d, e in zip(c, r1, carry)]
            want = a2 if mode == fx.MOD else [(a - v) * inv * (1 if mode == fx.TRUNC else -1) % p for a, v in zip(x, a2)]
            rc, (got,) = run(p, nl, FINISH, [None if mode == fx.MOD else x, c, r1, carry, [inv]], [0, m, 0, mode], [1], n)
            assert rc == 0 and got == want, (m, mode)
        # the leaves: bit i of c selects between (1 - b, b) and (0, 1 - b); b any residue
        count = 9
        cs = [0, (1 << m) - 1, 1 << m, p - 1] + [rnd.randrange(p) for _ in range(count - 4)]
        planes = [draw(rnd, p, count) for _ in range(m)]
        rc, (g, q) = run(p, nl, LEAVES, [cs, [v for row in planes for v in row]], [0, m], [m + 1, m + 1], count)
        assert rc == 0
        for j in range(m + 1):
            for e in range(count):
                if j == m:
                    want = (1, 0)
                else:
                    b = planes[m - 1 - j][e]
                    want = ((1 - b) % p, b) if (cs[e] >> (m - 1 - j)) & 1 else (0, (1 - b) % p)
                assert (g[j * count + e], q[j * count + e]) == want, (m, j, e)


@pytest.mark.parametrize("p, nl", FIELDS, ids=FIELD_IDS)
def test_carry_level_bodies(p, nl):
    rnd = random.Random(p % 1000 + 7)
    count = 5
    for nodes, root in ((2, 1), (2, 0), (3, 0), (4, 0), (5, 0), (9, 0), (64, 0), (101, 0)):
        triples = 1 if root else 2 * (nodes // 2)
        g, q = ([draw(rnd, p, count) for _ in range(nodes)] for _ in range(2))
        ta, tb, tab = ([draw(rnd, p, count) for _ in range(triples)] for _ in range(3))
        if nodes == 3:
            g, q, ta, tb, tab = ([[p - 1] * count for _ in v] for v in (g, q, ta, tb, tab))
        flat = lambda rows: [v for row in rows for v in row]     # noqa: E731
        rc, (masked,) = run(p, nl, CARRY_MASK, [flat(g), flat(q), flat(ta), flat(tb)], [0, 0, 0, nodes, root], [2 * triples], count)
        assert rc == 0
        want = []
        for t in range(triples):
            second = q if t & 1 else g
            want += [(q[2 * (t // 2)][e] - ta[t][e]) % p for e in range(count)] + [(second[2 * (t // 2) + 1][e] - tb[t][e]) % p for e in range(count)]
        assert masked == want, nodes
        opened = draw(rnd, p, 2 * triples * count)
        out_nodes = (nodes + 1) // 2
        rc, (g2, q2) = run(p, nl, CARRY_COMBINE, [opened, flat(g), flat(q), flat(ta), flat(tb), flat(tab)], [0, 0, 0, nodes, root], [out_nodes, None if root else out_nodes], count)
        assert rc == 0

        def beaver(t, e):
            d, f = opened[2 * t * count + e], opened[(2 * t + 1) * count + e]
            return (d * f + d * tb[t][e] + f * ta[t][e] + tab[t][e]) % p

        for j in range(out_nodes):
            for e in range(count):
                if 2 * j + 1 >= nodes:
                    assert (g2[j * count + e], q2[j * count + e]) == (g[2 * j][e], q[2 * j][e])
                    continue
                assert g2[j * count + e] == (g[2 * j][e] + beaver(2 * j, e)) % p, (nodes, j)
                if not root:
                    assert q2[j * count + e] == beaver(2 * j + 1, e), (nodes, j)


@pytest.mark.parametrize("m", [1, 2, 3, 7, 8, 31, 63, 64, 100])
def test_carry_tree_on_cleartext_shares(m):
    """degree-0 "shares": what a level opens is what its mask wrote.  The root's g is the carry bit of c2 + (2^m - 1 - r1) + 1, and
    the run consumes carry_levels(m) opens and carry_triples(m) triples."""
    rnd = random.Random(m)
    for p, nl in ((BLS, 4), (P64, 1)):
        if m > p.bit_length() - 2:
            continue
        count = 12
        c2 = [0, (1 << m) - 1, 0, (1 << m) - 1, 5 % (1 << m), 5 % (1 << m)] + [rnd.getrandbits(m) for _ in range(count - 6)]
        r1 = [0, 0, (1 << m) - 1, (1 << m) - 1, 5 % (1 << m), 6 % (1 << m)] + [rnd.getrandbits(m) for _ in range(count - 6)]
        high = [rnd.getrandbits(20) << m for _ in range(count)]                      # the bits of c above m do not matter
        planes = [(r >> i) & 1 for i in range(m) for r in r1]
        rc, (g, q) = run(p, nl, LEAVES, [[a + b for a, b in zip(c2, high)], planes], [0, m], [m + 1, m + 1], count)
        assert rc == 0
        nodes, levels, used = m + 1, 0, 0
        while nodes > 1:
            root = int(nodes == 2)
            triples = 1 if root else 2 * (nodes // 2)
            ta, tb = ([rnd.randrange(p) for _ in range(triples * count)] for _ in range(2))
            tab = [a * b % p for a, b in zip(ta, tb)]
            rc, (masked,) = run(p, nl, CARRY_MASK, [g, q, ta, tb], [0, 0, 0, nodes, root], [2 * triples], count)
            assert rc == 0
            out_nodes = (nodes + 1) // 2
            rc, (g, q) = run(p, nl, CARRY_COMBINE, [masked, g, q, ta, tb, tab], [0, 0, 0, nodes, root], [out_nodes, None if root else out_nodes], count)
            assert rc == 0
            nodes, levels, used = out_nodes, levels + 1, used + triples
        assert g == [(a + (1 << m) - 1 - b + 1) >> m for a, b in zip(c2, r1)] == [int(a >= b) for a, b in zip(c2, r1)]
        assert levels == fx.carry_levels(m) and used == fx.carry_triples(m)


def test_chained_bodies_give_the_reference_results():
    """mask -> (open) -> leaves -> tree -> finish on cleartext shares with the golden cases' bits: the reference's own outputs"""
    g = golden()
    p, nl, kappa = BLS, 4, g["KAPPA"]
    rnd = random.Random(9)
    for name, mode in (("div2m", fx.MOD), ("trunc", fx.TRUNC)):
        for (k, m), cases in itertools.groupby(sorted(g[name], key=lambda c: (c["k"], c["m"])), key=lambda c: (c["k"], c["m"])):
            cases = list(cases)
            count = len(cases)
            xs = [int(c["x"]) % p for c in cases]
            planes = [int(c["bits"][i]) for i in range(k + kappa) for c in cases]
            rc, (c_open, r1) = run(p, nl, MASK, [xs, planes], [k, m, kappa], [1, 1], count)
            assert rc == 0
            rc, (gg, qq) = run(p, nl, LEAVES, [c_open, planes[:m * count]], [0, m], [m + 1, m + 1], count)
            nodes = m + 1
            while nodes > 1:
                root = int(nodes == 2)
                triples = 1 if root else 2 * (nodes // 2)
                ta, tb = ([rnd.randrange(p) for _ in range(triples * count)] for _ in range(2))
                tab = [a * b % p for a, b in zip(ta, tb)]
                rc, (masked,) = run(p, nl, CARRY_MASK, [gg, qq, ta, tb], [0, 0, 0, nodes, root], [2 * triples], count)
                rc2, (gg, qq) = run(p, nl, CARRY_COMBINE, [masked, gg, qq, ta, tb, tab], [0, 0, 0, nodes, root], [(nodes + 1) // 2, None if root else (nodes + 1) // 2], count)
                assert rc == 0 and rc2 == 0
                nodes = (nodes + 1) // 2
            rc, (got,) = run(p, nl, FINISH, [xs, c_open, r1, gg, [pow(2, -m, p)]], [0, m, 0, mode], [1], count)
            assert rc == 0 and got == [int(c["out"]) for c in cases], (name, k, m)
    for (k, m), cases in itertools.groupby(sorted(g["trunc_pr"], key=lambda c: (c["k"], c["m"])), key=lambda c: (c["k"], c["m"])):
        cases = list(cases)
        count = len(cases)
        xs = [int(c["x"]) % p for c in cases]
        planes = [int(c["bits"][i]) for i in range(k + kappa) for c in cases]
        rc, (c_open, r1) = run(p, nl, MASK, [xs, planes], [k, m, kappa], [1, 1], count)
        rc2, (got,) = run(p, nl, TRUNC_PR, [xs, c_open, r1, [pow(2, -m, p)]], [0, m], [1], count)
        assert rc == 0 and rc2 == 0 and got == [int(c["out"]) for c in cases], (k, m)


# ---- the ABI -----------------------------------------------------------------------------------------------------------------
def test_abi_names_in_header_and_ctypes_table():
    from honeybadgermpc_amd import _capi

    text = open(os.path.join(REPO, "include", "hbmpc_hip.h")).read()
    for name in ("hb_fxp_mask", "hb_fxp_trunc_pr", "hb_fxp_ltl_leaves", "hb_fxp_carry_mask", "hb_fxp_carry_combine", "hb_fxp_div2m_finish", "hb_selftest_fxp"):
        assert re.search(r"\bint " + name + r"\s*\(", text) and name in _capi.SYMBOLS
    for name, value in (("HB_FXP_MOD", 0), ("HB_FXP_TRUNC", 1), ("HB_FXP_NEG_TRUNC", 2), ("HB_FXP_SELFTEST_MASK", 0), ("HB_FXP_SELFTEST_TRUNC_PR", 1),
                        ("HB_FXP_SELFTEST_LEAVES", 2), ("HB_FXP_SELFTEST_CARRY_MASK", 3), ("HB_FXP_SELFTEST_CARRY_COMBINE", 4), ("HB_FXP_SELFTEST_FINISH", 5)):
        assert re.search(r"#define " + name + r" " + str(value) + r"\b", text) and getattr(_capi, name) == value
    assert "progs/fixedpoint.py" in text


def test_selftest_rejects_bad_arguments():
    v = [1, 2, 3]
    for p, nl in ((BLS, 4), (P64, 1)):
        k, m, kappa = (64, 32, 32) if nl == 4 else (16, 8, 16)
        bits = [1] * ((k + kappa) * 3)
        inv = [pow(2, -m, p)]
        assert run(p, nl, MASK, [v, bits], [k, m, kappa], [1, 1], 3)[0] == 0
        assert run(p, nl, MASK, [v, bits], [k, k, kappa], [1, 1], 3)[0] == 2                     # m >= k
        assert run(p, nl, MASK, [v, bits], [k, 0, kappa], [1, 1], 3)[0] == 2
        assert run(p, nl, MASK, [v, bits], [k, m, p.bit_length() - 1 - k], [1, 1], 3)[0] == 2    # k + kappa + 1 = bits(p): would wrap
        assert run(p, nl, MASK, [v, bits], [k, m, -1], [1, 1], 3)[0] == 2
        assert run(p, nl, MASK, [v, None], [k, m, kappa], [1, 1], 3)[0] == 2
        assert run(p, nl, MASK, [v, bits], [k, m, kappa], [1, None], 3)[0] == 2
        assert run(p, nl, MASK, [v, bits], [k, m, kappa], [1, 1], -1)[0] == 2
        assert run(p, nl, MASK, [[], []], [k, m, kappa], [1, 1], 0)[0] == 0
        assert run(p, nl, TRUNC_PR, [v, v, v, inv], [0, m], [1], 3)[0] == 0
        assert run(p, nl, TRUNC_PR, [v, v, v, None], [0, m], [1], 3)[0] == 2
        assert run(p, nl, TRUNC_PR, [v, None, v, inv], [0, m], [1], 3)[0] == 2
        assert run(p, nl, TRUNC_PR, [v, v, v, inv], [0, p.bit_length() - 1], [1], 3)[0] == 2
        assert run(p, nl, LEAVES, [v, bits], [0, 0], [1, 1], 3)[0] == 2
        assert run(p, nl, CARRY_MASK, [bits, bits, bits, bits], [0, 0, 0, 1, 0], [2], 3)[0] == 2     # fewer than two planes
        assert run(p, nl, CARRY_MASK, [bits, bits, bits, bits], [0, 0, 0, 3, 1], [2], 3)[0] == 2     # a root of three
        assert run(p, nl, CARRY_COMBINE, [bits, bits, bits, bits, bits, None], [0, 0, 0, 2, 1], [1, None], 3)[0] == 2
        assert run(p, nl, FINISH, [v, v, v, v, inv], [0, m, 0, 3], [1], 3)[0] == 2                   # unknown mode
        assert run(p, nl, FINISH, [None, v, v, v, inv], [0, m, 0, fx.TRUNC], [1], 3)[0] == 2         # x is needed
        assert run(p, nl, FINISH, [None, v, v, v, None], [0, m, 0, fx.MOD], [1], 3)[0] == 0
        assert run(p, nl, 6, [v, v], [k, m, kappa], [1, 1], 3)[0] == 2
    assert run(P64, 2, MASK, [v, [1] * 96], [16, 8, 16], [1, 1], 3)[0] == 2                           # neither 1 nor 4 limbs

"""CPU-only: honeybadgermpc_amd.progs.bit_decomposition -- the wiring model against the counts of DESIGN.md section 3s, the prefix
network evaluated on Python ints from that model alone, bits_model, and the per-element bodies of csrc/hb_bd.hip run on the host
through hb_selftest_bd -- the same HB_HD functions the kernels call -- against Python ints: body by body on arbitrary residues, chained
on cleartext values at the corners of c and r, and chained on dealt Shamir shares.  Exact equality; the result does not depend on
the masks."""
import asyncio
import os
import random
import re

import pytest

import bitdec_cases as bc
from bitdec_cases import LEAVES, PREFIX_COMBINE, PREFIX_MASK, SUM_COMBINE, SUM_MASK, flat, run_bd
from conftest import BLS, REPO

from honeybadgermpc_amd.progs import bit_decomposition as bd
from honeybadgermpc_amd.progs import fixedpoint as fx

MS = list(range(1, 41)) + [63, 64, 65, 128, 129, 253]


# ---- the wiring ----------------------------------------------------------------------------------------------------------------
def test_counts_reproduce_the_table():
    for m, levels, per_level, prefix, total, opens in bc.TABLE:
        assert bd.prefix_levels(m) == levels, m
        assert [bd.prefix_level_triples(m, l) for l in range(levels)] == per_level, m
        assert [sum(1 if g_only else 2 for _, _, g_only in bd.prefix_nodes(m - 1, l)) for l in range(levels)] == per_level, m
        assert bd.prefix_triples(m) == prefix and bd.bit_triples(m) == total == prefix + m - 1 and bd.bit_opens(m) == opens, m
    assert bd.prefix_nodes(7, 1) == [(2, 1, True), (3, 1, True), (6, 5, False)]
    assert bd.prefix_nodes(7, 2) == [(4, 3, True), (5, 3, True), (6, 3, True)]
    assert bd.prefix_nodes(1, 0) == [] and bd.prefix_nodes(0, 0) == []
    for call in (lambda: bd.prefix_levels(0), lambda: bd.prefix_levels(2.0), lambda: bd.prefix_level_triples(5, 2), lambda: bd.prefix_level_triples(5, -1),
                 lambda: bd.prefix_level_triples(2, 0), lambda: bd.prefix_nodes(-1, 0), lambda: bd.bit_triples(0), lambda: bd.bit_triples(True)):
        with pytest.raises(ValueError):
            call()


@pytest.mark.parametrize("m", MS)
def test_network_on_cleartext_ints(m):
    """the network gives (c2 - r) mod 2^m; no partner is written in its own level; every g-only node's partner has p = 0 (asserted
    inside network_on_ints); the row numbering is a bijection onto range(level triples)"""
    rnd = random.Random(m)
    top = (1 << m) - 1
    pairs = [(0, 0), (0, top), (top, 0), (top, top), (5 & top, 5 & top), (5 & top, 6 & top), (1, 0), (0, 1)] + [(rnd.getrandbits(m), rnd.getrandbits(m)) for _ in range(12)]
    for c2, r in pairs:
        want = bd.difference_bits_model(c2 + (rnd.getrandbits(9) << m), r, m)
        assert want == [((c2 - r) % (1 << m) >> i) & 1 for i in range(m)]
        assert bc.network_on_ints(bd, c2, r, m) == want, (m, c2, r)
    n = m - 1
    for level in range(bd.prefix_levels(m)):
        nodes, rows = bd.prefix_nodes(n, level), bc.triple_rows(bd, n, level)
        assert [j for j, _, _ in nodes] == sorted(j for j in range(n) if (j >> level) & 1)
        assert all(q == ((j >> level) << level) - 1 and not (q >> level) & 1 for j, q, _ in nodes)
        assert [g_only for _, _, g_only in nodes] == [y < (1 << level) for y in range(len(nodes))]
        used = [r for pair in rows for r in pair if r is not None]
        assert sorted(used) == list(range(bd.prefix_level_triples(m, level))), (m, level)
    assert bd.prefix_levels(m) == (0 if n <= 1 else (n - 1).bit_length())


def test_bits_model():
    for p, k, m in ((BLS, 64, 32), (BLS, 64, 63), (BLS, 9, 8), (bc.P64, 16, 6), (bc.GOLDILOCKS, 32, 17), (bc.P256, 222, 200)):
        top = 1 << (k - 1)
        for x in (0, 1, -1, top - 1, -top, (1 << m) - 1, 1 << m, -(1 << m), 12345 % top, -(12345 % top)):
            if not -top <= x < top:
                continue
            got = bd.bits_model(x % p, p, k, m)
            assert got == [(x >> i) & 1 for i in range(m)] and sum(b << i for i, b in enumerate(got)) == x % (1 << m), (k, m, x)
        assert bd.bits_model(-1 % p, p, k, m) == [1] * m and bd.bits_model(-(1 << m) % p, p, k, m) == [0] * m
        # whatever masks are dealt: the opened c's low bits minus r1
        rnd = random.Random(k)
        for x in (0, -1, top - 1, -top, rnd.randrange(-top, top)):
            r1, r2 = rnd.getrandbits(m), rnd.getrandbits(k + 8 - m)
            c = fx.masked_model(x % p, r1, r2, p, k, m)
            assert bd.difference_bits_model(c, r1, m) == bd.bits_model(x % p, p, k, m)
    for call in (lambda: bd.bits_model(1, BLS, 8, 8), lambda: bd.bits_model(1, BLS, 8, 0), lambda: bd.bits_model(1 << 20, BLS, 8, 4), lambda: bd.difference_bits_model(1, 0, 0)):
        with pytest.raises(ValueError):
            call()


# ---- the kernels' bodies -----------------------------------------------------------------------------------------------------
def draw(rnd, p, n):
    return [rnd.choice([0, 1, p - 1, rnd.randrange(p), rnd.randrange(p)]) for _ in range(n)]


def ms_for(p):
    top = p.bit_length() - 2
    return [m for m in (1, 2, 3, 4, 5, 6, 8, 9, 17, 29, 33, 34, 62, 64, 65, 129, 253) if m <= top]


@pytest.mark.parametrize("p, nl", bc.HOST_FIELDS, ids=bc.HOST_FIELD_IDS)
def test_each_body_on_arbitrary_residues(p, nl):
    """the planes hold SHARES: any residues in every slot, corners of c in front"""
    rnd = random.Random(p % 1000 + 11)
    count = 6
    for m in ms_for(p):
        n = m - 1
        cs = ([0, (1 << m) - 1, (1 << m) % p, p - 1] + draw(rnd, p, count))[:count]
        planes = [draw(rnd, p, count) for _ in range(m)]
        if m == 5:
            planes = [[p - 1] * count for _ in range(m)]
        rc, (g, q) = run_bd(p, nl, LEAVES, [cs, flat(planes[:n])], [m], [n, n], count)
        assert rc == 0
        for i in range(n):
            for e in range(count):
                gg, qq = bc.leaf((cs[e] >> i) & 1, planes[i][e], p)
                want = ((gg + qq) % p, 0) if i == 0 else (gg, qq)
                assert (g[i * count + e], q[i * count + e]) == want, (m, i, e)
        # the levels over planes of any residues
        g, q = ([draw(rnd, p, count) for _ in range(n)] for _ in range(2))
        for level in range(bd.prefix_levels(m)):
            nodes, rows = bd.prefix_nodes(n, level), bc.triple_rows(bd, n, level)
            triples = bd.prefix_level_triples(m, level)
            ta, tb, tab = ([draw(rnd, p, count) for _ in range(triples)] for _ in range(3))
            rc, (masked,) = run_bd(p, nl, PREFIX_MASK, [flat(g), flat(q), flat(ta), flat(tb)], [m, level], [2 * triples], count)
            assert rc == 0
            want = [None] * (2 * triples)
            for (j, part, g_only), (r0, r1) in zip(nodes, rows):
                want[2 * r0] = [(q[j][e] - ta[r0][e]) % p for e in range(count)]
                want[2 * r0 + 1] = [(g[part][e] - tb[r0][e]) % p for e in range(count)]
                if not g_only:
                    want[2 * r1] = [(q[j][e] - ta[r1][e]) % p for e in range(count)]
                    want[2 * r1 + 1] = [(q[part][e] - tb[r1][e]) % p for e in range(count)]
            assert masked == flat(want), (m, level)
            opened = [draw(rnd, p, count) for _ in range(2 * triples)]
            rc, (g2, q2) = run_bd(p, nl, PREFIX_COMBINE, [flat(opened), flat(ta), flat(tb), flat(tab)], [m, level], [flat(g), flat(q)], count)
            assert rc == 0
            wg, wq = [list(r) for r in g], [list(r) for r in q]
            for (j, part, g_only), (r0, r1) in zip(nodes, rows):
                for e in range(count):
                    wg[j][e] = (g[j][e] + bc.beaver(opened[2 * r0][e], opened[2 * r0 + 1][e], ta[r0][e], tb[r0][e], tab[r0][e], p)) % p
                    if not g_only:
                        wq[j][e] = bc.beaver(opened[2 * r1][e], opened[2 * r1 + 1][e], ta[r1][e], tb[r1][e], tab[r1][e], p)
            assert g2 == flat(wg) and q2 == flat(wq), (m, level)          # and every plane that is no node is as it was
            g, q = wg, wq
        # the sum step
        carries = [draw(rnd, p, count) for _ in range(n)]
        ta, tb, tab = ([draw(rnd, p, count) for _ in range(n)] for _ in range(3))
        opened = [draw(rnd, p, count) for _ in range(2 * n)]
        leaf_p = [[bc.leaf((cs[e] >> i) & 1, planes[i][e], p)[1] for e in range(count)] for i in range(m)]
        if n:
            rc, (masked,) = run_bd(p, nl, SUM_MASK, [cs, flat(planes), flat(carries), flat(ta), flat(tb)], [m], [2 * n], count)
            assert rc == 0
            want = []
            for t in range(n):
                want += [(leaf_p[t + 1][e] - ta[t][e]) % p for e in range(count)] + [(carries[t][e] - tb[t][e]) % p for e in range(count)]
            assert masked == want, m
        ops = [flat(opened), cs, flat(planes), flat(carries), flat(ta), flat(tb), flat(tab)] if n else [None, cs, flat(planes), None, None, None, None]
        rc, (out,) = run_bd(p, nl, SUM_COMBINE, ops, [m], [m], count)
        assert rc == 0
        for e in range(count):
            b0 = planes[0][e]
            assert out[e] == ((1 - b0) % p if cs[e] & 1 else b0), (m, e)
            for i in range(1, m):
                t = i - 1
                prod = bc.beaver(opened[2 * t][e], opened[2 * t + 1][e], ta[t][e], tb[t][e], tab[t][e], p)
                assert out[i * count + e] == (leaf_p[i][e] + carries[t][e] - 2 * prod) % p, (m, i, e)


@pytest.mark.parametrize("p, nl", bc.HOST_FIELDS, ids=bc.HOST_FIELD_IDS)
def test_chained_bodies_on_cleartext_values(p, nl):
    """degree-0 "shares": what a step opens is what its mask wrote.  c in {0, 2^m - 1, 2^m, p - 1}, r all zeros, all ones (the borrow
    runs through every plane) and r = c2, and random pairs"""
    rnd = random.Random(p % 1000 + 13)
    for m in ms_for(p):
        top = (1 << m) - 1
        cs, rs = [], []
        for c in (0, top, (1 << m) % p, p - 1):
            for r in (0, top, c % (1 << m)):
                cs.append(c), rs.append(r)
        for _ in range(8):
            cs.append(rnd.randrange(p)), rs.append(rnd.getrandbits(m))
        count = len(cs)
        planes = [(r >> i) & 1 for i in range(m) for r in rs]
        out = bc.bodies_chain(bd, p, nl, cs, planes, m, count, rnd)
        for e in range(count):
            assert [out[i * count + e] for i in range(m)] == bd.difference_bits_model(cs[e], rs[e], m), (m, cs[e], rs[e])


@pytest.mark.parametrize("p, nl, k, m, kappa", [(BLS, 4, 64, 33, 32), (BLS, 4, 65, 64, 32), (BLS, 4, 16, 9, 8), (BLS, 4, 8, 1, 8), (BLS, 4, 8, 2, 8),
                                                (bc.P256, 4, 128, 65, 32), (bc.P64, 1, 32, 17, 16), (bc.GOLDILOCKS, 1, 16, 6, 8)])
def test_chained_bodies_on_dealt_shares(p, nl, k, m, kappa):
    """n = 4, t = 1: every party runs the bodies on its own shares, each step's array is reconstructed, and the planes reconstruct to
    bits_model"""
    n_parties, t = 4, 1
    rnd = random.Random(1000 * k + m)
    top = 1 << (k - 1)
    xs = [x for x in (0, 1, -1, top - 1, -top, (1 << m) - 1, 1 << m) if -top <= x < top] + [rnd.randrange(-top, top) for _ in range(3)]
    count = len(xs)
    bit_rows = [[rnd.getrandbits(1) for _ in range(count)] for _ in range(k + kappa)]
    for i in range(m):
        bit_rows[i][0] = 1                                       # an all-ones r1 under x = 0
    x_sh = bc.deal(rnd, p, n_parties, t, [x % p for x in xs])
    b_sh = bc.deal(rnd, p, n_parties, t, flat(bit_rows))
    masked = [bc.run_fxp_mask(p, nl, x_sh[i], b_sh[i], k, m, kappa, count)[0] for i in range(n_parties)]
    c = bc.reconstruct(p, t, masked)
    assert c == [(x + top + sum(bit_rows[i][e] << i for i in range(k + kappa))) % p for e, x in enumerate(xs)]

    # the parties move in lock step: each step is run for all of them before its array is opened
    need = bd.bit_triples(m)
    ta, tb = ([rnd.randrange(p) for _ in range(need * count)] for _ in range(2))
    tr_sh = [bc.deal(rnd, p, n_parties, t, v) for v in (ta, tb, [a * b % p for a, b in zip(ta, tb)])]
    nn = m - 1
    state = []
    for i in range(n_parties):
        rc, (g, q) = run_bd(p, nl, LEAVES, [c, b_sh[i][:nn * count]], [m], [nn, nn], count)
        assert rc == 0
        state.append([g, q])
    off = 0

    def rows(i, lo, hi):
        return [tr_sh[v][i][lo * count:hi * count] for v in range(3)]

    for level in range(bd.prefix_levels(m)):
        tr = bd.prefix_level_triples(m, level)
        sent = []
        for i in range(n_parties):
            a, b, _ = rows(i, off, off + tr)
            rc, (mk,) = run_bd(p, nl, PREFIX_MASK, [state[i][0], state[i][1], a, b], [m, level], [2 * tr], count)
            assert rc == 0
            sent.append(mk)
        opened = bc.reconstruct(p, t, sent)
        assert opened == bc.reconstruct(p, t, sent, first=2)                                                # any t + 1 parties agree
        for i in range(n_parties):
            a, b, ab = rows(i, off, off + tr)
            rc, (g, q) = run_bd(p, nl, PREFIX_COMBINE, [opened, a, b, ab], [m, level], state[i], count)
            assert rc == 0
            state[i] = [g, q]
        off += tr
    assert off == bd.prefix_triples(m)
    planes = [b_sh[i][:m * count] for i in range(n_parties)]
    if nn:
        sent = []
        for i in range(n_parties):
            a, b, _ = rows(i, off, off + nn)
            rc, (mk,) = run_bd(p, nl, SUM_MASK, [c, planes[i], state[i][0], a, b], [m], [2 * nn], count)
            assert rc == 0
            sent.append(mk)
        opened = bc.reconstruct(p, t, sent)
    outs = []
    for i in range(n_parties):
        a, b, ab = rows(i, off, off + nn)
        ops = [opened, c, planes[i], state[i][0], a, b, ab] if nn else [None, c, planes[i], None, None, None, None]
        rc, (out,) = run_bd(p, nl, SUM_COMBINE, ops, [m], [m], count)
        assert rc == 0
        outs.append(out)
    got = bc.reconstruct(p, t, outs)
    assert got == bc.reconstruct(p, t, outs, first=2)                                                       # parties 3 and 4 hold the same values
    for e, x in enumerate(xs):
        assert [got[i * count + e] for i in range(m)] == bd.bits_model(x % p, p, k, m), (k, m, x)


# ---- the ABI -----------------------------------------------------------------------------------------------------------------
def test_abi_names_in_header_and_ctypes_table():
    from honeybadgermpc_amd import _capi

    text = open(os.path.join(REPO, "include", "hbmpc_hip.h")).read()
    for name in ("hb_bd_leaves", "hb_bd_prefix_mask", "hb_bd_prefix_combine", "hb_bd_sum_mask", "hb_bd_sum_combine", "hb_selftest_bd"):
        assert re.search(r"\bint " + name + r"\s*\(", text) and name in _capi.SYMBOLS
    for name, value in (("HB_BD_SELFTEST_LEAVES", 0), ("HB_BD_SELFTEST_PREFIX_MASK", 1), ("HB_BD_SELFTEST_PREFIX_COMBINE", 2), ("HB_BD_SELFTEST_SUM_MASK", 3),
                        ("HB_BD_SELFTEST_SUM_COMBINE", 4)):
        assert re.search(r"#define " + name + r" " + str(value) + r"\b", text) and getattr(_capi, name) == value
    assert (LEAVES, PREFIX_MASK, PREFIX_COMBINE, SUM_MASK, SUM_COMBINE) == (0, 1, 2, 3, 4)


def test_selftest_rejects_bad_arguments():
    for p, nl in ((BLS, 4), (bc.P64, 1)):
        m, count = 9, 3
        n = m - 1
        v = [1] * (2 * 8 * count)                  # long enough for every operand of every step at m = 9 (level 0: 7 triples)
        top = p.bit_length() - 2
        assert run_bd(p, nl, LEAVES, [v, v], [m], [n, n], count)[0] == 0
        assert run_bd(p, nl, LEAVES, [v, v], [0], [n, n], count)[0] == 2
        assert run_bd(p, nl, LEAVES, [v, v], [top + 1], [n, n], count)[0] == 2                     # m out of range for the modulus
        assert run_bd(p, nl, LEAVES, [v, None], [m], [n, n], count)[0] == 2
        assert run_bd(p, nl, LEAVES, [v, v], [m], [n, None], count)[0] == 2
        assert run_bd(p, nl, LEAVES, [v, v], [m], [n, n], -1)[0] == 2
        assert run_bd(p, nl, LEAVES, [[], []], [m], [n, n], 0)[0] == 0
        assert run_bd(p, nl, LEAVES, [None, None], [1], [None, None], count)[0] == 0               # m = 1: no plane
        assert run_bd(p, nl, PREFIX_MASK, [v, v, v, v], [m, 0], [14], count)[0] == 0
        assert run_bd(p, nl, PREFIX_MASK, [v, v, v, v], [m, 3], [14], count)[0] == 2               # level >= the number of levels
        assert run_bd(p, nl, PREFIX_MASK, [v, v, v, v], [m, -1], [14], count)[0] == 2
        assert run_bd(p, nl, PREFIX_MASK, [v, v, v, v], [2, 0], [14], count)[0] == 2               # m = 2 has no level
        assert run_bd(p, nl, PREFIX_MASK, [v, v, None, v], [m, 0], [14], count)[0] == 2
        assert run_bd(p, nl, PREFIX_COMBINE, [v, v, v, v], [m, 2], [v[:n * count], v[:n * count]], count)[0] == 0
        assert run_bd(p, nl, PREFIX_COMBINE, [v, v, v, v], [m, 3], [v[:n * count], v[:n * count]], count)[0] == 2
        assert run_bd(p, nl, PREFIX_COMBINE, [v, v, v, None], [m, 2], [v[:n * count], v[:n * count]], count)[0] == 2
        assert run_bd(p, nl, PREFIX_COMBINE, [v, v, v, v], [m, 2], [v[:n * count], None], count)[0] == 2
        assert run_bd(p, nl, SUM_MASK, [v, v, v, v, v], [m], [2 * n], count)[0] == 0
        assert run_bd(p, nl, SUM_MASK, [v, v, None, v, v], [m], [2 * n], count)[0] == 2
        assert run_bd(p, nl, SUM_MASK, [v, v, v, v, v], [1 << 31], [2 * n], count)[0] == 2
        assert run_bd(p, nl, SUM_COMBINE, [v, v, v, v, v, v, v], [m], [m], count)[0] == 0
        assert run_bd(p, nl, SUM_COMBINE, [v, v, v, v, v, v, None], [m], [m], count)[0] == 2
        assert run_bd(p, nl, SUM_COMBINE, [v, v, v, v, v, v, v], [m], [None], count)[0] == 2
        assert run_bd(p, nl, SUM_COMBINE, [None, v, None, None, None, None, None], [1], [1], count)[0] == 2   # m = 1 still reads bits
        assert run_bd(p, nl, 5, [v, v], [m], [n, n], count)[0] == 2
        assert run_bd(p, nl, -1, [v, v], [m], [n, n], count)[0] == 2
    assert run_bd(bc.P64, 2, LEAVES, [[1] * 30, [1] * 30], [9], [8, 8], 3)[0] == 2                  # neither 1 nor 4 limbs


# ---- the coroutines' checks come before anything is opened -------------------------------------------------------------------
def test_coroutines_refuse_before_anything_is_opened_or_called_in_c():
    """a context over CPU tensors whose library refuses every call, and a coalescer that counts: short bits, short triples and bad
    (k, m, kappa) raise ValueError with co.batches unchanged"""
    import torch

    class NoLib:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was called")

    class Ctx:
        modulus, n_limbs, lib, torch = BLS, 4, NoLib(), None

        def elems(self, t, count=None, what="tensor"):
            if not isinstance(t, torch.Tensor):
                raise TypeError(what)
            if t.dim() < 1 or t.shape[-1] != self.n_limbs or (count is not None and t.numel() != count * self.n_limbs):
                raise ValueError(what)
            return t.contiguous()

        def empty(self, count):
            return torch.zeros((count, self.n_limbs), dtype=torch.int64)

        def check(self, rc, what):
            raise AssertionError(f"{what} returned")

    class Co:
        ctx, batches = Ctx(), 0

        async def open_share_array(self, shares):
            self.batches += 1
            raise AssertionError("something was opened")

    Ctx.torch = torch
    co = Co()
    count, k, m, kappa = 5, 16, 9, 8
    z = lambda *shape: torch.zeros(shape + (4,), dtype=torch.int64)           # noqa: E731
    x, bits = z(count), z(k + kappa, count)
    need = bd.bit_triples(m)
    tr = tuple(z(need, count) for _ in range(3))
    short_tr = tuple(v[:need - 1] for v in tr)
    calls = [
        lambda: bd.bit_decompose(co, x, bits[:k + kappa - 1], tr, k, m, kappa),                    # short bits
        lambda: bd.bit_decompose(co, x, bits, short_tr, k, m, kappa),                              # short triples
        lambda: bd.bit_decompose(co, x, bits, (tr[0], tr[1]), k, m, kappa),
        lambda: bd.bit_decompose(co, x, bits, (tr[0], tr[1], tr[2][:, :3]), k, m, kappa),
        lambda: bd.bit_decompose(co, x, bits[:, :3], tr, k, m, kappa),
        lambda: bd.bit_decompose(co, x[:2], bits, tr, k, m, kappa),
        lambda: bd.bit_decompose(co, x, bits, tr, k, k, kappa),                                    # m > k - 1
        lambda: bd.bit_decompose(co, x, bits, tr, k, 0, kappa),
        lambda: bd.bit_decompose(co, x, bits, tr, 250, m, kappa),                                  # would wrap
        lambda: bd.bit_decompose(co, x, bits, tr, k, m, -1),
        lambda: bd.bit_decompose(co, x, bits, tr, k, 2.0, kappa),
        lambda: bd.difference_bits(co, x, bits[:m], short_tr),
        lambda: bd.difference_bits(co, x, bits[:m, :3], tr),
        lambda: bd.difference_bits(co, x, bits[:0], tr),
        lambda: bd.difference_bits(co, x, bits.reshape(-1, 4), tr),
        lambda: bd.difference_bits(co, x, z(254, count), tuple(z(1, count) for _ in range(3))),   # m out of range for the modulus
        lambda: fx.FixedPointArray(co, x, 4, k, kappa).bits(m, bits[:k + kappa - 1], tr),
        lambda: fx.FixedPointArray(co, x, 4, k, kappa).bits(m, bits, short_tr),
        lambda: fx.FixedPointArray(co, x, 4, k, kappa).bits(k, bits, tr),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(ValueError):
            asyncio.run(call())
            pytest.fail(f"bad call {i} was accepted")
    assert co.batches == 0
    # a good call gets past the checks and reaches the library
    with pytest.raises(AssertionError, match="hb_fxp_mask was called"):
        asyncio.run(bd.bit_decompose(co, x, bits, tr, k, m, kappa))
    assert co.batches == 0

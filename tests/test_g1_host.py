"""CPU-only: the per-item bodies of the G1 kernels (csrc/hb_g1.hip) run on the host through hb_selftest_g1 -- the same HB_HD functions the
kernels call -- against the host model honeybadgermpc_amd.bls12_381, the reference crate's test vectors and Python ints.  Exact equality."""
import random

import numpy as np
import pytest

import fq_cases as fc
import g1_support as s
from g1_support import ADD, CHECK, COMMIT, DOUBLE, EVAL, FQ_MUL, GENERAL, K_BCAST, P_BCAST, SCALAR_MUL, SUBTRACT, TABLE, VERIFY

from honeybadgermpc_amd.bls12_381 import G1, Q, R


def test_fq_products():
    rnd = random.Random(11)
    ones13, ones_top = fc.ONES13, fc.ONES_TOP                # thirteen 29-bit digits of all ones, the top digit 0 or the largest below Q's
    assert ones13 < ones_top < Q
    a = [rnd.randrange(Q) for _ in range(200)] + [Q - 1, 0, ones13, ones_top, ones13, Q - 1, 1]
    b = [rnd.randrange(Q) for _ in range(200)] + [Q - 1, Q - 1, ones13, ones_top, ones_top, ones_top, Q - 1]
    rc, out = s.selftest(FQ_MUL, [s.words(a, 6), s.words(b, 6)], 0, 0, len(a), 6 * len(a))
    assert rc == 0 and s.unwords(out[:6 * len(a)], 6) == [x * y % Q for x, y in zip(a, b)]
    rc, _ = s.selftest(FQ_MUL, [s.words([Q], 6), s.words([1], 6)], 0, 0, 1, 6)
    assert rc != 0                                           # operands are residues below Q


def test_fq_products_over_every_ordered_pair_of_the_edge_pool():
    """fq_mul at fq_cases.fq_edge_pool(): digit and word boundaries, Q - 1, all-ones digits and the Montgomery pre-images of all of them;
    the pairing self test runs the same pairs through the tower's entry (test_pairing_host.py), the device through hb_debug_pair_op"""
    pool = fc.fq_edge_pool()
    w = s.words(pool, 6)
    n = len(pool)
    ia, ib = np.repeat(np.arange(n), n), np.tile(np.arange(n), n)
    rc, out = s.selftest(FQ_MUL, [w[ia], w[ib]], 0, 0, n * n, 6 * n * n)
    assert rc == 0 and s.unwords(out[:6 * n * n], 6) == [x * y % Q for x in pool for y in pool]


@pytest.mark.parametrize("flags", [0, SUBTRACT, GENERAL, GENERAL | SUBTRACT], ids=["mixed", "mixed-sub", "general", "general-sub"])
def test_additions_on_every_exceptional_pair(flags):
    pairs = s.exceptional_pairs()
    rc, out = s.selftest(ADD, [s.points([p for p, _ in pairs]), s.points([q for _, q in pairs])], flags, 0, len(pairs), 12 * len(pairs))
    assert rc == 0
    want = [p / q if flags & SUBTRACT else p * q for p, q in pairs]
    assert s.unpoints(out[:12 * len(pairs)]) == want
    assert want[0].is_one() and want[3 if flags & SUBTRACT else 4].is_one()      # the cases are what they claim to be


def test_doubling():
    ps = [G1.one(), G1.generator(), G1.generator() ** 5, s.off_subgroup_point()]
    rc, out = s.selftest(ADD, [s.points(ps)], DOUBLE, 0, len(ps), 12 * len(ps))
    assert rc == 0 and s.unpoints(out[:12 * len(ps)]) == [p * p for p in ps]


def test_scalar_mul_against_the_vectors():
    vs = s.vectors()
    rc, out = s.selftest(SCALAR_MUL, [s.words(range(1000), 4), s.points([G1.generator()])], P_BCAST, 0, 1000, 12000)
    assert rc == 0 and np.array_equal(out[:12000].reshape(1000, 12), s.points(vs))


def test_scalar_mul_edges_and_broadcasts():
    g = G1.generator()
    ks = s.EDGE_SCALARS
    rc, out = s.selftest(SCALAR_MUL, [s.words(ks, 4), s.points([g])], P_BCAST, 0, len(ks), 12 * len(ks))
    assert rc == 0 and s.unpoints(out[:12 * len(ks)]) == [s.mul_model(k, g) for k in ks]
    assert s.unpoints(out[:12])[0].is_one() and s.unpoints(out[48:60])[0].is_one()          # k = 0 and k = R
    ps = [G1.one(), g, g ** 3, s.vectors()[999]]
    for k in (R - 1, (1 << 256) - 1, 0):
        rc, out = s.selftest(SCALAR_MUL, [s.words([k], 4), s.points(ps)], K_BCAST, 0, len(ps), 12 * len(ps))
        assert rc == 0 and s.unpoints(out[:12 * len(ps)]) == [s.mul_model(k, p) for p in ps]
    ks, ps = s.scalar_mul_case(16, seed=4)
    rc, out = s.selftest(SCALAR_MUL, [s.words(ks, 4), s.points(ps)], 0, 0, 16, 12 * 16)
    assert rc == 0 and s.unpoints(out[:12 * 16]) == [s.mul_model(k, p) for k, p in zip(ks, ps)]
    rc, out = s.selftest(SCALAR_MUL, [s.words([5], 4), s.points([g])], K_BCAST | P_BCAST, 0, 3, 36)
    assert rc == 0 and s.unpoints(out[:36]) == [g ** 5] * 3
    # the order of a point outside the subgroup is not R: R * P is not the identity (g1.in_subgroup's test)
    p = s.off_subgroup_point()
    rc, out = s.selftest(SCALAR_MUL, [s.words([R], 4), s.points([p, g])], K_BCAST, 0, 2, 24)
    assert rc == 0 and out[:12].any() and not out[12:24].any()


def test_check():
    g = G1.generator()
    bad = s.off_curve_raw()
    not_below = s.raw_point(g.x + Q, g.y)                    # the right residue, not canonical
    ps = [G1.one(), g, s.off_subgroup_point(), bad, not_below, s.raw_point(0, 2), s.raw_point(1, 0)]
    rc, out = s.selftest(CHECK, [s.points(ps)], 0, 0, len(ps), len(ps))
    assert rc == 0 and out.view(np.int32)[:len(ps)].tolist() == [1, 1, 1, 0, 0, 1, 0]       # (0, 2): 4 = 0 + 4 is on the curve


def table_entry(tab, c, w, j):
    n = (1 << c) - 1
    at = (w * n + (j - 1)) * 32
    w32 = tab.view(np.uint32)[at:at + 32]
    assert not w32[14:16].any() and not w32[30:32].any()
    rinv = pow(1 << (29 * 14), -1, Q)
    x = sum(int(d) << (29 * k) for k, d in enumerate(w32[:14])) * rinv % Q
    y = sum(int(d) << (29 * k) for k, d in enumerate(w32[16:30])) * rinv % Q
    return G1(x, y)


@pytest.mark.parametrize("c", [4, 8])
def test_table(c):
    g, _ = s.crs()
    tg, _ = s.tables(c)
    n, W = (1 << c) - 1, 256 // c
    base = g
    for w in range(W):
        js = range(1, n + 1) if c == 4 else (1, 2, 3, 128, n - 1, n)
        run, last = G1.one(), 0
        for j in js:
            run, last = run * base ** (j - last), j
            assert table_entry(tg, c, w, j) == run, (w, j)
        base = base ** (1 << c)
    for base_words in (G1.one().to_limbs(), s.off_curve_raw()):
        rc, _ = s.selftest(TABLE, [s.points([base_words])], 0, c, 1, 8)
        assert rc != 0
    rc, _ = s.selftest(TABLE, [s.points([g])], 0, 5, 1, 8)
    assert rc != 0


@pytest.mark.parametrize("c", [4, 8])
def test_commit(c):
    g, h = s.crs()
    tg, th = s.tables(c)
    a, b = s.commit_case(40, c, seed=c)
    rc, out = s.selftest(COMMIT, [s.words(a, 4), s.words(b, 4), tg, th], 0, c, len(a), 12 * len(a))
    assert rc == 0 and s.unpoints(out[:12 * len(a)]) == [s.mul_model(x, g) * s.mul_model(y, h) for x, y in zip(a, b)]


@pytest.mark.parametrize("c", [4, 8])
def test_commit_meets_equal_operands_inside_the_comb(c):
    """h = 2^c g: the table of h is g's moved up a window, so b's digit d in window w and a's digit d in window w + 1 add the SAME
    point: midway the accumulator (b h so far) equals the entry being added (a's digit times g) and the mixed addition must take its
    doubling branch.  For the first pair a g = b h as a whole."""
    g, _ = s.crs()
    hs = g ** (1 << c)
    tg, th = s.tables(c, "shift")
    d = (1 << c) - 1
    a = [5 << c, d << c, (3 << c) | (7 << (2 * c)), 1 << c, 0]
    b = [5, d, 3 | (7 << c), 1, 1]
    rc, out = s.selftest(COMMIT, [s.words(a, 4), s.words(b, 4), tg, th], 0, c, len(a), 12 * len(a))
    assert rc == 0 and s.unpoints(out[:12 * len(a)]) == [g ** x * hs ** y for x, y in zip(a, b)]
    assert g ** a[0] == hs ** b[0]


@pytest.mark.parametrize("n_coef", [1, 2, 3, 22])
def test_eval(n_coef):
    B = 7
    cs = s.eval_case(B, n_coef, seed=n_coef)
    for i in s.INDICES:
        rc, out = s.selftest(EVAL, [s.flat_points(cs)], n_coef, i, B, 12 * B)
        assert rc == 0 and s.unpoints(out[:12 * B]) == [s.eval_model(row, i) for row in cs], i
    rc, _ = s.selftest(EVAL, [s.flat_points(cs)], n_coef, 1 << 32, B, 12 * B)
    assert rc != 0


def test_eval_exceptional_steps_at_index_one():
    """at i = 1 Horner's first step adds C_t to C_(t-1): equal entries make it a doubling, C_1 = -C_0 makes it the identity"""
    v = s.vectors()
    rows = [[v[4], v[4]], [v[4], v[4].invert()], [v[4]] * 5, [G1.one(), v[4]], [v[4], G1.one()]]
    want = [v[8], G1.one(), v[20], v[4], v[4]]
    for row, w in zip(rows, want):
        rc, out = s.selftest(EVAL, [s.points(row)], len(row), 1, 1, 12)
        assert rc == 0 and s.unpoints(out[:12]) == [w]


def run_verify(cs, shares, wits, c, i, tabs=None):
    tg, th = tabs or s.tables(c)
    B, n_coef = len(cs), len(cs[0])
    rc, out = s.selftest(VERIFY, [s.flat_points(cs), s.words(shares, 4), s.words(wits, 4), tg, th], n_coef | (c << 16), i, B, (B + 2) // 2 + 1)
    assert rc == 0
    v = out.view(np.int32)
    return v[:B].tolist(), int(v[B])


@pytest.mark.parametrize("c", [4, 8])
@pytest.mark.parametrize("t,i", [(1, 1), (2, 3), (2, 64), (5, 0), (21, 64)])
def test_verify_accepts_honest_items(c, t, i):
    cs, shares, wits, want = s.verify_case(5, t, i, seed=t)
    assert run_verify(cs, shares, wits, c, i) == (want, 0) and want == [1] * 5


@pytest.mark.parametrize("kind", ["share", "witness", "swap", "off"])
@pytest.mark.parametrize("pos", [0, 3, 5])
def test_verify_rejects_exactly_the_changed_item(kind, pos):
    cs, shares, wits, want = s.verify_case(6, 2, 3, bad=[(pos, kind)], seed=1)
    assert run_verify(cs, shares, wits, 8, 3) == (want, 1) and want.count(0) == 1 and want[pos] == 0


def test_verify_counts_every_rejected_item():
    bad = [(0, "share"), (2, "off"), (3, "swap"), (5, "witness")]
    cs, shares, wits, want = s.verify_case(6, 3, 2, bad=bad, seed=2)
    assert run_verify(cs, shares, wits, 4, 2) == (want, 4)


def test_selftest_argument_errors():
    g = s.points([G1.generator()])
    assert s.selftest(99, [g], 0, 0, 1, 12)[0] != 0
    assert s.selftest(SCALAR_MUL, [s.words([1], 4), g], 4, 0, 1, 12)[0] != 0
    assert s.selftest(COMMIT, [s.words([1], 4), s.words([1], 4), g, g], 0, 3, 1, 12)[0] != 0
    assert s.selftest(EVAL, [g], 0, 1, 1, 12)[0] != 0


def test_no_cpu_path():
    """without a GPU the commitment scheme refuses to compute, like the rest of the package; constructing it needs no device"""
    import torch

    from honeybadgermpc_amd._capi import HbmpcBackendError
    from honeybadgermpc_amd.field import GF
    from honeybadgermpc_amd.poly_commit_lin import PolyCommitLin
    from honeybadgermpc_amd.polynomial import polynomials_over

    pc = PolyCommitLin(list(s.crs()))
    assert pc.field is GF(R) and pc.create_witness(lambda i: i + 1, 4) == 5
    with pytest.raises(TypeError):
        PolyCommitLin([G1.generator(), 7])
    with pytest.raises(ValueError):
        PolyCommitLin(list(s.crs()), field=GF(13))
    if torch.cuda.is_available():
        return
    phi = polynomials_over(GF(R))([1, 2, 3])
    for call in (lambda: pc.commit(phi), lambda: pc.preprocess(8), lambda: pc.verify_eval([G1.generator()], 1, 1, 1),
                 lambda: pc.batch_verify_eval([[G1.generator()]], 1, [1], [1])):
        with pytest.raises(HbmpcBackendError):
            call()

"""CPU-only: hb_selftest_g1_crs runs the bodies of csrc/hb_crs.hip (the table of a base, the synthetic division in GF(R), a lane's units of
the fixed-base sum, the tree step -- the same HB_HD functions the kernels call) over host memory, the split path lane by lane with an
array in place of LDS, against the Python-int model of g1_crs_support.  Exact equality of words: affine canonical output is unique, so
every split and both window widths give the same words.

Reference parity: the reference's poly_commit_const.py needs its pairing extension, which cannot be imported where this suite is built;
a CRS with a known trapdoor stands in for it (g1_crs_support)."""
import numpy as np
import pytest

import g1_crs_support as cs
import g1_support as s

from honeybadgermpc_amd.bls12_381 import G1, R


# ---------------------------------------------------------------- the quotient
@pytest.mark.parametrize("t", [0, 1, 2, 21])
def test_quotient_against_the_model(t):
    phis, xs = cs.quotient_case(t)
    q, rem = cs.host_quotient(phis, xs)
    for b, phi in enumerate(phis):
        for i, x in enumerate(xs):
            wq, wr = cs.quotient_model(phi, x)
            assert q[b][i] == wq and rem[b][i] == wr, (t, b, i)
            assert wr == cs.poly_at(phi, x)
            # phi(X) - rem == (X - x) q(X), coefficient by coefficient
            prod = [0] * (t + 1)
            for j, c in enumerate(wq):
                prod[j + 1] = (prod[j + 1] + c) % R
                prod[j] = (prod[j] - x * c) % R
            assert prod == [(phi[0] - wr) % R] + phi[1:]


def test_quotient_counts_and_bad_arguments():
    rc, _ = cs.selftest(cs.QUOTIENT, [s.words([1, 2], 4), s.words([3], 4)], 2, 0, 1, 8)       # no points
    assert rc == 0
    rc, _ = cs.selftest(cs.QUOTIENT, [s.words([1, 2], 4), s.words([3], 4)], 2, 1, 0, 8)       # no polynomials
    assert rc == 0
    for flags, arg, count in ((0, 1, 1), (2, -1, 1), (2, 1, -1)):
        rc, _ = cs.selftest(cs.QUOTIENT, [s.words([1, 2], 4), s.words([3], 4)], flags, arg, count, 8)
        assert rc != 0, (flags, arg, count)
    rc, _ = cs.selftest(cs.QUOTIENT, [None, s.words([3], 4)], 2, 1, 1, 8)
    assert rc != 0


# ---------------------------------------------------------------- the tables
@pytest.mark.parametrize("c", [4, 8])
def test_table_k_is_the_single_base_table(c):
    gs, _ = cs.crs_points(3)
    tg, _ = cs.host_tables(3, c)
    tw = cs.table_words(c)
    assert tg.shape == (3 * tw,)
    for k in range(3):
        assert np.array_equal(tg[k * tw:(k + 1) * tw], s.host_table(gs[k], c)[:tw]), (c, k)


def test_table_refusals():
    g = G1.generator()
    tw = cs.table_words(4)
    for bases in ([g, G1.one(), g], [g, s.off_curve_raw()]):
        rc, _ = cs.selftest(cs.TABLE, [s.points(bases)], 0, 4, len(bases), len(bases) * tw)
        assert rc != 0
    for c in (0, 5, 16):
        rc, _ = cs.selftest(cs.TABLE, [s.points([g])], 0, c, 1, tw)
        assert rc != 0
    rc, _ = cs.selftest(cs.TABLE, [s.points([g])], 0, 4, 0, tw)
    assert rc == 0


# ---------------------------------------------------------------- the fixed-base sum
@pytest.mark.parametrize("split", cs.SPLITS)
@pytest.mark.parametrize("name", sorted(cs.msm_cases()))
def test_crs_msm_against_the_model(name, split):
    case = cs.msm_cases()[name]
    want = cs.model_msm(case)
    assert np.array_equal(cs.host_msm(case, split), want), (name, split)
    if name == "a == b over h = -g":
        assert not want.any()


def test_units_not_divisible_by_the_split_and_the_rule():
    case = cs.msm_cases()["two families, edge scalars"]          # U = 2 * 3 * 32 = 192
    want = cs.model_msm(case)
    for split in (128, 0, 4, 16):
        assert np.array_equal(cs.host_msm(case, split), want), split


def test_both_windows_give_the_same_words():
    a = cs.msm_cases()["two families, edge scalars"]
    b = dict(a, c=4)
    assert np.array_equal(cs.host_msm(a, 1), cs.host_msm(b, 64))


def test_commitment_and_witness_pass_the_trapdoor_checks():
    """the whole prover on the host: quotients, then the sum over gs[:t], hs[:t]; t = 2, n = 3"""
    t, xs = 2, [1, 2, 3]
    phis, _ = cs.quotient_case(t, B=4, seed=5)
    hats, _ = cs.quotient_case(t, B=4, seed=6)
    hats = hats[::-1]
    base = dict(name="prover", n=t + 1, c=8, alpha=cs.ALPHA, lam=cs.LAM)
    commits = s.unpoints(cs.host_msm(dict(base, terms=t + 1, a=phis, b=hats), 1))
    assert commits == [cs.commitment_model(p, h) for p, h in zip(phis, hats)]
    q, share = cs.host_quotient(phis, xs)
    qh, aux = cs.host_quotient(hats, xs)
    rows_a = [q[b][i] for b in range(4) for i in range(3)]
    rows_b = [qh[b][i] for b in range(4) for i in range(3)]
    wit = s.unpoints(cs.host_msm(dict(base, terms=t, a=rows_a, b=rows_b), 2))
    for b in range(4):
        for i, x in enumerate(xs):
            assert cs.witness_holds(commits[b], share[b][i], aux[b][i], wit[b * 3 + i], x), (b, i)
            assert not cs.witness_holds(commits[b], (share[b][i] + 1) % R, aux[b][i], wit[b * 3 + i], x)


def test_msm_counts_and_bad_arguments():
    case = cs.msm_cases()["one family"]
    tg, th = cs.host_tables(3, 8)
    a = s.words([v for row in case["a"] for v in row], 4)
    ok = lambda flags, arg, ops=None, count=3: cs.selftest(cs.MSM, ops or [tg, None, a, None], flags, arg, count, 36)[0]
    assert ok(8, 3 | 3 << 32) == 0
    assert ok(8, 4 | 3 << 32) != 0                               # terms > n_bases
    for split in (3, 6, 512, 257):
        assert ok(8 | split << 8, 3 | 3 << 32) != 0
    for c in (0, 5, 16):
        assert ok(c, 3 | 3 << 32) != 0
    assert ok(8, 3 | 3 << 32, [tg, th, a, None]) != 0            # half a second family
    assert ok(8, 3 | 3 << 32, [tg, None, a, a]) != 0
    assert ok(8, 3 | 3 << 32, [None, None, a, None]) != 0
    assert ok(8, 3 | 3 << 32, count=-1) != 0
    rc, out = cs.selftest(cs.MSM, [tg, None, a, None], 8, 0 | 3 << 32, 3, 36)            # no terms: identities
    assert rc == 0 and not out[:36].any()
    assert ok(8, 3 | 3 << 32, count=0) == 0

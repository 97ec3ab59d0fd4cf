"""The arithmetic of the matrix-core reductions with the high half of a sum folded on the matrix cores (k_mm8w, k_mm8), as a big-integer
model with every bound the kernels rely on asserted (tests/fold_model.py).  CPU only."""
import random

import pytest

import edge_values
import fold_model


def test_k_mm8w_reduction_model():
    fold_model.run_wide(400)


def test_k_mm8_epilogue_model():
    fold_model.run_mm8(300)


def test_every_t_b_has_32_balanced_digits():
    # t_b = 2^(256 + 8 b) mod p or that minus p: one of the two fits 32 balanced base-256 digits for every p < 2^256
    for p in fold_model.PRIMES + [(1 << 256) - 189, (1 << 254) + 1, (1 << 255) + 12345]:
        s, mu, c512, btot, tsum = fold_model.tables(p)
        assert len(s) == 32 and all(len(d) == 32 and all(-128 <= x <= 127 for x in d) for d in s)
        assert mu < 1 << 32


# ---- sums whose residue is an edge value (tests/edge_values.py) -------------------------------------------------------------
EDGE_PRIMES = fold_model.PRIMES[:4] + [(1 << 256) - 189, (1 << 255) + 95]


# The estimate q falls one short only when the residue v is small: it drops the low 240 bits of R and the fraction of mu, an error below
# 2^-14 in R / p, so v < 2^-14 p there and r = v + p < (1 + 2^-14) p.  That reaches 2^256 (top == 1) only for p above 2^256 / (1 + 2^-14):
# the three moduli next to 2^256 do, 2^255 + 95 cannot.
TOP_FROM = (1 << 256) - (1 << 241)


def _quotients(rng, q_lo, q_hi):
    """small, middle and the largest admissible quotients, and a few in between"""
    qs = {q_lo, q_lo + 1, q_lo + 2, (q_lo + q_hi) // 2, (q_lo + q_hi) // 2 + 1, q_hi - 2, q_hi - 1, q_hi}
    qs |= {rng.randrange(q_lo, q_hi + 1) for _ in range(8)}
    return sorted(q for q in qs if q_lo <= q <= q_hi)


@pytest.mark.parametrize("p", EDGE_PRIMES)
def test_k_mm8w_reduction_model_at_edge_residues(p):
    """S = q p + v - CRorig for every pool value v: the reduction must return v itself -- 0, p - 1, 2^256 - p and the other edges -- on
    both branches of the quotient estimate, and for p > 2^255 with a remainder at or above 2^256 before the last subtraction"""
    rng = random.Random(p % 9973)
    tb = fold_model.tables(p)
    facts = set()
    for v in edge_values.edge_pool(p, 4):
        for cr in (0, p - 1, rng.randrange(p)):
            q_lo = 0 if v >= cr else 1
            q_hi = ((1 << 527) - 1 - v + cr) // p
            for q in _quotients(rng, q_lo, q_hi):
                assert fold_model.reduce_model(q * p + v - cr, cr, p, tb, facts) == v
    assert {"exact", "under"} <= facts
    if p > TOP_FROM:
        assert "top1" in facts


@pytest.mark.parametrize("p", EDGE_PRIMES)
def test_k_mm8_epilogue_model_at_edge_residues(p):
    """the same through k_mm8's epilogue: the sum is laid out as its 47 columns (46 bytes and the rest in the last one)"""
    rng = random.Random(p % 9973 + 1)
    facts = set()
    hi = 2 * 5800000
    for v in edge_values.edge_pool(p, 4):
        for cr in (0, p - 1, rng.randrange(p)):
            q_lo = 0 if v >= cr else 1
            q_hi = ((hi << 368) - 1 - v + cr) // p
            for q in _quotients(rng, q_lo, q_hi):
                S = q * p + v - cr
                cols = [(S >> (8 * i)) & 0xff for i in range(46)] + [S >> 368]
                assert fold_model.mm8_model(cols, cr, p, rng, facts) == v
    assert {"exact", "under"} <= facts
    if p > TOP_FROM:
        assert "top1" in facts

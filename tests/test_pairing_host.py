"""The pairing of BLS12-381 without a GPU: the Python-int model (honeybadgermpc_amd.bls12_381_pairing) against the reference crate's
recorded results (tests/golden/pairing_generators_gt.json: e(G1 generator, G2 generator) of its test_pairing_result_against_relic;
g2_uncompressed_valid_test_vectors_first64.dat: the first 64 vectors of its file of that name, k * G2 generator from the identity on),
the model's own algebra, and hb_selftest_pairing (the bodies of csrc/hb_fq12_elem.hpp and csrc/hb_pair.hip on the host) against the
model.  Every comparison is exact: a value after the final exponentiation is one canonical element.

The model takes some 60 ms a pairing, so this file affords a handful of them; the self test's pairings cost a few milliseconds."""
import functools
import json
import os
import random
import re

import numpy as np
import pytest

import fq_cases as fc
import pairing_support as ps
from conftest import GOLDEN, REPO
from fq_cases import OPS

from honeybadgermpc_amd import _capi
from honeybadgermpc_amd.bls12_381 import G1, Q, R
from honeybadgermpc_amd.bls12_381_pairing import BLS_X, FROBENIUS_FQ12_C1, Fq2, Fq6, Fq12, G2, N_LINES, final_exponentiation, pair, pairing_product, prepare_g2


@functools.lru_cache(maxsize=None)
def e_gen():
    return pair(G1.generator(), G2.generator())


# ---------------------------------------------------------------- the model against the reference's recorded results
def test_model_pairing_of_the_generators_is_the_recorded_value():
    with open(os.path.join(GOLDEN, "pairing_generators_gt.json")) as f:
        want = [int(v) for v in json.load(f)["coords"]]
    assert len(want) == 12
    assert e_gen().coords() == want


def test_model_g2_vectors_round_trip_and_are_multiples_of_the_generator():
    with open(os.path.join(GOLDEN, "g2_uncompressed_valid_test_vectors_first64.dat"), "rb") as f:
        data = f.read()
    assert len(data) == 64 * 192
    acc, g = G2.one(), G2.generator()
    for k in range(64):
        raw = data[192 * k:192 * k + 192]
        p = G2.from_uncompressed(raw)
        assert p == acc and p.on_curve() and p.to_uncompressed() == raw and acc.to_uncompressed() == raw
        assert p.is_one() == (k == 0)
        acc = acc * g
    assert G2.from_uncompressed(data[192 * 37:192 * 38]) == g ** 37
    assert g ** R == G2.one() and (g ** 5) / (g ** 3) == g ** 2 and g.invert() * g == G2.one()


def test_model_g2_encoding_refuses_malformed_input():
    raw = bytearray(G2.generator().to_uncompressed())
    with pytest.raises(ValueError):
        G2.from_uncompressed(bytes(raw[:-1]))
    with pytest.raises(ValueError):
        G2.from_uncompressed(bytes([raw[0] | 0x80]) + bytes(raw[1:]))
    raw[-1] ^= 1
    with pytest.raises(ValueError):
        G2.from_uncompressed(bytes(raw))                       # off the twist
    with pytest.raises(ValueError):
        G2.from_uncompressed(bytes([0x40]) + bytes(190) + b"\x01")


# ---------------------------------------------------------------- the model's own algebra
def test_model_bilinearity_order_and_identities():
    g, h, e = G1.generator(), G2.generator(), e_gen()
    assert not e.is_one() and e.pow(R).is_one()
    for a, b in [(3, 5), (R - 1, 2), (0x1234567, R - 2)]:
        assert pair(g ** a, h ** b) == e.pow(a * b % R)
    assert pair(G1.one(), h).is_one() and pair(g, G2.one()).is_one()
    assert pairing_product([(g ** 6, h), (g.invert(), h ** 6)]).is_one()


def test_model_tower_laws():
    rnd = random.Random(11)
    a, b, c = (Fq12.from_coords([rnd.randrange(Q) for _ in range(12)]) for _ in range(3))
    assert (a * b) * c == a * (b * c) and a * (b + c) == a * b + a * c and a.square() == a * a
    assert (a * a.inverse()).is_one() and a.conjugate().conjugate() == a
    f = a
    for _ in range(12):
        f = f.frobenius_map(1)
    assert f == a and a.frobenius_map(2) == a.frobenius_map(1).frobenius_map(1) and a.frobenius_map(1) == a.pow(Q)
    assert FROBENIUS_FQ12_C1[1] == Fq2(1, 1).pow((Q - 1) // 6)
    sparse = Fq12(Fq6(b.c0.c0, b.c0.c1), Fq6(Fq2.zero(), b.c0.c2))
    assert a.mul_by_014(b.c0.c0, b.c0.c1, b.c0.c2) == a * sparse
    assert len(prepare_g2(G2.generator())) == N_LINES == 63 + 5 and prepare_g2(G2.one()) == []
    assert bin(BLS_X >> 1).count("1") == 6


# ---------------------------------------------------------------- the self test (the kernels' bodies on the host) against the model
_rand12 = fc.rand12


@pytest.mark.parametrize("name", [n for n in OPS if n not in ("FQ12_FINAL_EXP", "FQ12_CYCLO_SQR")])
def test_selftest_tower_operation_matches_the_model(name):
    """over fq_cases.tower_operands(): the random and 0 / 1 / Q - 1 operands, every value of the Fq edge pool at every coordinate, and
    the sparse elements; b is the list rotated by one"""
    for arg in ((1, 2, 3) if name == "FQ12_FROBENIUS" else (0,)):
        a, b, want = fc.tower_case(name, arg)
        got = ps.tower_words(OPS[name], a, b, arg)
        assert np.array_equal(got, want), (name, arg, [int(i) for i in np.nonzero((got != want).any(axis=1))[0]])
    assert len(fc.tower_operands()) > 64 + len(fc.fq_edge_pool())


def test_selftest_inverse_with_c1_zero_and_frobenius_twelve_times():
    rnd = random.Random(9)
    a = _rand12(rnd)
    flat = Fq12(a.c0)                                              # c1 = 0
    assert ps.tower(OPS["FQ12_INV"], [flat]) == [flat.inverse()] and (flat * flat.inverse()).is_one()
    f = [a, flat]
    for _ in range(12):
        f = ps.tower(OPS["FQ12_FROBENIUS"], f, arg=1)
    assert f == [a, flat]
    f = ps.tower(OPS["FQ12_FROBENIUS"], ps.tower(OPS["FQ12_FROBENIUS"], [a], arg=1), arg=2)
    assert f == ps.tower(OPS["FQ12_FROBENIUS"], [a], arg=3) == [a.pow(Q).pow(Q).pow(Q)]


def test_selftest_cyclotomic_squaring_equals_the_plain_one_after_the_easy_part():
    """Granger and Scott's squaring (the powers by |x| of the final exponentiation use it) is a squaring only in the cyclotomic subgroup:
    compared with fq12_sqr and with the model on elements that have been through the easy part f^((Q^6 - 1)(Q^2 + 1)), edge coordinates in
    the inputs included, and on 1; on an element outside the subgroup the two differ."""
    raw, cyc = fc.cyclotomic_operands()
    got = ps.tower(OPS["FQ12_CYCLO_SQR"], cyc)
    assert got == ps.tower(OPS["FQ12_SQR"], cyc) == [x.square() for x in cyc]
    assert all((x.conjugate() * x).is_one() for x in cyc)              # x^(Q^6 + 1) = 1
    assert ps.tower(OPS["FQ12_CYCLO_SQR"], raw[:1]) != ps.tower(OPS["FQ12_SQR"], raw[:1])


# ---------------------------------------------------------------- the Fq operations of the debug header, through the same self test
def test_selftest_fq_mul_over_every_ordered_pair_of_the_edge_pool():
    a, b, want = fc.fq_mul_case()
    assert len(a) == len(fc.fq_edge_pool()) ** 2 > 10000
    got = ps.tower_words(fc.FQ_OPS["FQ_MUL"], a, b)
    assert np.array_equal(got, want), [int(i) for i in np.nonzero((got != want).any(axis=1))[0]][:8]
    assert np.array_equal(got[:, 6:], a[:, 6:]) and a[:, 6:].any()           # the other eleven coordinates are copied through


@pytest.mark.parametrize("sa", range(4))
@pytest.mark.parametrize("sb", range(4))
def test_selftest_fq_mul_of_lazy_operand_sums_up_to_eight_q(sa, sb):
    """ka a and kb b formed without a conditional subtraction, as the Karatsuba factor sums are; with the pre-image of Q - 1 the
    Montgomery digits are Q - 1 themselves and sa = sb = 3 multiplies 8 (Q - 1) by 8 (Q - 1): the bound LAZY SUMS states"""
    arg, a, b, want = fc.fq_mul_lazy_case(sa, sb)
    assert len(a) == 36 and fc.pre_image(Q - 1) * fc.MONT % Q == Q - 1
    got = ps.tower_words(fc.FQ_OPS["FQ_MUL_LAZY"], a, b, arg)
    assert np.array_equal(got, want), (sa, sb, [int(i) for i in np.nonzero((got != want).any(axis=1))[0]])


def test_selftest_fq_inverse_over_the_edge_pool():
    a, want = fc.fq_inv_case()
    got = ps.tower_words(fc.FQ_OPS["FQ_INV"], a)
    assert np.array_equal(got, want)
    x, y = ps.s.unwords(a[:, :6], 6), ps.s.unwords(got[:, :6], 6)
    assert all((u * v % Q == 1) if u else (v == 0) for u, v in zip(x, y)) and 0 in x


def test_edge_pool_holds_what_it_claims():
    pool = fc.fq_edge_pool()
    assert list(pool) == sorted(set(pool)) and pool[0] == 0 and pool[-1] == Q - 1
    for v in (1, 2, Q - 2, (Q - 1) // 2, (Q + 1) // 2, fc.ONES13, fc.ONES_TOP, (1 << 29) - 1, (1 << 377) + 1, (1 << 352) - 1, (1 << 384) % Q):
        assert v in pool and fc.pre_image(v) in pool
    n = len(pool)
    walk = fc.tower_operands()[len(fc.edge_operands()):len(fc.edge_operands()) + n]
    for k in (0, 5, 11):                                                     # every value sits at every coordinate once
        assert sorted(x.coords()[k] for x in walk) == list(pool)
    assert _capi.HB_PAIR_OP_FQ_MUL == 17 and _capi.HB_PAIR_OP_FQ_MUL_LAZY == 18 and _capi.HB_PAIR_OP_FQ_INV == 19
    with open(os.path.join(REPO, "include", "hbmpc_hip_debug.h")) as f:
        text = f.read()
    for name, value in fc.FQ_OPS.items():
        assert re.search(r"#define HB_PAIR_OP_" + name + r" " + str(value) + r"\b", text)


def test_selftest_refuses_bad_arguments():
    a = ps.gt_words([Fq12.one()])
    assert ps.selftest(ps.TOWER, [a], 99, 0, 1, 72)[0] == _capi.HB_ERR_BAD_ARG
    assert ps.selftest(ps.TOWER, [a], OPS["FQ12_FROBENIUS"], 4, 1, 72)[0] == _capi.HB_ERR_BAD_ARG
    assert ps.selftest(ps.TOWER, [a], OPS["FQ12_MUL"], 0, 1, 72)[0] == _capi.HB_ERR_BAD_ARG        # the second operand is missing
    assert ps.selftest(ps.TOWER, [a], fc.FQ_OPS["FQ_MUL"], 0, 1, 72)[0] == _capi.HB_ERR_BAD_ARG
    assert ps.selftest(ps.TOWER, [a], fc.FQ_OPS["FQ_INV"], 1, 1, 72)[0] == _capi.HB_ERR_BAD_ARG
    for arg in (-1, 4, 0x40, 0x133):                                       # the shift counts are two bits each
        assert ps.selftest(ps.TOWER, [a, a], fc.FQ_OPS["FQ_MUL_LAZY"], arg, 1, 72)[0] == _capi.HB_ERR_BAD_ARG
    assert ps.selftest(ps.TOWER, [a], 20, 0, 1, 72)[0] == _capi.HB_ERR_BAD_ARG
    big = a.copy()
    big[0, :6] = ps.s.words([Q], 6)[0]
    assert ps.selftest(ps.TOWER, [big], OPS["FQ12_SQR"], 0, 1, 72)[0] == _capi.HB_ERR_BAD_ARG     # a residue not below Q
    co = ps.coeff_words(G2.generator())
    bad = co.copy()
    bad[5] = ps.s.words([Q], 6)[0]
    assert ps.selftest(ps.PREPARE, [bad], 0, 0, 1, 4000)[0] == _capi.HB_ERR_BAD_ARG
    pts = ps.s.points([G1.generator()])
    tab = ps.host_table(G2.generator())
    for K in (0, 5):
        assert ps.selftest(ps.PRODUCT, [pts, tab, tab, tab, tab], K, ps.GT, 1, 72)[0] == _capi.HB_ERR_BAD_ARG
    assert ps.selftest(ps.PRODUCT, [pts, tab], 1, 2, 1, 72)[0] == _capi.HB_ERR_BAD_ARG


def test_selftest_final_exponentiation_and_pairings_match_the_model():
    """six pairings of the model"""
    rnd = random.Random(3)
    a = _rand12(rnd)
    assert ps.tower(OPS["FQ12_FINAL_EXP"], [a]) == [final_exponentiation(a)]
    g, h = G1.generator(), G2.generator()
    q2 = h ** 0xABCDEF
    rows = [[g, g ** 7], [g ** (R - 1), G1.one()], [G1.one(), G1.one()]]
    got = ps.host_product(rows, [h, q2])
    assert got[0] == ps.model_product(rows[0], [h, q2])
    assert got[1] == ps.model_product(rows[1], [h, q2]) == e_gen().inverse()
    assert got[2].is_one()
    assert ps.host_product([[g]], [h]) == [e_gen()]
    # raw Miller values differ by factors the final exponentiation kills: only the value after it is compared
    three = ps.host_product([[g ** 2, g ** 3, g.invert()]], [h, h ** 5, h ** 17])
    assert three[0].is_one()
    four = ps.host_product([[g, g, g, g]], [h, h ** 2, h ** 3, h ** 4])
    assert four == [e_gen().pow(10)]


def test_selftest_verdict_mode_counts_rejections_and_refuses_points_off_the_curve():
    g, h = G1.generator(), G2.generator()
    rows = [[g ** 3, g.invert()], [g, g], [G1.one(), G1.one()], [g ** 3, g.invert()]]
    verdicts, rejected = ps.host_product(rows, [h, h ** 3], mode=ps.VERDICT)
    assert verdicts == [1, 0, 1, 1] and rejected == 1
    off = ps.s.off_curve_raw()
    pts = ps.s.points([off, G1.one()])
    rc, out = ps.selftest(ps.PRODUCT, [pts, ps.host_table(h), ps.host_table(h)], 2, ps.VERDICT, 1, 2)
    assert rc == 0 and list(out.view("int32")[:2]) == [0, 1]


# ---------------------------------------------------------------- the KZG check in its two-pairing form
@pytest.mark.parametrize("t", [0, 1, 3])
def test_kzg_cases_on_a_trapdoor_crs(t):
    """e(c - share g0 - aux h0 + i w, ghat0) e(-w, ghat1) == 1 through the self test's verdict mode, every case of
    pairing_support.kzg_cases; the honest item and one wrong one also through the model.  At t = 0 the polynomial is a constant, so the
    same share at another index is a TRUE claim and the witness is the identity: the second pair is skipped."""
    gh = ps.ghats()
    cases = ps.kzg_cases(t)
    names = list(cases)
    rows = [list(ps.kzg_lhs(*cases[n][0])) for n in names]
    verdicts, rejected = ps.host_product(rows, gh, mode=ps.VERDICT)
    want = [cases[n][1] for n in names]
    assert [bool(v) for v in verdicts] == want and rejected == want.count(False)
    assert want[0] and want[1:5] == [False] * 4 and (want[5] is (t == 0))
    if t == 0:
        assert rows[0][1].is_one()
    if t == 3:
        assert ps.model_product(rows[0], gh).is_one() and not ps.model_product(rows[1], gh).is_one()


def test_kzg_identity_left_side_with_a_witness_is_rejected():
    g = G1.generator()
    verdicts, rejected = ps.host_product([[G1.one(), g], [G1.one(), G1.one()]], ps.ghats(), mode=ps.VERDICT)
    assert verdicts == [0, 1] and rejected == 1


# ---------------------------------------------------------------- surface
def test_pairing_symbols_are_declared_and_typed():
    with open(os.path.join(REPO, "include", "hbmpc_hip.h")) as f:
        text = f.read()
    for name in ("hb_pair_prepare", "hb_pair_product", "hb_selftest_pairing"):
        assert re.search(r"\bint " + name + r"\s*\(", text) and name in _capi.SYMBOLS
    assert re.search(r"\bint64_t hb_pair_table_bytes\s*\(", text) and "hb_pair_table_bytes" in _capi.SYMBOLS
    for name, value in OPS.items():
        assert re.search(r"#define HB_PAIR_OP_" + name + r" " + str(value) + r"\b", text) and getattr(_capi, "HB_PAIR_OP_" + name) == value
    assert _capi.load_library().hb_pair_table_bytes() == N_LINES * 3 * 2 * 14 * 4


def test_poly_commit_const_without_ghats_still_raises_and_with_ghats_validates():
    from honeybadgermpc_amd.poly_commit_const import PolyCommitConst

    gs, hs = ps.cs.crs_points(2)
    pc = PolyCommitConst([gs, None, hs])
    for call in (lambda: pc.verify_eval(gs[0], 1, 0, 0, gs[0]), lambda: pc.batch_verify_eval([], 1, [], [], []), lambda: pc.preprocess_verifier(),
                 lambda: pc.verify_batch(None, 1, None, None, None)):
        with pytest.raises(NotImplementedError, match="pairing") as info:
            call()
        assert "G2 half" in str(info.value)
    with pytest.raises(TypeError):
        PolyCommitConst([gs, [gs[0], gs[1]], hs])
    with pytest.raises(ValueError):
        PolyCommitConst([gs, [G2.generator(), G2.one()], hs])
    pc = PolyCommitConst([gs, ps.ghats(), hs])
    assert pc.batch_verify_eval([], 3, [], [], []) is True              # the reference's empty products and sums
    import torch

    if not torch.cuda.is_available():                                   # there is no CPU path: every computing method says so
        for call in (lambda: pc.verify_eval(gs[0], 1, 0, 0, gs[0]), lambda: pc.batch_verify_eval([gs[0]], 1, [0], [0], [gs[0]]),
                     lambda: pc.preprocess_verifier()):
            with pytest.raises(_capi.HbmpcBackendError):
                call()

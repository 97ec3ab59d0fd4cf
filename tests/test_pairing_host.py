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

import pytest

import pairing_support as ps
from conftest import GOLDEN, REPO

from honeybadgermpc_amd import _capi
from honeybadgermpc_amd.bls12_381 import G1, Q, R
from honeybadgermpc_amd.bls12_381_pairing import BLS_X, FROBENIUS_FQ12_C1, Fq2, Fq6, Fq12, G2, N_LINES, final_exponentiation, pair, pairing_product, prepare_g2

OPS = dict(FQ2_MUL=0, FQ2_SQR=1, FQ2_MUL_NR=2, FQ2_INV=3, FQ6_MUL=4, FQ6_MUL_BY_01=5, FQ6_MUL_BY_1=6, FQ6_MUL_NR=7, FQ6_INV=8, FQ12_MUL=9, FQ12_SQR=10,
           FQ12_MUL_BY_014=11, FQ12_CONJ=12, FQ12_FROBENIUS=13, FQ12_INV=14, FQ12_FINAL_EXP=15, FQ12_CYCLO_SQR=16)


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
def _rand12(rnd):
    return Fq12.from_coords([rnd.randrange(Q) for _ in range(12)])


def _edge_operands():
    """Fq12 operands: random ones, then 0, 1 and Q - 1 in every coordinate in turn (the others random), then all-equal edge values"""
    rnd = random.Random(5)
    out = [_rand12(rnd) for _ in range(4)]
    for k in range(12):
        for v in (0, 1, Q - 1):
            co = [rnd.randrange(Q) for _ in range(12)]
            co[k] = v
            out.append(Fq12.from_coords(co))
    out += [Fq12.from_coords([v] * 12) for v in (0, 1, Q - 1)] + [Fq12.one()]
    return out


def _model_op(name, a, b, arg):
    f2 = lambda x: Fq12(Fq6(x, a.c0.c1, a.c0.c2), a.c1)
    f6 = lambda x: Fq12(x, a.c1)
    return {
        "FQ2_MUL": lambda: f2(a.c0.c0 * b.c0.c0),
        "FQ2_SQR": lambda: f2(a.c0.c0.square()),
        "FQ2_MUL_NR": lambda: f2(a.c0.c0.mul_by_nonresidue()),
        "FQ2_INV": lambda: f2(a.c0.c0.inverse()),
        "FQ6_MUL": lambda: f6(a.c0 * b.c0),
        "FQ6_MUL_BY_01": lambda: f6(a.c0.mul_by_01(b.c0.c0, b.c0.c1)),
        "FQ6_MUL_BY_1": lambda: f6(a.c0.mul_by_1(b.c0.c0)),
        "FQ6_MUL_NR": lambda: f6(a.c0.mul_by_nonresidue()),
        "FQ6_INV": lambda: f6(a.c0.inverse()),
        "FQ12_MUL": lambda: a * b,
        "FQ12_SQR": lambda: a.square(),
        "FQ12_MUL_BY_014": lambda: a.mul_by_014(b.c0.c0, b.c0.c1, b.c0.c2),
        "FQ12_CONJ": lambda: a.conjugate(),
        "FQ12_FROBENIUS": lambda: a.frobenius_map(arg),
        "FQ12_INV": lambda: a.inverse(),
    }[name]()


@pytest.mark.parametrize("name", [n for n in OPS if n not in ("FQ12_FINAL_EXP", "FQ12_CYCLO_SQR")])
def test_selftest_tower_operation_matches_the_model(name):
    a = _edge_operands()
    b = a[1:] + a[:1]
    two = name in ("FQ2_MUL", "FQ6_MUL", "FQ6_MUL_BY_01", "FQ6_MUL_BY_1", "FQ12_MUL", "FQ12_MUL_BY_014")
    for arg in ((1, 2, 3) if name == "FQ12_FROBENIUS" else (0,)):
        got = ps.tower(OPS[name], a, b if two else None, arg)
        want = [_model_op(name, x, y, arg) for x, y in zip(a, b)]
        assert got == want, (name, arg)


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
    def easy(f):
        r = f.conjugate() * f.inverse()
        return r.frobenius_map(2) * r

    raw = [x for x in _edge_operands()[:12] if not (x.c0.is_zero() and x.c1.is_zero())]
    cyc = [easy(x) for x in raw] + [Fq12.one()]
    got = ps.tower(OPS["FQ12_CYCLO_SQR"], cyc)
    assert got == ps.tower(OPS["FQ12_SQR"], cyc) == [x.square() for x in cyc]
    assert all((x.conjugate() * x).is_one() for x in cyc)              # x^(Q^6 + 1) = 1
    assert ps.tower(OPS["FQ12_CYCLO_SQR"], raw[:1]) != ps.tower(OPS["FQ12_SQR"], raw[:1])


def test_selftest_refuses_bad_arguments():
    a = ps.gt_words([Fq12.one()])
    assert ps.selftest(ps.TOWER, [a], 99, 0, 1, 72)[0] == _capi.HB_ERR_BAD_ARG
    assert ps.selftest(ps.TOWER, [a], OPS["FQ12_FROBENIUS"], 4, 1, 72)[0] == _capi.HB_ERR_BAD_ARG
    assert ps.selftest(ps.TOWER, [a], OPS["FQ12_MUL"], 0, 1, 72)[0] == _capi.HB_ERR_BAD_ARG        # the second operand is missing
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

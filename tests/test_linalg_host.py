"""CPU-only: the matrix-product kernels (csrc/hb_mat.hip) run on the host through hb_selftest_mat -- the same HB_HD bodies the kernels
call, walked workgroup by workgroup and lane by lane, the split path with its reduction launch included -- against Python ints.
Inner dimensions sit on every arithmetic boundary of both element widths (the carry pass every GROUP products, the reduction every L,
the staged depth TILE_K), outputs on every tile edge; every operand p - 1 with C = p - 1 at inner = L, L + 1, 4 L is the case the
REDC precondition L p <= R is tight for.  Exact equality everywhere."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

from conftest import BLS, REPO

import edge_values
from honeybadgermpc_amd import linalg

GOLDILOCKS = 0xFFFFFFFF00000001
P64 = (1 << 64) - 59
P256 = (1 << 256) - 189
P25519 = (1 << 255) - 19
FIELDS = [(BLS, 4), (P256, 4), (P25519, 4), (53, 4), (13, 4), (P64, 1), (GOLDILOCKS, 1), (13, 1)]
FIELD_IDS = ["bls", "2^256-189", "2^255-19", "53", "13-wide", "2^64-59", "goldilocks", "13-narrow"]
NONE, ADD, SUB = 0, 1, 2
SPLIT, AUTO = 0x100, 0x200
TM, TN, TK = linalg.TILE_M, linalg.TILE_N, linalg.TILE_K


def _lib():
    from honeybadgermpc_amd._capi import load_library

    return load_library()


def _limbs(values, p, nl):
    from honeybadgermpc_amd._capi import ints_to_limbs

    return ints_to_limbs(list(values) or [0], p, 8 * nl)


def _raw(p, nl, what, ptrs, params, out_ptr):
    from honeybadgermpc_amd._capi import ints_to_limbs, np_ptr

    ops = (ctypes.c_void_p * 3)(*ptrs)
    prm = np.array(list(params), dtype=np.int64)
    return _lib().hb_selftest_mat(np_ptr(ints_to_limbs([p], p + 1, 8 * nl)), nl, what, ops, np_ptr(prm), out_ptr)


def mat(p, nl, a, b, c, op, batch, m, k, n, mode=0, slices=1, out_is_c=False):
    """-> (rc, out as ints)"""
    from honeybadgermpc_amd._capi import limbs_to_ints

    count = batch * m * n
    arrs = [_limbs(v, p, nl) for v in (a, b, c)]
    out = arrs[2] if out_is_c else np.full((max(count, 1), nl), 7, dtype=np.uint64)
    rc = _raw(p, nl, op | mode, [x.ctypes.data for x in arrs], (batch, m, k, n, slices), out.ctypes.data)
    return rc, (limbs_to_ints(out[:count], 8 * nl) if count else [])


def model(p, a, b, c, op, batch, m, k, n):
    out = []
    for bt in range(batch):
        for i in range(m):
            row = a[(bt * m + i) * k:(bt * m + i + 1) * k]
            for j in range(n):
                s = sum(x * b[(bt * k + l) * n + j] for l, x in enumerate(row))
                cv = c[(bt * m + i) * n + j] if op != NONE else 0
                out.append((s + cv if op != SUB else s - cv) % p)
    return out


def operands(p, rnd, batch, m, k, n, fill=None):
    draw = (lambda: fill) if fill is not None else (lambda: rnd.randrange(p))
    return ([draw() for _ in range(batch * m * k)], [draw() for _ in range(batch * k * n)], [draw() for _ in range(batch * m * n)])


def inner_boundaries(nl):
    g, big = linalg.LAZY_GROUP[nl], linalg.LAZY_L[nl]
    return sorted({1, g - 1, g, g + 1, big - 1, big, big + 1, 2 * big, 4 * big + 3, TK - 1, TK + 1})


def test_constants_are_the_librarys():
    assert (TM, TN, TK) == (16, 32, 16) and linalg.LAZY_GROUP == {4: 7, 1: 21} and linalg.LAZY_L == {4: 28, 1: 84}
    for nl in (4, 1):
        # the bound hb_pm.hip derives: L p <= R = 2^(29 NL) for every p below 2^(64 limbs); GROUP products of NL terms below 2^58 a column
        digits = 9 if nl == 4 else 3
        assert linalg.LAZY_L[nl] << (64 * nl) <= 1 << (29 * digits) and linalg.LAZY_L[nl] == 4 * linalg.LAZY_GROUP[nl]
        assert linalg.LAZY_GROUP[nl] * digits * (2 ** 29 - 1) ** 2 + 2 ** 30 < 2 ** 64
    out = (ctypes.c_int32 * 8)()
    assert _lib().hb_mat_constants(2, out) == 2 and _lib().hb_mat_constants(4, None) == 2
    assert linalg.takes_split(1, 1, linalg.SPLIT_MIN_K, 1) and not linalg.takes_split(1, 1, linalg.SPLIT_MIN_K - 1, 1)
    assert not linalg.takes_split(linalg.SPLIT_MAX_WORKGROUPS + 1, 1, 1 << 20, 1)


@pytest.mark.parametrize("p, nl", FIELDS, ids=FIELD_IDS)
def test_inner_dimension_boundaries(p, nl):
    rnd = random.Random(p % 997 + nl)
    for e, k in enumerate(inner_boundaries(nl)):
        m, n = (2, 3) if e % 2 else (3, 2)
        a, b, c = operands(p, rnd, 1, m, k, n)
        for op in (NONE, ADD, SUB):
            assert mat(p, nl, a, b, c, op, 1, m, k, n) == (0, model(p, a, b, c, op, 1, m, k, n)), (k, op)


@pytest.mark.parametrize("p, nl", FIELDS, ids=FIELD_IDS)
def test_output_tile_edges(p, nl):
    rnd = random.Random(p % 991 + nl)
    k = TK + 1
    for e, (m, n) in enumerate((m, n) for m in (1, 2, TM - 1, TM, TM + 1) for n in (1, 2, TN - 1, TN, TN + 1)):
        a, b, c = operands(p, rnd, 1, m, k, n)
        op = e % 3
        assert mat(p, nl, a, b, c, op, 1, m, k, n) == (0, model(p, a, b, c, op, 1, m, k, n)), (m, n)
    # a ragged batch of 3, and one of whole tiles and a bit
    for batch, m, k, n in ((3, 5, 9, 4), (3, TM + 1, 3, TN + 1)):
        a, b, c = operands(p, rnd, batch, m, k, n)
        for op in (NONE, ADD, SUB):
            assert mat(p, nl, a, b, c, op, batch, m, k, n) == (0, model(p, a, b, c, op, batch, m, k, n)), (batch, op)
        assert mat(p, nl, a, b, c, ADD, batch, m, k, n, out_is_c=True) == (0, model(p, a, b, c, ADD, batch, m, k, n))


@pytest.mark.parametrize("p, nl", [(P256, 4), (P64, 1)], ids=["2^256-189", "2^64-59"])
def test_worst_case_every_operand_p_minus_1(p, nl):
    """inner (p - 1)^2 + (p - 1) and inner (p - 1)^2 - (p - 1): the largest T a reduction sees, at and around L"""
    big = linalg.LAZY_L[nl]
    for k in (big, big + 1, 4 * big):
        for m, n in ((1, 1), (2, 3)):
            a, b, c = operands(p, None, 1, m, k, n, fill=p - 1)
            for op, want in ((ADD, (k + p - 1) % p), (SUB, (k - (p - 1)) % p), (NONE, k % p)):
                assert model(p, a, b, c, op, 1, m, k, n) == [want] * (m * n)
                assert mat(p, nl, a, b, c, op, 1, m, k, n) == (0, [want] * (m * n)), (k, op)
                assert mat(p, nl, a, b, c, op, 1, m, k, n, SPLIT, 3) == (0, [want] * (m * n)), (k, op)


@pytest.mark.parametrize("p, nl", FIELDS, ids=FIELD_IDS)
def test_zeros_and_edge_values(p, nl):
    big = linalg.LAZY_L[nl]
    m, k, n = 3, big + 1, 4
    a, b, c = operands(p, None, 1, m, k, n, fill=0)
    for op in (NONE, ADD, SUB):
        assert mat(p, nl, a, b, c, op, 1, m, k, n) == (0, [0] * (m * n))
    assert mat(p, nl, [], [], [5 % p] * (m * n), SUB, 1, m, 0, n) == (0, [-5 % p] * (m * n))           # k == 0: 0 (op) C
    assert mat(p, nl, [], [], [5 % p] * (m * n), ADD, 1, m, 0, n) == (0, [5 % p] * (m * n))
    assert mat(p, nl, [], [], [], NONE, 1, m, 0, n) == (0, [0] * (m * n))
    pool = edge_values.operands(p, nl)
    k = max(len(pool), big + 1)
    a = [pool[(7 * i + l) % len(pool)] for i in range(m) for l in range(k)]
    b = [pool[(3 * l + 11 * j + 1) % len(pool)] for l in range(k) for j in range(n)]
    c = [pool[(5 * e + 2) % len(pool)] for e in range(m * n)]
    for op in (NONE, ADD, SUB):
        want = model(p, a, b, c, op, 1, m, k, n)
        assert mat(p, nl, a, b, c, op, 1, m, k, n) == (0, want), op
        assert mat(p, nl, a, b, c, op, 1, m, k, n, SPLIT, 4) == (0, want), op


@pytest.mark.parametrize("p, nl", [(BLS, 4), (P256, 4), (P64, 1), (13, 1)], ids=["bls", "2^256-189", "2^64-59", "13-narrow"])
def test_split_and_unsplit_agree(p, nl):
    rnd = random.Random(p % 983 + nl)
    big = linalg.LAZY_L[nl]
    for batch, m, k, n in ((1, 1, 4 * big + 3, 1), (2, 3, 2 * TK + 1, 5), (1, TM + 1, TK, TN + 1), (1, 2, 5 * TK, 2)):
        a, b, c = operands(p, rnd, batch, m, k, n)
        for op in (NONE, ADD, SUB):
            rc, plain = mat(p, nl, a, b, c, op, batch, m, k, n)
            assert rc == 0 and plain == model(p, a, b, c, op, batch, m, k, n)
            for slices in (1, 2, 3, 5, 64):
                assert mat(p, nl, a, b, c, op, batch, m, k, n, SPLIT, slices) == (0, plain), (k, op, slices)
        assert mat(p, nl, a, b, c, SUB, batch, m, k, n, SPLIT, 3, out_is_c=True) == (0, model(p, a, b, c, SUB, batch, m, k, n))
    # the library's own rule at its threshold: a dot product one element below it (one launch) and at it (two slices)
    for k in (linalg.SPLIT_MIN_K - 1, linalg.SPLIT_MIN_K, linalg.SPLIT_MIN_K + 1):
        a, b, c = operands(p, rnd, 1, 1, k, 1)
        want = model(p, a, b, c, ADD, 1, 1, k, 1)
        assert mat(p, nl, a, b, c, ADD, 1, 1, k, 1, AUTO) == (0, want) and mat(p, nl, a, b, c, ADD, 1, 1, k, 1) == (0, want), k


def test_bad_arguments():
    p, nl = BLS, 4
    one = _limbs([1], p, nl)
    out = np.zeros((4, nl), dtype=np.uint64)
    A = B = C = one.ctypes.data
    O = out.ctypes.data
    ok = (1, 1, 1, 1, 1)
    assert _raw(p, nl, NONE, [A, B, C], ok, O) == 0
    for params in ((-1, 1, 1, 1, 1), (1, -1, 1, 1, 1), (1, 1, -1, 1, 1), (1, 1, 1, -1, 1)):                # negative sizes
        assert _raw(p, nl, NONE, [A, B, C], params, O) == 2, params
    assert _raw(p, nl, 3, [A, B, C], ok, O) == 2 and _raw(p, nl, 0xff, [A, B, C], ok, O) == 2              # unknown c_op
    assert _raw(p, nl, NONE | 0x400, [A, B, C], ok, O) == 2                                                # unknown mode
    assert _raw(p, nl, ADD, [A, B, None], ok, O) == 2 and _raw(p, nl, SUB, [A, B, None], ok, O) == 2       # no C for an epilogue
    assert _raw(p, nl, ADD, [A, B, None], (0, 1, 1, 1, 1), O) == 2                                         # ... whatever the shape
    assert _raw(p, nl, NONE, [A, B, None], ok, O) == 0
    assert _raw(p, nl, NONE, [O, B, C], ok, O) == 2 and _raw(p, nl, NONE, [A, O, C], ok, O) == 2           # out over a or b
    assert _raw(p, nl, ADD, [A, B, O], ok, O) == 0                                                         # out over c
    assert _raw(p, nl, NONE, [None, B, C], ok, O) == 2 and _raw(p, nl, NONE, [A, None, C], ok, O) == 2     # null operands, non-empty shape
    assert _raw(p, nl, NONE, [A, B, C], ok, None) == 2
    assert _raw(p, nl, NONE, [None, None, None], (1, 1, 0, 1, 1), O) == 0                                  # k == 0 reads neither
    out[:] = 9
    for params in ((0, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 1, 1, 0, 1)):                                     # nothing to do: nothing is written
        assert _raw(p, nl, NONE, [None, None, None], params, None) == 0 and _raw(p, nl, NONE, [A, B, C], params, O) == 0
    assert (out == 9).all()
    assert _raw(p, nl, NONE | SPLIT, [A, B, C], (1, 1, 1, 1, 0), O) == 2
    from honeybadgermpc_amd._capi import np_ptr

    ops = (ctypes.c_void_p * 3)(A, B, C)
    prm = np.array(ok, dtype=np.int64)
    assert _lib().hb_selftest_mat(np_ptr(_limbs([p], p + 1, nl)), 2, NONE, ops, np_ptr(prm), O) == 2        # neither width
    assert _lib().hb_selftest_mat(None, nl, NONE, ops, np_ptr(prm), O) == 2
    assert _lib().hb_selftest_mat(np_ptr(_limbs([p], p + 1, nl)), nl, NONE, None, np_ptr(prm), O) == 2
    assert _lib().hb_selftest_mat(np_ptr(_limbs([p], p + 1, nl)), nl, NONE, ops, None, O) == 2


def test_costs_and_parameters_are_checked_before_the_device():
    import asyncio

    from honeybadgermpc_amd import offline
    from honeybadgermpc_amd.progs import fixedpoint

    for m, k, n in ((1, 1, 1), (3, 5, 2), (4, 29, 4), (64, 64, 64)):
        assert linalg.count_opens(linalg.DOUBLE_SHARING, m, k, n) == m * n
        assert linalg.count_opens(linalg.BEAVER, m, k, n) == m * k + k * n
        assert linalg.count_opens(linalg.ELEMENTWISE, m, k, n) == 2 * m * k * n
        assert linalg.count_opens(linalg.BEAVER, m, k, n, batch=3) == 3 * (m * k + k * n)
        assert [linalg.count_triples(w, m, k, n) for w in (linalg.DOUBLE_SHARING, linalg.BEAVER, linalg.ELEMENTWISE)] == [0, 0, m * k * n]
        assert [linalg.count_matrix_triples(w) for w in (linalg.DOUBLE_SHARING, linalg.BEAVER)] == [0, 1]
        assert [linalg.count_double_sharings(w, m, k, n) for w in (linalg.DOUBLE_SHARING, linalg.BEAVER)] == [m * n, 0]
    for bad in ("triples", None, 0):
        with pytest.raises(ValueError):
            linalg.count_opens(bad, 1, 1, 1)
    with pytest.raises(ValueError):
        linalg.count_opens(linalg.BEAVER, -1, 1, 1)
    assert fixedpoint.matmul_width(64, 1) == 128 and fixedpoint.matmul_width(64, 28) == 133 and fixedpoint.matmul_width(64, 3) == 130
    with pytest.raises(ValueError):
        fixedpoint.matmul_width(64, 0)
    fixedpoint.check_params(BLS, fixedpoint.matmul_width(64, 28), 32, 32)
    with pytest.raises(ValueError):
        fixedpoint.check_params(BLS, fixedpoint.matmul_width(110, 3), 32, 32)

    class Co:
        ctx, myid, n, t = None, 0, 4, 1

    for args in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 1, 0), (1.0, 1, 1), (True, 1, 1)):
        with pytest.raises(ValueError):
            asyncio.run(offline.generate_matrix_triples(Co(), *args))


def test_entry_points_are_declared_and_bound():
    from honeybadgermpc_amd import _capi

    text = open(os.path.join(REPO, "include", "hbmpc_hip.h")).read()
    for name in ("hb_mat_mul", "hb_mat_constants", "hb_selftest_mat"):
        assert re.search(r"\bint " + name + r"\s*\(", text) and name in _capi.SYMBOLS
    for name, value in (("HB_MAT_NONE", 0), ("HB_MAT_ADD", 1), ("HB_MAT_SUB", 2)):
        assert re.search(rf"#define {name}\s+{value}\b", text) and getattr(_capi, name) == value
    debug = open(os.path.join(REPO, "include", "hbmpc_hip_debug.h")).read()
    assert "hb_debug_mat_split" in debug and "hb_debug_mat_split" in _capi.DEBUG_SYMBOLS and "hb_debug_mat_split" not in text
    for name in ("matmul", "dot", "double_sharing_matmul", "beaver_matmul", "count_opens", "count_triples"):
        assert callable(getattr(linalg, name))

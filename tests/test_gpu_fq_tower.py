"""The Fq, Fq2, Fq6 and Fq12 bodies of csrc/hb_fq12_elem.hpp and the bare square root and phi of csrc/hb_g1_wire_elem.hpp ON THE DEVICE at
chosen operands: hb_debug_pair_op (k_pair_op) and hb_debug_g1_wire_op (k_g1_wire_op) run one operation a launch over the per-item
functions the host self tests call.  The device build differs from the host's where it matters -- fq_mul is the non-inlined fq_mul_call on
14-lane vectors, the Fq6 and Fq12 products are real calls, an Fq12 lives in private memory -- and inside k_pair_product or the G1 kernels
these bodies only ever see pseudo-random values.  Here they get fq_cases: 0, 1, Q - 1, digit and word boundaries, all-ones digits, the
Montgomery pre-images of all of them, lazy operand sums at their stated bound 8 Q, and sparse tower elements.

Every comparison is exact, against Python ints (fq_cases, bls12_381_pairing); bit-equality with the host self test on the same words is
asserted beside it, so a failure says whether the body or the device build is wrong.  The operand lists are longer than one workgroup:
221 items are three workgroups of k_pair_op and a partial fourth."""
import ctypes

import numpy as np
import pytest

import fq_cases as fc
import g1_wire_cases as wc
import pairing_support as ps

from honeybadgermpc_amd import _capi
from honeybadgermpc_amd.bls12_381 import G1, Q, R
from honeybadgermpc_amd.bls12_381_pairing import Fq12, final_exponentiation

pytestmark = pytest.mark.gpu

s = ps.s
OPS, FQ_OPS = fc.OPS, fc.FQ_OPS
FILL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def ctx():
    from honeybadgermpc_amd._capi import Context

    return Context.get(R)


def dev(ctx, arr):
    return ctx.torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).to(ctx.tdev)


def device_op(ctx, op, a, b=None, arg=0):
    """(count, 72) uint64 words -> (out (count, 72) uint64, status list); what the launch does not write stays FILL / -7"""
    count = len(a)
    ad, bd = dev(ctx, a), (dev(ctx, b) if b is not None else None)
    out = ctx.torch.full((count, 72), FILL, dtype=ctx.torch.int64, device=ctx.tdev)
    status = ctx.torch.full((count,), -7, dtype=ctx.torch.int32, device=ctx.tdev)
    rc = ctx.lib.hb_debug_pair_op(ctx.h, op, arg, ctx.ptr(ad), ctx.ptr(bd) if bd is not None else None, ctx.ptr(out), ctx.ptr(status), count, ctx.stream())
    assert rc == _capi.HB_OK, (op, arg, rc)
    return out.cpu().numpy().view(np.uint64), status.cpu().tolist()


def rows_that_differ(got, want):
    return [int(i) for i in np.nonzero((got != want).any(axis=1))[0]][:12]


def check(ctx, op, a, b, want, arg=0):
    got, status = device_op(ctx, op, a, b, arg)
    assert status == [1] * len(a)
    assert np.array_equal(got, want), ("device differs from Python ints at items", rows_that_differ(got, want))
    host = ps.tower_words(op, a, b, arg)
    assert np.array_equal(got, host), ("device differs from the host self test at items", rows_that_differ(got, host))
    return got


# ---------------------------------------------------------------- the tower
@pytest.mark.parametrize("name", fc.MODELLED)
def test_tower_operation_on_the_device_matches_the_model(ctx, name):
    assert len(fc.tower_operands()) > 3 * 64 and len(fc.tower_operands()) % 64
    for arg in ((1, 2, 3) if name == "FQ12_FROBENIUS" else (0,)):
        a, b, want = fc.tower_case(name, arg)
        check(ctx, OPS[name], a, b, want, arg)


def test_cyclotomic_squaring_on_the_device(ctx):
    raw, cyc = fc.cyclotomic_operands()
    a = ps.gt_words(cyc)
    want = ps.gt_words([x.square() for x in cyc])
    got = check(ctx, OPS["FQ12_CYCLO_SQR"], a, None, want)
    assert np.array_equal(got, device_op(ctx, OPS["FQ12_SQR"], a)[0])
    # outside the cyclotomic subgroup it is no squaring, on the device as on the host
    out = ps.gt_words(raw[:1])
    cyclo, plain = device_op(ctx, OPS["FQ12_CYCLO_SQR"], out)[0], device_op(ctx, OPS["FQ12_SQR"], out)[0]
    assert not np.array_equal(cyclo, plain)
    assert np.array_equal(cyclo, ps.tower_words(OPS["FQ12_CYCLO_SQR"], out)) and np.array_equal(plain, ps.gt_words([raw[0].square()]))


def test_final_exponentiation_on_the_device(ctx):
    ops = fc.final_exp_operands()
    assert len(ops) == 8
    a = ps.gt_words(ops)
    got, status = device_op(ctx, OPS["FQ12_FINAL_EXP"], a)
    assert status == [1] * 8
    assert np.array_equal(got, ps.tower_words(OPS["FQ12_FINAL_EXP"], a))
    for m in fc.MODEL_FINAL_EXP:
        assert ps.gt_unwords(got[m]) == [final_exponentiation(ops[m])], m


# ---------------------------------------------------------------- Fq
def test_fq_mul_on_the_device_over_every_ordered_pair_of_the_edge_pool(ctx):
    a, b, want = fc.fq_mul_case()
    check(ctx, FQ_OPS["FQ_MUL"], a, b, want)


@pytest.mark.parametrize("sa", range(4))
@pytest.mark.parametrize("sb", range(4))
def test_fq_mul_on_the_device_of_lazy_operand_sums_up_to_eight_q(ctx, sa, sb):
    arg, a, b, want = fc.fq_mul_lazy_case(sa, sb)
    check(ctx, FQ_OPS["FQ_MUL_LAZY"], a, b, want, arg)


def test_fq_inverse_on_the_device_over_the_edge_pool(ctx):
    a, want = fc.fq_inv_case()
    got = check(ctx, FQ_OPS["FQ_INV"], a, None, want)
    x, y = s.unwords(a[:, :6], 6), s.unwords(got[:, :6], 6)
    assert all((u * v % Q == 1) if u else (v == 0) for u, v in zip(x, y))


# ---------------------------------------------------------------- the wire bodies
def device_wire(ctx, what, rows, width):
    """rows (count, width) uint64 -> (out (count, width) uint64, flags list or None)"""
    count = len(rows)
    ind = dev(ctx, rows)
    out = ctx.torch.full((count, width), FILL, dtype=ctx.torch.int64, device=ctx.tdev)
    flags = ctx.torch.full((count,), -7, dtype=ctx.torch.int32, device=ctx.tdev)
    rc = ctx.lib.hb_debug_g1_wire_op(ctx.h, what, ctx.ptr(ind), ctx.ptr(out), ctx.ptr(flags) if what == wc.SQRT else None, count, ctx.stream())
    assert rc == _capi.HB_OK, (what, rc)
    return out.cpu().numpy().view(np.uint64), flags.cpu().tolist()


def test_square_root_on_the_device_over_the_pool_and_its_squares(ctx):
    vals, flags, roots = fc.sqrt_case()
    assert len(vals) > 256 and 0 in flags and 1 in flags                  # two workgroups of k_g1_wire_op; residues and non-residues
    out, got_flags = device_wire(ctx, wc.SQRT, s.words(vals, 6), 6)
    got = s.unwords(out, 6)
    assert got_flags == flags                                             # Euler's criterion
    assert all(r * r % Q == a for a, f, r in zip(vals, flags, got) if f)
    assert all(r == 0 for f, r in zip(flags, got) if not f)               # a non-residue: flag 0 and a zero output
    assert got == roots                                                   # a^((Q + 1) / 4): which of the two roots
    host, host_flags = wc.host_sqrt(vals)
    assert got == host and got_flags == host_flags


def test_square_root_on_the_device_flags_a_value_not_below_q(ctx):
    vals = [4, Q, 9, (1 << 384) - 1, Q - 1, 16]
    out, flags = device_wire(ctx, wc.SQRT, s.words(vals, 6), 6)
    assert flags == [1, -1, 1, -1, 0, 1]
    assert s.unwords(out, 6) == [pow(4, (Q + 1) // 4, Q), 0, pow(9, (Q + 1) // 4, Q), 0, 0, pow(16, (Q + 1) // 4, Q)]


def test_phi_on_the_device(ctx):
    pts = [G1.one(), G1.generator(), s.raw_point(0, 2)] + s.vectors()[1:13]
    rows = s.points(pts)
    once, _ = device_wire(ctx, wc.PHI, rows, 12)
    assert np.array_equal(once, wc.host_phi(rows))
    want = [[0] * 12 if isinstance(p, G1) and p.is_one() else s.raw_point(wc.BETA * int(s.unwords(r[:6], 6)[0]) % Q, int(s.unwords(r[6:], 6)[0])) for p, r in zip(pts, rows)]
    assert once.tolist() == want
    assert not once[0].any() and once[2].tolist() == s.raw_point(0, 2)    # the identity stays; beta 0 = 0
    assert not np.array_equal(once[1], rows[1])
    twice, _ = device_wire(ctx, wc.PHI, once, 12)
    thrice, _ = device_wire(ctx, wc.PHI, twice, 12)
    assert np.array_equal(thrice, rows) and not np.array_equal(twice[1:2], rows[1:2])


# ---------------------------------------------------------------- status and refusals
def test_an_operand_not_below_q_gets_status_zero_and_its_neighbours_are_untouched(ctx):
    a, b, want = fc.tower_case("FQ12_MUL")
    a, b, want = a[:70].copy(), b[:70].copy(), want[:70].copy()
    a[3, 30:36] = s.words([Q], 6)[0]                                      # coordinate 5 of item 3 is Q
    a[64, :6] = s.words([(1 << 384) - 1], 6)[0]                           # coordinate 0 of the second workgroup's first item: all ones
    b[66, 66:72] = s.words([Q], 6)[0]                                     # the second operand's last coordinate
    bad = [3, 64, 66]
    got, status = device_op(ctx, OPS["FQ12_MUL"], a, b)
    assert status == [0 if m in bad else 1 for m in range(70)]
    want[bad] = 0
    assert np.array_equal(got, want), rows_that_differ(got, want)
    # an operation that does not read b does not judge it
    got, status = device_op(ctx, OPS["FQ12_SQR"], a, None)
    assert status == [0 if m in (3, 64) else 1 for m in range(70)] and not got[[3, 64]].any()
    assert np.array_equal(got[66], ps.tower_words(OPS["FQ12_SQR"], a[66:67])[0])
    # the self test refuses the same words outright
    assert ps.selftest(ps.TOWER, [a[3:4]], OPS["FQ12_SQR"], 0, 1, 72)[0] == _capi.HB_ERR_BAD_ARG


def test_argument_errors(ctx):
    from honeybadgermpc_amd._capi import Context

    lib, st = ctx.lib, ctx.stream()
    torch = ctx.torch
    n = 3
    a = dev(ctx, ps.gt_words([Fq12.one()] * n))
    out = torch.zeros((n + 1, 72), dtype=torch.int64, device=ctx.tdev)
    status = torch.zeros((n,), dtype=torch.int32, device=ctx.tdev)
    A, O, S = ctx.ptr(a), ctx.ptr(out), ctx.ptr(status)
    call = lambda op, arg, pa, pb, po, pst, count, h=ctx.h: lib.hb_debug_pair_op(h, op, arg, pa, pb, po, pst, count, st)
    BAD = _capi.HB_ERR_BAD_ARG
    assert call(OPS["FQ12_SQR"], 0, A, None, O, S, n) == _capi.HB_OK          # one operand: b may be null
    assert call(OPS["FQ12_MUL"], 0, A, A, O, S, n) == _capi.HB_OK             # a and b may be the same words
    assert status.cpu().tolist() == [1] * n
    for op in (-1, 20, 99):
        assert call(op, 0, A, A, O, S, n) == BAD
    assert call(OPS["FQ12_SQR"], 1, A, None, O, S, n) == BAD
    for arg in (0, 4):
        assert call(OPS["FQ12_FROBENIUS"], arg, A, None, O, S, n) == BAD
    for arg in (-1, 4, 0x40):
        assert call(FQ_OPS["FQ_MUL_LAZY"], arg, A, A, O, S, n) == BAD
    assert call(OPS["FQ12_SQR"], 0, A, None, O, S, -1) == BAD
    assert call(OPS["FQ12_SQR"], 0, None, None, O, S, n) == BAD
    assert call(OPS["FQ12_SQR"], 0, A, None, None, S, n) == BAD
    assert call(OPS["FQ12_SQR"], 0, A, None, O, None, n) == BAD
    assert call(OPS["FQ12_MUL"], 0, A, None, O, S, n) == BAD                  # the second operand is missing
    assert call(FQ_OPS["FQ_MUL"], 0, A, None, O, S, n) == BAD
    assert call(OPS["FQ12_SQR"], 0, None, None, None, None, 0) == _capi.HB_OK  # nothing to do, nothing launched
    assert call(OPS["FQ12_SQR"], 0, A, None, A, S, n) == BAD                  # out overlaps a
    assert call(OPS["FQ12_MUL"], 0, O, A, ctypes.c_void_p(out.data_ptr() + 576), S, n) == BAD
    assert call(OPS["FQ12_MUL"], 0, A, O, ctypes.c_void_p(out.data_ptr() + 576), S, n) == BAD      # ... or b
    assert call(OPS["FQ12_SQR"], 0, A, None, O, ctypes.c_void_p(out.data_ptr() + 64), n) == BAD    # the status inside the output
    assert call(OPS["FQ12_SQR"], 0, A, None, O, ctypes.c_void_p(a.data_ptr() + 64), n) == BAD
    assert call(OPS["FQ12_SQR"], 0, ctypes.c_void_p(a.data_ptr() + 8), None, O, S, 1) == BAD       # aligned to 8, not to 16
    assert call(OPS["FQ12_SQR"], 0, A, None, O, S, n, None) == BAD                                  # no context
    other = Context.get((1 << 255) - 19, n_limbs=4)                                                 # a context over another modulus
    assert call(OPS["FQ12_SQR"], 0, A, None, O, S, n, other.h) == BAD
    # the wire entry
    wire = lambda what, pi, po, pf, count, h=ctx.h: lib.hb_debug_g1_wire_op(h, what, pi, po, pf, count, st)
    assert wire(wc.SQRT, A, O, S, n) == _capi.HB_OK and wire(wc.PHI, A, O, None, n) == _capi.HB_OK
    for what in (wc.SUBGROUP, wc.DECOMPRESS, wc.COMPRESS, 5, -1):
        assert wire(what, A, O, S, n) == BAD
    assert wire(wc.SQRT, A, O, None, n) == BAD and wire(wc.SQRT, None, O, S, n) == BAD and wire(wc.PHI, A, None, None, n) == BAD
    assert wire(wc.SQRT, A, O, S, -1) == BAD and wire(wc.SQRT, None, None, None, 0) == _capi.HB_OK
    assert wire(wc.SQRT, A, A, S, n) == BAD and wire(wc.PHI, A, ctypes.c_void_p(a.data_ptr() + 96), None, n) == BAD
    assert wire(wc.SQRT, A, O, ctypes.c_void_p(out.data_ptr() + 32), n) == BAD
    assert wire(wc.PHI, ctypes.c_void_p(a.data_ptr() + 8), O, None, 1) == BAD
    assert wire(wc.SQRT, A, O, S, n, other.h) == BAD
    torch.cuda.synchronize()

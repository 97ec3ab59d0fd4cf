"""Drivers of the host self tests of csrc/hb_lt.hip, hb_eq.hip, hb_jj.hip, hb_ew.hip, hb_off.hip, hb_mimc.hip and hb_bf.hip over lists
of Python ints, shared by the host suites (test_less_than_host.py, test_share_comparison_host.py, test_jubjub_host.py,
test_share_arithmetic_host.py, test_offline_host.py, test_mimc_host.py, test_butterfly_network_host.py) and by the GPU suites, which
hold every device step bit-equal to the self test of the same row.  Every operand and output is a buffer of exactly the documented
size (one element where the size is zero), so a row that reads or writes a row too far does not stay inside its array."""
import ctypes

import numpy as np


def _operands(operands, p, nb, slots):
    from honeybadgermpc_amd._capi import ints_to_limbs

    arrays = [None if o is None else ints_to_limbs(list(o) or [0], p, nb) for o in operands]
    return arrays, (ctypes.c_void_p * slots)(*([None if x is None else x.ctypes.data for x in arrays] + [None] * (slots - len(arrays))))


def run_lt(p, nl, what, operands, mode, out_rows, count, L=None):
    """hb_selftest_lt over lists of ints (None: a NULL operand; arrays of several rows are flat, row-major).  out_rows: rows of
    elements of each output -> (rc, [out lists])"""
    from honeybadgermpc_amd._capi import ints_to_limbs, limbs_to_ints, load_library, np_ptr

    lib = load_library()
    nb = 8 * nl
    arrays, ptrs = _operands(operands, p, nb, 12)
    outs = [np.zeros((max(r * count, 1), nl), dtype=np.uint64) for r in out_rows]
    optrs = (ctypes.c_void_p * 3)(*([o.ctypes.data for o in outs] + [None] * (3 - len(outs))))
    prm = (ctypes.c_int64 * 2)(p.bit_length() if L is None else L, mode)
    rc = lib.hb_selftest_lt(np_ptr(ints_to_limbs([p], p + 1, nb)), nl, what, ptrs, prm, optrs, count)
    return rc, [limbs_to_ints(o[:r * count], nb) for o, r in zip(outs, out_rows)]


def run_eq(p, nl, what, operands, rows, mode, out_rows, count):
    """hb_selftest_eq over lists of ints (None: a NULL operand; arrays of several rows are flat, row-major).  out_rows: rows of
    elements of each output, "i8" for the Legendre symbols, "zr" for zero_rows -> (rc, [out lists])"""
    from honeybadgermpc_amd._capi import ints_to_limbs, limbs_to_ints, load_library, np_ptr

    lib = load_library()
    nb = 8 * nl
    arrays, ptrs = _operands(operands, p, nb, 12)
    outs = []
    for r in out_rows:
        if r == "i8":
            outs.append(np.full(max(count, 1), 7, dtype=np.int8))
        elif r == "zr":
            outs.append(np.zeros(max(rows, 1), dtype=np.int32))
        else:
            outs.append(np.zeros((max(r * count, 1), nl), dtype=np.uint64))
    optrs = (ctypes.c_void_p * 2)(*([o.ctypes.data for o in outs] + [None] * (2 - len(outs))))
    prm = (ctypes.c_int64 * 2)(rows, mode)
    rc = lib.hb_selftest_eq(np_ptr(ints_to_limbs([p], p + 1, nb)), nl, what, ptrs, prm, optrs, count)
    res = []
    for o, r in zip(outs, out_rows):
        res.append(o[:count].tolist() if r == "i8" else (o[:rows].tolist() if r == "zr" else limbs_to_ints(o[:r * count], nb)))
    return rc, res


def run_jj(p, nl, what, operands, count, out_rows, a=None, d=None, flags=0, arg=0):
    """hb_selftest_jj over lists of ints (None: a NULL operand) -> (rc, [rows of `count` ints])"""
    from honeybadgermpc_amd._capi import ints_to_limbs, limbs_to_ints, load_library, np_ptr

    lib = load_library()
    nb = 8 * nl
    arrays, ptrs = _operands(operands, p, nb, 6)
    consts = [None if v is None else ints_to_limbs([v], v + 1, nb) for v in (a, d)]
    out = np.zeros((max(count * out_rows, 1), nl), dtype=np.uint64)
    rc = lib.hb_selftest_jj(np_ptr(ints_to_limbs([p], p + 1, nb)), nl, what, ptrs, *[None if c is None else np_ptr(c) for c in consts], flags, arg, np_ptr(out), count)
    flat = limbs_to_ints(out[:count * out_rows], nb)
    return rc, [flat[r * count:(r + 1) * count] for r in range(out_rows)]


def run_ew(p, nl, what, operands, count, extra=None):
    """hb_selftest_ew over lists of ints (a broadcast b is its one element) -> list of ints; extra: the array operand slot 1 points at
    (the inversion's count of zeros)"""
    from honeybadgermpc_amd._capi import ints_to_limbs, limbs_to_ints, load_library, np_ptr

    lib = load_library()
    nb = 8 * nl
    arrays = [ints_to_limbs(list(o), p, nb) for o in operands]
    ptrs = (ctypes.c_void_p * 5)(*[a.ctypes.data for a in arrays])
    if extra is not None:
        ptrs[1] = extra.ctypes.data
    out = np.zeros((max(count, 1), nl), dtype=np.uint64)
    rc = lib.hb_selftest_ew(np_ptr(ints_to_limbs([p], p + 1, nb)), nl, what, ptrs, np_ptr(out), count)
    assert rc == 0, rc
    return limbs_to_ints(out[:count], nb)


def run_off(p, nl, what, ptrs, out, count):
    """hb_selftest_off over raw addresses (None: a NULL operand): the callers own the arrays, which may be one another's -> rc"""
    from honeybadgermpc_amd._capi import ints_to_limbs, load_library, np_ptr

    ops = (ctypes.c_void_p * 3)(*(list(ptrs) + [None] * (3 - len(ptrs))))
    return load_library().hb_selftest_off(np_ptr(ints_to_limbs([p], p + 1, 8 * nl)), nl, what, ops, out, count)


def run_off_mul_add(p, nl, a, b, c, b_is_a=False, out_is=None):
    """a b + c by hb_selftest_off -> (rc, out); b_is_a: the b pointer is a's; out_is: 0, 1 or 2 -- the output pointer is that operand's"""
    from honeybadgermpc_amd._capi import ints_to_limbs, limbs_to_ints

    count = len(a)
    arrs = [ints_to_limbs(list(v) or [0], p, 8 * nl) for v in (a, b, c)]
    if b_is_a:
        arrs[1] = arrs[0]
    out = arrs[out_is] if out_is is not None else np.zeros((max(count, 1), nl), dtype=np.uint64)
    rc = run_off(p, nl, 0, [x.ctypes.data for x in arrs], out.ctypes.data, count)
    return rc, limbs_to_ints(out[:count], 8 * nl) if count else []


def run_mimc(p, nl, what, operands, count, arg=0, start=None, bcast=0, flags=0):
    """hb_selftest_mimc over lists of ints (None: a NULL operand; a key for all is its one element) -> (rc, list of ints)"""
    from honeybadgermpc_amd._capi import ints_to_limbs, limbs_to_ints, load_library, np_ptr

    lib = load_library()
    nb = 8 * nl
    arrays, ptrs = _operands(operands, p, nb, 6)
    st = None if start is None else ints_to_limbs([start], start + 1, nb)
    out = np.zeros((max(count, 1), nl), dtype=np.uint64)
    rc = lib.hb_selftest_mimc(np_ptr(ints_to_limbs([p], p + 1, nb)), nl, what, ptrs, None if st is None else np_ptr(st), bcast, flags, arg, np_ptr(out), count)
    return rc, limbs_to_ints(out[:count], nb)


def run_bf(p, nl, what, operands, k, a, n_out):
    """hb_selftest_bf over lists of ints (None: a NULL operand) -> (rc, list of n_out ints)"""
    from honeybadgermpc_amd._capi import ints_to_limbs, limbs_to_ints, load_library, np_ptr

    lib = load_library()
    nb = 8 * nl
    arrays, ptrs = _operands(operands, p, nb, 6)
    out = np.zeros((max(n_out, 1), nl), dtype=np.uint64)
    rc = lib.hb_selftest_bf(np_ptr(ints_to_limbs([p], p + 1, nb)), nl, what, ptrs, k, a, np_ptr(out))
    return rc, limbs_to_ints(out[:n_out], nb)

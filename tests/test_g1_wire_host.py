"""The bodies of csrc/hb_g1_wire.hip on the host, through hb_selftest_g1_wire: decompression, compression, the membership test by the
endomorphism, and the bare square root and phi.  No GPU.  Every comparison is exact equality of words or bytes against the host model
honeybadgermpc_amd.bls12_381.G1 (cases and labels: g1_wire_cases)."""
import os
import random
import re

import numpy as np

import g1_support as s
import g1_wire_cases as wc
from conftest import REPO

from honeybadgermpc_amd.bls12_381 import G1, GX, GY, Q, R


def test_valid_vectors_decompress_to_the_models_words_and_compress_back():
    v = wc.vector_bytes()
    pts, status, rejected = wc.host_decompress(v)
    assert status.tolist() == [wc.OK] * 1000 and rejected == 0
    assert np.array_equal(pts, wc.vector_points())
    assert not pts[0].any()                                              # vector 0 is the identity
    assert wc.host_compress(wc.vector_points()) == v
    assert wc.host_compress(pts) == v


def test_valid_vectors_pass_the_subgroup_check_inside_decompression():
    n = 48
    v = wc.vector_bytes()[:n * wc.ENC]
    assert all(p.in_subgroup() for p in s.vectors()[:n])
    pts, status, rejected = wc.host_decompress(v, check_subgroup=True)
    assert status.tolist() == [wc.OK] * n and rejected == 0
    assert np.array_equal(pts, wc.vector_points()[:n])


def test_malformed_encodings_take_the_models_label():
    names = [name for name, _ in wc.malformed()]
    data = b"".join(enc for _, enc in wc.malformed())
    for check in (False, True):
        want_status, want_pts = wc.malformed_labels(check)
        pts, status, rejected = wc.host_decompress(data, check_subgroup=check)
        assert status.tolist() == want_status, [(n, g, w) for n, g, w in zip(names, status.tolist(), want_status) if g != w]
        assert np.array_equal(pts, want_pts)
        assert rejected == sum(1 for st in want_status if st)
        assert not pts[status != 0].any()
    # the table holds every status, and the first failed check wins
    plain, checked = wc.malformed_labels(False)[0], wc.malformed_labels(True)[0]
    assert set(plain) == {0, 1, 2, 3, 4} and set(checked) >= {1, 2, 3, 4, 5}
    assert all(c == (wc.NOT_IN_SUBGROUP if p == wc.OK else p) for p, c in zip(plain, checked))    # none of these x belongs to a member
    by_name = dict(zip(names, plain))
    assert by_name["0x40 alone"] == wc.NOT_COMPRESSED and by_name["0xC0 with a non-zero last byte"] == wc.BAD_IDENTITY
    assert by_name["0xE0 followed by zeros"] == wc.BAD_IDENTITY
    assert by_name["x = Q"] == by_name["x = Q + 1"] == by_name["the 381 low bits all set"] == wc.X_NOT_BELOW_Q


def test_x_zero_is_a_point_of_order_three_not_the_identity():
    data = wc.encode_x(0, 4) + wc.encode_x(0, 5)
    pts, status, rejected = wc.host_decompress(data)
    assert status.tolist() == [0, 0] and rejected == 0
    assert pts.tolist() == [s.raw_point(0, 2), s.raw_point(0, Q - 2)]
    assert (G1(0, 2) ** 3).is_one()
    pts, status, rejected = wc.host_decompress(data, check_subgroup=True)
    assert status.tolist() == [wc.NOT_IN_SUBGROUP] * 2 and rejected == 2 and not pts.any()
    assert wc.host_compress(np.array([s.raw_point(0, 2), s.raw_point(0, Q - 2)], dtype=np.uint64)) == data


def test_membership_flags_equal_the_models_in_subgroup():
    rows, want = wc.subgroup_set()
    assert wc.host_subgroup(rows) == want
    assert sum(want) == 9 and len(want) == 9 + 82 + 4                    # the identity and eight multiples of the generator; nothing else


def test_square_root_of_squares_and_non_residues():
    rnd = random.Random(379)
    roots = [0, 1, Q - 1, 2, (Q - 1) // 2, (Q + 1) // 2] + [rnd.randrange(Q) for _ in range(300)]
    squares = [r * r % Q for r in roots]
    got, flags = wc.host_sqrt(squares)
    assert flags == [1] * len(squares)
    assert got == [pow(a, (Q + 1) // 4, Q) for a in squares]
    assert all(g in (r, (Q - r) % Q) for g, r in zip(got, roots))
    # Q = 3 mod 4: -1 is no square, so neither is the negative of a non-zero square
    non = [Q - 1 if a == 0 else Q - a for a in squares[:40]]
    assert all(pow(a, (Q - 1) // 2, Q) == Q - 1 for a in non)
    got, flags = wc.host_sqrt(non)
    assert flags == [0] * len(non) and got == [0] * len(non)


def test_phi_has_order_three_and_acts_as_minus_x_squared_on_the_generator():
    g = G1.generator()
    pts = s.points([g, g ** 7, G1.one(), wc.lifted()[0], s.vectors()[9]])
    once = wc.host_phi(pts)
    assert np.array_equal(wc.host_phi(wc.host_phi(once)), pts)
    assert not np.array_equal(once[:2], pts[:2]) and not once[2].any()
    assert once[0].tolist() == s.raw_point(wc.BETA * GX % Q, GY)
    assert G1.from_limbs(once[0].tolist()) == (g ** (wc.X * wc.X % R)).invert()
    other = wc.BETA * wc.BETA % Q                                        # the other non-trivial cube root of unity fails
    assert pow(wc.BETA, 3, Q) == 1 and G1(other * GX % Q, GY) != (g ** (wc.X * wc.X % R)).invert()


def test_selftest_refuses_bad_arguments():
    import ctypes

    from honeybadgermpc_amd._capi import load_library

    lib = load_library()
    src, out = wc.aligned(96 + 16), wc.aligned(256)
    ptrs = (ctypes.c_void_p * 1)(src.ctypes.data)
    call = lambda what, flags, arg, p, o: lib.hb_selftest_g1_wire(what, p, flags, arg, ctypes.c_void_p(o), 1)
    assert call(wc.SUBGROUP, 0, 0, ptrs, out.ctypes.data) == 0
    assert call(9, 0, 0, ptrs, out.ctypes.data) != 0
    assert call(wc.SUBGROUP, 1, 0, ptrs, out.ctypes.data) != 0
    assert call(wc.DECOMPRESS, 2, 0, ptrs, out.ctypes.data) != 0
    assert call(wc.SUBGROUP, 0, 1, ptrs, out.ctypes.data) != 0
    assert call(wc.SUBGROUP, 0, 0, ptrs, out.ctypes.data + 8) != 0       # aligned to 8, not to 16
    assert call(wc.SUBGROUP, 0, 0, (ctypes.c_void_p * 1)(src.ctypes.data + 4), out.ctypes.data) != 0
    assert call(wc.SUBGROUP, 0, 0, (ctypes.c_void_p * 1)(None), out.ctypes.data) != 0
    rc, _ = wc.selftest(wc.SQRT, s.words([Q], 6), 0, 1, 52)              # a residue not below Q
    assert rc != 0


def test_status_constants_mirror_the_header():
    from honeybadgermpc_amd import _capi, g1

    text = open(os.path.join(REPO, "include", "hbmpc_hip.h")).read()
    header = dict((name, int(value)) for name, value in re.findall(r"#define (HB_G1_WIRE_[A-Z_]+) (\d+)", text))
    names = ["OK", "NOT_COMPRESSED", "BAD_IDENTITY", "X_NOT_BELOW_Q", "NOT_ON_CURVE", "NOT_IN_SUBGROUP"]
    for code, name in enumerate(names):
        assert header["HB_G1_WIRE_" + name] == code == getattr(g1, "STATUS_" + name) == getattr(_capi, "HB_G1_WIRE_" + name) == getattr(wc, name)
    for code, name in enumerate(["SUBGROUP", "DECOMPRESS", "COMPRESS", "SQRT", "PHI"]):
        assert header["HB_G1_WIRE_SELFTEST_" + name] == code == getattr(_capi, "HB_G1_WIRE_SELFTEST_" + name) == getattr(wc, name)
    for name in ("hb_g1_subgroup", "hb_g1_decompress", "hb_g1_compress", "hb_selftest_g1_wire"):
        assert re.search(r"\bint " + name + r"\s*\(", text) and name in _capi.SYMBOLS

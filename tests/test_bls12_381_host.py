"""CPU-only: the host model honeybadgermpc_amd.bls12_381 (Python ints) against tests/golden/g1_compressed_valid_test_vectors.dat, the data
file of that name of the reference's Rust pairing crate (pairing/src/bls12_381/tests/): k * G for k = 0..999, 48 bytes each.  Exact."""
import os
import random

import pytest

from conftest import BLS, GOLDEN

from honeybadgermpc_amd import bls12_381 as bls
from honeybadgermpc_amd.bls12_381 import G1, GX, GY, H, Q, R
from honeybadgermpc_amd.field import GF


def vectors():
    with open(os.path.join(GOLDEN, "g1_compressed_valid_test_vectors.dat"), "rb") as f:
        data = f.read()
    assert len(data) == 48000
    return [data[48 * k:48 * k + 48] for k in range(1000)]


def off_subgroup_point():
    """a curve point that is NOT in the subgroup: the first x >= 1 with x^3 + 4 a square, cofactor not cleared"""
    x = 1
    while True:
        p = G1.lift_x(x)
        if p is not None and not p.in_subgroup():
            return p
        x += 1


def test_constants():
    assert R == BLS and Q % 4 == 3 and Q.bit_length() == 381
    assert H * R == Q + 1 - (bls.X_PARAM + 1)
    assert (GY * GY - GX ** 3 - 4) % Q == 0
    g = G1.generator()
    assert g.on_curve() and g.in_subgroup()
    assert G1._from_jac(bls._jac_mul(g._j, R)).is_one()             # R * G, the exponent NOT reduced
    assert not G1._from_jac(bls._jac_mul(g._j, R - 1)).is_one() and pow(g, R - 1) * g == G1.one()


def test_vectors_decompress_and_compress():
    vs = vectors()
    assert vs[0][0] >> 5 == 0b110 and not any(vs[0][1:]) and vs[0][0] & 0x1F == 0
    g, acc = G1.generator(), G1.one()
    for k, v in enumerate(vs):
        p = G1.decompress(v)
        assert p == acc and p.compress() == v and acc.compress() == v, k
        if k:
            assert int.from_bytes(bytes([v[0] & 0x1F]) + v[1:], "big") == acc.x
            assert bool(v[0] & 0x20) == (acc.y > (Q - 1) // 2)
        acc = acc * g
    assert G1.decompress(vs[999]) == g ** 999


def test_group_laws():
    rnd = random.Random(3)
    g, one = G1.generator(), G1.one()
    a, b, c = (g ** rnd.randrange(R) for _ in range(3))
    assert a * b == b * a and (a * b) * c == a * (b * c)
    assert a * one == a and one * a == a and one * one == one
    assert a * a == a ** 2 and a * a.invert() == one and a / a == one and a / b == a * b.invert()
    assert one.invert() == one and a.invert().invert() == a
    k, m = rnd.randrange(R), rnd.randrange(R)
    assert (a ** k) ** m == a ** (k * m % R) and a ** k * a ** m == a ** (k + m)
    assert a.duplicate() == a and a.duplicate() is not a and hash(a.duplicate()) == hash(a) and hash(a ** 2) == hash(a * a)
    assert a != b and a != one and not (a == 5)
    assert (g ** R) == one and g ** 0 == one and g ** 1 == g


def test_pow_exponents():
    g = G1.generator()
    f = GF(R)
    assert g ** -1 == g.invert() and g ** -5 == (g ** 5).invert() and pow(g, -R) == G1.one() and g ** (R + 3) == g ** 3
    assert pow(g, f(12345)) == g ** 12345 and g ** f(-2) == g ** (R - 2)
    with pytest.raises(TypeError):
        g ** 1.5
    with pytest.raises(TypeError):
        pow(g, 3, 7)


def test_cofactor_clearing_and_subgroup():
    p = off_subgroup_point()
    assert p.on_curve() and not p.in_subgroup()
    assert not G1._from_jac(bls._jac_mul(p._j, R)).is_one()
    c = p.clear_cofactor()
    assert c.on_curve() and c.in_subgroup() and not c.is_one()
    assert G1._from_jac(bls._jac_mul(p._j, H * R)).is_one()
    with pytest.raises(ValueError):
        G1.decompress(p.compress(), check_subgroup=True)
    assert G1.decompress(p.compress()) == p


def test_rand():
    a, b = G1.rand(1), G1.rand(2)
    assert a == G1.rand(1) and a != b and a.in_subgroup() and b.in_subgroup() and not a.is_one()
    assert G1.rand([1, 2, 3, 4]) == G1.rand([1, 2, 3, 4]) and G1.rand(b"x") != G1.rand(b"y")
    assert G1.rand().in_subgroup()


def test_refuses_points_off_the_curve():
    with pytest.raises(ValueError):
        G1(GX, GY + 1)
    with pytest.raises(ValueError):
        G1(0, 0)
    with pytest.raises(ValueError):
        G1(GX + Q, GY)
    with pytest.raises(ValueError):
        G1.from_limbs([1] + [0] * 11)
    x = 1
    while G1.lift_x(x) is not None:
        x += 1
    raw = bytearray(x.to_bytes(48, "big"))
    raw[0] |= 0x80
    with pytest.raises(ValueError):
        G1.decompress(bytes(raw))                       # no point has this x
    with pytest.raises(ValueError):
        G1.decompress(bytes(48))                        # compression flag missing
    with pytest.raises(ValueError):
        G1.decompress(bytes([0xE0]) + bytes(47))        # identity with a sign flag
    with pytest.raises(ValueError):
        G1.decompress(bytes([0x9F]) + bytes([0xFF]) * 47)   # x >= Q
    with pytest.raises(ValueError):
        G1.decompress(bytes(47))


def test_limbs_round_trip():
    g = G1.generator()
    for p in (G1.one(), g, g ** 77, off_subgroup_point()):
        limbs = p.to_limbs()
        assert len(limbs) == 12 and all(0 <= v < 1 << 64 for v in limbs) and G1.from_limbs(limbs) == p
    assert G1.one().to_limbs() == [0] * 12

"""
The group G1 of BLS12-381 on Python ints: the host model the kernels of csrc/hb_g1.hip are checked against, with the multiplicative
surface of the reference's betterpairing.G1 as poly_commit_lin.py and hbavss.py use it (`a * b`, `a / b`, `a ** k`, `G1.one()`,
`G1.rand()`), the 48-byte compressed encoding of the reference's Rust crate, and the limb form of the tensor API (g1.py).

    E: y^2 = x^3 + 4 over GF(Q),   #E = H * R,   G1 = the subgroup of order R = Subgroup.BLS12_381

No device is needed.  Points are kept in Jacobian coordinates (X : Y : Z), x = X / Z^2, y = Y / Z^3, Z = 0 the identity, so that a
test can afford a few thousand scalar multiplications; `x`, `y` normalise on demand.
"""
import hashlib

from .elliptic_curve import Subgroup

Q = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R = Subgroup.BLS12_381
B = 4
H = 0x396C8C005555E1568C00AAAB0000AAAB
X_PARAM = -0xD201000000010000
GX = 0x17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB
GY = 0x08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1
LIMBS = 6          # 64-bit words a coordinate in the tensor form
COMPRESSED_BYTES = 48

assert Q % 4 == 3 and H * R == Q + 1 - (X_PARAM + 1)


def _jac_double(p):
    X, Y, Z = p
    if Z == 0:
        return p
    A = X * X % Q
    Bq = Y * Y % Q
    C = Bq * Bq % Q
    D = 2 * ((X + Bq) * (X + Bq) - A - C) % Q
    E = 3 * A % Q
    X3 = (E * E - 2 * D) % Q
    return X3, (E * (D - X3) - 8 * C) % Q, 2 * Y * Z % Q


def _jac_add(p, q):
    X1, Y1, Z1 = p
    X2, Y2, Z2 = q
    if Z1 == 0:
        return q
    if Z2 == 0:
        return p
    Z1Z1, Z2Z2 = Z1 * Z1 % Q, Z2 * Z2 % Q
    U1, U2 = X1 * Z2Z2 % Q, X2 * Z1Z1 % Q
    S1, S2 = Y1 * Z2 * Z2Z2 % Q, Y2 * Z1 * Z1Z1 % Q
    Hh, r = (U2 - U1) % Q, (S2 - S1) % Q
    if Hh == 0:
        return _jac_double(p) if r == 0 else (1, 1, 0)
    HH = Hh * Hh % Q
    HHH = Hh * HH % Q
    V = U1 * HH % Q
    X3 = (r * r - HHH - 2 * V) % Q
    return X3, (r * (V - X3) - S1 * HHH) % Q, Z1 * Z2 * Hh % Q


def _jac_mul(p, k):
    acc = (1, 1, 0)
    for bit in bin(k)[2:] if k else "":
        acc = _jac_double(acc)
        if bit == "1":
            acc = _jac_add(acc, p)
    return acc


def _exponent(k):
    if isinstance(k, (bool, float)) or not (isinstance(k, int) or hasattr(k, "__int__")):
        raise TypeError(f"exponent: expected an int or a field element, got {type(k).__name__}")
    return int(k) % R


class G1:
    """An element of E(GF(Q)), written multiplicatively as the reference's betterpairing.G1 is.  Construct with affine
    coordinates (`G1(x, y)`), or through one(), generator(), rand(), decompress(), from_limbs(); a point off the curve is refused."""

    __slots__ = ("_j", "_aff")

    def __init__(self, x, y):
        x, y = int(x), int(y)
        if not (0 <= x < Q and 0 <= y < Q):
            raise ValueError("G1: coordinates must be residues below Q")
        if (y * y - x * x * x - B) % Q:
            raise ValueError("G1: the point is not on the curve y^2 = x^3 + 4")
        self._j = (x, y, 1)
        self._aff = (x, y)

    @classmethod
    def _from_jac(cls, j):
        p = object.__new__(cls)
        p._j = j
        p._aff = None
        return p

    # ---- constructors
    @classmethod
    def one(cls):
        return cls._from_jac((1, 1, 0))

    identity = one

    @classmethod
    def generator(cls):
        return cls(GX, GY)

    @classmethod
    def rand(cls, seed=None):
        """A point of the subgroup derived from `seed` (an int, bytes, str or a list of ints; None: from os.urandom): hash the seed
        to an x, step x until x^3 + 4 is a square, take the root with exponent (Q + 1) / 4 and clear the cofactor.  The reference's
        own G1.rand lives in its Rust crate (a ChaCha stream over the seed words) and cannot be reproduced here: the points differ
        from the reference's for the same seed, which no caller relies on -- a CRS is made once and shared."""
        if seed is None:
            import os

            data = os.urandom(64)
        elif isinstance(seed, (bytes, bytearray)):
            data = bytes(seed)
        else:
            data = repr(seed).encode()
        x = int.from_bytes(hashlib.sha512(b"hbmpc-g1-rand" + data).digest(), "big") % Q
        while True:
            p = cls.lift_x(x)
            if p is not None:
                p = p.clear_cofactor()
                if not p.is_one():
                    return p
            x = (x + 1) % Q

    @classmethod
    def lift_x(cls, x, greatest=False):
        """the curve point with this x whose y is the smaller (or the greater) root, None if x^3 + 4 is not a square.  NOT
        necessarily in the subgroup."""
        rhs = (x * x * x + B) % Q
        y = pow(rhs, (Q + 1) // 4, Q)
        if y * y % Q != rhs:
            return None
        if (y > (Q - 1) // 2) != bool(greatest):
            y = (Q - y) % Q
        return cls(x, y)

    # ---- coordinates
    def _affine(self):
        if self._aff is None:
            X, Y, Z = self._j
            if Z == 0:
                self._aff = (0, 0)
            else:
                zi = pow(Z, Q - 2, Q)
                zi2 = zi * zi % Q
                self._aff = (X * zi2 % Q, Y * zi2 * zi % Q)
        return self._aff

    @property
    def x(self):
        return self._affine()[0]

    @property
    def y(self):
        return self._affine()[1]

    def is_one(self):
        return self._j[2] == 0

    def on_curve(self):
        if self.is_one():
            return True
        x, y = self._affine()
        return (y * y - x * x * x - B) % Q == 0

    def in_subgroup(self):
        return G1._from_jac(_jac_mul(self._j, R)).is_one()

    def clear_cofactor(self):
        return G1._from_jac(_jac_mul(self._j, H))

    # ---- the group, written multiplicatively
    def __mul__(self, other):
        if not isinstance(other, G1):
            return NotImplemented
        return G1._from_jac(_jac_add(self._j, other._j))

    def invert(self):
        X, Y, Z = self._j
        return G1._from_jac((X, (Q - Y) % Q, Z))

    def __truediv__(self, other):
        if not isinstance(other, G1):
            return NotImplemented
        return self * other.invert()

    def __pow__(self, k, modulus=None):
        if modulus is not None:
            raise TypeError("G1: pow() takes no modulus")
        return G1._from_jac(_jac_mul(self._j, _exponent(k)))

    def duplicate(self):
        return G1._from_jac(self._j)

    def __eq__(self, other):
        if not isinstance(other, G1):
            return NotImplemented
        X1, Y1, Z1 = self._j
        X2, Y2, Z2 = other._j
        if Z1 == 0 or Z2 == 0:
            return Z1 == 0 and Z2 == 0
        a, b = Z1 * Z1 % Q, Z2 * Z2 % Q
        return (X1 * b - X2 * a) % Q == 0 and (Y1 * b * Z2 - Y2 * a * Z1) % Q == 0

    def __hash__(self):
        return hash(self._affine() + (self.is_one(),))

    def __repr__(self):
        return "G1.one()" if self.is_one() else f"G1({hex(self.x)}, {hex(self.y)})"

    # ---- serialisation
    def compress(self):
        """48 bytes as the reference's Rust crate writes them: big-endian x; in byte 0, 0x80 always set (compressed), 0x40 the
        identity (x = 0), 0x20 set when y > (Q - 1) / 2."""
        if self.is_one():
            return bytes([0xC0]) + bytes(COMPRESSED_BYTES - 1)
        x, y = self._affine()
        raw = bytearray(x.to_bytes(COMPRESSED_BYTES, "big"))
        raw[0] |= 0x80 | (0x20 if y > (Q - 1) // 2 else 0)
        return bytes(raw)

    @classmethod
    def decompress(cls, data, check_subgroup=False):
        data = bytes(data)
        if len(data) != COMPRESSED_BYTES:
            raise ValueError(f"G1.decompress: expected {COMPRESSED_BYTES} bytes, got {len(data)}")
        flags = data[0] >> 5
        if not flags & 4:
            raise ValueError("G1.decompress: the compression flag is not set")
        x = int.from_bytes(bytes([data[0] & 0x1F]) + data[1:], "big")
        if flags & 2:
            if x or flags & 1:
                raise ValueError("G1.decompress: the identity carries a non-zero x or a sign flag")
            return cls.one()
        if x >= Q:
            raise ValueError("G1.decompress: x is not below Q")
        p = cls.lift_x(x, greatest=bool(flags & 1))
        if p is None:
            raise ValueError("G1.decompress: x is not the abscissa of a curve point")
        if check_subgroup and not p.in_subgroup():
            raise ValueError("G1.decompress: the point is not in the subgroup")
        return p

    def to_limbs(self):
        """-> 12 ints below 2^64: x then y, little-endian words; the identity is all zeros ((0, 0) is not on the curve)"""
        x, y = self._affine()
        return [(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for v in (x, y) for k in range(LIMBS)]

    @classmethod
    def from_limbs(cls, limbs):
        limbs = [int(v) & 0xFFFFFFFFFFFFFFFF for v in limbs]
        if len(limbs) != 2 * LIMBS:
            raise ValueError(f"G1.from_limbs: expected {2 * LIMBS} words, got {len(limbs)}")
        x = sum(v << (64 * k) for k, v in enumerate(limbs[:LIMBS]))
        y = sum(v << (64 * k) for k, v in enumerate(limbs[LIMBS:]))
        return cls.one() if x == 0 and y == 0 else cls(x, y)

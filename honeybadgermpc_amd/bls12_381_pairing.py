"""
The pairing of BLS12-381 on Python ints: the host model the kernels of csrc/hb_pair.hip are checked against.  The tower, the twist and
the ate loop are those of the reference's Rust crate (pairing/src/bls12_381), so that a value after the final exponentiation equals
the crate's word for word:

    Fq2 = Fq[u] / (u^2 + 1),   Fq6 = Fq2[v] / (v^3 - (1 + u)),   Fq12 = Fq6[w] / (w^2 - v)
    E': y^2 = x^3 + 4 (1 + u) over Fq2, the twist G2 lives on
    e(P, Q) = FE(ML(P, Q)),  ML the ate loop over |x| = 0xd201000000010000, FE the power 3 (Q^12 - 1) / R

The factor 3 is the crate's: its final_exponentiation chain (easy part, then five powers by |x|) computes f^(3 (Q^12 - 1) / R), and the
value recorded in its test_pairing_result_against_relic is that power.  Verdicts (== 1) do not depend on it, GT values do.

Coordinate order of an Fq12, everywhere: c0.c0.c0, c0.c0.c1, c0.c1.c0, ..., c1.c2.c1 (twelve residues below Q).

prepare_g2(Q) gives the 68 line coefficients of the loop (63 doublings, 5 additions, in the order the loop reads them): the verifier's
G2 arguments are fixed by the CRS, so the device never does G2 arithmetic.  An Fq2 scaling of a triple changes a Miller value by a
factor the final exponentiation kills; raw Miller values are therefore not part of any interface.

Out of scope: compressed G2 (a square root in Fq2) and G2.rand.  No device is needed.
"""
from .bls12_381 import G1, Q, R, _exponent

BLS_X = 0xD201000000010000
G2_UNCOMPRESSED_BYTES = 192
N_LINES = 68


class Fq2:
    __slots__ = ("c0", "c1")

    def __init__(self, c0, c1=0):
        self.c0, self.c1 = int(c0) % Q, int(c1) % Q

    @classmethod
    def one(cls):
        return cls(1, 0)

    @classmethod
    def zero(cls):
        return cls(0, 0)

    def __add__(self, o):
        return Fq2(self.c0 + o.c0, self.c1 + o.c1)

    def __sub__(self, o):
        return Fq2(self.c0 - o.c0, self.c1 - o.c1)

    def __neg__(self):
        return Fq2(-self.c0, -self.c1)

    def __mul__(self, o):
        if isinstance(o, int):
            return Fq2(self.c0 * o, self.c1 * o)
        a0, a1, b0, b1 = self.c0, self.c1, o.c0, o.c1
        return Fq2(a0 * b0 - a1 * b1, a0 * b1 + a1 * b0)

    def square(self):
        a0, a1 = self.c0, self.c1
        return Fq2((a0 + a1) * (a0 - a1), 2 * a0 * a1)

    def mul_by_nonresidue(self):
        """times 1 + u"""
        return Fq2(self.c0 - self.c1, self.c0 + self.c1)

    def conjugate(self):
        return Fq2(self.c0, -self.c1)

    def frobenius_map(self, power):
        return self.conjugate() if power & 1 else Fq2(self.c0, self.c1)

    def inverse(self):
        t = pow(self.c0 * self.c0 + self.c1 * self.c1, Q - 2, Q)
        return Fq2(self.c0 * t, -self.c1 * t)

    def pow(self, e):
        acc, base = Fq2.one(), self
        while e:
            if e & 1:
                acc = acc * base
            base = base.square()
            e >>= 1
        return acc

    def is_zero(self):
        return self.c0 == 0 and self.c1 == 0

    def __eq__(self, o):
        return isinstance(o, Fq2) and self.c0 == o.c0 and self.c1 == o.c1

    def __hash__(self):
        return hash((self.c0, self.c1))

    def coords(self):
        return [self.c0, self.c1]

    def __repr__(self):
        return f"Fq2({hex(self.c0)}, {hex(self.c1)})"


XI = Fq2(1, 1)
# the Frobenius constants, by exponentiation of 1 + u: gamma_k[i] = (1 + u)^(k (Q^i - 1) / 6)
FROBENIUS_FQ6_C1 = [XI.pow((Q ** i - 1) // 3) for i in range(6)]
FROBENIUS_FQ6_C2 = [XI.pow((2 * Q ** i - 2) // 3) for i in range(6)]
FROBENIUS_FQ12_C1 = [XI.pow((Q ** i - 1) // 6) for i in range(12)]


class Fq6:
    __slots__ = ("c0", "c1", "c2")

    def __init__(self, c0, c1=None, c2=None):
        self.c0, self.c1, self.c2 = c0, Fq2.zero() if c1 is None else c1, Fq2.zero() if c2 is None else c2

    @classmethod
    def one(cls):
        return cls(Fq2.one())

    @classmethod
    def zero(cls):
        return cls(Fq2.zero())

    def __add__(self, o):
        return Fq6(self.c0 + o.c0, self.c1 + o.c1, self.c2 + o.c2)

    def __sub__(self, o):
        return Fq6(self.c0 - o.c0, self.c1 - o.c1, self.c2 - o.c2)

    def __neg__(self):
        return Fq6(-self.c0, -self.c1, -self.c2)

    def __mul__(self, o):
        a0, a1, a2, b0, b1, b2 = self.c0, self.c1, self.c2, o.c0, o.c1, o.c2
        aa, bb, cc = a0 * b0, a1 * b1, a2 * b2
        t0 = ((a1 + a2) * (b1 + b2) - bb - cc).mul_by_nonresidue() + aa
        t1 = (a0 + a1) * (b0 + b1) - aa - bb + cc.mul_by_nonresidue()
        t2 = (a0 + a2) * (b0 + b2) - aa - cc + bb
        return Fq6(t0, t1, t2)

    def square(self):
        return self * self

    def mul_by_nonresidue(self):
        """times v"""
        return Fq6(self.c2.mul_by_nonresidue(), self.c0, self.c1)

    def mul_by_1(self, c1):
        return Fq6((self.c2 * c1).mul_by_nonresidue(), self.c0 * c1, self.c1 * c1)

    def mul_by_01(self, c0, c1):
        aa, bb = self.c0 * c0, self.c1 * c1
        t1 = (self.c2 * c1).mul_by_nonresidue() + aa
        t2 = (c0 + c1) * (self.c0 + self.c1) - aa - bb
        t3 = self.c2 * c0 + bb
        return Fq6(t1, t2, t3)

    def frobenius_map(self, power):
        return Fq6(self.c0.frobenius_map(power), self.c1.frobenius_map(power) * FROBENIUS_FQ6_C1[power % 6],
                   self.c2.frobenius_map(power) * FROBENIUS_FQ6_C2[power % 6])

    def inverse(self):
        a0, a1, a2 = self.c0, self.c1, self.c2
        c0 = a0.square() - (a1 * a2).mul_by_nonresidue()
        c1 = a2.square().mul_by_nonresidue() - a0 * a1
        c2 = a1.square() - a0 * a2
        t = ((a2 * c1 + a1 * c2).mul_by_nonresidue() + a0 * c0).inverse()
        return Fq6(t * c0, t * c1, t * c2)

    def pow(self, e):
        acc, base = Fq6.one(), self
        while e:
            if e & 1:
                acc = acc * base
            base = base * base
            e >>= 1
        return acc

    def is_zero(self):
        return self.c0.is_zero() and self.c1.is_zero() and self.c2.is_zero()

    def __eq__(self, o):
        return isinstance(o, Fq6) and self.c0 == o.c0 and self.c1 == o.c1 and self.c2 == o.c2

    def __hash__(self):
        return hash(tuple(self.coords()))

    def coords(self):
        return self.c0.coords() + self.c1.coords() + self.c2.coords()

    def __repr__(self):
        return f"Fq6({self.c0!r}, {self.c1!r}, {self.c2!r})"


class Fq12:
    __slots__ = ("c0", "c1")

    def __init__(self, c0, c1=None):
        self.c0, self.c1 = c0, Fq6.zero() if c1 is None else c1

    @classmethod
    def one(cls):
        return cls(Fq6.one())

    @classmethod
    def from_coords(cls, v):
        v = [int(x) for x in v]
        if len(v) != 12 or not all(0 <= x < Q for x in v):
            raise ValueError("Fq12.from_coords: twelve residues below Q")
        f = [Fq2(v[2 * k], v[2 * k + 1]) for k in range(6)]
        return cls(Fq6(f[0], f[1], f[2]), Fq6(f[3], f[4], f[5]))

    def coords(self):
        return self.c0.coords() + self.c1.coords()

    def __add__(self, o):
        return Fq12(self.c0 + o.c0, self.c1 + o.c1)

    def __sub__(self, o):
        return Fq12(self.c0 - o.c0, self.c1 - o.c1)

    def __mul__(self, o):
        aa, bb = self.c0 * o.c0, self.c1 * o.c1
        return Fq12(bb.mul_by_nonresidue() + aa, (self.c0 + self.c1) * (o.c0 + o.c1) - aa - bb)

    def square(self):
        ab = self.c0 * self.c1
        c0 = (self.c1.mul_by_nonresidue() + self.c0) * (self.c0 + self.c1) - ab - ab.mul_by_nonresidue()
        return Fq12(c0, ab + ab)

    def mul_by_014(self, c0, c1, c4):
        aa = self.c0.mul_by_01(c0, c1)
        bb = self.c1.mul_by_1(c4)
        t = (self.c1 + self.c0).mul_by_01(c0, c1 + c4) - aa - bb
        return Fq12(bb.mul_by_nonresidue() + aa, t)

    def conjugate(self):
        return Fq12(self.c0, -self.c1)

    def frobenius_map(self, power):
        c1 = self.c1.frobenius_map(power)
        g = FROBENIUS_FQ12_C1[power % 12]
        return Fq12(self.c0.frobenius_map(power), Fq6(c1.c0 * g, c1.c1 * g, c1.c2 * g))

    def inverse(self):
        t = (self.c0.square() - self.c1.square().mul_by_nonresidue()).inverse()
        return Fq12(self.c0 * t, -(self.c1 * t))

    def pow(self, e):
        e = int(e)
        if e < 0:
            return self.inverse().pow(-e)
        acc = Fq12.one()
        for bit in bin(e)[2:] if e else "":
            acc = acc.square()
            if bit == "1":
                acc = acc * self
        return acc

    __pow__ = pow

    def is_one(self):
        return self == Fq12.one()

    def __eq__(self, o):
        return isinstance(o, Fq12) and self.c0 == o.c0 and self.c1 == o.c1

    def __hash__(self):
        return hash(tuple(self.coords()))

    def __repr__(self):
        return f"Fq12({self.c0!r}, {self.c1!r})"


# ---------------------------------------------------------------- G2
B2 = Fq2(4, 4)
G2X = Fq2(0x024AA2B2F08F0A91260805272DC51051C6E47AD4FA403B02B4510B647AE3D1770BAC0326A805BBEFD48056C8C121BDB8,
          0x13E02B6052719F607DACD3A088274F65596BD0D09920B61AB5DA61BBDC7F5049334CF11213945D57E5AC7D055D042B7E)
G2Y = Fq2(0x0CE5D527727D6E118CC9CDC6DA2E351AADFD9BAA8CBDD3A76D429A695160D12C923AC9CC3BACA289E193548608B82801,
          0x0606C4A02EA734CC32ACD2B02BC28B99CB3E287E85A763AF267492AB572E99AB3F370D275CEC1DA1AAA9075FF05F79BE)
_F2_ONE, _F2_ZERO = Fq2.one(), Fq2.zero()
_J2_ID = (_F2_ONE, _F2_ONE, _F2_ZERO)


def _j2_double(p):
    X, Y, Z = p
    if Z.is_zero():
        return p
    A, Bq = X.square(), Y.square()
    C = Bq.square()
    D = ((X + Bq).square() - A - C) * 2
    E = A * 3
    X3 = E.square() - D * 2
    return X3, E * (D - X3) - C * 8, Y * Z * 2


def _j2_add(p, q):
    X1, Y1, Z1 = p
    X2, Y2, Z2 = q
    if Z1.is_zero():
        return q
    if Z2.is_zero():
        return p
    Z1Z1, Z2Z2 = Z1.square(), Z2.square()
    U1, U2 = X1 * Z2Z2, X2 * Z1Z1
    S1, S2 = Y1 * Z2 * Z2Z2, Y2 * Z1 * Z1Z1
    Hh, r = U2 - U1, S2 - S1
    if Hh.is_zero():
        return _j2_double(p) if r.is_zero() else _J2_ID
    HH = Hh.square()
    HHH = Hh * HH
    V = U1 * HH
    X3 = r.square() - HHH - V * 2
    return X3, r * (V - X3) - S1 * HHH, Z1 * Z2 * Hh


def _j2_mul(p, k):
    acc = _J2_ID
    for bit in bin(k)[2:] if k else "":
        acc = _j2_double(acc)
        if bit == "1":
            acc = _j2_add(acc, p)
    return acc


class G2:
    """An element of E'(Fq2), written multiplicatively as the reference's betterpairing.G2 is.  G2(x, y) takes two Fq2 and refuses a
    point off the twist; membership in the subgroup of order R is not checked (in_subgroup tells)."""

    __slots__ = ("_j", "_aff")

    def __init__(self, x, y):
        if not (isinstance(x, Fq2) and isinstance(y, Fq2)):
            raise TypeError("G2: coordinates are Fq2 elements")
        if not (y.square() - x.square() * x - B2).is_zero():
            raise ValueError("G2: the point is not on the twist y^2 = x^3 + 4 (1 + u)")
        self._j = (x, y, _F2_ONE)
        self._aff = (x, y)

    @classmethod
    def _from_jac(cls, j):
        p = object.__new__(cls)
        p._j, p._aff = j, None
        return p

    @classmethod
    def one(cls):
        return cls._from_jac(_J2_ID)

    identity = one

    @classmethod
    def generator(cls):
        return cls(G2X, G2Y)

    def _affine(self):
        if self._aff is None:
            X, Y, Z = self._j
            if Z.is_zero():
                self._aff = (_F2_ZERO, _F2_ZERO)
            else:
                zi = Z.inverse()
                zi2 = zi.square()
                self._aff = (X * zi2, Y * zi2 * zi)
        return self._aff

    @property
    def x(self):
        return self._affine()[0]

    @property
    def y(self):
        return self._affine()[1]

    def is_one(self):
        return self._j[2].is_zero()

    def on_curve(self):
        if self.is_one():
            return True
        x, y = self._affine()
        return (y.square() - x.square() * x - B2).is_zero()

    def in_subgroup(self):
        return G2._from_jac(_j2_mul(self._j, R)).is_one()

    def __mul__(self, other):
        if not isinstance(other, G2):
            return NotImplemented
        return G2._from_jac(_j2_add(self._j, other._j))

    def invert(self):
        X, Y, Z = self._j
        return G2._from_jac((X, -Y, Z))

    def __truediv__(self, other):
        if not isinstance(other, G2):
            return NotImplemented
        return self * other.invert()

    def __pow__(self, k, modulus=None):
        if modulus is not None:
            raise TypeError("G2: pow() takes no modulus")
        return G2._from_jac(_j2_mul(self._j, _exponent(k)))

    def __eq__(self, other):
        if not isinstance(other, G2):
            return NotImplemented
        X1, Y1, Z1 = self._j
        X2, Y2, Z2 = other._j
        if Z1.is_zero() or Z2.is_zero():
            return Z1.is_zero() and Z2.is_zero()
        a, b = Z1.square(), Z2.square()
        return (X1 * b - X2 * a).is_zero() and (Y1 * b * Z2 - Y2 * a * Z1).is_zero()

    def __hash__(self):
        return hash(self._affine() + (self.is_one(),))

    def __repr__(self):
        return "G2.one()" if self.is_one() else f"G2({self.x!r}, {self.y!r})"

    # ---- the crate's uncompressed encoding: x.c1, x.c0, y.c1, y.c0, 48 big-endian bytes each; in byte 0, 0x80 clear
    # (uncompressed), 0x40 the identity (everything else zero)
    def to_uncompressed(self):
        if self.is_one():
            return bytes([0x40]) + bytes(G2_UNCOMPRESSED_BYTES - 1)
        x, y = self._affine()
        return b"".join(v.to_bytes(48, "big") for v in (x.c1, x.c0, y.c1, y.c0))

    @classmethod
    def from_uncompressed(cls, data, check_subgroup=False):
        data = bytes(data)
        if len(data) != G2_UNCOMPRESSED_BYTES:
            raise ValueError(f"G2.from_uncompressed: expected {G2_UNCOMPRESSED_BYTES} bytes, got {len(data)}")
        if data[0] & 0x80:
            raise ValueError("G2.from_uncompressed: the compression flag is set")
        if data[0] & 0x20:
            raise ValueError("G2.from_uncompressed: a sign flag on an uncompressed point")
        if data[0] & 0x40:
            if data[0] != 0x40 or any(data[1:]):
                raise ValueError("G2.from_uncompressed: the identity carries non-zero coordinates")
            return cls.one()
        v = [int.from_bytes(data[48 * k:48 * k + 48], "big") for k in range(4)]
        if any(c >= Q for c in v):
            raise ValueError("G2.from_uncompressed: a coordinate is not below Q")
        p = cls(Fq2(v[1], v[0]), Fq2(v[3], v[2]))
        if check_subgroup and not p.in_subgroup():
            raise ValueError("G2.from_uncompressed: the point is not in the subgroup")
        return p


# ---------------------------------------------------------------- the ate loop
def _loop_bits():
    """the bits of |x| >> 1 below the leading one, from the top"""
    return [c == "1" for c in bin(BLS_X >> 1)[3:]]


def _doubling_step(r):
    """Algorithm 26 of eprint 2010/354 in the crate's arrangement: r <- 2 r, -> the line's coefficients"""
    X, Y, Z = r
    t0, t1 = X.square(), Y.square()
    t2 = t1.square()
    t3 = ((t1 + X).square() - t0 - t2) * 2
    t4 = t0 * 3
    t6 = X + t4
    t5 = t4.square()
    zsq = Z.square()
    X3 = t5 - t3 * 2
    Z3 = (Z + Y).square() - t1 - zsq
    Y3 = (t3 - X3) * t4 - t2 * 8
    c1 = -(t4 * zsq * 2)
    c2 = t6.square() - t0 - t5 - t1 * 4
    c0 = Z3 * zsq * 2
    return (X3, Y3, Z3), (c0, c1, c2)


def _addition_step(r, q):
    """Algorithm 27 of eprint 2010/354: r <- r + q (q affine), -> the line's coefficients"""
    X, Y, Z = r
    qx, qy = q
    zsq, ysq = Z.square(), qy.square()
    t0 = zsq * qx
    t1 = ((qy + Z).square() - ysq - zsq) * zsq
    t2 = t0 - X
    t3 = t2.square()
    t4 = t3 * 4
    t5 = t4 * t2
    t6 = t1 - Y * 2
    t9 = t6 * qx
    t7 = t4 * X
    X3 = t6.square() - t5 - t7 * 2
    Z3 = (Z + t2).square() - zsq - t3
    t10 = qy + Z3
    t8 = (t7 - X3) * t6
    Y3 = t8 - Y * t5 * 2
    t10 = t10.square() - ysq - Z3.square()
    t9 = t9 * 2 - t10
    return (X3, Y3, Z3), (Z3 * 2, -t6 * 2, t9)


def prepare_g2(q):
    """-> the 68 line-coefficient triples (Fq2, Fq2, Fq2) of q, in the order the loop consumes them; [] for the identity"""
    if not isinstance(q, G2):
        raise TypeError(f"prepare_g2: expected a host G2, got {type(q).__name__}")
    if q.is_one():
        return []
    aff = (q.x, q.y)
    r = (aff[0], aff[1], _F2_ONE)
    coeffs = []
    for bit in _loop_bits():
        r, c = _doubling_step(r)
        coeffs.append(c)
        if bit:
            r, c = _addition_step(r, aff)
            coeffs.append(c)
    r, c = _doubling_step(r)
    coeffs.append(c)
    assert len(coeffs) == N_LINES
    return coeffs


def _ell(f, c, p):
    return f.mul_by_014(c[2], c[1] * p[0], c[0] * p[1])


def miller_loop(pairs):
    """pairs: [(G1, G2 or prepared coefficients)] -> the raw Miller value of the product (not an interface: see the module's head).
    A pair with an identity on either side is skipped, as the reference does."""
    live = []
    for p, q in pairs:
        if not isinstance(p, G1):
            raise TypeError(f"miller_loop: expected a host G1, got {type(p).__name__}")
        coeffs = prepare_g2(q) if isinstance(q, G2) else list(q)
        if p.is_one() or not coeffs:
            continue
        if len(coeffs) != N_LINES:
            raise ValueError(f"miller_loop: a prepared point has {N_LINES} lines, got {len(coeffs)}")
        live.append(((p.x, p.y), coeffs))
    f = Fq12.one()
    k = 0
    for bit in _loop_bits():
        for p, c in live:
            f = _ell(f, c[k], p)
        k += 1
        if bit:
            for p, c in live:
                f = _ell(f, c[k], p)
            k += 1
        f = f.square()
    for p, c in live:
        f = _ell(f, c[k], p)
    return f.conjugate()


def _exp_by_x(f, x):
    return f.pow(x).conjugate()


def final_exponentiation(f):
    """-> f^(3 (Q^12 - 1) / R) by the reference's chain; None for f = 0"""
    if f.c0.is_zero() and f.c1.is_zero():
        return None
    r = f.conjugate() * f.inverse()
    r = r.frobenius_map(2) * r
    x = BLS_X
    y0 = r.square()
    y1 = _exp_by_x(y0, x)
    y2 = _exp_by_x(y1, x >> 1)
    y1 = (y1 * r.conjugate()).conjugate() * y2
    y2 = _exp_by_x(y1, x)
    y3 = _exp_by_x(y2, x)
    y3 = y3 * y1.conjugate()
    y1 = y1.frobenius_map(3) * y2.frobenius_map(2)
    y2 = _exp_by_x(y3, x) * y0 * r
    return y1 * y2 * y3.frobenius_map(1)


def pair(p, q):
    """e(p, q) as the reference's Bls12::pairing gives it"""
    return final_exponentiation(miller_loop([(p, q)]))


def pairing_product(pairs):
    return final_exponentiation(miller_loop(pairs))

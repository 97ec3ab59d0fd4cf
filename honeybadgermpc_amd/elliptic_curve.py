"""
The reference's elliptic_curve.py on Python ints: the constant `Subgroup.BLS12_381` (:4-5) and the twisted Edwards curve Jubjub
(:8-48) with its points (:51-145) and the point at infinity (:148-177) -- the host model the device kernels of csrc/hb_jj.hip and
progs/jubjub.py are checked against, restated from the reference's behaviour: the same names, the refusal to construct a point off
the curve, the affine unified addition law, `n < 0` negates and `n == 0` gives `Ideal`.

    Jubjub(a=-1, d=-(10240/10241), p=BLS12-381 Fr)       a x^2 + y^2 = 1 + d x^2 y^2 over GF(p)
    Point(x, y, curve=None)                              coordinates are ints, reduced mod p
    Ideal(curve)

Differences, all on purpose: coordinates are plain ints, not field objects; the modulus is an argument, so the 64-bit field can carry a
curve; a sum stays on the summands' curve (the reference hands its sums to the default curve); and the addition law reads
y3 = (y1 y2 - a x1 x2) / (1 - d x1 x2 y1 y2), which is the reference's `y1 y2 + x1 x2` at its a = -1.
"""


class Subgroup:
    # order of the BLS12-381 G1/G2 subgroups = the scalar field all shares live in
    BLS12_381 = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


class Jubjub(object):
    """a x^2 + y^2 = 1 + d x^2 y^2 over GF(p); the defaults are the reference's: a = -1, d = -(10240 / 10241)"""

    def __init__(self, a=None, d=None, p=Subgroup.BLS12_381):
        if not isinstance(p, int) or isinstance(p, bool) or p < 3:
            raise ValueError(f"p must be an odd prime, got {p!r}")
        self.p = p
        self.a = (p - 1) if a is None else a % p
        self.d = (-10240 * pow(10241, -1, p)) % p if d is None else d % p
        a_d_diff = (self.a - self.d) % p
        self.disc = self.a * self.d * pow(a_d_diff, 4, p) % p
        if not self.is_smooth():
            raise Exception(f"The curve {self} is not smooth!")

    def __str__(self):
        return "%sx^2 + y^2 = 1 + %sx^2y^2" % (self.a, self.d)

    def __repr__(self):
        return str(self)

    def __eq__(self, other):
        return isinstance(other, Jubjub) and (self.a, self.d, self.p) == (other.a, other.d, other.p)

    def __hash__(self):
        return hash((self.a, self.d, self.p))

    def is_smooth(self):
        return self.disc != 0

    def is_complete(self):
        """a a square and d a non-square: no denominator of the addition law vanishes for points on the curve"""
        p = self.p
        return pow(self.a, (p - 1) // 2, p) == 1 and pow(self.d, (p - 1) // 2, p) == p - 1

    def contains_point(self, pt):
        """Checks whether or not the given point sits on the curve"""
        p, x, y = self.p, pt.x, pt.y
        return (self.a * x * x + y * y - 1 - self.d * x * x * y * y) % p == 0


class Point(object):
    """A point of the curve in affine coordinates (the 'local' class of the reference, no shares)"""

    def __init__(self, x, y, curve=None):
        if curve is None:
            curve = Jubjub()
        if not isinstance(curve, Jubjub):
            raise Exception(f"Could not create Point-- given curve not of type Jubjub ({type(curve)})")
        self.curve = curve
        self.x = int(x) % curve.p
        self.y = int(y) % curve.p
        if not self.curve.contains_point(self):
            raise Exception(f"Could not create Point({self})-- not on the given curve {curve}!")

    def __str__(self):
        return "(%r, %r)" % (self.x, self.y)

    def __repr__(self):
        return str(self)

    def __neg__(self):
        return Point(-self.x, self.y, self.curve)

    def __add__(self, other):
        if self.curve != other.curve:
            raise Exception("Can't add points on different curves!")
        if isinstance(other, Ideal):
            return self
        c = self.curve
        p = c.p
        x1, y1, x2, y2 = self.x, self.y, other.x, other.y
        d_prod = c.d * x1 * x2 * y1 * y2 % p
        x3 = (x1 * y2 + y1 * x2) * pow(1 + d_prod, -1, p)
        y3 = (y1 * y2 - c.a * x1 * x2) * pow(1 - d_prod, -1, p)
        return Point(x3, y3, c)

    def __sub__(self, other):
        return self + -other

    def __mul__(self, n):
        if not isinstance(n, int) or isinstance(n, bool):
            raise Exception("Can't scale a point by something which isn't an int!")
        if n < 0:
            return -self * -n
        elif n == 0:
            return Ideal(self.curve)
        current = self
        product = Point(0, 1, self.curve)
        i = 1
        while i <= n:
            if n & i == i:
                product += current
            current += current
            i <<= 1
        return product

    def __rmul__(self, n):
        return self * n

    def __list__(self):
        return [self.x, self.y]

    def __eq__(self, other):
        if type(other) is Ideal:
            return False
        elif not isinstance(other, Point) or self.curve != other.curve:
            return False
        return (self.x, self.y) == (other.x, other.y)

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash((self.x, self.y, self.curve))

    def __getitem__(self, index):
        return [self.x, self.y][index]

    def double(self):
        return self + self


class Ideal(Point):
    """Represents the point at infinity of the curve"""

    def __init__(self, curve):
        self.curve = curve

    def __neg__(self):
        return self

    def __str__(self):
        return "Ideal"

    def __add__(self, other):
        if not isinstance(other, Point):
            raise Exception("Can't add something that's not a point to a point")
        elif self.curve != other.curve:
            raise Exception("Can't add points on different curves!")
        return other

    def __mul__(self, n):
        if not isinstance(n, int) or isinstance(n, bool):
            raise Exception("Can't scale a point by something which isn't an int!")
        return self

    def __eq__(self, other):
        return type(other) is Ideal

    def __hash__(self):
        return hash(("Ideal", self.curve))

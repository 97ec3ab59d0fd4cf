"""Plain-Python model for the root-finding tests (csrc/hb_rf.hip, honeybadgermpc_amd/solver.py): polynomials over GF(p) as lists of
ints, the coefficient of x^i at index i.  Nothing here touches the library."""


def trim(a):
    a = list(a)
    while a and a[-1] == 0:
        a.pop()
    return a


def poly_from_roots(roots, p):
    """prod (x - r), monic, len(roots) + 1 coefficients"""
    f = [1]
    for r in roots:
        g = [0] * (len(f) + 1)
        for i, c in enumerate(f):
            g[i + 1] = (g[i + 1] + c) % p
            g[i] = (g[i] - r * c) % p
        f = g
    return f


def poly_mul(a, b, p):
    if not a or not b:
        return []
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] = (out[i + j] + x * y) % p
    return out


def poly_rem(a, b, p):
    """a mod b (b non-zero); as many coefficients as deg b, zero padded"""
    b = trim(b)
    a = [x % p for x in a]
    inv = pow(b[-1], -1, p)
    for i in range(len(a) - 1, len(b) - 2, -1):
        q = a[i] * inv % p
        if q:
            for j, y in enumerate(b):
                a[i - len(b) + 1 + j] = (a[i - len(b) + 1 + j] - q * y) % p
    a = a[:len(b) - 1]
    return a + [0] * (len(b) - 1 - len(a))


def poly_gcd(a, b, p):
    """the monic gcd ([] for gcd(0, 0))"""
    a, b = trim(x % p for x in a), trim(x % p for x in b)
    while b:
        a, b = b, trim(poly_rem(a, b, p))
    if not a:
        return []
    inv = pow(a[-1], -1, p)
    return [x * inv % p for x in a]


def power_sums_from_poly(coeffs, p):
    """S_1 .. S_k of the k roots (in the algebraic closure) of a monic polynomial: Newton's identities run backwards,
    S_m = (-1)^(m-1) m e_m + sum_{i=1..m-1} (-1)^(i-1) e_i S_(m-i) -- defined for ANY monic polynomial, so invalid inputs can be made"""
    k = len(coeffs) - 1
    assert coeffs[k] % p == 1
    e = [(coeffs[k - m] if m % 2 == 0 else -coeffs[k - m]) % p for m in range(k + 1)]
    s = [0] * (k + 1)
    for m in range(1, k + 1):
        acc = (m * e[m]) % p if m % 2 else (-m * e[m]) % p
        for i in range(1, m):
            term = e[i] * s[m - i]
            acc = acc + term if i % 2 else acc - term
        s[m] = acc % p
    return s[1:]


def power_sums_from_roots(roots, p):
    cur, out = [1] * len(roots), []
    for _ in roots:
        cur = [c * r % p for c, r in zip(cur, roots)]
        out.append(sum(cur) % p)
    return out


def non_residue(p):
    c = 2
    while pow(c, (p - 1) // 2, p) != p - 1:
        c += 1
    return c


def irreducible_cubic(p):
    """x^3 + x + c without a root in GF(p) (a cubic without a root is irreducible); p small enough to try every element, or p = BLS-sized where
    the search is by gcd with x^p - x"""
    for c in range(1, 200):
        f = [c, 1, 0, 1]
        # x^p mod f
        r, base, e = [1], [0, 1], p
        while e:
            if e & 1:
                r = poly_rem(poly_mul(r, base, p), f, p)
            base = poly_rem(poly_mul(base, base, p), f, p)
            e >>= 1
        r = list(r) + [0] * (3 - len(r))
        r[1] = (r[1] - 1) % p
        if len(poly_gcd(f, r, p)) == 1:
            return f
    raise AssertionError("no irreducible cubic found")

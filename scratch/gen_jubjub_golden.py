#!/usr/bin/env python3
"""Writes tests/golden/jubjub.json from the REFERENCE's own Jubjub, Point (honeybadgermpc/elliptic_curve.py) and mimc_plain
(honeybadgermpc/progs/mimc.py), as decimal strings:

  * the modulus, the curve constants a and d, the generator GP hard-coded in progs/mimc_jubjub_pkc.py and r_J (GP has order 8 r_J:
    asserted here with the reference's Point);
  * "adds": P + Q for pairs drawn from {(0, 1), (0, -1), GP, -GP, GP * r_J, 6 seeded multiples of GP} -- every unordered pair, P + P
    among them, and P + (-P) for the seeded ones;
  * "muls": n * P for n in {1, 2, 3, 8 r_J - 1, 8 r_J, 8 r_J + 1, p - 1, -5} on GP and 8 seeded 255-bit n on seeded multiples of GP;
  * "encrypts": 4 cases of 3 blocks of the reference's mimc_encrypt.  Its module progs/mimc_jubjub_pkc.py does not import without
    the NTL extension (it pulls in progs/jubjub.py -> mpc.py), so the expectation is computed as its four lines read (:46-52):
    a_ = a * GP, k = (a * pub_key).x, ciphertext[i] = mimc_plain(i, k) + ms[i], from the reference's Point.__mul__ and mimc_plain.

Needs a checkout of the reference (its path is argv[1]); it is imported, never copied, and no test runs this script -- the tests read
the JSON only.  Imported as scratch/gen_mimc_golden.py does.

    python scratch/gen_jubjub_golden.py PATH_TO_THE_REFERENCE
"""
import json
import os
import random
import sys
import types

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if len(sys.argv) != 2:
    raise SystemExit(__doc__)
REF = sys.argv[1]
R_J = 6554484396890773809930967563523245729705921265872317281365359162392183254199
GP_XY = (5, 6846412461894745224441235558443359243034138132682534265960483512729196124138)


def install_reference():
    from sympy import isprime

    gmpy2 = types.ModuleType("gmpy2")
    gmpy2.is_prime = lambda n: bool(isprime(int(n)))
    gmpy2.mpz = int
    sys.modules["gmpy2"] = gmpy2
    pkg = types.ModuleType("honeybadgermpc")
    pkg.__path__ = [os.path.join(REF, "honeybadgermpc")]
    sys.modules["honeybadgermpc"] = pkg
    sys.path.insert(0, REF)


def main():
    install_reference()
    from honeybadgermpc.elliptic_curve import Ideal, Jubjub, Point, Subgroup
    from honeybadgermpc.progs.mimc import mimc_plain

    p = Subgroup.BLS12_381
    field = Jubjub.Field
    curve = Jubjub()

    def pt(x, y):
        return Point(x % p, y % p)

    def val(v):
        return int(v.value) if hasattr(v, "value") else int(v) % p

    def xy(q):
        return [str(val(q.x)), str(val(q.y))]

    def neg(q):
        # the reference's __neg__ takes int coordinates (its sums carry field elements)
        return -Point(val(q.x), val(q.y))

    gp = pt(*GP_XY)
    neutral = pt(0, 1)
    assert gp * (8 * R_J) == neutral and gp * R_J != neutral and gp * (4 * R_J) != neutral
    rnd = random.Random(20261017)
    seeded = [gp * rnd.randrange(1, 8 * R_J) for _ in range(6)]
    special = [neutral, pt(0, -1), gp, neg(gp), gp * R_J]
    pts = special + seeded
    pairs = [(pts[i], pts[j]) for i in range(len(pts)) for j in range(i, len(pts))] + [(q, neg(q)) for q in seeded]
    adds = []
    for a, b in pairs:
        s = a + b
        adds.append({"P": xy(a), "Q": xy(b), "sum": xy(s)})
    muls = []
    for n in (1, 2, 3, 8 * R_J - 1, 8 * R_J, 8 * R_J + 1, p - 1, -5):
        r = gp * n
        assert not isinstance(r, Ideal)
        muls.append({"n": str(n), "P": xy(gp), "out": xy(r)})
    for q in seeded + seeded[:2]:
        n = rnd.randrange(1 << 254, p)                   # 255 bits, a canonical residue
        muls.append({"n": str(n), "P": xy(q), "out": xy(q * n)})
    encrypts = []
    for _ in range(4):
        priv, a = rnd.getrandbits(32), rnd.randrange(1, p)
        pub = gp * priv
        a_ = a * gp
        k = (a * pub).x
        ms = [rnd.randrange(p) for _ in range(3)]
        cs = [mimc_plain(field(idx), k) + field(m) for idx, m in enumerate(ms)]
        encrypts.append({"priv": str(priv), "pub": xy(pub), "a": str(a), "a_": xy(a_), "k": str(val(k)), "ms": [str(m) for m in ms],
                         "cs": [str(int(c.value)) for c in cs]})
    out = {"modulus": str(p), "a": str(int(curve.a.value)), "d": str(int(curve.d.value)), "GP": xy(gp), "r_J": str(R_J), "adds": adds, "muls": muls,
           "encrypts": encrypts}
    path = os.path.join(REPO, "tests", "golden", "jubjub.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(f"wrote {path} ({os.path.getsize(path)} bytes): {len(adds)} adds, {len(muls)} muls, {len(encrypts)} encrypts")


main()

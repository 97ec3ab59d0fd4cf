#!/usr/bin/env python3
"""Writes tests/golden/mimc.json from the REFERENCE's own mimc_plain and ROUND (honeybadgermpc/progs/mimc.py): the modulus
(BLS12-381 Fr), ROUND, and 41 (x, k, out) cases as decimal strings -- every pair of {0, 1, 2, p - 2, p - 1} and 16 seeded random
pairs.  The reference's function is handed its own field elements (GF(p) of honeybadgermpc/field.py), as its tests do.

Needs a checkout of the reference (its path is argv[1]); it is imported, never copied, and no test runs this script -- the tests
read the JSON only.  How it is imported: as scratch/gen_butterfly_golden.py does, a bare `honeybadgermpc` package object pointing
at the reference (its __init__ opens log files) and `gmpy2` stubbed with sympy's isprime.

    python scratch/gen_mimc_golden.py PATH_TO_THE_REFERENCE
"""
import itertools
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
BLS = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


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
    from honeybadgermpc.elliptic_curve import Subgroup
    from honeybadgermpc.field import GF
    from honeybadgermpc.progs.mimc import ROUND, mimc_plain

    p = Subgroup.BLS12_381
    assert p == BLS
    field = GF(p)
    rnd = random.Random(20261016)
    corners = [0, 1, 2, p - 2, p - 1]
    pairs = list(itertools.product(corners, repeat=2)) + [(rnd.randrange(p), rnd.randrange(p)) for _ in range(16)]
    cases = [{"x": str(x), "k": str(k), "out": str(int(mimc_plain(field(x), field(k)).value))} for x, k in pairs]
    path = os.path.join(REPO, "tests", "golden", "mimc.json")
    with open(path, "w") as f:
        json.dump({"modulus": str(p), "ROUND": ROUND, "cases": cases}, f, separators=(",", ":"))
    print(f"wrote {path} ({os.path.getsize(path)} bytes), ROUND = {ROUND}, {len(cases)} cases")


main()

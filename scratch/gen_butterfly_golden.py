#!/usr/bin/env python3
"""Writes tests/golden/butterfly_network.json from the REFERENCE's own iterated_butterfly_network
(apps/asynchromix/butterfly_network.py), run in the clear: for k in {2, 4, 8, 32} the inputs, the signs per layer and switch
(in the order the reference draws them) and the reference's output.

Needs a checkout of the reference (its path is argv[1]); it is imported, never copied, and no test runs this
script -- the tests read the JSON only.  How it is imported: as oracle/gen_golden.py does, a bare `honeybadgermpc` package object
pointing at the reference (its __init__ opens log files), `gmpy2` stubbed with sympy's isprime, and
`honeybadgermpc.preprocessing` -- which the module imports for its command-line entry only -- stubbed with an empty class.  The
stand-in for the MPC context below computes on field VALUES where the reference computes on shares: a "share" is the value itself,
a ShareArray product is the element-wise product, and get_one_minus_ones hands out the recorded signs.

    python scratch/gen_butterfly_golden.py PATH_TO_THE_REFERENCE
"""
import asyncio
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
    pre = types.ModuleType("honeybadgermpc.preprocessing")
    pre.PreProcessedElements = type("PreProcessedElements", (), {})
    sys.modules["honeybadgermpc.preprocessing"] = pre
    sys.path.insert(0, REF)


class ClearShare:
    def __init__(self, v):
        self.v = v

    def __add__(self, other):
        return ClearShare(self.v + other.v)

    def __sub__(self, other):
        return ClearShare(self.v - other.v)


class ClearArray:
    def __init__(self, values):
        self._shares = [v if isinstance(v, ClearShare) else ClearShare(v) for v in values]

    def __sub__(self, other):
        return ClearArray([a - b for a, b in zip(self._shares, other._shares)])

    def __mul__(self, other):
        async def product():
            return ClearArray([ClearShare(a.v * b.v) for a, b in zip(self._shares, other._shares)])

        return product()


class ClearContext:
    """what batch_switch and iterated_butterfly_network ask of an Mpc context"""

    def __init__(self, field, signs):
        self.field, self.myid, self.ShareArray = field, 0, ClearArray
        self.drawn = []
        it = iter(signs)
        ctx = self

        class Preproc:
            def get_one_minus_ones(self, _):
                b = next(it)
                ctx.drawn.append(b)
                return ClearShare(field(b))

        self.preproc = Preproc()


def main():
    install_reference()
    from honeybadgermpc.field import GF
    from apps.asynchromix.butterfly_network import iterated_butterfly_network

    field = GF(BLS)
    rnd = random.Random(20261016)
    cases = []
    for k in (2, 4, 8, 32):
        n = k.bit_length() - 1
        inputs = [rnd.randrange(BLS) for _ in range(k)]
        signs = [rnd.choice((1, -1)) for _ in range(n * n * (k // 2))]
        ctx = ClearContext(field, signs)
        out = asyncio.run(iterated_butterfly_network(ctx, [field(v) for v in inputs], k))
        assert ctx.drawn == signs, "the reference drew another number of signs"
        out = [int(v.value) for v in out]
        assert sorted(out) == sorted(inputs)
        half = k // 2
        cases.append({"k": k, "inputs": [str(v) for v in inputs], "signs": [signs[l * half:(l + 1) * half] for l in range(n * n)],
                      "output": [str(v) for v in out]})
    path = os.path.join(REPO, "tests", "golden", "butterfly_network.json")
    with open(path, "w") as f:
        json.dump({"modulus": str(BLS), "cases": cases}, f, separators=(",", ":"))
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


main()

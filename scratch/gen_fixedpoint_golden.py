#!/usr/bin/env python3
"""Writes tests/golden/fixedpoint.json from the REFERENCE's own progs/fixedpoint.py, integers as decimal strings:

  * the constants F, KAPPA, K and the modulus;
  * "to_fixed": to_fixed_point_repr(x, f) for negative, zero, tiny, large and seeded floats and ints (the float is stored as its
    hex form, so the test feeds the very same double);
  * "binary": binary_repr(x, k);
  * "from_fixed": from_fixed_point_repr(Field(v), k, f, signed) for residues at 0, +-1, around 2^(k-1), p - 1 and seeded ones;
  * "trunc_pr", "div2m", "trunc": the reference's coroutines driven with a small fake context here -- cleartext "shares" (a class
    with the operators the coroutines use over the reference's own field, a product that is an awaitable, an open that returns
    the value) and a preproc whose get_bit hands out seeded bits and records them.  Each case keeps k, m, x, the bits in the
    order they were drawn (r1's m bits, then r2's k + KAPPA - m, least significant first: the plane order of the device code) and
    the value the result holds.

The reference's module imports mpc.py and preprocessing.py, which need its NTL extension; they are replaced by empty stand-ins
before the import (fixedpoint.py only uses them in its tutorial program).  Needs a checkout of the reference (its path is
argv[1]); it is imported, never copied, and no test runs this script -- the tests read the JSON only.

    python scratch/gen_fixedpoint_golden.py PATH_TO_THE_REFERENCE
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


def install_reference():
    try:
        import gmpy2  # noqa: F401
    except ImportError:
        from sympy import isprime

        gmpy2 = types.ModuleType("gmpy2")
        gmpy2.is_prime = lambda n: bool(isprime(int(n)))
        gmpy2.mpz = int
        sys.modules["gmpy2"] = gmpy2
    pkg = types.ModuleType("honeybadgermpc")
    pkg.__path__ = [os.path.join(REF, "honeybadgermpc")]
    sys.modules["honeybadgermpc"] = pkg
    for name, attrs in (("honeybadgermpc.mpc", ("TaskProgramRunner",)), ("honeybadgermpc.preprocessing", ("PreProcessedElements",)),
                        ("honeybadgermpc.progs.mixins.share_arithmetic", ("BeaverMultiply", "MixinConstants"))):
        mod = types.ModuleType(name)
        for a in attrs:
            setattr(mod, a, type(a, (), {"MultiplyShare": "multiply_share"}))
        sys.modules[name] = mod
    sys.path.insert(0, REF)


def main():
    install_reference()
    from honeybadgermpc.progs import fixedpoint as fx

    p, field = fx.p, fx.Field
    rnd = random.Random(20261017)

    class Share:
        def __init__(self, v):
            self.v = v if isinstance(v, type(field(0))) else field(int(v))

        def __add__(self, o):
            return Share(self.v + (o.v if isinstance(o, Share) else o))

        __radd__ = __add__

        def __sub__(self, o):
            return Share(self.v - (o.v if isinstance(o, Share) else o))

        def __mul__(self, o):
            async def product():
                return Share(self.v * o.v)

            return product()

        def __rmul__(self, o):                     # a public factor
            return Share(self.v * o)

        def open(self):
            async def opened():
                return self.v

            return opened()

    class Preproc:
        def __init__(self, mode):
            self.mode, self.bits = mode, []

        def get_bit(self, ctx):
            b = rnd.getrandbits(1) if self.mode == "random" else int(self.mode)
            self.bits.append(b)
            return Share(b)

    class Ctx:
        pass

    Ctx.Share = Share

    def drive(fn, x, k, m, mode):
        ctx = Ctx()
        ctx.preproc = Preproc(mode)
        out = asyncio.run(fn(ctx, Share(x % p), k, m))
        assert len(ctx.preproc.bits) == k + fx.KAPPA
        return {"k": k, "m": m, "x": str(x), "bits": "".join(map(str, ctx.preproc.bits)), "out": str(int(out.v.value))}

    # ---- the pure functions
    k, f = fx.K, fx.F
    floats = [0.0, -0.0, 1.0, -1.0, 2.5, -3.8, 0.1, -0.1, 2.0 ** -32, -(2.0 ** -32), 2.0 ** -33, -(2.0 ** -33), 1e-12, -1e-12, 0.5 - 2.0 ** -34,
              99.99999, -99.99999, 2.0 ** 31 - 2.0 ** -20, -(2.0 ** 31), 2.0 ** 31 - 1.0, 1.0 / 3.0, -1.0 / 3.0, 1.0 / 7.0, 1e6 + 1e-6]
    floats += [rnd.uniform(-100, 100) for _ in range(20)] + [rnd.uniform(-1e-6, 1e-6) for _ in range(6)]
    to_fixed = [{"x": x.hex(), "f": ff, "out": str(fx.to_fixed_point_repr(x, ff))} for x in floats for ff in ((f,) if abs(x) > 1e5 else (f, 8))]
    to_fixed += [{"x": str(x), "f": f, "out": str(fx.to_fixed_point_repr(x, f))} for x in (0, 1, -1, 100, -100, 2 ** 31 - 1, -(2 ** 31))]
    ints = [0, 1, 2, 3, 5, 255, 256, 2 ** 31, 2 ** 32 - 1, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1] + [rnd.getrandbits(rnd.choice([8, 16, 32, 64])) for _ in range(30)]
    binary = [{"x": str(x), "k": kk, "out": "".join(map(str, fx.binary_repr(x, kk)))} for x in ints for kk in (8, 32, 64) if kk == 64 or x < 2 ** 40][:60]
    residues = [0, 1, 2, p - 1, p - 2, 2 ** (k - 1) - 1, 2 ** (k - 1), 2 ** (k - 1) + 1, p - 2 ** (k - 1), p - 2 ** (k - 1) + 1, 2 ** f, p - 2 ** f, 2 ** (f - 1), 3 * 2 ** (f - 2)]
    residues += [rnd.getrandbits(63) for _ in range(12)] + [p - rnd.getrandbits(63) for _ in range(12)] + [fx.to_fixed_point_repr(rnd.uniform(-100, 100)) % p for _ in range(10)]
    from_fixed = [{"v": str(v), "k": k, "f": f, "signed": s, "out": fx.from_fixed_point_repr(field(v), k, f, s).hex()} for v in residues for s in ((True, False) if v < 2 ** 70 else (True,))]
    from_fixed += [{"v": str(v), "k": 16, "f": 8, "signed": True, "out": fx.from_fixed_point_repr(field(v), 16, 8, True).hex()} for v in (0, 255, 256, 2 ** 15 - 1, 2 ** 15, p - 1, p - 2 ** 15)]

    # ---- the coroutines, over the fake context
    out = {"modulus": str(p), "F": fx.F, "KAPPA": fx.KAPPA, "K": fx.K, "to_fixed": to_fixed, "binary": binary, "from_fixed": from_fixed}
    for name, fn, shapes in (("trunc_pr", fx.trunc_pr, [(64, 32), (128, 32), (64, 63), (64, 1)]), ("div2m", fx.div2m, [(64, 32), (64, 63), (16, 5)]),
                             ("trunc", fx.trunc, [(64, 32), (64, 63), (16, 5)])):
        cases = []
        for kk, m in shapes:
            xs = [0, 1, -1, 2 ** (kk - 1) - 1, -(2 ** (kk - 1) - 1), -(2 ** (kk - 1)), rnd.getrandbits(kk - 2), -rnd.getrandbits(kk - 2)]
            for i, x in enumerate(xs):
                cases.append(drive(fn, x, kk, m, "random"))
                if i in (1, 2, 5):
                    cases.append(drive(fn, x, kk, m, "0"))
                    cases.append(drive(fn, x, kk, m, "1"))
        out[name] = cases
    path = os.path.join(REPO, "tests", "golden", "fixedpoint.json")
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
    print(f"wrote {path} ({os.path.getsize(path)} bytes): " + ", ".join(f"{len(v)} {n}" for n, v in out.items() if isinstance(v, list)))


main()

#!/usr/bin/env python3
"""Writes tests/golden/share_comparison.json from the REFERENCE's own progs/mixins/share_comparison.py (the Equality mixin), integers
as decimal strings:

  * "modulus", and "nr": the constant of the reference's _b = 5 - 4 b;
  * "legendre": Equality.legendre_mod_p(Field(a)) for 0, 1, p - 1, 5, squares, non-squares and seeded residues;
  * "test_bit": Equality._gen_test_bit and Equality.gen_test_bit over cleartext stand-in shares: diff, the drawn b, r, rp, the opened c
    and the value the returned share holds -- equal and unequal diffs, both values of b;
  * "equal": whole Equality._prog runs at security parameter 1, 2, 3, 5 and 32: x, y, the drawn values in the order they were drawn
    (bits, rs, rps: one of each a test bit) and the value the result holds.

The stand-ins: a cleartext "share" (a class with the operators the coroutines use over the reference's own field; a product is
immediate, an open an awaitable that returns the value), a share array with multiplicative_product, and a preproc whose get_bit and
get_rand hand out seeded values and record them.  The reference's mpc.py and preprocessing.py need its NTL extension; they are
replaced by stand-ins before the import, and TypeCheck is told to accept them: run under python -O with DISABLE_TYPECHECKING set
(utils/typecheck.py:68), which this script does for itself.  Needs a checkout of the reference (its path is argv[1]); it is
imported, never copied, and no test runs this script -- the tests read the JSON only.

    python scratch/gen_share_comparison_golden.py PATH_TO_THE_REFERENCE
"""
import asyncio
import json
import os
import random
import subprocess
import sys
import types

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if len(sys.argv) != 2:
    raise SystemExit(__doc__)
REF = sys.argv[1]
if __debug__ or "DISABLE_TYPECHECKING" not in os.environ:
    raise SystemExit(subprocess.call([sys.executable, "-O", os.path.abspath(__file__), REF], env=dict(os.environ, DISABLE_TYPECHECKING="1")))


def install_reference():
    try:
        import gmpy2  # noqa: F401
    except ImportError:
        from sympy import isprime

        gmpy2 = types.ModuleType("gmpy2")
        gmpy2.is_prime = lambda n: bool(isprime(int(n)))
        gmpy2.mpz = int
        sys.modules["gmpy2"] = gmpy2
    for name in ("honeybadgermpc", "honeybadgermpc.progs", "honeybadgermpc.progs.mixins", "honeybadgermpc.utils"):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(REF, *name.split("."))]
        sys.modules[name] = pkg
    sys.path.insert(0, REF)
    from honeybadgermpc.field import GFElement

    mpc = types.ModuleType("honeybadgermpc.mpc")
    mpc.Mpc = type("Mpc", (), {})
    mpc.GFElement = GFElement
    sys.modules["honeybadgermpc.mpc"] = mpc
    sys.modules["honeybadgermpc.preprocessing"] = types.ModuleType("honeybadgermpc.preprocessing")


def main():
    install_reference()
    from honeybadgermpc.elliptic_curve import Subgroup
    from honeybadgermpc.field import GF
    from honeybadgermpc.progs.mixins.share_comparison import Equality

    p = Subgroup.BLS12_381
    field = GF(p)
    elem = type(field(0))
    rnd = random.Random(20261017)

    class Share:
        def __init__(self, v):
            self.v = v if isinstance(v, elem) else field(int(v))

        @staticmethod
        def _val(o):
            return o.v if isinstance(o, Share) else o

        def __add__(self, o):
            return Share(self.v + self._val(o))

        __radd__ = __add__

        def __sub__(self, o):
            return Share(self.v - self._val(o))

        def __mul__(self, o):
            return Share(self.v * self._val(o))

        __rmul__ = __mul__

        def open(self):
            async def opened():
                Share.opened.append(int(self.v.value))
                return self.v

            return opened()

    Share.opened = []

    class ShareArray:
        def __init__(self, shares):
            self.shares = shares

        async def multiplicative_product(self):
            out = Share(1)
            for s in self.shares:
                out = out * s
            return out

    class Preproc:
        """bit: "random", 0 or 1; replay: a list of values handed out again in order"""

        def __init__(self, bit="random", rands=None, replay=None):
            self.bit, self.rands, self.replay, self.drawn = bit, rands, replay, []

        def _next(self, fresh):
            v = self.replay.pop(0) if self.replay is not None else fresh()
            self.drawn.append(v)
            return Share(v)

        def get_bit(self, ctx):
            return self._next(lambda: rnd.getrandbits(1) if self.bit == "random" else int(self.bit))

        def get_rand(self, ctx):
            return self._next(lambda: self.rands.pop(0) if self.rands else rnd.randrange(p))

    class Ctx:
        pass

    Ctx.Share, Ctx.ShareArray, Ctx.field = Share, ShareArray, field

    def context(**kw):
        ctx = Ctx()
        ctx.preproc = Preproc(**kw)
        return ctx

    # ---- legendre_mod_p
    roots = [2, 3, 7, 12345, p - 2, rnd.randrange(p), rnd.randrange(p), rnd.randrange(p)]
    squares = [r * r % p for r in roots]
    values = [0, 1, p - 1, 5, 25, 2, 3, 4, p - 5, (p - 1) // 2, (p + 1) // 2] + squares + [5 * s % p for s in squares] + [rnd.randrange(p) for _ in range(24)]
    legendre = [{"a": str(a), "out": Equality.legendre_mod_p(field(a))} for a in values]
    assert all(c["out"] == 1 for c in legendre[11:19]) and all(c["out"] == -1 for c in legendre[19:27]) and legendre[3]["out"] == -1

    # ---- one test bit
    test_bit = []
    for diff in [0, 0, 0, 1, p - 1, 5, rnd.randrange(p), rnd.randrange(p), rnd.randrange(p), rnd.randrange(p)]:
        for b in (0, 1):
            ctx = context(bit=b)
            c, _b = asyncio.run(Equality._gen_test_bit(ctx, Share(diff)))
            drawn = list(ctx.preproc.drawn)
            assert len(drawn) == 3 and drawn[0] == b and int(_b.v.value) == 5 - 4 * b
            Share.opened.clear()
            out = asyncio.run(Equality.gen_test_bit(context(replay=list(drawn)), Share(diff)))
            assert Share.opened == [int(c.value)] and int(c.value) != 0
            test_bit.append({"diff": str(diff), "b": b, "r": str(drawn[1]), "rp": str(drawn[2]), "c": str(int(c.value)), "out": str(int(out.v.value))})

    # ---- the whole program
    equal = []
    for kappa in (1, 2, 3, 5, 32):
        for kind in ("equal", "unequal", "equal", "unequal", "off by one"):
            x = rnd.randrange(p)
            y = x if kind == "equal" else ((x + 1) % p if kind == "off by one" else rnd.randrange(p))
            ctx = context()
            Share.opened.clear()
            out = asyncio.run(Equality._prog(ctx, Share(x), Share(y), kappa))
            drawn = ctx.preproc.drawn
            assert len(drawn) == 3 * kappa and len(Share.opened) == kappa and 0 not in Share.opened
            equal.append({"kappa": kappa, "x": str(x), "y": str(y), "bits": "".join(str(v) for v in drawn[0::3]), "rs": [str(v) for v in drawn[1::3]],
                          "rps": [str(v) for v in drawn[2::3]], "cs": [str(v) for v in Share.opened], "out": str(int(out.v.value))})
            assert (int(out.v.value) != 0) if kind == "equal" else True

    out = {"modulus": str(p), "nr": 5, "legendre": legendre, "test_bit": test_bit, "equal": equal}
    path = os.path.join(REPO, "tests", "golden", "share_comparison.json")
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
    print(f"wrote {path} ({os.path.getsize(path)} bytes): " + ", ".join(f"{len(v)} {n}" for n, v in out.items() if isinstance(v, list)))


main()

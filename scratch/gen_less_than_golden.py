#!/usr/bin/env python3
"""Writes tests/golden/less_than.json from the REFERENCE's own progs/mixins/share_comparison.py (the LessThan mixin, Reistad's
comparison), integers as decimal strings: "modulus", and "cases": whole LessThan._prog runs over cleartext stand-in shares -- a, b, the
two dealt residues r and s (get_share_bits is called twice: _transform_comparison, _extract_lsb), the two opened values c and d, and
the value the result holds.  a < b, a > b, a == b, b = a + 1, b = a - 1, a = 0 and b = (p - 3) / 2, the largest value the mixin allows,
all with a, b < (p - 1) / 2.

The stand-ins: a cleartext "share" (a class with + - * and the reflected operators over the reference's own field; a product is
immediate, an open an awaitable that returns the value) and a preproc whose get_share_bits hands out a seeded residue with its bits,
least significant first, and records it.  The reference's mpc.py and preprocessing.py need its NTL extension; they are replaced by
stand-ins before the import, and TypeCheck is told to accept them: run under python -O with DISABLE_TYPECHECKING set
(utils/typecheck.py:68), which this script does for itself.  Needs a checkout of the reference (its path is argv[1]); it is
imported, never copied, and no test runs this script -- the tests read the JSON only.

    python scratch/gen_less_than_golden.py PATH_TO_THE_REFERENCE
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
    from honeybadgermpc.progs.mixins.share_comparison import LessThan

    p = Subgroup.BLS12_381
    field = GF(p)
    elem = type(field(0))
    rnd = random.Random(20261018)
    L = p.bit_length()
    assert L == 255                                      # _transform_comparison formats c in 255 bits (:128)

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

        def __rsub__(self, o):
            return Share(self._val(o) - self.v)

        def __mul__(self, o):
            return Share(self.v * self._val(o))

        __rmul__ = __mul__

        def open(self):
            async def opened():
                Share.opened.append(int(self.v.value))
                return self.v

            return opened()

    Share.opened = []

    class Preproc:
        def __init__(self):
            self.drawn = []

        def get_share_bits(self, ctx):
            v = rnd.randrange(p)
            self.drawn.append(v)
            return Share(v), [Share((v >> i) & 1) for i in range(L)]

    class Ctx:
        pass

    Ctx.Share, Ctx.field = Share, field

    half = (p - 1) // 2                                  # a, b < half
    below = lambda: rnd.randrange(half)                  # noqa: E731
    pairs = []
    for _ in range(8):
        a, b = sorted((below(), below()))
        pairs += [("less", a, b), ("greater", b, a)]
    for _ in range(5):
        a = below()
        pairs.append(("equal", a, a))
    pairs += [("equal", 0, 0), ("equal", half - 1, half - 1)]
    for _ in range(4):
        a = rnd.randrange(1, half - 1)
        pairs += [("less", a, a + 1), ("greater", a, a - 1)]
    pairs += [("less", 0, 1), ("greater", 1, 0), ("less", 0, below()), ("less", 0, half - 1), ("greater", below(), 0)]
    pairs += [("less", below(), half - 1), ("less", half - 2, half - 1), ("greater", half - 1, below()), ("greater", half - 1, half - 2), ("greater", half - 1, 0)]
    assert half - 1 == (p - 3) // 2

    cases = []
    for kind, a, b in pairs:
        ctx = Ctx()
        ctx.preproc = Preproc()
        Share.opened.clear()
        out = asyncio.run(LessThan._prog(ctx, Share(a), Share(b)))
        r, s = ctx.preproc.drawn
        c, d = Share.opened
        res = int(out.v.value)
        assert c == (2 * (a - b) + r) % p and res == (1 if a < b else 0) == (kind == "less"), (kind, a, b, res)
        cases.append({"a": str(a), "b": str(b), "r": str(r), "s": str(s), "c": str(c), "d": str(d), "out": str(res)})

    out = {"modulus": str(p), "cases": cases}
    path = os.path.join(REPO, "tests", "golden", "less_than.json")
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
    print(f"wrote {path} ({os.path.getsize(path)} bytes): {len(cases)} cases")


main()

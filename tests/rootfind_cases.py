"""One table of root-finding cases for tests/test_solver_host.py (the level loop over host memory) and tests/test_gpu_solver.py (the
same inputs on the device, whose unsorted output must equal the host walk's element for element).  Plain Python ints,
rootfind_model and edge_values only: nothing here touches the library.

A case is Case(id, p, n_limbs, roots, coeffs, expected): exactly one of `roots` (the polynomial is their product; `expected` is the
list ascending) and `coeffs` (a monic polynomial with a factor of degree above one; `expected` is None) is set; coeffs_of(case) gives
the coefficients either way.  What each group is for:

  tile-*      degrees either side of the 64-output tiles of k_rf_sqr / k_rf_red (RF_TI) and of the four waves that split a sum
  seq-*       degrees 2, 3 and 200 over BLS12-381 for the tests that reuse one context's temporaries (large, then small)
  edge-*      tests/edge_values.py as roots: the pool, the pool with its Montgomery pre-images (crosses a tile), the pool with every
              third value doubled (the repeated-root loop on edge values)
  small-*     small fields above SMALL_DEGREE: shifts hit roots (gcd(s, h) is not trivial) and, at 61 and 67 -- either side of the 64
              draws of a node --, most of the field is a root; each also with a few roots repeated
  mult-*      multiplicities above SMALL_DEGREE: a gcd(f, f') of degree 50 at degree 150, 65 rounds, a repeated root beside a tile edge
  invalid-*   an irreducible factor times enough linear factors for the tiled chain: the verdict after one level
  seeds-*     a degree-70 case for sixteen consecutive seeds

NEWTON is the table for Newton's identities alone: the power sums of k random roots and one vector of pool values at k = 255, 256,
257 -- either side of the k at which a thread of the 256 owns two integers of the 1 / m table and a step's sum two terms."""
import collections
import functools
import random

import edge_values as ev
import rootfind_model as model

BLS = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
P256 = (1 << 256) - 189
P25519 = (1 << 255) - 19
P64 = (1 << 64) - 59
GOLDILOCKS = (1 << 64) - (1 << 32) + 1

# name -> (modulus, limbs of the context)
MODULI = {"bls": (BLS, 4), "p256": (P256, 4), "p25519": (P25519, 4), "p64": (P64, 1), "gold": (GOLDILOCKS, 1),
          "65537": (65537, 1), "257": (257, 1), "67": (67, 1), "61": (61, 1), "13": (13, 1)}
LARGE = ("bls", "p256", "p25519", "p64", "gold")
WIDE = ("bls", "p256", "p25519")

Case = collections.namedtuple("Case", "id p n_limbs roots coeffs expected")


def _rnd(tag):
    return random.Random("rootfind_cases:" + tag)


def _distinct(tag, p, n, avoid=()):
    """n distinct residues, none in `avoid`"""
    rnd = _rnd(tag)
    if p < 1 << 20:
        return rnd.sample([v for v in range(p) if v not in avoid], n)
    out = set()
    while len(out) < n:
        v = rnd.randrange(p)
        if v not in avoid:
            out.add(v)
    out = sorted(out)
    rnd.shuffle(out)
    return out


def _valid(cid, name, roots):
    p, nl = MODULI[name]
    roots = [r % p for r in roots]
    assert 1 <= len(roots) < p, cid
    return Case(cid, p, nl, roots, None, sorted(roots))


def _invalid(cid, name, factor, roots):
    """factor (no root in GF(p), or a power of such a polynomial) times prod (x - r)"""
    p, nl = MODULI[name]
    coeffs = model.poly_mul(factor, model.poly_from_roots([r % p for r in roots], p), p)
    assert coeffs[-1] == 1 and len(coeffs) - 1 < p, cid
    return Case(cid, p, nl, None, coeffs, None)


def _repeat_a_few(roots):
    """the same number of roots, the first one twice and the second three times"""
    return roots[:-3] + [roots[0], roots[1], roots[1]]


def _build():
    out = []
    # ---- tile and wave edges, distinct random roots
    for name, degrees in (("bls", (63, 64, 65, 127, 128, 129)), ("p256", (64, 65, 129)), ("p64", (64, 65, 129)), ("p25519", (129,))):
        for d in degrees:
            out.append(_valid(f"tile-{name}-{d}", name, _distinct(f"tile-{name}-{d}", MODULI[name][0], d)))
    # ---- the call sequence of the reuse tests: large, small, large
    out.append(_valid("seq-bls-200", "bls", _distinct("seq-200", BLS, 200)))
    out.append(_valid("seq-bls-3", "bls", _distinct("seq-3", BLS, 3)))
    out.append(_valid("seq-bls-2", "bls", _distinct("seq-2", BLS, 2)))
    # ---- edge-valued roots
    for name in LARGE:
        p, nl = MODULI[name]
        pool = ev.edge_pool(p, nl)
        out.append(_valid(f"edge-pool-{name}", name, pool))
        out.append(_valid(f"edge-operands-{name}", name, ev.operands(p, nl)))
        out.append(_valid(f"edge-doubled-{name}", name, pool + pool[::3]))
    # ---- small fields in the tiled path
    small = [("small-257-256", "257", [v for v in range(257) if v != 100]),
             ("small-257-100", "257", _distinct("small-257-100", 257, 100)),
             ("small-65537-300", "65537", [v % 65537 for v in range(65400, 65700)]),          # consecutive, through p - 1, 0, 1
             ("small-65537-130", "65537", _distinct("small-65537-130", 65537, 130)),
             ("small-67-66", "67", _distinct("small-67-66", 67, 66)),
             ("small-61-60", "61", _distinct("small-61-60", 61, 60)),
             ("small-13-12", "13", _distinct("small-13-12", 13, 12))]
    for cid, name, roots in small:
        out.append(_valid(cid, name, roots))
        out.append(_valid(cid + "-rep", name, _repeat_a_few(roots)))
    # ---- multiplicities
    for name in ("bls", "p64"):
        p = MODULI[name][0]
        r = _distinct(f"mult-150-{name}", p, 100)
        out.append(_valid(f"mult-150-{name}", name, r[:60] + 2 * r[60:90] + 3 * r[90:]))
        out.append(_valid(f"mult-65x-{name}", name, [r[0]] * 65))
    r = _distinct("mult-33x+40", BLS, 41)
    out.append(_valid("mult-33x+40-bls", "bls", [r[0]] * 33 + r[1:]))
    r = _distinct("mult-2x+127", BLS, 128)
    out.append(_valid("mult-2x+127-bls", "bls", [r[0]] * 2 + r[1:]))
    # ---- invalid: an irreducible factor times linear factors
    for name in ("bls", "p64", "p256", "257"):
        p = MODULI[name][0]
        c = model.non_residue(p)
        quad = [(-c) % p, 0, 1]
        # (x^2 - c has no root, so the linear factors may be any distinct residues)
        for n in (63, 64, 127):
            out.append(_invalid(f"invalid-quad-{n}-{name}", name, quad, _distinct(f"invalid-quad-{n}-{name}", p, n)))
        out.append(_invalid(f"invalid-cubic-100-{name}", name, model.irreducible_cubic(p), _distinct(f"invalid-cubic-{name}", p, 100)))
        out.append(_invalid(f"invalid-quadsq-70-{name}", name, model.poly_mul(quad, quad, p), _distinct(f"invalid-quadsq-{name}", p, 70)))
        r = _distinct(f"invalid-quad-rep-{name}", p, 45)
        out.append(_invalid(f"invalid-quad-rep-65-{name}", name, quad, r[:30] + 2 * r[30:40] + 3 * r[40:]))
    # ---- sixteen seeds
    out.append(_valid("seeds-p64-70", "p64", _distinct("seeds-p64-70", P64, 70)))
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids)
    return out


CASES = _build()
BY_ID = {c.id: c for c in CASES}

# (case, seed) pairs beyond seed 0, which every case runs with
SEEDS = {"tile-p256-65": (1, 1 << 63, (1 << 64) - 1),
         "mult-150-p64": (1, 1 << 63, (1 << 64) - 1),
         "small-67-66": (1, 1 << 63, (1 << 64) - 1),
         "seeds-p64-70": tuple(range(1, 16))}

# what the reuse tests call, in order, on one context and stream
SEQUENCE = ("seq-bls-200", "seq-bls-3", "tile-bls-129", "seq-bls-2", "invalid-quad-63-bls", "seq-bls-200")
# ... and on two contexts in turn
ALTERNATING = ("tile-bls-65", "tile-p64-129", "seq-bls-3", "tile-p64-64", "invalid-quad-64-bls", "mult-150-p64", "mult-33x+40-bls",
               "invalid-quad-63-p64", "tile-bls-64", "seeds-p64-70")


@functools.lru_cache(maxsize=None)
def coeffs_of(case_id):
    """the monic polynomial of a case, coefficient of x^i at index i (a tuple: shared, not to be changed)"""
    c = BY_ID[case_id]
    return tuple(c.coeffs if c.coeffs is not None else model.poly_from_roots(c.roots, c.p))


@functools.lru_cache(maxsize=None)
def power_sums_of(case_id):
    return tuple(model.power_sums_from_poly(list(coeffs_of(case_id)), BY_ID[case_id].p))


def degree(case):
    return len(case.roots) if case.roots is not None else len(case.coeffs) - 1


def multiplicity(case):
    """the largest multiplicity among the roots of a valid case: the rounds of the repeated-root loop"""
    return max(collections.Counter(case.roots).values())


NewtonCase = collections.namedtuple("NewtonCase", "id p n_limbs sums")


def _build_newton():
    out = []
    for name in ("bls", "p256", "p64"):
        p, nl = MODULI[name]
        pool = ev.edge_pool(p, nl)
        for k in (255, 256, 257):
            out.append(NewtonCase(f"newton-roots-{name}-{k}", p, nl, model.power_sums_from_roots(_distinct(f"newton-{name}-{k}", p, k), p)))
            rnd = _rnd(f"newton-pool-{name}-{k}")
            out.append(NewtonCase(f"newton-pool-{name}-{k}", p, nl, [rnd.choice(pool) for _ in range(k)]))
    return out


NEWTON = _build_newton()


def newton_pool_vector(k=1024):
    """k pool values over BLS12-381: the longest vector hb_rf_newton takes"""
    pool = ev.edge_pool(BLS, 4)
    rnd = _rnd(f"newton-pool-bls-{k}")
    return [rnd.choice(pool) for _ in range(k)]

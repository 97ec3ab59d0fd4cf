"""Shared by tests/test_pairing_host.py and tests/test_gpu_pairing.py: marshalling for hb_selftest_pairing (the bodies of
csrc/hb_fq12_elem.hpp and csrc/hb_pair.hip run on the host), the trapdoor CRS of g1_crs_support with its G2 half, and the KZG cases both
files run.  The model is honeybadgermpc_amd.bls12_381_pairing (Python ints); every comparison is exact."""
import ctypes
import functools
import random

import numpy as np

import g1_crs_support as cs
import g1_support as s

from honeybadgermpc_amd import _capi
from honeybadgermpc_amd.bls12_381 import G1, Q, R
from honeybadgermpc_amd.bls12_381_pairing import Fq12, G2, pairing_product, prepare_g2

TOWER, PREPARE, PRODUCT = 0, 1, 2
GT, VERDICT = 0, 1
ALPHA, LAM = cs.ALPHA, cs.LAM


def selftest(what, operands, flags, arg, count, out_words):
    lib = _capi.load_library()
    operands = [np.ascontiguousarray(o) for o in operands]
    ptrs = (ctypes.c_void_p * 5)(*([o.ctypes.data for o in operands] + [None] * (5 - len(operands))))
    out = np.full(max(out_words, 2), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    rc = lib.hb_selftest_pairing(what, ptrs, flags, arg, _capi.np_ptr(out), count)
    return rc, out


def gt_words(elems):
    """list of Fq12 -> (count, 72) uint64"""
    return s.words([c for e in elems for c in e.coords()], 6).reshape(len(elems), 72)


def gt_unwords(arr):
    vals = s.unwords(np.ascontiguousarray(arr).reshape(-1), 6)
    return [Fq12.from_coords(vals[12 * k:12 * k + 12]) for k in range(len(vals) // 12)]


def fq12_of(coords):
    return Fq12.from_coords([c % Q for c in coords])


def tower(op, a, b=None, arg=0):
    """the self test's tower operation on lists of Fq12 -> list of Fq12"""
    ops = [gt_words(a)] + ([gt_words(b)] if b is not None else [])
    rc, out = selftest(TOWER, ops, op, arg, len(a), 72 * len(a))
    assert rc == 0, (op, rc)
    return gt_unwords(out[:72 * len(a)])


def tower_words(op, a, b=None, arg=0):
    """the same on (count, 72) uint64 words -> (count, 72) uint64"""
    rc, out = selftest(TOWER, [a] + ([b] if b is not None else []), op, arg, len(a), 72 * len(a))
    assert rc == 0, (op, rc)
    return out[:72 * len(a)].reshape(len(a), 72)


def coeff_words(q):
    """the 204 Fq2 coefficients of a host G2 as hb_pair_prepare takes them"""
    return s.words([v for triple in prepare_g2(q) for c in triple for v in (c.c0, c.c1)], 6)


@functools.lru_cache(maxsize=None)
def _host_table_cached(raw):
    q = G2.from_uncompressed(raw)
    words = _capi.load_library().hb_pair_table_bytes() // 8
    rc, out = selftest(PREPARE, [coeff_words(q)], 0, 0, 1, words)
    assert rc == 0
    return out[:words].copy()


def host_table(q):
    return _host_table_cached(q.to_uncompressed())


def host_product(rows, qs, mode=GT):
    """rows: `count` lists of K host G1; qs: K host G2 -> list of Fq12, or (verdicts, rejected)"""
    count, K = len(rows), len(qs)
    pts = s.points([p for row in rows for p in row])
    out_words = 72 * count if mode == GT else (count + 2) // 2 + 1
    rc, out = selftest(PRODUCT, [pts] + [host_table(q) for q in qs], K, mode, count, out_words)
    assert rc == 0
    if mode == GT:
        return gt_unwords(out[:72 * count])
    v = out.view(np.int32)
    return [int(x) for x in v[:count]], int(v[count])


def model_product(row, qs):
    return pairing_product(list(zip(row, qs)))


# ---- the trapdoor CRS: gs[j] = alpha^j g, hs[j] = lam alpha^j g, ghats = [ghat, alpha ghat]
def ghats(alpha=ALPHA):
    gh = G2.generator() ** 0x5EED5EED5EED
    return [gh, gh ** alpha]


def kzg_item(t, x, seed=0):
    """-> (c, x, share, aux, w): an honest opening at x of a random polynomial of degree t under the trapdoor CRS"""
    rnd = random.Random(700 + 10 * t + seed)
    phi = [rnd.randrange(R) for _ in range(t + 1)]
    hat = [rnd.randrange(R) for _ in range(t + 1)]
    g = G1.generator()
    c = cs.commitment_model(phi, hat)
    share, aux = cs.poly_at(phi, x), cs.poly_at(hat, x)
    q, _ = cs.quotient_model(phi, x)
    qh, _ = cs.quotient_model(hat, x)
    w = g ** ((cs.poly_at(q, ALPHA) + LAM * cs.poly_at(qh, ALPHA)) % R) if t else G1.one()
    assert cs.witness_holds(c, share, aux, w, x)
    return c, x, share, aux, w


def kzg_lhs(c, x, share, aux, w):
    """-> (A, -w): A = c - share g0 - aux h0 + x w, the left sides of the two-pairing form e(A, ghat0) e(-w, ghat1) == 1"""
    g = G1.generator()
    h = g ** LAM
    return c * (g ** share).invert() * (h ** aux).invert() * (w ** x), w.invert()


def kzg_cases(t, x=5):
    """name -> ((c, x, share, aux, w), expected verdict)"""
    c, x, share, aux, w = kzg_item(t, x)
    g = G1.generator()
    cases = {
        "honest": ((c, x, share, aux, w), True),
        "wrong share": ((c, x, (share + 1) % R, aux, w), False),
        "wrong aux": ((c, x, share, (aux + 1) % R, w), False),
        "wrong witness": ((c, x, share, aux, w * g), False),
        "wrong commitment": ((c * g, x, share, aux, w), False),
        "wrong index": ((c, x + 1, share, aux, w), t == 0),       # t = 0: a constant opens to the same value everywhere
    }
    return cases

"""Shared by tests/test_g1_crs_host.py and tests/test_gpu_g1_crs.py: marshalling for hb_selftest_g1_crs (the bodies of csrc/hb_crs.hip run
on the host), the Python-int model, and the cases both files run.

Model.  The common reference string has a KNOWN trapdoor: gs[j] = alpha^j g, hs[j] = alpha^j h, h = lam g.  So
    sum_k a_k gs[k] + b_k hs[k] = (a(alpha) + lam b(alpha)) g                                one host exponentiation a row,
a commitment to (phi, hat) must equal (phi(alpha) + lam hat(alpha)) g, and a witness w of the evaluation at x is checked by the KZG
identity inside G1, with no pairing:  c - share g - aux h == (alpha - x) w.
The scalars are plain 256-bit integers; the points have order R, so the model reduces mod R."""
import ctypes
import functools
import random

import numpy as np

import g1_support as s

from honeybadgermpc_amd.bls12_381 import G1, R

TABLE, QUOTIENT, MSM = 0, 1, 2
FULL = (1 << 256) - 1
SPLITS = [1, 2, 64, 256]
ALPHA, LAM = 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA99887766554433221100F1E2 % R, 0x0123456789ABCDEF00112233445566778899AABBCCDDEEFF0F1E2D3C4B5A6978 % R


def selftest(what, operands, flags, arg, count, out_words, fill=0x5A5A5A5A5A5A5A5A):
    """-> (rc, uint64 array of out_words words, `fill` where nothing was written); an operand may be None"""
    from honeybadgermpc_amd._capi import load_library, np_ptr

    lib = load_library()
    operands = [None if o is None else np.ascontiguousarray(o) for o in operands]
    ptrs = (ctypes.c_void_p * 4)(*([None if o is None else o.ctypes.data for o in operands] + [None] * (4 - len(operands))))
    out = np.full(max(out_words, 2), fill, dtype=np.uint64)
    rc = lib.hb_selftest_g1_crs(what, ptrs, flags, arg, np_ptr(out), count)
    return rc, out


def table_words(c):
    from honeybadgermpc_amd._capi import load_library

    nbytes = load_library().hb_g1_table_bytes(c)
    assert nbytes > 0 and nbytes % 16 == 0
    return nbytes // 8


def crs_points(n, alpha=ALPHA, lam=LAM):
    """-> (gs, hs): n host G1 each"""
    g = G1.generator()
    return [g ** pow(alpha, j, R) for j in range(n)], [g ** (lam * pow(alpha, j, R) % R) for j in range(n)]


@functools.lru_cache(maxsize=None)
def host_tables(n, c, alpha=ALPHA, lam=LAM):
    """-> (tables of gs, tables of hs) built by the self test, (n * table_words(c),) uint64 each.  Computed once a CRS."""
    out = []
    for fam in crs_points(n, alpha, lam):
        rc, tab = selftest(TABLE, [s.points(fam)], 0, c, n, n * table_words(c), fill=0)
        assert rc == 0
        out.append(tab)
    return tuple(out)


def host_msm(case, split):
    """the self test on a case of msm_cases() -> (rows, 12) uint64"""
    tg, th = host_tables(case["n"], case["c"], case["alpha"], case["lam"])
    a, b = case["a"], case["b"]
    rows, terms = len(a), case["terms"]
    aw = s.words([v for row in a for v in row], 4) if rows * terms else np.zeros((1, 4), dtype=np.uint64)
    bw = None if b is None else (s.words([v for row in b for v in row], 4) if rows * terms else np.zeros((1, 4), dtype=np.uint64))
    rc, out = selftest(MSM, [tg, None if b is None else th, aw, bw], case["c"] | split << 8, terms | case["n"] << 32, rows, rows * 12)
    assert rc == 0, (case["name"], split)
    return out[:rows * 12].reshape(rows, 12)


def model_msm(case):
    """(a(alpha) + lam b(alpha)) g a row -> (rows, 12) uint64"""
    g = G1.generator()
    alpha, lam = case["alpha"], case["lam"]
    pw = [pow(alpha, k, R) for k in range(case["terms"])]
    rows = []
    for m, ra in enumerate(case["a"]):
        e = sum(v * p for v, p in zip(ra, pw))
        if case["b"] is not None:
            e += lam * sum(v * p for v, p in zip(case["b"][m], pw))
        rows.append(g ** (e % R))
    return s.points(rows)


@functools.lru_cache(maxsize=None)
def msm_cases():
    """name -> case.  Scalars: rows of `terms` plain 256-bit integers.  The t = 21 case is the only one at c = 4 with many bases."""
    rnd = random.Random(2024)
    cases = {}

    def add(name, n, terms, c, a, b=None, alpha=ALPHA, lam=LAM):
        assert all(len(r) == terms for r in a) and (b is None or all(len(r) == terms for r in b))
        cases[name] = dict(name=name, n=n, terms=terms, c=c, a=a, b=b, alpha=alpha, lam=lam)

    big = lambda: rnd.randrange(1 << 256)
    top8, top4 = 0xFF << 248, 0xF << 252
    edge = [0, 1, R - 1, FULL, top8, 1 << 248]
    # F = 2, terms < n_bases, K = 3 at c = 8: U = 192 is no multiple of S = 128
    add("two families, edge scalars", 4, 3, 8, [edge[:3], edge[3:], [big(), big(), big()]], [edge[3:], edge[:3], [big(), 0, big()]])
    add("one family", 3, 3, 8, [[big(), R - 1, top8], [0, 0, 0], [1, 0, FULL]])
    add("one family, window 4", 3, 2, 4, [[big(), top4], [FULL, 1 << 252], [0, 1]])
    add("two families, window 4", 3, 3, 4, [[big(), R - 1, top4], [FULL, 0, 1]], [[0, big(), 1 << 252], [R - 1, FULL, big()]])
    # alpha = 1: every base of a family is the same point; equal digits meet it twice: the doubling branch of the mixed addition
    add("all bases equal", 3, 3, 8, [[5, 5, 5], [big()] * 3], [[7, 7, 0], [R - 1, R - 1, 1]], alpha=1)
    # h = -g and a == b: every row is the identity
    x, y = big(), big()
    add("a == b over h = -g", 2, 2, 8, [[x, y], [1, 0], [FULL, FULL]], [[x, y], [1, 0], [FULL, FULL]], lam=R - 1)
    # alpha = 1, h = -g: x g, then -x g window by window down to the identity, then z (-g) from the identity on
    add("through the identity and on", 2, 2, 8, [[x, 0], [0, y]], [[x, y], [y, 0]], alpha=1, lam=R - 1)
    # K = 1, F = 1, c = 8: U = 32 < S = 256, most lanes hold the identity
    add("one term", 1, 1, 8, [[big()], [0], [top8], [3]])
    # the commitment's shape at t = 21
    add("t = 21, window 4", 22, 22, 4, [[big() % R for _ in range(22)]], [[big() % R for _ in range(22)]])
    return cases


# ---- the quotient
def quotient_model(phi, x):
    """-> (q, rem): phi(X) - rem = (X - x) q(X), ints mod R"""
    t = len(phi) - 1
    q, acc = [0] * t, phi[t]
    for j in range(t - 1, -1, -1):
        q[j] = acc
        acc = (phi[j] + x * acc) % R
    return q, acc


def host_quotient(phis, xs):
    """-> (q[b][i] lists, rem[b][i]) from the self test"""
    B, n, n_coef = len(phis), len(xs), len(phis[0])
    pw = s.words([v for p in phis for v in p], 4)
    xw = s.words(xs, 4) if n else np.zeros((1, 4), dtype=np.uint64)
    nq = B * n * (n_coef - 1)
    rc, out = selftest(QUOTIENT, [pw, xw], n_coef, n, B, (nq + B * n) * 4)
    assert rc == 0
    q = s.unwords(out[:nq * 4], 4) if nq else []
    rem = s.unwords(out[nq * 4:(nq + B * n) * 4], 4) if B * n else []
    t = n_coef - 1
    return [[q[(b * n + i) * t:(b * n + i + 1) * t] for i in range(n)] for b in range(B)], [rem[b * n:(b + 1) * n] for b in range(B)]


def quotient_case(t, B=4, seed=0):
    """-> (phis, xs): all R - 1, all zero, a zero top coefficient, random; x in 0, 1, R - 1, random"""
    rnd = random.Random(100 + t + seed)
    phis = [[R - 1] * (t + 1), [0] * (t + 1), [rnd.randrange(R) for _ in range(t)] + [0]]
    while len(phis) < B:
        phis.append([rnd.randrange(R) for _ in range(t + 1)])
    return phis[:B], [0, 1, R - 1, rnd.randrange(R)]


# ---- the trapdoor checks
def poly_at(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def commitment_model(phi, hat, alpha=ALPHA, lam=LAM):
    return G1.generator() ** ((poly_at(phi, alpha) + lam * poly_at(hat, alpha)) % R)


def witness_holds(c, share, aux, w, x, alpha=ALPHA, lam=LAM):
    """c - share g - aux h == (alpha - x) w, on host G1 (written multiplicatively)"""
    g = G1.generator()
    return c * (g ** ((share + lam * aux) % R)).invert() == w ** ((alpha - x) % R)

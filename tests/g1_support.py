"""Shared by tests/test_g1_host.py and tests/test_gpu_g1.py: marshalling for hb_selftest_g1 (the G1 kernels' bodies run on the host),
the Python-int models of the entry points, and the inputs with the edge scalars and exceptional operands both files use."""
import ctypes
import functools
import os
import random

import numpy as np

from conftest import GOLDEN

from honeybadgermpc_amd.bls12_381 import G1, Q, R

FQ_MUL, SCALAR_MUL, ADD, CHECK, TABLE, COMMIT, EVAL, VERIFY = range(8)
K_BCAST, P_BCAST = 1, 2
SUBTRACT, GENERAL, DOUBLE = 1, 2, 4
M64 = (1 << 64) - 1
EDGE_SCALARS = [0, 1, 2, R - 1, R, 1 << 255, (1 << 256) - 1]
INDICES = [0, 1, 2, 3, 64, 255, 256, 65535, (1 << 32) - 1]


def words(values, n):
    """ints -> (len, n) uint64, little-endian words"""
    return np.array([[(int(v) >> (64 * k)) & M64 for k in range(n)] for v in values], dtype=np.uint64).reshape(len(values), n)


def unwords(arr, n):
    flat = np.asarray(arr, dtype=np.uint64).reshape(-1, n)
    return [sum(int(w) << (64 * k) for k, w in enumerate(row)) for row in flat]


def points(ps):
    """host G1 (or raw 12-word lists, for points off the curve) -> (len, 12) uint64"""
    return np.array([p.to_limbs() if isinstance(p, G1) else list(p) for p in ps], dtype=np.uint64).reshape(len(ps), 12)


def raw_point(x, y):
    return [(v >> (64 * k)) & M64 for v in (x, y) for k in range(6)]


def unpoints(arr):
    return [G1.from_limbs(row.tolist()) for row in np.asarray(arr, dtype=np.uint64).reshape(-1, 12)]


def selftest(what, operands, flags, arg, count, out_words):
    """-> (rc, uint64 array of out_words words)"""
    from honeybadgermpc_amd._capi import load_library, np_ptr

    lib = load_library()
    operands = [np.ascontiguousarray(o) for o in operands]
    ptrs = (ctypes.c_void_p * 6)(*([o.ctypes.data for o in operands] + [None] * (6 - len(operands))))
    out = np.zeros(max(out_words, 2), dtype=np.uint64)
    rc = lib.hb_selftest_g1(what, ptrs, flags, arg, np_ptr(out), count)
    return rc, out


def host_table(base, c):
    from honeybadgermpc_amd._capi import load_library

    nbytes = load_library().hb_g1_table_bytes(c)
    assert nbytes > 0 and nbytes % 16 == 0
    rc, tab = selftest(TABLE, [points([base])], 0, c, 1, nbytes // 8)
    assert rc == 0
    return tab


@functools.lru_cache(maxsize=None)
def crs():
    """(g, h): g the generator, h an independent-looking point"""
    return G1.generator(), G1.rand("h")


@functools.lru_cache(maxsize=None)
def tables(c, which="h"):
    """host tables (tg, th) for window c; which = 'h': the CRS; 'shift': h = 2^c * g, whose table is g's moved up a window"""
    g, h = crs()
    if which == "shift":
        h = g ** (1 << c)
    return host_table(g, c), host_table(h, c)


@functools.lru_cache(maxsize=None)
def vectors():
    with open(os.path.join(GOLDEN, "g1_compressed_valid_test_vectors.dat"), "rb") as f:
        data = f.read()
    assert len(data) == 48000
    return [G1.decompress(data[48 * k:48 * k + 48]) for k in range(1000)]


def off_subgroup_point():
    x = 1
    while True:
        p = G1.lift_x(x)
        if p is not None and not p.in_subgroup():
            return p
        x += 1


def off_curve_raw():
    """12 words of a point that is NOT on the curve, coordinates below Q"""
    g = G1.generator()
    return raw_point(g.x, (g.y + 1) % Q)


def window_scalars(c):
    """every window digit 0, every digit 2^c - 1, a single non-zero digit in the top window (1 and 2^c - 1), a single digit at the bottom"""
    top = 256 - c
    return [0, (1 << 256) - 1, 1 << top, ((1 << c) - 1) << top, (1 << c) - 1]


def exceptional_pairs():
    g = G1.generator()
    p, o = g ** 5, G1.one()
    return [(o, o), (o, p), (p, o), (p, p), (p, p.invert()), (p, g ** 7)]


def mul_model(k, p):
    """k a plain integer (not reduced: the kernel reads 256 bits as they are; the points used have order R)"""
    return p ** (k % R)


def eval_model(cs, i):
    acc = G1.one()
    for c in reversed(cs):
        acc = acc ** i * c
    return acc


def scalar_mul_case(count, seed=0):
    """-> (ks, pts): edge scalars at both ends, points from the test vectors"""
    rnd = random.Random(seed)
    vs = vectors()
    ks = [rnd.randrange(1 << 256) for _ in range(count)]
    pts = [vs[1 + (i % 999)] for i in range(count)]
    for j, k in enumerate(EDGE_SCALARS):
        if j < count:
            ks[j] = k
        if count - 1 - j >= 0:
            ks[count - 1 - j] = k
    return ks, pts


def add_case(count, seed=0):
    rnd = random.Random(seed)
    vs = vectors()
    pairs = [(vs[rnd.randrange(1, 1000)], vs[rnd.randrange(1, 1000)]) for _ in range(count)]
    ex = exceptional_pairs()
    for j, pr in enumerate(ex):
        if j < count:
            pairs[j] = pr
        if count - 1 - j >= 0:
            pairs[count - 1 - j] = pr
    return pairs


def commit_case(count, c, seed=0):
    rnd = random.Random(seed)
    a = [rnd.randrange(R) for _ in range(count)]
    b = [rnd.randrange(R) for _ in range(count)]
    ws = window_scalars(c)
    edge = [(x, y) for x in ws for y in (ws[0], ws[1], ws[3])]
    for j, (x, y) in enumerate(edge):
        if j < count:
            a[j], b[j] = x, y
        if count - 1 - j >= 0:
            a[count - 1 - j], b[count - 1 - j] = y, x
    return a, b


def eval_case(B, n_coef, seed=0):
    """B vectors of n_coef commitments: random multiples of the generator, with at the first and last item identity entries, all-equal
    entries and C_1 = -C_0"""
    rnd = random.Random(seed)
    vs = vectors()
    cs = [[vs[rnd.randrange(1, 1000)] for _ in range(n_coef)] for _ in range(B)]
    o = G1.one()
    special = [[vs[7]] * n_coef, [o] * n_coef, [o if j % 2 else vs[9] for j in range(n_coef)]]
    if n_coef >= 2:
        special.append([vs[11], vs[11].invert()] + [vs[3]] * (n_coef - 2))
        special.append([vs[5]] * (n_coef - 1) + [o])
    for j, row in enumerate(special):
        if j < B:
            cs[j] = row
        if B - 1 - j > j:
            cs[B - 1 - j] = row
    return cs


def verify_case(B, t, i, bad=(), seed=0):
    """honest items for recipient i, then one change an entry of `bad`: (position, kind), kind in 'share', 'witness', 'swap', 'off'.
    -> (cs rows (host G1 or raw words), shares, witnesses, expected verdicts)"""
    rnd = random.Random(seed)
    g, h = crs()
    vs = vectors()
    n_coef = t + 1
    # commitments from SMALL exponents keep the model cheap: cs[b][j] = phi_j g + hat_j h with phi_j, hat_j < 1000 from the vectors of g and a table of h
    hs = [G1.one()]
    for _ in range(40):
        hs.append(hs[-1] * h)
    phi = [[rnd.randrange(1000) for _ in range(n_coef)] for _ in range(B)]
    hat = [[rnd.randrange(len(hs)) for _ in range(n_coef)] for _ in range(B)]
    if B > 2:
        phi[1], hat[1] = [0] * n_coef, [0] * n_coef                       # every commitment the identity: O == 0 g + 0 h
    cs = [[vs[phi[b][j]] * hs[hat[b][j]] for j in range(n_coef)] for b in range(B)]
    shares = [sum(c * i ** j for j, c in enumerate(phi[b])) % R for b in range(B)]
    wits = [sum(c * i ** j for j, c in enumerate(hat[b])) % R for b in range(B)]
    want = [1] * B
    for pos, kind in bad:
        want[pos] = 0
        if kind == "share":
            shares[pos] = (shares[pos] + 1) % R
        elif kind == "witness":
            wits[pos] = (wits[pos] - 1) % R
        elif kind == "swap":
            cs[pos] = list(cs[pos])
            cs[pos][t // 2] = cs[pos][t // 2] * g
        elif kind == "off":
            cs[pos] = list(cs[pos])
            cs[pos][t] = off_curve_raw()
        else:
            raise ValueError(kind)
    return cs, shares, wits, want


def flat_points(rows):
    return points([p for row in rows for p in row])

"""Shared by tests/test_g1_msm_host.py and tests/test_gpu_g1_msm.py: marshalling for hb_selftest_g1_msm (the per-lane steps of the MSM
kernels driven on the host), the Python-int model, and the cases both files run.

Model.  g1_support.vectors()[e] = e * g for e < 1000, so a row over bases with known logarithms e_k is g ** (sum_k s_k e_k mod R): one
host exponentiation a row whatever K.  The scalars are plain 256-bit integers; the points have order R, so the model reduces mod R."""
import functools
import random

import numpy as np

import g1_support as s

from honeybadgermpc_amd.bls12_381 import G1, R

DIRECT, BUCKET, HEAVY = 1, 2, 3
FULL = (1 << 256) - 1
EDGE_SCALARS = [0, 1, R - 1, R, 1 << 255, FULL]


def selftest(scalars, pts, M, K, method, chunk=0, per_row=False):
    """scalars: M rows of K ints; pts: K (shared) or M * K points as (n, 12) uint64 -> (rc, (M, 12) uint64)"""
    from honeybadgermpc_amd._capi import load_library, np_ptr

    lib = load_library()
    sw = np.ascontiguousarray(s.words([v for row in scalars for v in row], 4)) if M * K else np.zeros((1, 4), dtype=np.uint64)
    pw = np.ascontiguousarray(pts) if K else np.zeros((1, 12), dtype=np.uint64)
    assert sw.shape[0] == max(M * K, 1) and pw.shape[0] == max((M if per_row else 1) * K, 1)
    out = np.full((max(M, 1), 12), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    rc = lib.hb_selftest_g1_msm(np_ptr(sw), np_ptr(pw), 1 if per_row else 0, np_ptr(out), M, K, method, chunk)
    return rc, out[:M]


def model_logs(scalars, logs, per_row=False):
    """rows of scalars over bases logs[k] * g (logs: K ints, or M rows of K) -> (M, 12) uint64"""
    g = G1.generator()
    rows = []
    for m, row in enumerate(scalars):
        e = logs[m] if per_row else logs
        rows.append(g ** (sum(a * b for a, b in zip(row, e)) % R))
    return s.points(rows) if rows else np.zeros((0, 12), dtype=np.uint64)


def model_generic(scalars, bases):
    """the product of powers on host G1 objects (bases opaque); keep K small"""
    rows = []
    for row in scalars:
        acc = G1.one()
        for k, p in zip(row, bases):
            acc = acc * p ** (k % R)
        rows.append(acc)
    return s.points(rows)


def log_points(logs):
    vs = s.vectors()
    return s.points([vs[e] for e in logs])


def random_case(M, K, seed, per_row=False):
    """-> (scalars M x K, logs, points): random 256-bit scalars with the edge scalars at both ends of every row, bases from the vectors"""
    rnd = random.Random(seed)
    scalars = [[rnd.randrange(1 << 256) for _ in range(K)] for _ in range(M)]
    for row in scalars:
        for j, k in enumerate(EDGE_SCALARS):
            if j < K:
                row[j] = k
            if K - 1 - j >= 0:
                row[K - 1 - j] = k
    if per_row:
        logs = [[rnd.randrange(1, 1000) for _ in range(K)] for _ in range(M)]
        pts = log_points([e for row in logs for e in row])
    else:
        logs = [rnd.randrange(1, 1000) for _ in range(K)]
        pts = log_points(logs)
    return scalars, logs, pts


@functools.lru_cache(maxsize=None)
def special_cases():
    """name -> (scalars, logs, points, expected (M, 12)): the inputs whose shape, not whose size, is the test.  Computed once."""
    rnd = random.Random(77)
    g = G1.generator()
    cases = {}

    def add(name, scalars, logs, pts=None, want=None):
        cases[name] = (scalars, logs, log_points(logs) if pts is None else pts, model_logs(scalars, logs) if want is None else want)

    logs300 = [rnd.randrange(1, 1000) for _ in range(300)]
    add("all-zero rows", [[0] * 70, [0] * 70], logs300[:70])
    # every window puts its whole chunk into one bucket: the heavy-bucket path (chunk = 64: 64 > thr = 16)
    add("all-equal scalars", [[0x0123456789ABCDEF0123456789ABCDEF0123456789ABCDEF0123456789ABCDEF] * 300, [1] * 300], logs300)
    add("every byte 255", [[FULL] * 70], logs300[:70])
    add("single top byte", [[(1 + k % 255) << 248 for k in range(70)], [0xFF << 248] + [0] * 69], logs300[:70])
    # identity bases: vectors()[0] is 0 * g
    add("identity bases", [[rnd.randrange(1 << 256) for _ in range(70)]], [0 if k % 3 else logs300[k] for k in range(70)])
    add("all bases the identity", [[rnd.randrange(1 << 256) for _ in range(70)]], [0] * 70)
    # one base repeated: equal digits meet the SAME point in a bucket (the doubling branch of the mixed addition)
    add("one base repeated", [[rnd.randrange(1 << 256) for _ in range(70)], [5] * 70], [17] * 70)
    # P and -P with equal scalars: every bucket that receives P receives -P; the row is the identity
    p = s.vectors()[123]
    pair = s.points([p, p.invert()] * 35)
    ks = [rnd.randrange(1 << 256) for _ in range(35)]
    want = np.zeros((2, 12), dtype=np.uint64)
    add("P and -P", [[k for k in ks for _ in range(2)], [9] * 70], None, pts=pair, want=want)
    return cases


def generic_case():
    """K = 40 bases taken as opaque points, against the host product of powers"""
    rnd = random.Random(5)
    vs = s.vectors()
    bases = [vs[rnd.randrange(1, 1000)] * G1.rand("h") for _ in range(40)]
    scalars = [[rnd.randrange(1 << 256) for _ in range(40)], [rnd.randrange(R) for _ in range(40)]]
    for j, k in enumerate(EDGE_SCALARS):
        scalars[0][j] = k
    return scalars, s.points(bases), model_generic(scalars, bases)


def lagrange_definition(xs, targets):
    """the definition, term by term, one division a weight (the reference's lagrange_at_x, betterpairing.py:787)"""
    rows = []
    for t in targets:
        row = []
        for k, xk in enumerate(xs):
            num = den = 1
            for j, xj in enumerate(xs):
                if j != k:
                    num = num * (t - xj) % R
                    den = den * (xk - xj) % R
            row.append(num * pow(den, -1, R) % R)
        rows.append(row)
    return rows

"""Shared by tests/test_bit_decomposition_host.py and tests/test_gpu_bit_decomposition.py: the fields and shapes, the prefix network
evaluated on Python ints from the wiring model alone, the hb_selftest_bd / hb_selftest_fxp runners, Shamir dealing, and the in-process
party harness and tensor sampling of tests/test_gpu_fixedpoint.py (restated, not imported: that file stays as it is)."""
import asyncio
import ctypes
import random

import numpy as np

from conftest import BLS

GOLDILOCKS = 0xFFFFFFFF00000001
P64 = (1 << 64) - 59
P256 = (1 << 256) - 189
P255 = (1 << 255) - 19
GPU_FIELDS = [BLS, P256, P64, GOLDILOCKS]
GPU_FIELD_IDS = ["bls", "2^256-189", "2^64-59", "goldilocks"]
HOST_FIELDS = [(BLS, 4), (P256, 4), (P255, 4), (13, 4), (P64, 1), (GOLDILOCKS, 1)]
HOST_FIELD_IDS = ["bls", "2^256-189", "2^255-19", "13", "2^64-59", "goldilocks"]
COUNTS = (0, 1, 255, 256, 257, 5000)
LEAVES, PREFIX_MASK, PREFIX_COMBINE, SUM_MASK, SUM_COMBINE = range(5)

# m | levels | triples per level | prefix | total | opens: the issue's table
TABLE = [
    (1, 0, [], 0, 0, 1),
    (2, 0, [], 0, 1, 2),
    (3, 1, [1], 1, 3, 3),
    (5, 2, [3, 2], 5, 9, 4),
    (8, 3, [5, 4, 3], 12, 19, 5),
    (9, 3, [7, 6, 4], 17, 25, 5),
    (17, 4, [15, 14, 12, 8], 49, 65, 6),
    (33, 5, [31, 30, 28, 24, 16], 129, 161, 7),
    (64, 6, [61, 60, 58, 54, 46, 31], 310, 373, 8),
    (65, 6, [63, 62, 60, 56, 48, 32], 321, 385, 8),
    (253, 8, [251, 250, 244, 240, 232, 216, 184, 124], 1741, 1993, 10),
]


def gpu_shapes(p):
    """(k, m, kappa): no level; one g-only level; N a power of two; N ragged; a level whose last block is cut short"""
    if p >> 64:
        return [(8, 1, 8), (8, 2, 8), (8, 3, 8), (16, 5, 8), (16, 6, 8), (16, 9, 8), (64, 33, 32)]
    return [(8, 1, 8), (8, 3, 8), (16, 6, 8), (32, 17, 16)]


# ---- the network on Python ints ---------------------------------------------------------------------------------------------
def leaf(a, b, p):
    """(g, p) of public bit a against the value b of the mask's bit (any residue)"""
    return ((1 - b) % p, b % p) if a else (0, (1 - b) % p)


def triple_rows(bd, n_planes, level):
    """-> [(row of p_j g_q, row of p_j p_q or None)] for the nodes of prefix_nodes(n_planes, level), by the issue's numbering"""
    nodes = bd.prefix_nodes(n_planes, level)
    G = min(1 << level, len(nodes))
    return [(y, None) if g_only else (G + 2 * (y - G), G + 2 * (y - G) + 1) for y, (_, _, g_only) in enumerate(nodes)]


def network_on_ints(bd, c2, r, m):
    """the low m bits of c2 + (2^m - 1 - r) + 1 by leaves, prefix levels and sum bits on 0 / 1 ints, following prefix_nodes; the
    properties the in-place schedule rests on are asserted on the way"""
    a = [(c2 >> i) & 1 for i in range(m)]
    b = [(r >> i) & 1 for i in range(m)]
    n = m - 1
    g, q = [0] * n, [0] * n
    for i in range(n):
        g[i], q[i] = leaf(a[i], b[i], 1 << 62)
    if n:
        g[0], q[0] = g[0] + q[0], 0
    full_p = list(q)                                            # every node's true propagate, as if all nodes were full
    for level in range(bd.prefix_levels(m)):
        nodes = bd.prefix_nodes(n, level)
        written = {j for j, _, _ in nodes}
        assert all(0 <= part < j <= n - 1 and part not in written for j, part, _ in nodes), (m, level)
        for j, part, g_only in nodes:
            if g_only:
                assert full_p[part] == 0, (m, level, j)
            g[j] = g[j] + q[j] * g[part]
            full_p[j] = full_p[j] * full_p[part]
            if not g_only:
                q[j] = q[j] * q[part]
    out = [a[0] ^ b[0]]
    for i in range(1, m):
        pi = leaf(a[i], b[i], 1 << 62)[1]
        out.append(pi + g[i - 1] - 2 * pi * g[i - 1])
    return out


# ---- the bodies on the host ---------------------------------------------------------------------------------------------------
def _run(fn_name, n_params, p, nl, what, operands, params, outs, count):
    """outs: a row count (zero-filled), a list of ints (an array the body updates in place) or None -> (rc, [out lists])"""
    from honeybadgermpc_amd._capi import ints_to_limbs, limbs_to_ints, load_library, np_ptr

    lib = load_library()
    nb = 8 * nl
    arrays = [None if o is None else ints_to_limbs(list(o) or [0], p, nb) for o in operands]
    ptrs = (ctypes.c_void_p * 8)(*([None if x is None else x.ctypes.data for x in arrays] + [None] * (8 - len(arrays))))
    bufs, sizes = [], []
    for o in outs:
        if o is None:
            bufs.append(None), sizes.append(0)
        elif isinstance(o, int):
            bufs.append(np.zeros((max(o * count, 1), nl), dtype=np.uint64)), sizes.append(o * count)
        else:
            bufs.append(np.array(ints_to_limbs(list(o) or [0], p, nb))), sizes.append(len(o))
    optrs = (ctypes.c_void_p * 2)(*([None if b is None else b.ctypes.data for b in bufs] + [None] * (2 - len(bufs))))
    prm = (ctypes.c_int64 * n_params)(*(list(params) + [0] * (n_params - len(params))))
    rc = getattr(lib, fn_name)(np_ptr(ints_to_limbs([p], p + 1, nb)), nl, what, ptrs, prm, optrs, count)
    return rc, [None if b is None else limbs_to_ints(b[:s], nb) for b, s in zip(bufs, sizes)]


def run_bd(p, nl, what, operands, params, outs, count):
    """hb_selftest_bd over lists of ints; params = [m, level]"""
    return _run("hb_selftest_bd", 2, p, nl, what, operands, params, outs, count)


def run_fxp(p, nl, what, operands, params, outs, count):
    """hb_selftest_fxp over lists of ints; params = [k, m, kappa, aux, root]"""
    return _run("hb_selftest_fxp", 5, p, nl, what, operands, params, outs, count)


def run_fxp_mask(p, nl, xs, planes, k, m, kappa, count):
    """hb_selftest_fxp's mask body -> (masked, r1)"""
    rc, (masked, r1) = _run("hb_selftest_fxp", 5, p, nl, 0, [xs, planes], [k, m, kappa], [1, 1], count)
    assert rc == 0
    return masked, r1


def flat(rows):
    return [v for row in rows for v in row]


def beaver(d, e, a, b, ab, p):
    return (d * e + d * b + e * a + ab) % p


def bodies_chain(bd, p, nl, c, planes, m, count, rnd, opener=None, triples=None):
    """leaves -> levels -> sum through hb_selftest_bd for ONE holder of (c, planes [m][count] flat); opener(masked) -> the opened
    array (default: degree-0 shares, what the mask wrote); triples(level or 'sum', rows) -> (ta, tb, tab) flat.  -> the m planes, flat"""
    opener = opener or (lambda masked: masked)

    def fresh(_, rows):
        ta, tb = ([rnd.randrange(p) for _ in range(rows * count)] for _ in range(2))
        return ta, tb, [x * y % p for x, y in zip(ta, tb)]

    triples = triples or fresh
    n = m - 1
    rc, (g, q) = run_bd(p, nl, LEAVES, [c, planes[:n * count]], [m], [n, n], count)
    assert rc == 0
    for level in range(bd.prefix_levels(m)):
        ta, tb, tab = triples(level, bd.prefix_level_triples(m, level))
        rc, (masked,) = run_bd(p, nl, PREFIX_MASK, [g, q, ta, tb], [m, level], [2 * bd.prefix_level_triples(m, level)], count)
        assert rc == 0
        rc, (g, q) = run_bd(p, nl, PREFIX_COMBINE, [opener(masked), ta, tb, tab], [m, level], [g, q], count)
        assert rc == 0
    if n == 0:
        rc, (out,) = run_bd(p, nl, SUM_COMBINE, [None, c, planes, None, None, None, None], [m], [m], count)
        assert rc == 0
        return out
    ta, tb, tab = triples("sum", n)
    rc, (masked,) = run_bd(p, nl, SUM_MASK, [c, planes, g, ta, tb], [m], [2 * n], count)
    assert rc == 0
    rc, (out,) = run_bd(p, nl, SUM_COMBINE, [opener(masked), c, planes, g, ta, tb, tab], [m], [m], count)
    assert rc == 0
    return out


# ---- Shamir shares ------------------------------------------------------------------------------------------------------------
def deal(rnd, p, n, degree, values):
    """-> [party][k]: Shamir shares of values[k] at the points 1..n"""
    out = [[0] * len(values) for _ in range(n)]
    for k, v in enumerate(values):
        coeffs = [rnd.randrange(p) for _ in range(degree)]
        for i in range(n):
            acc = 0
            for co in reversed(coeffs):
                acc = (acc + co) * (i + 1) % p
            out[i][k] = (acc + v) % p
    return out


def reconstruct(p, degree, shares, first=0):
    """[party][k] -> [k]: the values at 0 from the degree + 1 parties first, first + 1, ..."""
    pts = list(range(first + 1, first + degree + 2))
    shares = shares[first:]
    lam = []
    for i in pts:
        num = den = 1
        for j in pts:
            if j != i:
                num, den = num * (-j) % p, den * (i - j) % p
        lam.append(num * pow(den, -1, p) % p)
    return [sum(l * shares[i][k] for i, l in enumerate(lam)) % p for k in range(len(shares[0]))]


# ---- GPU side -------------------------------------------------------------------------------------------------------------------
def gpu_ctx(p):
    from honeybadgermpc_amd._capi import Context

    return Context.get(p)


def random_tensor(ctx, seed, count, rows=None):
    """uniform canonical residues made on the device side (numpy limbs, reduced by hb_reduce)"""
    g = np.random.default_rng(seed)
    n = count if rows is None else rows * count
    limbs = g.integers(-(1 << 63), (1 << 63) - 1, size=(n, ctx.n_limbs), dtype=np.int64, endpoint=True)
    t = ctx.reduce_(ctx.to_device(limbs))
    return t if rows is None else t.view(rows, count, ctx.n_limbs)


def rows_of(ctx, t):
    """(rows, count, limbs) -> [row][element] ints"""
    vals, count = ctx.download_ints(t.reshape(-1, ctx.n_limbs)), t.shape[1]
    return [vals[r * count:(r + 1) * count] for r in range(t.shape[0])]


def sample(count):
    return list(range(count)) if count <= 257 else sorted({0, 1, 2, 3, 255, 256, 257, count - 1} | set(random.Random(count).sample(range(count), 24)))


def bit_elem(ctx, c, i):
    """bit i of c as a field element array"""
    out = ctx.torch.zeros_like(c)
    out[:, 0] = (c[:, i // 64] >> (i % 64)) & 1
    return out


class TaggedNet:
    """get_send_recv(tag) -> (send, recv) for party i, as the runtime hands out per-share-id channels"""

    def __init__(self, n):
        self.n, self.q = n, [dict() for _ in range(n)]

    def _queue(self, party, tag):
        return self.q[party].setdefault(tag, asyncio.Queue())

    def get_send_recv(self, i, tamper=None):
        def factory(tag):
            def send(dest, msg):
                self._queue(dest, tag).put_nowait((i, tamper(msg) if tamper else msg))

            return send, self._queue(i, tag).get

        return factory


def deal_planes(ctx, rnd, p, n, t, rows):
    """rows: [row][element] values -> [party] tensors (rows, count, limbs)"""
    count = len(rows[0])
    dealt = deal(rnd, p, n, t, [v for row in rows for v in row])
    return [ctx.upload_ints(d).view(len(rows), count, ctx.n_limbs) for d in dealt]


def run_parties(p, n, t, bad, rnd, body):
    """every party runs `body(co, i)` over its own OpenCoalescer -> [result per party]"""
    from honeybadgermpc_amd import wire
    from honeybadgermpc_amd.open_coalescer import OpenCoalescer

    def garble(msg):
        tag, blob = msg
        count = wire.unpack_limbs(blob).shape[0]
        return (tag, wire.pack_ints([rnd.randrange(p) for _ in range(count)], p))

    async def party(i, net):
        co = OpenCoalescer(p, n, t, i, net.get_send_recv(i, garble if i in bad else None))
        return await body(co, i)

    async def main():
        net = TaggedNet(n)
        return await asyncio.gather(*[party(i, net) for i in range(n)])

    results = asyncio.run(main())
    gpu_ctx(p).torch.cuda.synchronize()
    return results

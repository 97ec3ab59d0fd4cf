"""Shared by tests/test_demux_host.py and tests/test_gpu_demux.py: the counts of the issue's table, the demultiplexer's plan evaluated
on Python ints from the wiring model alone, triples laid out as the kernels read them, and the hb_selftest_demux runner with the
lock-step chain of several holders.  Dealing, reconstruction and the party harness are those of tests/bitdec_cases.py."""
import bitdec_cases as bc
from conftest import BLS

P64 = bc.P64
HOST_FIELDS = [(BLS, 4), (P64, 1)]
GPU_FIELDS = [BLS, P64]
FIELD_IDS = ["bls", "2^64-59"]
LEAVES, MASK, FINISH = range(3)
BAD_ARG = 2

# m | levels | opened by level | products by level: the issue's table
TABLE = [
    (1, 0, [], []),
    (2, 1, [4], [4]),
    (3, 2, [4, 6], [4, 8]),
    (4, 2, [8, 8], [8, 16]),
    (5, 3, [8, 8, 18], [8, 16, 32]),
    (10, 4, [20, 16, 32, 260], [20, 32, 256, 1024]),
]


def bits_of(s, m):
    return [(s >> i) & 1 for i in range(m)]


# ---- the plan on Python ints ----------------------------------------------------------------------------------------------------
def factor(level_sources, k, high, width, bits, groups, p):
    """the vector of one factor of merge k: (1 - b, b) of a bit plane's value, or the stored rows"""
    row = level_sources[k][1 if high else 0]
    if width == 1:
        return [(1 - bits[row]) % p, bits[row] % p]
    return groups[row:row + (1 << width)]


def tab_rows(level):
    """-> {(merge, hi, lo): row of tab}, merge by merge, row hi 2^wl + lo"""
    rows, off = {}, 0
    for k, (_, wl, wh) in enumerate(level.merges):
        for hi in range(1 << wh):
            for lo in range(1 << wl):
                rows[(k, hi, lo)] = off + (hi << wl) + lo
        off += 1 << (wl + wh)
    return rows


def plan_on_ints(dx, bits, m, p=1 << 62):
    """the one-hot vector from the m bit values by demux_plan alone: products of ints, no masks"""
    if m == 1:
        return [(1 - bits[0]) % p, bits[0] % p]
    plan = dx.demux_plan(m)
    groups = [None] * dx.demux_group_rows(m)
    for level in plan:
        rows = tab_rows(level)
        for k, (_, wl, wh) in enumerate(level.merges):
            A, B = factor(level.sources, k, False, wl, bits, groups, p), factor(level.sources, k, True, wh, bits, groups, p)
            for hi in range(1 << wh):
                for lo in range(1 << wl):
                    assert groups[level.out_row + rows[(k, hi, lo)]] is None                # no row is written twice
                    groups[level.out_row + rows[(k, hi, lo)]] = A[lo] * B[hi] % p
    assert None not in groups and plan[-1].out_row + (1 << m) == len(groups)
    return groups[-(1 << m):]


def level_triples(dx, m, level, count, p, rnd, zero=False):
    """-> (ta, tab) as [row][element] values: P then Q of every merge, and their outer products row hi 2^wl + lo"""
    lv = dx.demux_plan(m)[level]
    ta, tab = [], []
    for _, wl, wh in lv.merges:
        P, Q = ([[0 if zero else rnd.randrange(p) for _ in range(count)] for _ in range(1 << w)] for w in (wl, wh))
        ta += P + Q
        tab += [[P[lo][e] * Q[hi][e] % p for e in range(count)] for hi in range(1 << wh) for lo in range(1 << wl)]
    return ta, tab


# ---- one level composed from share_arithmetic (GPU) -----------------------------------------------------------------------------
def level_rows(lv, m):
    """-> (src, d, e): for every row of the level's opened array its row in the pool [1 - b planes | b planes | groups], and for
    every product the rows of its two factors in the opened array"""
    src, d, e, off = [], [], [], 0
    for k, (_, wl, wh) in enumerate(lv.merges):
        for w, row in ((wl, lv.sources[k][0]), (wh, lv.sources[k][1])):
            src += [row, m + row] if w == 1 else [2 * m + row + r for r in range(1 << w)]
        for hi in range(1 << wh):
            for lo in range(1 << wl):
                d.append(off + lo), e.append(off + (1 << wl) + hi)
        off += (1 << wl) + (1 << wh)
    return src, d, e


def composed_mask(ctx, sa, lv, bits, groups, ta):
    """what demux_mask writes, from neg, add, index_select and ONE sub"""
    m, count, L = bits.shape[0], bits.shape[1], ctx.n_limbs
    t = ctx.torch
    src, _, _ = level_rows(lv, m)
    nb = sa.add(ctx, sa.neg(ctx, bits.reshape(m * count, L)), 1).view(m, count, L)
    pool = t.cat([nb, bits] + ([] if groups is None else [groups]))
    rows = pool.index_select(0, t.tensor(src, dtype=t.int64, device=ctx.tdev))
    return sa.sub(ctx, rows.reshape(-1, L), ta[:len(src)].reshape(-1, L)).view(len(src), count, L)


def composed_finish(ctx, sa, lv, m, opened, ta, tab):
    """the level's products, from index_select and ONE beaver_combine"""
    count, L = ta.shape[1], ctx.n_limbs
    t = ctx.torch
    src, d, e = level_rows(lv, m)
    di, ei = (t.tensor(v, dtype=t.int64, device=ctx.tdev) for v in (d, e))
    opened = opened.view(len(src), count, L)
    flat = [v.index_select(0, i).reshape(-1, L) for v, i in ((opened, di), (opened, ei), (ta, di), (ta, ei))]
    return sa.beaver_combine(ctx, *flat, tab[:len(d)].reshape(-1, L)).view(len(d), count, L)


# ---- the rows on the host -------------------------------------------------------------------------------------------------------
def run_demux(p, nl, what, operands, params, outs, count):
    """hb_selftest_demux over lists of ints; params = [m, level]"""
    return bc._run("hb_selftest_demux", 2, p, nl, what, operands, params, outs, count)


def chain(dx, p, nl, degree, planes, m, count, triples):
    """mask -> open -> finish, level by level, for the holders planes[i] ([m][count] flat) in lock step; the open is host
    interpolation at `degree` from the first degree + 1 holders (degree 0, one holder: what the mask wrote).  triples(level) ->
    [holder] of (ta, tab) flat.  -> [holder] the 2^m planes, flat"""
    n = len(planes)
    if m == 1:
        outs = []
        for i in range(n):
            rc, (out,) = run_demux(p, nl, LEAVES, [planes[i]], [1, 0], [2], count)
            assert rc == 0
            outs.append(out)
        return outs
    groups = [[0] * (dx.demux_group_rows(m) * count) for _ in range(n)]
    for level in range(dx.demux_levels(m)):
        trip, masked = triples(level), []
        for i in range(n):
            rc, (mk,) = run_demux(p, nl, MASK, [planes[i], groups[i], trip[i][0]], [m, level], [dx.demux_opened(m, level)], count)
            assert rc == 0
            masked.append(mk)
        opened = bc.reconstruct(p, degree, masked) if count else []
        for i in range(n):
            rc, (groups[i],) = run_demux(p, nl, FINISH, [opened, trip[i][0], trip[i][1]], [m, level], [groups[i]], count)
            assert rc == 0
    return [g[len(g) - (count << m):] for g in groups]

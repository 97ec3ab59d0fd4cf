"""The demultiplexer's kernels and protocol timed on the device:
   python scratch/time_demux.py [reps] [--label TEXT] > profiles/demux.txt

BLS12-381 Fr, m = 10, count = 2^8 and 2^12.

(a) every level, demux_mask + demux_finish (2 launches), beside the same level composed from index_select, sub and beaver_combine
    (the gathers of the factor rows, ONE sub over the level's array, ONE beaver_combine over the level's products; the index tensors
    and the pool of 1 - b planes are made before the clock starts, which favours the composition).  What the level "opens" is what its
    mask wrote (degree-0 shares): no open is timed.  HIP events around one group, `reps` (at least 20) runs after a warm-up, the two
    versions alternated run by run; median (min .. max).  Outputs are compared bit for bit.  GB/s: the bytes the two fused launches
    must move (mask: source, ta in, one out a row; finish: PQ in, one out a product, and the level's opened and ta rows once) over the
    fused median.
(b) a whole demux plus lookup of a public table of 2^m rows, beside the bit-by-bit chain composed from share_arithmetic (one bit a
    round: a gather, two subs and a beaver_combine a round, m - 1 opens, 2 (2^m - 2) opened elements) plus the same lookup: four parties
    (t = 1) in one process over an in-memory network, every party's coroutine on the one device, wall clock from the first coroutine's
    start to the last one's end with the device synchronised, 3 runs after a warm-up.  The dealing is not timed.  Every looked-up
    value is opened and compared with the table.

No GPU: fails (there is nothing to fall back to)."""
import asyncio
import random
import socket
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from honeybadgermpc_amd import share_arithmetic as sa  # noqa: E402
from honeybadgermpc_amd._capi import Context  # noqa: E402
from honeybadgermpc_amd.open_coalescer import OpenCoalescer  # noqa: E402
from honeybadgermpc_amd.progs import demux as dx  # noqa: E402

BLS = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
N, T = 4, 1
M = 10


def rnd(ctx, gen, count, rows=None):
    n = count if rows is None else rows * count
    t = ctx.reduce_(torch.randint(-(1 << 63), (1 << 63) - 1, (n, ctx.n_limbs), dtype=torch.int64, device="cuda", generator=gen))
    return t if rows is None else t.view(rows, count, ctx.n_limbs)


def fmt(ts, unit="us"):
    return f"{np.median(ts):10.1f} {unit} ({min(ts):.1f} .. {max(ts):.1f})"


def alternate(reps, fused, composed):
    fused(); composed()
    torch.cuda.synchronize()
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(reps)]
    for e3 in evs:
        e3[0].record()
        fused()
        e3[1].record()
        composed()
        e3[2].record()
    torch.cuda.synchronize()
    return [e3[0].elapsed_time(e3[1]) * 1e3 for e3 in evs], [e3[1].elapsed_time(e3[2]) * 1e3 for e3 in evs]


def level_rows(lv, m):
    """-> (src, d, e): rows of the pool [1 - b planes | b planes | groups] behind the level's opened array, and the two factor rows
    of every product"""
    src, d, e, off = [], [], [], 0
    for k, (_, wl, wh) in enumerate(lv.merges):
        for w, row in ((wl, lv.sources[k][0]), (wh, lv.sources[k][1])):
            src += [row, m + row] if w == 1 else [2 * m + row + r for r in range(1 << w)]
        for hi in range(1 << wh):
            for lo in range(1 << wl):
                d.append(off + lo), e.append(off + (1 << wl) + hi)
        off += (1 << wl) + (1 << wh)
    return src, d, e


class Net:
    def __init__(self, n):
        self.q = [dict() for _ in range(n)]

    def get_send_recv(self, i):
        def factory(tag):
            def send(dest, msg):
                self.q[dest].setdefault(tag, asyncio.Queue()).put_nowait((i, msg))

            return send, self.q[i].setdefault(tag, asyncio.Queue()).get

        return factory


def deal(ctx, gen, values):
    flat = values.reshape(-1, ctx.n_limbs)
    slope = rnd(ctx, gen, flat.shape[0])
    return [sa.add(ctx, flat, sa.mul(ctx, slope, i + 1)).view(values.shape) for i in range(N)]


def run_parties(p, body):
    """-> (seconds, [results]): the parties' coroutines gathered, the device synchronised at both ends"""
    async def main():
        net = Net(N)
        return await asyncio.gather(*[body(OpenCoalescer(p, N, T, i, net.get_send_recv(i)), i) for i in range(N)])

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = asyncio.run(main())
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res


async def chain(co, bits, trip):
    """the one-hot planes bit by bit from share_arithmetic: round i multiplies the 2^i planes so far by bit i"""
    ctx = co.ctx
    m, count, L = bits.shape[0], bits.shape[1], ctx.n_limbs
    ta, tb, tab = trip
    v = torch.cat([sa.add(ctx, sa.neg(ctx, bits[0]), 1).view(1, count, L), bits[0:1]])
    off = 0
    for i in range(1, m):
        r = 1 << i
        y = bits[i].expand(r, count, L).reshape(-1, L)
        a, b, ab = (t[off:off + r].reshape(-1, L) for t in (ta, tb, tab))
        f = co.open_share_array(sa.sub(ctx, v.reshape(-1, L), a))
        g = co.open_share_array(sa.sub(ctx, y, b))
        prod = sa.beaver_combine(ctx, await f, await g, a, b, ab)
        v = torch.cat([sa.sub(ctx, v.reshape(-1, L), prod).view(r, count, L), prod.view(r, count, L)])
        off += r
    return v


def main():
    args = sys.argv[1:]
    if not torch.cuda.is_available():
        raise SystemExit("scratch/time_demux.py needs the GPU")
    reps = max(20, int(args[0])) if args and args[0].isdigit() else 20
    label = args[args.index("--label") + 1] if "--label" in args else "working tree"
    print(f"# scratch/time_demux.py, {reps} runs a figure: median (min .. max); {torch.cuda.get_device_name(0)} on {socket.gethostname()}; {label}")
    p, m = BLS, M
    ctx = Context.get(p)
    L, eb = ctx.n_limbs, 8 * ctx.n_limbs
    gen = torch.Generator(device="cuda")
    gen.manual_seed(23)
    plan = dx.demux_plan(m)
    # ---- (a)
    for count in (1 << 8, 1 << 12):
        bits, groups0 = rnd(ctx, gen, count, rows=m), rnd(ctx, gen, count, rows=dx.demux_group_rows(m))
        pool = torch.cat([sa.add(ctx, sa.neg(ctx, bits.reshape(m * count, L)), 1).view(m, count, L), bits, groups0])
        for level, lv in enumerate(plan):
            n_open, n_prod = dx.demux_opened(m, level), dx.demux_products(m, level)
            ta, tab = rnd(ctx, gen, count, rows=n_open), rnd(ctx, gen, count, rows=n_prod)
            si, di, ei = (torch.tensor(v, dtype=torch.int64, device="cuda") for v in level_rows(lv, m))
            groups = groups0.clone()

            def fused_a():
                masked = dx.demux_mask(ctx, bits, groups, level, ta)
                return dx.demux_finish(ctx, masked, groups, level, ta, tab)

            def composed_a():
                masked = sa.sub(ctx, pool.index_select(0, si).reshape(-1, L), ta.reshape(-1, L)).view(n_open, count, L)
                flat = [v.index_select(0, i).reshape(-1, L) for v, i in ((masked, di), (masked, ei), (ta, di), (ta, ei))]
                return sa.beaver_combine(ctx, *flat, tab.reshape(-1, L)).view(n_prod, count, L)

            same = bool(torch.equal(fused_a(), composed_a()))
            tf, tc = alternate(reps, fused_a, composed_a)
            moved = (3 * n_open + 2 * n_prod + 2 * n_open) * count * eb
            print(f"(a) level {level} of {len(plan)}, m = {m}  count = 2^{count.bit_length() - 1}  merges {[(wl, wh) for _, wl, wh in lv.merges]}  {n_open} opened, {n_prod} products   "
                  f"fused (2 launches) {fmt(tf)}   composed (7 launches) {fmt(tc)}   composed / fused = {np.median(tc) / np.median(tf):5.2f}   "
                  f"{moved / np.median(tf) / 1e3:7.1f} GB/s needed bytes over the two launches   {'bit-equal' if same else 'MISMATCH'}", flush=True)
        del bits, groups0, pool, groups, ta, tab
        torch.cuda.empty_cache()
    # ---- (b)
    py = random.Random(5)
    table = [[py.randrange(p)] for _ in range(1 << m)]
    table_dev = ctx.upload_ints([row[0] for row in table]).view(1 << m, 1, L)
    for count in (1 << 8, 1 << 12):
        ss = [0, 1, (1 << m) - 1, (1 << m) - 2] + [py.randrange(1 << m) for _ in range(count - 4)]
        want = [table[s][0] for s in ss]
        planes = torch.zeros((m, count, L), dtype=torch.int64, device="cuda")
        planes[:, :, 0] = torch.tensor([[(s >> i) & 1 for s in ss] for i in range(m)], device="cuda")
        dbits = deal(ctx, gen, planes)
        dtrip = [[] for _ in range(N)]
        for level, lv in enumerate(plan):
            ta = rnd(ctx, gen, count, rows=dx.demux_opened(m, level))
            _, di, ei = (torch.tensor(v, dtype=torch.int64, device="cuda") for v in level_rows(lv, m))
            tab = sa.mul(ctx, ta.index_select(0, di).reshape(-1, L), ta.index_select(0, ei).reshape(-1, L)).view(len(di), count, L)
            for i, (a, ab) in enumerate(zip(deal(ctx, gen, ta), deal(ctx, gen, tab))):
                dtrip[i].append((a, ab))
        rows = (1 << m) - 2
        ca, cb = rnd(ctx, gen, count, rows=rows), rnd(ctx, gen, count, rows=rows)
        cab = sa.mul(ctx, ca.reshape(-1, L), cb.reshape(-1, L)).view(rows, count, L)
        ctrip = [deal(ctx, gen, v) for v in (ca, cb, cab)]
        del ca, cb, cab

        async def by_demux(co, i):
            return dx.lookup(ctx, await dx.demux(co, dbits[i], dtrip[i]), table_dev)

        async def by_chain(co, i):
            return dx.lookup(ctx, await chain(co, dbits[i], tuple(v[i] for v in ctrip)), table_dev)

        def opened(route):
            async def body(co, i):
                return ctx.download_ints(await co.open_share_array((await route(co, i)).reshape(-1, L)))
            return body

        for name, route, opens, elems, entries in (("demux + lookup", by_demux, dx.demux_levels(m), dx.demux_triples(m)[0], dx.demux_triples(m)[1]),
                                                    ("bit-by-bit chain + lookup", by_chain, m - 1, 2 * rows, rows)):
            ok = all(got == want for got in run_parties(p, opened(route))[1])
            ts = [run_parties(p, route)[0] * 1e3 for _ in range(3)]
            print(f"(b) {name:26s} m = {m}  count = 2^{count.bit_length() - 1}  n = {N}, t = {T}  {opens} opens, {elems} elements opened, {entries} triple entries an index   "
                  f"{fmt(ts, 'ms')}, all four parties   {'opens to the table' if ok else 'MISMATCH'}", flush=True)
        del dbits, dtrip, ctrip
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

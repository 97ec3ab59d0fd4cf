"""The bit decomposition kernels and protocol timed on the device:
   python scratch/time_bit_decomposition.py [reps] [--label TEXT] > profiles/bit_decomposition.txt

BLS12-381 Fr, m = 64 (N = 63 planes), count = 2^16.

(a) one whole level of the prefix network, prefix_mask + prefix_combine (2 launches), for the first level (61 triples, 1 g-only node)
    and the last (31 triples, every node g-only), beside the same planes composed from share_arithmetic calls: two subs a triple, a
    beaver_combine a triple and an add a node, on copies of g and p (the copy is inside both clocks).  What the level "opens" is
    what its mask wrote (degree-0 shares): no open is timed.
(b) the sum step, sum_mask + sum_combine (2 launches), beside the composition: the leaf's propagate from the reference-style
    formulas (the public bit as an array, made before the clock starts, which favours the composition), two subs, a beaver_combine,
    an add, a doubling and a sub a bit.
    (a), (b): HIP events around one group, `reps` (at least 20) runs after a warm-up, the two versions alternated run by run; median
    (min .. max).  Outputs are compared bit for bit.
(c) one whole bit_decompose at k = 65, kappa = 32 beside the m div2m calls that give the same bits on the parent's API (bit i =
    (x mod 2^(i+1) - x mod 2^i) / 2^i; timed at m' = 8 bits and scaled, the full 64 would spend 4 096 triple rows an element): four
    parties (t = 1) in one process over an in-memory network, every party's coroutine on the one device, wall clock from the first
    coroutine's start to the last one's end with the device synchronised, 3 runs after a warm-up.  The dealing is not timed.  Every
    opened plane is checked against bits_model.

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
from honeybadgermpc_amd.progs import bit_decomposition as bd  # noqa: E402
from honeybadgermpc_amd.progs import fixedpoint as fx  # noqa: E402

BLS = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
N, T = 4, 1
M, K, KAPPA = 64, 65, 32


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


def triple_rows(n_planes, level):
    nodes = bd.prefix_nodes(n_planes, level)
    G = min(1 << level, len(nodes))
    return nodes, [(y, None) if g_only else (G + 2 * (y - G), G + 2 * (y - G) + 1) for y, (_, _, g_only) in enumerate(nodes)]


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


def triples(ctx, gen, rows, count):
    tp, tq = rnd(ctx, gen, count, rows), rnd(ctx, gen, count, rows)
    tpq = sa.mul(ctx, tp.view(-1, ctx.n_limbs), tq.view(-1, ctx.n_limbs)).view(tp.shape)
    return [deal(ctx, gen, v) for v in (tp, tq, tpq)]


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


def main():
    args = sys.argv[1:]
    if not torch.cuda.is_available():
        raise SystemExit("scratch/time_bit_decomposition.py needs the GPU")
    reps = max(20, int(args[0])) if args and args[0].isdigit() else 20
    label = args[args.index("--label") + 1] if "--label" in args else "working tree"
    print(f"# scratch/time_bit_decomposition.py, {reps} runs a figure: median (min .. max); {torch.cuda.get_device_name(0)} on {socket.gethostname()}; {label}")
    p, m, n, count = BLS, M, M - 1, 1 << 16
    ctx = Context.get(p)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(17)
    eb = 8 * ctx.n_limbs
    # ---- (a)
    g0, q0 = rnd(ctx, gen, count, rows=n), rnd(ctx, gen, count, rows=n)
    for level in (0, bd.prefix_levels(m) - 1):
        nodes, rows = triple_rows(n, level)
        tr = bd.prefix_level_triples(m, level)
        ta, tb, tab = (rnd(ctx, gen, count, rows=tr) for _ in range(3))

        def fused_a():
            g, q = g0.clone(), q0.clone()
            masked = bd.prefix_mask(ctx, g, q, level, ta, tb)
            return bd.prefix_combine(ctx, masked, g, q, level, ta, tb, tab)

        def composed_a():
            g, q = g0.clone(), q0.clone()
            for (j, part, g_only), (r0, r1) in zip(nodes, rows):
                d, e = sa.sub(ctx, q0[j], ta[r0]), sa.sub(ctx, g0[part], tb[r0])
                sa.add(ctx, g0[j], sa.beaver_combine(ctx, d, e, ta[r0], tb[r0], tab[r0]), out=g[j])
                if not g_only:
                    d, e = sa.sub(ctx, q0[j], ta[r1]), sa.sub(ctx, q0[part], tb[r1])
                    sa.beaver_combine(ctx, d, e, ta[r1], tb[r1], tab[r1], out=q[j])
            return g, q

        same = all(bool(torch.equal(a, b)) for a, b in zip(fused_a(), composed_a()))
        tf, tc = alternate(reps, fused_a, composed_a)
        full = sum(1 for _, _, g_only in nodes if not g_only)
        # fused traffic an element: the mask reads 4 and writes 2 a triple; the combine reads g_j and writes it a node, reads 5 a triple, writes p_j a full node
        moved = (6 * tr + 2 * len(nodes) + 5 * tr + full) * count * eb
        print(f"(a) prefix level {level} of {bd.prefix_levels(m)}, m = {m}  count = 2^16  {len(nodes)} nodes, {tr} triples   fused (2 launches) {fmt(tf)}   "
              f"composed ({3 * tr + len(nodes)} launches) {fmt(tc)}   composed / fused = {np.median(tc) / np.median(tf):5.2f}   "
              f"{moved / np.median(tf) / 1e3:7.1f} GB/s read + written by the two launches (the two copies of g, p are in both clocks)   {'bit-equal' if same else 'MISMATCH'}", flush=True)
    # ---- (b)
    c, bits = rnd(ctx, gen, count), rnd(ctx, gen, count, rows=m)
    ta, tb, tab = (rnd(ctx, gen, count, rows=n) for _ in range(3))
    abits = []
    for i in range(m):
        a = torch.zeros_like(c)
        a[:, 0] = (c[:, i // 64] >> (i % 64)) & 1
        abits.append(a)

    def fused_b():
        masked = bd.sum_mask(ctx, c, bits, g0, m, ta, tb)
        return bd.sum_combine(ctx, masked, c, bits, g0, m, ta, tb, tab)

    def composed_b():
        out = torch.empty((m, count, ctx.n_limbs), dtype=torch.int64, device="cuda")
        sa.sub(ctx, sa.add(ctx, abits[0], bits[0]), sa.mul(ctx, sa.mul(ctx, abits[0], bits[0]), 2), out=out[0])
        for i in range(1, m):
            t = i - 1
            nb = sa.add(ctx, sa.neg(ctx, bits[i]), 1)
            lp = sa.sub(ctx, sa.add(ctx, abits[i], nb), sa.mul(ctx, sa.mul(ctx, abits[i], nb), 2))
            d, e = sa.sub(ctx, lp, ta[t]), sa.sub(ctx, g0[t], tb[t])
            prod = sa.beaver_combine(ctx, d, e, ta[t], tb[t], tab[t])
            sa.sub(ctx, sa.add(ctx, lp, g0[t]), sa.add(ctx, prod, prod), out=out[i])
        return out

    same = bool(torch.equal(fused_b(), composed_b()))
    tf, tc = alternate(reps, fused_b, composed_b)
    moved = (7 * n + 10 * n + 3) * count * eb            # mask: c, b, g, ta, tb in, 2 out a bit; combine: c, b, g, 2 opened, 3 triples in, 1 out
    print(f"(b) sum step, m = {m}  count = 2^16  {n} triples   fused (2 launches) {fmt(tf)}   composed ({4 + 13 * n} launches) {fmt(tc)}   "
          f"composed / fused = {np.median(tc) / np.median(tf):5.2f}   {moved / np.median(tf) / 1e3:7.1f} GB/s read + written   {'bit-equal' if same else 'MISMATCH'}", flush=True)
    del g0, q0, bits, ta, tb, tab, abits
    torch.cuda.empty_cache()
    # ---- (c)
    py = random.Random(5)
    top = 1 << (K - 1)
    xs = [0, 1, -1, top - 1, -top] + [py.randrange(-top, top) for _ in range(count - 5)]
    want = [bd.bits_model(x % p, p, K, m) for x in xs]
    planes = torch.zeros((K + KAPPA, count, ctx.n_limbs), dtype=torch.int64, device="cuda")
    planes[:, :, 0] = torch.randint(0, 2, (K + KAPPA, count), device="cuda", generator=gen)
    dx, dbits = deal(ctx, gen, ctx.upload_ints([v % p for v in xs])), deal(ctx, gen, planes)
    dtrip = triples(ctx, gen, bd.bit_triples(m), count)

    async def body(co, i):
        return await bd.bit_decompose(co, dx[i], dbits[i], tuple(v[i] for v in dtrip), K, m, KAPPA)

    async def opened(co, i):
        got = await co.open_share_array((await body(co, i)).reshape(m * count, ctx.n_limbs))
        return ctx.download_ints(got.view(m, count, ctx.n_limbs)[:, ::97].reshape(-1, ctx.n_limbs))       # every 97th element is compared

    picked = range(0, count, 97)
    ok = all(got == [want[e][b] for b in range(m) for e in picked] for got in run_parties(p, opened)[1])
    ts = [run_parties(p, body)[0] * 1e3 for _ in range(3)]
    print(f"(c) bit_decompose m = {m}, k = {K}  count = 2^16  n = {N}, t = {T}  {bd.bit_opens(m)} opens, {bd.bit_triples(m)} triples an element   {fmt(ts, 'ms')}, all four parties   "
          f"{'opens to bits_model' if ok else 'MISMATCH'}", flush=True)
    mp = 8
    inv = [pow(2, -i, p) for i in range(mp)]

    async def by_div2m(co, i):
        """bits 0 .. mp - 1 from div2m alone: x mod 2^(i+1) for i < mp, differences scaled"""
        tr = tuple(v[i] for v in dtrip)
        mods, off = [], 0
        for b in range(1, mp + 1):
            need = fx.carry_triples(b)
            mods.append(await fx.div2m(co, dx[i], dbits[i], tuple(v[off:off + need] for v in tr), K, b, KAPPA))
            off += need
        return [mods[0]] + [sa.mul(ctx, sa.sub(ctx, mods[b], mods[b - 1]), inv[b]) for b in range(1, mp)]

    async def by_div2m_opened(co, i):
        return [ctx.download_ints((await co.open_share_array(v))[::97].contiguous()) for v in await by_div2m(co, i)]

    ok = all(got == [[want[e][b] for e in picked] for b in range(mp)] for got in run_parties(p, by_div2m_opened)[1])
    ts2 = [run_parties(p, by_div2m)[0] * 1e3 for _ in range(3)]
    spent = sum(fx.carry_triples(b) for b in range(1, mp + 1))
    full = sum(fx.carry_triples(b) for b in range(1, m + 1))
    print(f"(c) the low {mp} bits by {mp} div2m calls  count = 2^16  n = {N}, t = {T}  {sum(1 + fx.carry_levels(b) for b in range(1, mp + 1))} opens, {spent} triples an element   "
          f"{fmt(ts2, 'ms')}, all four parties   {'opens to bits_model' if ok else 'MISMATCH'}   (all {m} bits: {sum(1 + fx.carry_levels(b) for b in range(1, m + 1))} opens, {full} triples an element; "
          f"by triples {np.median(ts2) * full / spent:.0f} ms against {np.median(ts):.0f} ms)", flush=True)


main()

"""The sorting kernels and protocol timed on the device:
   python scratch/time_sorting.py [reps] [--label TEXT] > profiles/sorting.txt

BLS12-381 Fr, (k, kappa) = (64, 32), width 2 (a key and one payload column).

(a) the three fused launches of ONE layer (cmp_mask, swap_mask, swap_finish) beside the same layer composed from index_select,
    share_arithmetic and fixedpoint calls (trunc_mask, div2m_finish NEG_TRUNC, 1 - b, beaver_combine, index_copy_), at 2^16 and 2^20
    slots: arrays of n = 1024 rows, batch = 128 and 2048, the network's first layer (a = 9: pairs 512 rows apart) and the first layer
    of its last group (a = 0: neighbours).  The composition is given its index tensors ready made and keeps what it gathered from
    step to step, which favours it.  What lies between the steps in a protocol (the opens, the carry tree) is the same for both and
    is not run: c, the carry and the opened array are uniform residues.  HIP events around one group of three steps, `reps` (at least
    20) runs after a warm-up, the two versions alternated run by run; median (min .. max).  Outputs are compared bit for bit.
(b) one whole sort of n = 1024 (55 layers, 24063 comparators, 440 batches): four parties (t = 1) in one process over an in-memory
    network, every party's coroutine on the one device, wall clock from the first coroutine's start to the last one's end with the
    device synchronised, 3 runs after a warm-up at n = 16.  The dealing is not timed.  The opened table is checked against
    sort_model.

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
from honeybadgermpc_amd.progs import fixedpoint as fx  # noqa: E402
from honeybadgermpc_amd.progs import sorting as so  # noqa: E402

BLS = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
N, T = 4, 1
K, KAPPA, WIDTH = 64, 32, 2


def rnd(ctx, gen, count, rows=None):
    n = count if rows is None else rows * count
    t = ctx.reduce_(torch.randint(-(1 << 63), (1 << 63) - 1, (n, ctx.n_limbs), dtype=torch.int64, device="cuda", generator=gen))
    return t if rows is None else t.view(rows, count, ctx.n_limbs)


def fmt(ts):
    return f"{np.median(ts):10.1f} us ({min(ts):.1f} .. {max(ts):.1f})"


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


def time_layer(ctx, gen, reps, n, batch, layer):
    a, r, d, cnt = layer
    slots, plane, m, L = batch * cnt, batch * n, K - 1, ctx.n_limbs
    table, bits = rnd(ctx, gen, plane, WIDTH), rnd(ctx, gen, slots, K + KAPPA)
    c, carry = rnd(ctx, gen, slots), rnd(ctx, gen, slots)
    tp, tq, tpq = (rnd(ctx, gen, slots, WIDTH) for _ in range(3))
    opened = rnd(ctx, gen, slots, 2 * WIDTH)
    e = torch.arange(cnt, device="cuda")
    lo1 = ((e >> a) << (a + 1)) | (e & ((1 << a) - 1)) | r
    lo = (torch.arange(batch, device="cuda").unsqueeze(1) * n + lo1.unsqueeze(0)).reshape(-1)
    hi = lo + d
    bufs = (ctx.empty(slots), ctx.empty(slots), torch.empty((2 * WIDTH, slots, L), dtype=torch.int64, device="cuda"))

    def fused(work):
        masked, r1 = so.cmp_mask(ctx, work, layer, n, batch, bits, K, KAPPA, out=bufs[0], r1_out=bufs[1])
        out = so.swap_mask(ctx, work, layer, n, batch, c, r1, carry, tp, tq, K, out=bufs[2])
        so.swap_finish(ctx, work, layer, n, batch, opened, tp, tq, tpq)
        return masked, r1, out, work

    def composed(work):
        got = [(work[w].index_select(0, lo), work[w].index_select(0, hi)) for w in range(WIDTH)]
        diffs = [sa.sub(ctx, x, y) for x, y in got]
        masked, r1 = fx.trunc_mask(ctx, diffs[0], bits, K, m, KAPPA)
        u = sa.add(ctx, sa.neg(ctx, fx.div2m_finish(ctx, diffs[0], c, r1, carry, m, fx.NEG_TRUNC)), 1)
        out = torch.empty((2 * WIDTH, slots, L), dtype=torch.int64, device="cuda")
        for w in range(WIDTH):
            sa.sub(ctx, u, tp[w], out=out[2 * w])
            sa.sub(ctx, diffs[w], tq[w], out=out[2 * w + 1])
        for w in range(WIDTH):
            prod = sa.beaver_combine(ctx, opened[2 * w], opened[2 * w + 1], tp[w], tq[w], tpq[w])
            work[w].index_copy_(0, lo, sa.sub(ctx, got[w][0], prod))
            work[w].index_copy_(0, hi, sa.add(ctx, got[w][1], prod))
        return masked, r1, out, work

    same = all(bool(torch.equal(u, v)) for u, v in zip(fused(table.clone()), composed(table.clone())))
    w1, w2 = table.clone(), table.clone()
    tf, tc = alternate(reps, lambda: fused(w1), lambda: composed(w2))
    # element reads and writes of the fused steps, counted from the rows: cmp_mask 2 + (k + kappa) | 2; swap_mask 2 + 3 + 2 (width - 1) + 2 width | 2 width;
    # swap_finish 5 width + 2 width | 2 width
    elems = (2 + K + KAPPA + 2) + (5 + 2 * (WIDTH - 1) + 2 * WIDTH + 2 * WIDTH) + 9 * WIDTH
    print(f"(a) layer a = {a} r = {r} d = {d}  n = {n} batch = {batch}  slots = 2^{slots.bit_length() - 1}  fused (3 launches) {fmt(tf)}   "
          f"composed ({4 + 10 * WIDTH} launches) {fmt(tc)}   composed / fused = {np.median(tc) / np.median(tf):5.2f}   "
          f"{elems * slots * 8 * L / np.median(tf) / 1e3:7.1f} GB/s read + written   {'bit-equal' if same else 'MISMATCH'}", flush=True)


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


def time_sort(ctx, gen, n, runs):
    p, L = ctx.modulus, ctx.n_limbs
    plan = so.SortPlan(n, 1, WIDTH, K, KAPPA)
    py = random.Random(n)
    lim = 1 << (K - 2)
    keys = [py.choice([-lim, lim - 1, 0]) if i % 16 == 0 else py.randrange(-lim, lim) for i in range(n)]
    clear = [keys, list(range(n))]
    want = [[v % p for v in col] for col in so.sort_model(clear, n, K)]
    dtable = deal(ctx, gen, ctx.upload_ints([v % p for col in clear for v in col]).view(WIDTH, n, L))
    bits = torch.zeros((plan.size("bits"), L), dtype=torch.int64, device="cuda")
    bits[:, 0] = torch.randint(0, 2, (plan.size("bits"),), device="cuda", generator=gen)
    dbits = deal(ctx, gen, bits)

    def triples(kind):
        tp, tq = rnd(ctx, gen, plan.size(kind)), rnd(ctx, gen, plan.size(kind))
        return [deal(ctx, gen, v) for v in (tp, tq, sa.mul(ctx, tp, tq))]

    dcarry, dswap = triples("carry"), triples("swap")

    async def body(co, i):
        return await so.sort(co, dtable[i].clone(), plan, dbits[i], tuple(v[i] for v in dcarry), tuple(v[i] for v in dswap))

    async def opened(co, i):
        return ctx.download_ints(await co.open_share_array((await body(co, i)).view(-1, L)))

    ok = all(got == want[0] + want[1] for got in run_parties(p, opened)[1])
    return plan, [run_parties(p, body)[0] for _ in range(runs)], ok


def main():
    args = sys.argv[1:]
    if not torch.cuda.is_available():
        raise SystemExit("scratch/time_sorting.py needs the GPU")
    reps = max(20, int(args[0])) if args and args[0].isdigit() else 20
    label = args[args.index("--label") + 1] if "--label" in args else "working tree"
    print(f"# scratch/time_sorting.py, {reps} runs a figure: median (min .. max); {torch.cuda.get_device_name(0)} on {socket.gethostname()}; {label}")
    ctx = Context.get(BLS)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(31)
    n = 1024
    for batch in (128, 2048):
        for layer in ((9, 0, 512, 512), (0, 0, 1, 512)):
            assert layer in so.layers(n)
            time_layer(ctx, gen, reps, n, batch, layer)
            torch.cuda.empty_cache()
    time_sort(ctx, gen, 16, 1)
    plan, ts, ok = time_sort(ctx, gen, n, 3)
    print(f"(b) sort n = {n} width = {WIDTH}  parties = {N}, t = {T}  {plan.n_layers} layers, {plan.total_slots} comparators, {plan.opens} batches   "
          f"{np.median(ts) * 1e3:9.1f} ms ({min(ts) * 1e3:.1f} .. {max(ts) * 1e3:.1f}), all four parties   {np.median(ts) * 1e3 / plan.opens:6.2f} ms a batch   "
          f"{'opens to sort_model' if ok else 'MISMATCH'}", flush=True)


main()

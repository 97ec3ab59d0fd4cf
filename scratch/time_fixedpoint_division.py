"""The division kernels and protocol timed on the device:
   python scratch/time_fixedpoint_division.py [reps] [--label TEXT] > profiles/fixedpoint_division.txt

BLS12-381 Fr, k = 64, f = 32, kappa = 32 (truncation width 128: 160 bit planes a value).

(a) one Goldschmidt iteration between three opens, at count = 2^16 and 2^20: trunc_step(T_GOLD) finishes the truncations of y and x
    and writes the masked pairs of Y = [y (alpha + x)] and X = [x x]; product_step(TRUNC) combines the two products and writes their
    truncation masks: 2 launches.  Beside it the same iteration composed from the parent's calls: two trunc_pr_finish, an add, four
    subs, two beaver_combine and two trunc_mask: 11 launches.  What a step "opens" is what its mask wrote (degree-0 shares): no open
    is timed.  HIP events around one group, `reps` (at least 20) runs after a warm-up, the two versions alternated run by run; median
    (min .. max).  Outputs are compared bit for bit (the fused s = Y + r1 against the composed Y and r1 added).
(b) one whole div at count = 2^12: four parties (t = 1) in one process over an in-memory network, every party's coroutine on the one
    device, wall clock from the first coroutine's start to the last one's end with the device synchronised, 3 runs after a warm-up.
    The dealing is not timed.  Every opened quotient is checked against div_model.

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
from honeybadgermpc_amd.progs import fixedpoint_division as fd  # noqa: E402

BLS = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
N, T = 4, 1
K, F, KAPPA = 64, 32, 32


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


def main():
    args = sys.argv[1:]
    if not torch.cuda.is_available():
        raise SystemExit("scratch/time_fixedpoint_division.py needs the GPU")
    reps = max(20, int(args[0])) if args and args[0].isdigit() else 20
    label = args[args.index("--label") + 1] if "--label" in args else "working tree"
    print(f"# scratch/time_fixedpoint_division.py, {reps} runs a figure: median (min .. max); {torch.cuda.get_device_name(0)} on {socket.gethostname()}; {label}")
    p, k, f, kappa = BLS, K, F, KAPPA
    ctx = Context.get(p)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(23)
    eb = 8 * ctx.n_limbs
    theta, width = fd.goldschmidt_iterations(k, f), fd.div_width(k, f)
    nb, alpha, m = width + kappa, 1 << (2 * f), 2 * f
    # ---- (a)
    for count in (1 << 16, 1 << 20):
        vals, r1s, c = rnd(ctx, gen, count, rows=2), rnd(ctx, gen, count, rows=2), rnd(ctx, gen, count, rows=2)
        s = sa.add(ctx, vals.view(-1, ctx.n_limbs), r1s.view(-1, ctx.n_limbs)).view(vals.shape)
        ta, tb, tab = (rnd(ctx, gen, count, rows=2) for _ in range(3))
        bits = rnd(ctx, gen, count, rows=2 * nb)
        alpha_t = ctx.upload_ints([alpha]).expand(count, ctx.n_limbs).contiguous()

        def fused_a():
            masked = fd.trunc_step(ctx, fd.T_GOLD, c, s, m, ta, tb, alpha=alpha)
            return fd.product_step(ctx, fd.TRUNC, masked, ta, tb, tab, bits=bits, width=width, m=m, kappa=kappa)

        def composed_a():
            y, x = fx.trunc_pr_finish(ctx, vals[0], c[0], r1s[0], m), fx.trunc_pr_finish(ctx, vals[1], c[1], r1s[1], m)
            ax = sa.add(ctx, x, alpha_t)
            d0, e0, d1, e1 = sa.sub(ctx, y, ta[0]), sa.sub(ctx, ax, tb[0]), sa.sub(ctx, x, ta[1]), sa.sub(ctx, x, tb[1])
            big_y, big_x = sa.beaver_combine(ctx, d0, e0, ta[0], tb[0], tab[0]), sa.beaver_combine(ctx, d1, e1, ta[1], tb[1], tab[1])
            return fx.trunc_mask(ctx, big_y, bits[:nb], width, m, kappa), fx.trunc_mask(ctx, big_x, bits[nb:], width, m, kappa), big_y, big_x

        masked, kept = fused_a()
        (m0, r0), (m1, r1), by, bx = composed_a()
        same = bool(torch.equal(masked[0], m0) and torch.equal(masked[1], m1) and torch.equal(kept[0], sa.add(ctx, by, r0)) and torch.equal(kept[1], sa.add(ctx, bx, r1)))
        tf, tc = alternate(reps, fused_a, composed_a)
        # fused traffic an element: trunc_step's two rows read 2 s, 2 c, ta, tb each and write 2 each; product_step reads 4 opened, 6 triple rows, 2 nb planes, writes 4
        moved = (12 + 4 + 10 + 2 * nb + 4) * count * eb
        # composed: 2 finishes (3 in, 1 out), an add (2, 1), 4 subs (2, 1), 2 combines (5, 1), 2 masks (1 + nb in, 2 out)
        moved_c = (8 + 3 + 12 + 12 + 2 * (nb + 3)) * count * eb
        print(f"(a) one Goldschmidt iteration, k = {k}, f = {f}, width {width}  count = 2^{count.bit_length() - 1}   fused (2 launches) {fmt(tf)}   composed (11 launches) {fmt(tc)}   "
              f"composed / fused = {np.median(tc) / np.median(tf):5.2f}   {moved / np.median(tf) / 1e3:7.1f} GB/s read + written by the two launches "
              f"({moved / count // eb} elements an element against {moved_c / count // eb} composed)   {'bit-equal' if same else 'MISMATCH'}", flush=True)
        del vals, r1s, c, s, ta, tb, tab, bits, masked, kept, m0, r0, m1, r1, by, bx
        torch.cuda.empty_cache()
    # ---- (b)
    count = 1 << 12
    py = random.Random(5)
    lay = fd.div_layout(k, f, kappa, theta, True)
    bvals, avals = [], []
    for _ in range(count):
        nbits = py.randrange(1, k)
        b = py.randrange(1 << (nbits - 1), 1 << nbits) * py.choice((1, -1))
        lim = min(((abs(b) << (k - 2)) - 1) >> f, (1 << (k - 1)) - 1)
        bvals.append(b), avals.append(py.randrange(-lim, lim + 1))
    planes = torch.zeros((lay["n_planes"], count, ctx.n_limbs), dtype=torch.int64, device="cuda")
    planes[:, :, 0] = torch.randint(0, 2, (lay["n_planes"], count), device="cuda", generator=gen)
    names = ["w", "y0"] + [f"iter{i}.{v}" for i in range(1, theta) for v in "yx"] + ["last"]
    limits = [2 * (k - 1 - f), f] + [2 * f] * (2 * theta - 1)
    host = planes[:, :, 0].cpu().numpy()
    r1 = [[sum(int(host[lay["planes"][name][0] + i][e]) << i for i in range(mm)) for name, mm in zip(names, limits)] for e in range(0, count, 97)]
    want = [fd.div_model(avals[e], bvals[e], p, k, f, r1[j], theta) for j, e in enumerate(range(0, count, 97))]
    da, db, dbits = deal(ctx, gen, ctx.upload_ints([v % p for v in avals])), deal(ctx, gen, ctx.upload_ints([v % p for v in bvals])), deal(ctx, gen, planes)
    tp, tq = rnd(ctx, gen, count, lay["n_triples"]), rnd(ctx, gen, count, lay["n_triples"])
    tpq = sa.mul(ctx, tp.view(-1, ctx.n_limbs), tq.view(-1, ctx.n_limbs)).view(tp.shape)
    dtrip = [deal(ctx, gen, v) for v in (tp, tq, tpq)]

    async def body(co, i):
        return await fd.div(co, da[i], db[i], dbits[i], tuple(v[i] for v in dtrip), f, k, kappa)

    async def opened(co, i):
        return ctx.download_ints((await co.open_share_array(await body(co, i)))[::97].contiguous())

    ok = all(got == want for got in run_parties(p, opened)[1])
    ts = [run_parties(p, body)[0] * 1e3 for _ in range(3)]
    print(f"(b) div k = {k}, f = {f}, theta = {theta}  count = 2^12  n = {N}, t = {T}  {lay['opens']} opens, {lay['n_triples']} triples and {lay['n_planes']} bit planes an element   "
          f"{fmt(ts, 'ms')}, all four parties   {'opens to div_model' if ok else 'MISMATCH'}", flush=True)


main()

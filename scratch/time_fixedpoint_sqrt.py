"""The square root's kernels and protocol timed on the device:
   python scratch/time_fixedpoint_sqrt.py [reps] [--label TEXT] > profiles/fixedpoint_sqrt.txt

BLS12-381 Fr, k = 64, f = 32, kappa = 32 (N = 63 planes, truncation width 140).

(a) every fused launch of csrc/hb_fxsqrt.hip at count = 2^16 and 2^20, beside the same step composed from calls the package had before:
      norm_mask   sqrt_norm_mask with one and with two sets of weights | fixedpoint_division.norm_mask (v and the masked pair) and, a plane
                  a set, one mul by the public D_i and one add: 1 + 2 N sets launches
      first       sqrt_first | beaver_combine, mul, neg, add, two subs: 6 launches
      GH          sqrt_trunc_step(GH), two rows | two trunc_pr_finish, two subs: 4 launches
      R           sqrt_trunc_step(R, BOTH) | trunc_pr_finish, neg, add, four subs: 7 launches
      OUT         sqrt_trunc_step(OUT, BOTH) | two trunc_pr_finish, four subs: 6 launches
    HIP events around one group, `reps` (at least 20) runs after a warm-up, the two versions alternated run by run; median (min ..
    max).  Outputs are compared bit for bit.
(b) one whole sqrt at count = 2^12: four parties (t = 1) in one process over an in-memory network, every party's coroutine on the one
    device, wall clock from the first coroutine's start to the last one's end with the device synchronised, 3 runs after a warm-up.
    The dealing is not timed.  Sampled opened roots are checked against sqrt_model.

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
from honeybadgermpc_amd.progs import fixedpoint_sqrt as fs  # noqa: E402

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
        raise SystemExit("scratch/time_fixedpoint_sqrt.py needs the GPU")
    reps = max(20, int(args[0])) if args and args[0].isdigit() else 20
    label = args[args.index("--label") + 1] if "--label" in args else "working tree"
    print(f"# scratch/time_fixedpoint_sqrt.py, {reps} runs a figure: median (min .. max); {torch.cuda.get_device_name(0)} on {socket.gethostname()}; {label}")
    p, k, f, kappa = BLS, K, F, KAPPA
    ctx = Context.get(p)
    L = ctx.n_limbs
    gen = torch.Generator(device="cuda")
    gen.manual_seed(29)
    eb = 8 * L
    n, beta, m = k - 1, 1 << (k - 1), k
    # ---- (a)
    for count in (1 << 16, 1 << 20):
        x, na, nb = (rnd(ctx, gen, count) for _ in range(3))
        y = rnd(ctx, gen, count, rows=n)
        vals, r1s, c, kept, ta, tb, tab = (rnd(ctx, gen, count, rows=2) for _ in range(7))
        s = sa.add(ctx, vals.view(-1, L), r1s.view(-1, L)).view(vals.shape)

        def report(name, launches, fused, composed, same, moved):
            tf, tc = alternate(reps, fused, composed)
            slower = np.median(tf) > max(tc)
            print(f"(a) {name:<22} count = 2^{count.bit_length() - 1}   fused (1 launch) {fmt(tf)}   composed ({launches} launches) {fmt(tc)}   composed / fused = "
                  f"{np.median(tc) / np.median(tf):6.2f}   {moved * count * eb / np.median(tf) / 1e3:7.1f} GB/s read + written   {'bit-equal' if same else 'MISMATCH'}"
                  f"{'   FUSED SLOWER THAN THE COMPOSED FORM AND ITS SPREAD' if slower else ''}", flush=True)

        for what in (fs.SQRT, fs.BOTH):
            w = fs.weight_rows(ctx, k, f, what)
            sets = w.shape[0]
            wi = ctx.download_ints(w.reshape(-1, L))

            def fused_n():
                return fs.sqrt_norm_mask(ctx, x, y, w, ta[:1], tb[:1])

            def composed_n():
                masked, v = fd.norm_mask(ctx, x, y, None, ta[:1], tb[:1])
                ts = []
                for q in range(sets):
                    acc = sa.mul(ctx, y[0], wi[q * n])
                    for i in range(1, n):
                        acc = sa.add(ctx, acc, sa.mul(ctx, y[i], wi[q * n + i]), out=acc)
                    ts.append(acc)
                return masked, v, ts

            masked, kp = fused_n()
            cm, cv, cts = composed_n()
            same = bool(torch.equal(masked, cm) and torch.equal(kp[0], cv) and all(torch.equal(kp[1 + q], t) for q, t in enumerate(cts)))
            report(f"norm_mask, {sets} set{'s' if sets > 1 else ''}", 1 + 2 * (n - 1) * sets + sets, fused_n, composed_n, same, n + 3 + 2 + 1 + sets)

        def fused_f():
            return fs.sqrt_first(ctx, c, ta[:1], tb[:1], tab[:1], (na, nb), k)

        def composed_f():
            cc = sa.beaver_combine(ctx, c[0], c[1], ta[0], tb[0], tab[0])
            y0 = sa.add(ctx, sa.neg(ctx, sa.mul(ctx, cc, fs.Y0_SLOPE)), fs.a_prime(k))
            return sa.sub(ctx, cc, na), sa.sub(ctx, y0, nb), y0

        masked, h = fused_f()
        c0, c1, cy = composed_f()
        report("first", 6, fused_f, composed_f, bool(torch.equal(masked[0], c0) and torch.equal(masked[1], c1) and torch.equal(h, cy)), 7 + 3)

        def fused_g():
            return fs.sqrt_trunc_step(ctx, fs.GH, c, s, m, ta[:1], tb[:1])

        def composed_g():
            g, hh = fx.trunc_pr_finish(ctx, vals[0], c[0], r1s[0], m), fx.trunc_pr_finish(ctx, vals[1], c[1], r1s[1], m)
            return sa.sub(ctx, g, ta[0]), sa.sub(ctx, hh, tb[0]), g, hh

        masked, gh = fused_g()
        c0, c1, cg, ch = composed_g()
        report("trunc_step GH", 4, fused_g, composed_g, bool(torch.equal(masked[0], c0) and torch.equal(masked[1], c1) and torch.equal(gh[0], cg) and torch.equal(gh[1], ch)),
               6 + 4)

        def fused_r():
            return fs.sqrt_trunc_step(ctx, fs.R, c[:1], s[:1], m, ta, tb, kept=kept, which=fs.BOTH, cst=3 * beta)

        def composed_r():
            t = fx.trunc_pr_finish(ctx, vals[0], c[0], r1s[0], m)
            r = sa.add(ctx, sa.neg(ctx, t), 3 * beta)
            return sa.sub(ctx, kept[0], ta[0]), sa.sub(ctx, r, tb[0]), sa.sub(ctx, kept[1], ta[1]), sa.sub(ctx, r, tb[1])

        masked = fused_r()
        report("trunc_step R, both", 7, fused_r, composed_r, all(bool(torch.equal(masked[q], v)) for q, v in enumerate(composed_r())), 2 * 5 + 4)

        def fused_o():
            return fs.sqrt_trunc_step(ctx, fs.OUT, c, s, m, ta, tb, kept=kept, which=fs.BOTH)

        def composed_o():
            t0, t1 = fx.trunc_pr_finish(ctx, vals[0], c[0], r1s[0], m), fx.trunc_pr_finish(ctx, vals[1], c[1], r1s[1], m)
            return sa.sub(ctx, t0, ta[0]), sa.sub(ctx, kept[0], tb[0]), sa.sub(ctx, t1, ta[1]), sa.sub(ctx, kept[1], tb[1])

        masked = fused_o()
        report("trunc_step OUT, both", 6, fused_o, composed_o, all(bool(torch.equal(masked[q], v)) for q, v in enumerate(composed_o())), 2 * 5 + 4)
        del x, na, nb, y, vals, r1s, c, kept, ta, tb, tab, s, masked, kp, cm, cv, cts
        torch.cuda.empty_cache()
    # ---- (b)
    count = 1 << 12
    py = random.Random(5)
    lay = fs.sqrt_layout(k, f, kappa, None, fs.SQRT)
    theta = lay["theta"]
    xs = []
    for _ in range(count):
        nbits = py.randrange(1, k)
        xs.append(py.randrange(1 << (nbits - 1), 1 << nbits))
    planes = torch.zeros((lay["n_planes"], count, L), dtype=torch.int64, device="cuda")
    planes[:, :, 0] = torch.randint(0, 2, (lay["n_planes"], count), device="cuda", generator=gen)
    nbp = lay["width"] + kappa
    starts = [st for name, (a, b) in sorted(lay["planes"].items(), key=lambda kv: kv[1]) if name != "bit_decompose" for st in range(a, b, nbp)]
    limits = fs.sqrt_shifts(k, theta, fs.SQRT)
    host = planes[:, :, 0].cpu().numpy()
    r1 = [[sum(int(host[st + i][e]) << i for i in range(mm)) for st, mm in zip(starts, limits)] for e in range(0, count, 97)]
    want = [fs.sqrt_model(xs[e], p, k, f, r1[j], theta, fs.SQRT) for j, e in enumerate(range(0, count, 97))]
    dx, dbits = deal(ctx, gen, ctx.upload_ints(xs)), deal(ctx, gen, planes)
    tp, tq = rnd(ctx, gen, count, lay["n_triples"]), rnd(ctx, gen, count, lay["n_triples"])
    tpq = sa.mul(ctx, tp.view(-1, L), tq.view(-1, L)).view(tp.shape)
    dtrip = [deal(ctx, gen, v) for v in (tp, tq, tpq)]

    async def body(co, i):
        return await fs.sqrt(co, dx[i], dbits[i], tuple(v[i] for v in dtrip), f, k, kappa)

    async def opened(co, i):
        return ctx.download_ints((await co.open_share_array(await body(co, i)))[::97].contiguous())

    ok = all(got == want for got in run_parties(p, opened)[1])
    ts = [run_parties(p, body)[0] * 1e3 for _ in range(3)]
    print(f"(b) sqrt k = {k}, f = {f}, theta = {theta}  count = 2^12  n = {N}, t = {T}  {lay['opens']} opens, {lay['n_triples']} triples and {lay['n_planes']} bit planes an element   "
          f"{fmt(ts, 'ms')}, all four parties   {'opens to sqrt_model' if ok else 'MISMATCH'}", flush=True)


main()

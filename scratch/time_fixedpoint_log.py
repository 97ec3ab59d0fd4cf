"""The logarithm's kernels and protocol timed on the device:
   python scratch/time_fixedpoint_log.py [reps] [--label TEXT] > profiles/fixedpoint_log.txt

BLS12-381 Fr, k = 64, f = 32, kappa = 32 (N = 63 planes, degree 12, truncation width 128).

(a) every fused launch of csrc/hb_fxlog.hip at count = 2^12, 2^16 and 2^20, beside the same step composed from calls the package had
    before:
      first       log_first | beaver_combine, two muls, three subs: 6 launches
      level 2     log_level(2, d = 12): two powers finished, four products masked | two trunc_pr_finish, eight subs: 10 launches
      level 3     log_level(3, d = 12): four powers finished, four products masked | four trunc_pr_finish, eight subs: 12 launches
      poly_mask   log_poly_mask(d = 12): four powers finished, 13 terms, the mask | four trunc_pr_finish, 13 muls, 12 adds, trunc_mask, add:
                  31 launches
      finish      log_finish | trunc_pr_finish, add: 2 launches
    HIP events around one group, `reps` (at least 20) runs after a warm-up, the two versions alternated run by run; median (min ..
    max).  Outputs are compared bit for bit.  A fused step slower than its composition and the composition's spread is reported as such.
(b) one whole log2 at count = 2^12: four parties (t = 1) in one process over an in-memory network, every party's coroutine on the one
    device, wall clock from the first coroutine's start to the last one's end with the device synchronised, 3 runs after a warm-up.
    The dealing is not timed.  Sampled opened results are checked against log_model.

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
from honeybadgermpc_amd.progs import fixedpoint_log as fl  # noqa: E402

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
        raise SystemExit("scratch/time_fixedpoint_log.py needs the GPU")
    reps = max(20, int(args[0])) if args and args[0].isdigit() else 20
    label = args[args.index("--label") + 1] if "--label" in args else "working tree"
    print(f"# scratch/time_fixedpoint_log.py, {reps} runs a figure: median (min .. max); {torch.cuda.get_device_name(0)} on {socket.gethostname()}; {label}")
    p, k, f, kappa = BLS, K, F, KAPPA
    ctx = Context.get(p)
    L = ctx.n_limbs
    gen = torch.Generator(device="cuda")
    gen.manual_seed(31)
    eb = 8 * L
    lay = fl.log_layout(k, f, kappa)
    d, width, m, m_out = lay["degree"], lay["width"], k - 1, k - 1 + fl.GUARD_BITS
    coef = fl.coefficient_rows(ctx, k, f, 2, d)
    coef_ints = [c % p for c in fl.log_coefficients(k, f, 2, d)]
    # ---- (a)
    for count in (1 << 12, 1 << 16, 1 << 20):
        ybig, na, nb, ipart = (rnd(ctx, gen, count) for _ in range(4))
        vals, r1s, c, ta, tb, tab = (rnd(ctx, gen, count, rows=4) for _ in range(6))
        pw0 = rnd(ctx, gen, count, rows=d)
        planes = torch.zeros((width + kappa, count, L), dtype=torch.int64, device="cuda")
        planes[:, :, 0] = torch.randint(0, 2, (width + kappa, count), device="cuda", generator=gen)
        s = sa.add(ctx, vals.view(-1, L), r1s.view(-1, L)).view(vals.shape)

        def report(name, launches, fused, composed, same, moved):
            tf, tc = alternate(reps, fused, composed)
            slower = np.median(tf) > max(tc)
            print(f"(a) {name:<22} count = 2^{count.bit_length() - 1}   fused (1 launch) {fmt(tf)}   composed ({launches} launches) {fmt(tc)}   composed / fused = "
                  f"{np.median(tc) / np.median(tf):6.2f}   {moved * count * eb / np.median(tf) / 1e3:7.1f} GB/s read + written   {'bit-equal' if same else 'MISMATCH'}"
                  f"{'   FUSED SLOWER THAN THE COMPOSED FORM AND ITS SPREAD' if slower else ''}", flush=True)

        def fused_f():
            return fl.log_first(ctx, c[:2], ta[:1], tb[:1], tab[:1], ybig, (na, nb), d)

        def composed_f():
            cc = sa.beaver_combine(ctx, c[0], c[1], ta[0], tb[0], tab[0])
            t = sa.sub(ctx, sa.mul(ctx, cc, 4), sa.mul(ctx, ybig, 3))
            return sa.sub(ctx, t, na), sa.sub(ctx, t, nb), t

        masked, pw = fused_f()
        c0, c1, ct = composed_f()
        report("first", 6, fused_f, composed_f, bool(torch.equal(masked[0], c0) and torch.equal(masked[1], c1) and torch.equal(pw[0], ct)), 8 + 3)

        def finished(rows):
            return [fx.trunc_pr_finish(ctx, vals[q], c[q], r1s[q], m) for q in range(rows)]

        for level, done in ((2, 2), (3, 4)):
            half = 1 << (level - 1)
            work = pw0.clone()

            def fused_l():
                return fl.log_level(ctx, level, d, c[:done], s[:done], m, ta, tb, work)

            def composed_l():
                allp = [pw0[j] for j in range(half)] + finished(done)
                return [v for q in range(4) for v in (sa.sub(ctx, allp[2 * half - 1], ta[q]), sa.sub(ctx, allp[q], tb[q]))], allp

            masked = fused_l()
            cm, allp = composed_l()
            same = all(bool(torch.equal(masked[q], v)) for q, v in enumerate(cm)) and all(bool(torch.equal(work[half + q], allp[half + q])) for q in range(done))
            report(f"level {level}", done + 8, fused_l, composed_l, same, 2 * done + 4 + 8 + done + 8)

        def fused_p():
            return fl.log_poly_mask(ctx, d, c, s, m, pw0, ybig, coef, planes, width, m_out, kappa)

        def composed_p():
            allp = [pw0[j] for j in range(8)] + finished(4)
            poly = sa.mul(ctx, ybig, coef_ints[0])
            for j in range(1, d + 1):
                poly = sa.add(ctx, poly, sa.mul(ctx, allp[j - 1], coef_ints[j]), out=poly)
            mk, r1 = fx.trunc_mask(ctx, poly, planes, width, m_out, kappa)
            return mk, sa.add(ctx, poly, r1)

        masked, kept = fused_p()
        cm, ck = composed_p()
        report("poly_mask", 4 + 13 + 12 + 2, fused_p, composed_p, bool(torch.equal(masked[0], cm) and torch.equal(kept[0], ck)), 8 + 8 + 1 + width + kappa + 2)

        def fused_e():
            return fl.log_finish(ctx, c[0], s[:1], m_out, ipart)

        def composed_e():
            return sa.add(ctx, fx.trunc_pr_finish(ctx, vals[0], c[0], r1s[0], m_out), ipart)

        report("finish", 2, fused_e, composed_e, bool(torch.equal(fused_e(), composed_e())), 3 + 1)
        del ybig, na, nb, ipart, vals, r1s, c, ta, tb, tab, pw0, planes, s, masked, kept, cm, ck, work, pw
        torch.cuda.empty_cache()
    # ---- (b)
    count = 1 << 12
    py = random.Random(5)
    xs = []
    for _ in range(count):
        nbits = py.randrange(1, k)
        xs.append(py.randrange(1 << (nbits - 1), 1 << nbits))
    planes = torch.zeros((lay["n_planes"], count, L), dtype=torch.int64, device="cuda")
    planes[:, :, 0] = torch.randint(0, 2, (lay["n_planes"], count), device="cuda", generator=gen)
    nbp = width + kappa
    starts = [st for name, (a, b) in sorted(lay["planes"].items(), key=lambda kv: kv[1]) if name != "bit_decompose" for st in range(a, b, nbp)]
    limits = fl.log_shifts(k, f)
    host = planes[:, :, 0].cpu().numpy()
    r1 = [[sum(int(host[st + i][e]) << i for i in range(mm)) for st, mm in zip(starts, limits)] for e in range(0, count, 97)]
    want = [fl.log_model(xs[e], p, k, f, r1[j]) for j, e in enumerate(range(0, count, 97))]
    dx, dbits = deal(ctx, gen, ctx.upload_ints(xs)), deal(ctx, gen, planes)
    tp, tq = rnd(ctx, gen, count, lay["n_triples"]), rnd(ctx, gen, count, lay["n_triples"])
    tpq = sa.mul(ctx, tp.view(-1, L), tq.view(-1, L)).view(tp.shape)
    dtrip = [deal(ctx, gen, v) for v in (tp, tq, tpq)]

    async def body(co, i):
        return await fl.log2(co, dx[i], dbits[i], tuple(v[i] for v in dtrip), f, k, kappa)

    async def opened(co, i):
        return ctx.download_ints((await co.open_share_array(await body(co, i)))[::97].contiguous())

    ok = all(got == want for got in run_parties(p, opened)[1])
    ts = [run_parties(p, body)[0] * 1e3 for _ in range(3)]
    print(f"(b) log2 k = {k}, f = {f}, degree {d}  count = 2^12  n = {N}, t = {T}  {lay['opens']} opens, {lay['n_triples']} triples and {lay['n_planes']} bit planes an element   "
          f"{fmt(ts, 'ms')}, all four parties   {'opens to log_model' if ok else 'MISMATCH'}", flush=True)


main()

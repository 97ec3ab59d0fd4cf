"""The arctangent's kernels and protocol timed on the device:
   python scratch/time_fixedpoint_atan.py [reps] [--label TEXT] > profiles/fixedpoint_atan.txt

BLS12-381 Fr, k = 64, f = 32, kappa = 32 (N = 63, degree 23: 12 odd powers, 15 products over 5 levels, truncation width 128).

(a) every fused launch of csrc/hb_fxatan.hip at count = 2^12 and 2^18, beside the same step composed from calls the package had before:
      sign_mask    sign_mask | sigma (mul, neg, add), six subs: 9 launches
      abs          abs_step | three beaver_combine, two muls, three subs, trunc_mask: 9 launches
      select_mask  select_mask | two sigmas, four subs: 10 launches
      select       select | two beaver_combine, add, sub: 4 launches
      first        atan_first | mul, sigma, four subs: 8 launches
      level 0      atan_level(0): u finished, two products masked | trunc_pr_finish, four subs: 5 launches
      level 3      atan_level(3): four odd powers and a square finished, four products masked | five trunc_pr_finish, eight subs: 13 launches
      poly_mask    atan_poly_mask: four powers finished, 12 terms, the mask | four trunc_pr_finish, 12 muls, 11 adds, trunc_mask, add: 29 launches
      assemble     atan_assemble | trunc_pr_finish, beaver_combine, sigma, two muls, add, three subs: 11 launches
      finish       atan_finish | beaver_combine, add: 2 launches
    HIP events around one group, `reps` (at least 20) runs after a warm-up, the two versions alternated run by run; median (min ..
    max).  Outputs are compared bit for bit.  A fused step whose median is above its composition's is marked FUSED DOES NOT WIN, and
    OUTSIDE THE COMPOSITION'S SPREAD where it is above the composition's slowest run too.
(b) one whole atan2 at count = 2^12: four parties (t = 1) in one process over an in-memory network, every party's coroutine on the one
    device, wall clock from the first coroutine's start to the last one's end with the device synchronised, 7 runs after a warm-up.
    The dealing is not timed.  Sampled opened results are checked against atan2_model.

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
from honeybadgermpc_amd.progs import fixedpoint_atan as fa  # noqa: E402

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
        raise SystemExit("scratch/time_fixedpoint_atan.py needs the GPU")
    reps = max(20, int(args[0])) if args and args[0].isdigit() else 20
    label = args[args.index("--label") + 1] if "--label" in args else "working tree"
    print(f"# scratch/time_fixedpoint_atan.py, {reps} runs a figure: median (min .. max); {torch.cuda.get_device_name(0)} on {socket.gethostname()}; {label}")
    p, k, f, kappa = BLS, K, F, KAPPA
    ctx = Context.get(p)
    L = ctx.n_limbs
    gen = torch.Generator(device="cuda")
    gen.manual_seed(37)
    eb = 8 * L
    lay = fa.atan_layout(k, f, kappa)
    d, width, m, m_out = lay["degree"], lay["width"], k - 1, k - 1 + fa.GUARD_BITS
    rows = (d + 1) // 2
    assert (d, lay["products"]) == (23, [1, 2, 3, 5, 4])
    coef = fa.coefficient_rows(ctx, k, f, False, d)
    coef_ints = [c % p for c in fa.atan_coefficients(k, f, False, d)]
    consts = fa.assemble_constants(p, f, False)
    sigma = lambda b: sa.add(ctx, sa.neg(ctx, sa.mul(ctx, b, 2)), 1)
    eq = lambda a, b: bool(torch.equal(a, b))
    # ---- (a)
    for count in (1 << 12, 1 << 18):
        x, y, cc, w, g = (rnd(ctx, gen, count) for _ in range(5))
        vals, r1s, c, ta, tb, tab = (rnd(ctx, gen, count, rows=6) for _ in range(6))
        pw0 = rnd(ctx, gen, count, rows=rows)
        planes = torch.zeros((width + kappa, count, L), dtype=torch.int64, device="cuda")
        planes[:, :, 0] = torch.randint(0, 2, (width + kappa, count), device="cuda", generator=gen)
        s = sa.add(ctx, vals.view(-1, L), r1s.view(-1, L)).view(vals.shape)
        sxy = c[4:6].reshape(2 * count, L)
        sx, sy = c[4], c[5]

        def report(name, launches, fused, composed, same, moved):
            tf, tc = alternate(reps, fused, composed)
            mark = ""
            if np.median(tf) > np.median(tc):
                mark = "   FUSED DOES NOT WIN" + (", OUTSIDE THE COMPOSITION'S SPREAD" if np.median(tf) > max(tc) else " (within the composition's spread)")
            print(f"(a) {name:<12} count = 2^{count.bit_length() - 1}   fused (1 launch) {fmt(tf)}   composed ({launches} launches) {fmt(tc)}   composed / fused = "
                  f"{np.median(tc) / np.median(tf):6.2f}   {moved * count * eb / np.median(tf) / 1e3:7.1f} GB/s read + written   {'bit-equal' if same else 'MISMATCH'}"
                  f"{mark}", flush=True)

        def pairs_masked(pairs):
            return [v for r, (a, b) in enumerate(pairs) for v in (sa.sub(ctx, a, ta[r]), sa.sub(ctx, b, tb[r]))]

        def beaver(r):
            return sa.beaver_combine(ctx, c[2 * r], c[2 * r + 1], ta[r], tb[r], tab[r])

        def finished(n_rows):
            return [fx.trunc_pr_finish(ctx, vals[q], c[q], r1s[q], m) for q in range(n_rows)]

        fused_f = lambda: fa.sign_mask(ctx, sxy, x, y, ta[:3], tb[:3])
        composed_f = lambda: pairs_masked([(sx, x), (sy, y), (sigma(sy), sx)])
        report("sign_mask", 9, fused_f, composed_f, all(eq(a, b) for a, b in zip(fused_f(), composed_f())), 10 + 6)

        fused_f = lambda: fa.abs_step(ctx, c, ta[:3], tb[:3], tab[:3], x, y, planes, k, kappa)

        def composed_f():
            pr = [beaver(r) for r in range(3)]
            ax, ay = sa.sub(ctx, x, sa.mul(ctx, pr[0], 2)), sa.sub(ctx, y, sa.mul(ctx, pr[1], 2))
            ww = sa.sub(ctx, ax, ay)
            mk, r1 = fx.trunc_mask(ctx, ww, planes, k, k - 1, kappa)
            return mk, [ax, ay, pr[2], ww, r1]

        (fm, fk), (cm, ck) = fused_f(), composed_f()
        report("abs", 9, fused_f, composed_f, eq(fm[0], cm) and all(eq(a, b) for a, b in zip(fk, ck)), 6 + 9 + 2 + k + kappa + 6)

        fused_f = lambda: fa.select_mask(ctx, cc, w, sx, ta[:2], tb[:2])
        composed_f = lambda: pairs_masked([(cc, w), (sigma(cc), sigma(sx))])
        report("select_mask", 10, fused_f, composed_f, all(eq(a, b) for a, b in zip(fused_f(), composed_f())), 3 + 4 + 4)

        fused_f = lambda: fa.select(ctx, c[:4], ta[:2], tb[:2], tab[:2], x, y)

        def composed_f():
            pr = [beaver(r) for r in range(2)]
            return [sa.add(ctx, y, pr[0]), sa.sub(ctx, x, pr[0]), pr[1]]

        report("select", 4, fused_f, composed_f, all(eq(a, b) for a, b in zip(fused_f(), composed_f())), 4 + 6 + 2 + 3)

        fused_f = lambda: fa.atan_first(ctx, x, m - f, sy, g, ta[:2], tb[:2], d)

        def composed_f():
            t = sa.mul(ctx, x, 1 << (m - f))
            return pairs_masked([(t, t), (sigma(sy), g)]), t

        (fm, fp), (cm, ct) = fused_f(), composed_f()
        report("first", 8, fused_f, composed_f, all(eq(a, b) for a, b in zip(fm, cm)) and eq(fp[0], ct), 3 + 4 + 4 + 1)

        for level in (0, 3):
            done, nxt, odd = lay["products"][level], lay["products"][level + 1], len(fa._level_odd(level + 1, d))
            half = 1 << (level - 1) if level else 0
            work = pw0.clone()

            def fused_l():
                return fa.atan_level(ctx, level, d, c[:done], s[:done], m, ta[:nxt], tb[:nxt], work)

            def composed_l():
                new = finished(done)
                allp = [pw0[j] for j in range(max(half, 1))] + new[:done - 1]
                return pairs_masked([(allp[q] if q < odd else new[-1], new[-1]) for q in range(nxt)]), new

            masked = fused_l()
            cm, new = composed_l()
            same = all(eq(masked[q], v) for q, v in enumerate(cm)) and all(eq(work[half + q], new[q]) for q in range(done - 1))
            report(f"level {level}", done + 2 * nxt, fused_l, composed_l, same, 2 * done + 2 * nxt + min(odd, max(half, 1)) + (done - 1) + 2 * nxt)

        done = lay["products"][-1]
        half = 1 << (lay["levels"] - 1)
        fused_f = lambda: fa.atan_poly_mask(ctx, d, c[:done], s[:done], m, pw0, coef, planes, width, m_out, kappa)

        def composed_f():
            allp = [pw0[j] for j in range(half)] + finished(done)
            poly = sa.mul(ctx, allp[0], coef_ints[0])
            for j in range(1, rows):
                poly = sa.add(ctx, poly, sa.mul(ctx, allp[j], coef_ints[j]), out=poly)
            mk, r1 = fx.trunc_mask(ctx, poly, planes, width, m_out, kappa)
            return mk, sa.add(ctx, poly, r1)

        (fm, fk), (cm, ck) = fused_f(), composed_f()
        report("poly_mask", done + rows + rows - 1 + 2, fused_f, composed_f, eq(fm[0], cm) and eq(fk[0], ck), 2 * done + half + width + kappa + 2)

        fused_f = lambda: fa.atan_assemble(ctx, c[0], s[:1], m_out, c[2:4], ta[1], tb[1], tab[1], sy, g, consts, ta[2], tb[2])

        def composed_f():
            a = fx.trunc_pr_finish(ctx, vals[0], c[0], r1s[0], m_out)
            e = beaver(1)
            cst = sa.add(ctx, sa.mul(ctx, g, consts[0]), sa.mul(ctx, sa.sub(ctx, sigma(sy), e), consts[1]))
            return [sa.sub(ctx, e, ta[2]), sa.sub(ctx, a, tb[2])], cst

        (fm, fc), (cm, cst) = fused_f(), composed_f()
        report("assemble", 11, fused_f, composed_f, eq(fm[0], cm[0]) and eq(fm[1], cm[1]) and eq(fc, cst), 2 + 2 + 3 + 2 + 2 + 2 + 1)

        fused_f = lambda: fa.atan_finish(ctx, c[:2], ta[0], tb[0], tab[0], cc)
        composed_f = lambda: sa.add(ctx, cc, beaver(0))
        report("finish", 2, fused_f, composed_f, eq(fused_f(), composed_f()), 2 + 3 + 1 + 1)
        del x, y, cc, w, g, vals, r1s, c, ta, tb, tab, pw0, planes, s, sxy, sx, sy, work, masked, cm, new, fm, fk, ck, fc, cst, fp, ct
        torch.cuda.empty_cache()
    # ---- (b)
    count = 1 << 12
    py = random.Random(5)
    lim = 1 << (k - 1)
    pairs = [(py.randrange(-lim + 1, lim) >> py.randrange(k - 1), py.randrange(-lim + 1, lim) >> py.randrange(k - 1)) for _ in range(count)]
    planes = torch.zeros((lay["n_planes"], count, L), dtype=torch.int64, device="cuda")
    planes[:, :, 0] = torch.randint(0, 2, (lay["n_planes"], count), device="cuda", generator=gen)
    nbp = width + kappa
    base = lay["planes"]["div"][0]
    starts = [base + a for name, (a, b) in sorted(lay["div"]["planes"].items(), key=lambda kv: kv[1]) if name != "bit_decompose"]
    starts += [st for name, (a, b) in sorted(lay["planes"].items(), key=lambda kv: kv[1]) if name.startswith("level") or name == "poly" for st in range(a, b, nbp)]
    limits = fa.atan_shifts(k, f)
    host = planes[:, :, 0].cpu().numpy()
    r1 = [[sum(int(host[st + i][e]) << i for i in range(mm)) for st, mm in zip(starts, limits)] for e in range(0, count, 97)]
    want = [fa.atan2_model(*pairs[e], p, k, f, r1[j]) for j, e in enumerate(range(0, count, 97))]
    dy, dx, dbits = deal(ctx, gen, ctx.upload_ints([v % p for v, _ in pairs])), deal(ctx, gen, ctx.upload_ints([v % p for _, v in pairs])), deal(ctx, gen, planes)
    tp, tq = rnd(ctx, gen, count, lay["n_triples"]), rnd(ctx, gen, count, lay["n_triples"])
    tpq = sa.mul(ctx, tp.view(-1, L), tq.view(-1, L)).view(tp.shape)
    dtrip = [deal(ctx, gen, v) for v in (tp, tq, tpq)]

    async def body(co, i):
        return await fa.atan2(co, dy[i], dx[i], dbits[i], tuple(v[i] for v in dtrip), f, k, kappa)

    async def opened(co, i):
        return ctx.download_ints((await co.open_share_array(await body(co, i)))[::97].contiguous())

    ok = all(got == want for got in run_parties(p, opened)[1])
    ts = [run_parties(p, body)[0] * 1e3 for _ in range(7)]
    print(f"(b) atan2 k = {k}, f = {f}, degree {d}  count = 2^12  n = {N}, t = {T}  {lay['opens']} opens, {lay['n_triples']} triples and {lay['n_planes']} bit planes an element   "
          f"{fmt(ts, 'ms')}, all four parties   {'opens to atan2_model' if ok else 'MISMATCH'}", flush=True)


main()

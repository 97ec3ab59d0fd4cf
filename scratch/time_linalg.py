"""The matrix-product kernel and the two shared-product protocols timed on the device:
   python scratch/time_linalg.py [reps] [--label TEXT] > profiles/linalg.txt

BLS12-381 Fr (32-byte elements) and 2^64 - 59 (8-byte elements).

(a) linalg.matmul at 64^3, 256^3, 1024 x 64 x 1024 and linalg.dot at k = 2^20: HIP events around one call, `reps` (at least 20) runs
    after a warm-up; median (min .. max) and field multiply-accumulates a second (m k n over the median; k_pm_direct, the same lazy
    arithmetic, reaches 209 G/s over BLS: profiles/power_mixing.txt).  Beside it the only route to the same product before this
    kernel: the left factor downloaded, hb_matrix_from_host, hb_matvec over the right factor's columns -- host clock from before the
    download to a device synchronise after the mat-vec, table build and synchronisations included, 5 runs -- for the shapes that
    route accepts.  Outputs are compared bit for bit.
(b) the split over the inner dimension: the library's rule against the single launch (hb_debug_mat_split(-1)) on the same operands,
    alternated run by run.
(c) the fused epilogue: matmul(add=c) against matmul followed by share_arithmetic.add, alternated run by run.
(d) one double_sharing_matmul and one beaver_matmul at 64^3 beside share_arithmetic.beaver_multiply_arrays on the expanded array of
    64^3 scalar products (without the sum that route still needs): four parties (t = 1) in one process over an in-memory network,
    every party's coroutine on the one device, wall clock from the first coroutine's start to the last one's end with the device
    synchronised, 3 runs after a warm-up.  The dealing is not timed.  Every opened result is checked.

No GPU: fails (there is nothing to fall back to)."""
import asyncio
import ctypes
import socket
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from honeybadgermpc_amd import linalg  # noqa: E402
from honeybadgermpc_amd import share_arithmetic as sa  # noqa: E402
from honeybadgermpc_amd._capi import Context, HbmpcBackendError, HbView, np_ptr  # noqa: E402
from honeybadgermpc_amd.open_coalescer import OpenCoalescer  # noqa: E402

BLS = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
P64 = (1 << 64) - 59
N, T = 4, 1


def rnd(ctx, gen, *shape):
    count = int(np.prod(shape))
    t = ctx.reduce_(torch.randint(-(1 << 63), (1 << 63) - 1, (count, ctx.n_limbs), dtype=torch.int64, device="cuda", generator=gen))
    return t.view(*shape, ctx.n_limbs)


def fmt(ts):
    return f"{np.median(ts):10.1f} us ({min(ts):.1f} .. {max(ts):.1f})"


def timed(reps, fn):
    fn()
    torch.cuda.synchronize()
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(reps)]
    for e in evs:
        e[0].record()
        fn()
        e[1].record()
    torch.cuda.synchronize()
    return [e[0].elapsed_time(e[1]) * 1e3 for e in evs]


def alternate(reps, one, two):
    one(); two()
    torch.cuda.synchronize()
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(reps)]
    for e3 in evs:
        e3[0].record()
        one()
        e3[1].record()
        two()
        e3[2].record()
    torch.cuda.synchronize()
    return [e3[0].elapsed_time(e3[1]) * 1e3 for e3 in evs], [e3[1].elapsed_time(e3[2]) * 1e3 for e3 in evs]


def matvec_route(ctx, a, b, m, k, n):
    """-> the product by hb_matrix_from_host + hb_matvec, the left factor downloaded first"""
    host = np.ascontiguousarray(a.reshape(m * k, ctx.n_limbs).cpu().numpy().view(np.uint64))
    h = ctypes.c_void_p()
    ctx.check(ctx.lib.hb_matrix_from_host(ctx.h, np_ptr(host), m, k, ctypes.byref(h), ctx.stream()), "hb_matrix_from_host")
    out = ctx.empty(m * n)
    view = HbView(1, n)
    try:
        ctx.check(ctx.lib.hb_matvec(ctx.h, h, ctx.ptr(b), view, None, ctx.ptr(out), view, n, ctx.stream()), "hb_matvec")
        torch.cuda.synchronize()
    finally:
        ctx.lib.hb_matrix_destroy(h)
    return out


class Net:
    def __init__(self, n):
        self.q = [dict() for _ in range(n)]

    def get_send_recv(self, i):
        def factory(tag):
            def send(dest, msg):
                self.q[dest].setdefault(tag, asyncio.Queue()).put_nowait((i, msg))

            return send, self.q[i].setdefault(tag, asyncio.Queue()).get

        return factory


def deal(ctx, gen, values, degree=1):
    flat = values.reshape(-1, ctx.n_limbs)
    coeffs = [rnd(ctx, gen, flat.shape[0]) for _ in range(degree)]
    out = []
    for i in range(N):
        acc = flat
        for e, c in enumerate(coeffs):
            acc = sa.add(ctx, acc, sa.mul(ctx, c, pow(i + 1, e + 1, ctx.modulus)))
        out.append(acc.view(values.shape))
    return out


def run_parties(p, body):
    async def main():
        net = Net(N)
        return await asyncio.gather(*[body(OpenCoalescer(p, N, T, i, net.get_send_recv(i)), i) for i in range(N)])

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = asyncio.run(main())
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res


def section_a(ctx, gen, name, reps):
    L = ctx.n_limbs
    for m, k, n in ((64, 64, 64), (256, 256, 256), (1024, 64, 1024), (1, 1 << 20, 1)):
        a, b = rnd(ctx, gen, m, k), rnd(ctx, gen, k, n)
        ts = timed(reps, lambda: linalg.matmul(ctx, a, b))
        got = linalg.matmul(ctx, a, b)
        shape = "dot k = 2^20" if m == 1 else f"{m} x {k} x {n}"
        line = f"(a) {name:8s} {shape:18s} matmul {fmt(ts)}  {m * k * n / np.median(ts) / 1e3:7.1f} G mac/s  ({'split' if linalg.takes_split(1, m, k, n) else 'one launch'})"
        try:
            same = bool(torch.equal(matvec_route(ctx, a, b, m, k, n).view(m, n, L), got))
            hs = []
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                matvec_route(ctx, a, b, m, k, n)
                hs.append((time.perf_counter() - t0) * 1e6)
            line += f"   from_host + matvec {fmt(hs)}  route / matmul = {np.median(hs) / np.median(ts):7.1f}   {'bit-equal' if same else 'MISMATCH'}"
        except HbmpcBackendError as e:
            line += f"   from_host + matvec refuses the shape ({str(e)[:90]})"
        print(line, flush=True)


def section_b(ctx, gen, name, reps):
    for batch, m, k, n in ((1, 1, 1 << 20, 1), (1, 1, 1 << 14, 1), (1, 16, 4096, 32), (1, 64, 2048, 64), (16, 16, 2048, 32)):
        a, b = rnd(ctx, gen, batch, m, k), rnd(ctx, gen, batch, k, n)

        def auto():
            return linalg.matmul(ctx, a, b)

        def single():
            ctx.lib.hb_debug_mat_split(-1)
            try:
                return linalg.matmul(ctx, a, b)
            finally:
                ctx.lib.hb_debug_mat_split(0)

        same = bool(torch.equal(auto(), single()))
        ta, tb = alternate(reps, auto, single)
        print(f"(b) {name:8s} batch {batch:2d} {m:3d} x {k:7d} x {n:3d}  split {fmt(ta)}   one launch {fmt(tb)}   one launch / split = {np.median(tb) / np.median(ta):6.2f}   "
              f"{'bit-equal' if same else 'MISMATCH'}", flush=True)


def section_c(ctx, gen, name, reps):
    for m, k, n in ((64, 64, 64), (256, 256, 256), (1024, 64, 1024)):
        a, b, c = rnd(ctx, gen, m, k), rnd(ctx, gen, k, n), rnd(ctx, gen, m, n)

        def fused():
            return linalg.matmul(ctx, a, b, add=c)

        def composed():
            return sa.add(ctx, linalg.matmul(ctx, a, b).view(-1, ctx.n_limbs), c.view(-1, ctx.n_limbs))

        same = bool(torch.equal(fused().view(-1, ctx.n_limbs), composed()))
        tf, tc = alternate(reps, fused, composed)
        print(f"(c) {name:8s} {m} x {k} x {n}  fused epilogue {fmt(tf)}   matmul then add {fmt(tc)}   composed / fused = {np.median(tc) / np.median(tf):5.2f}   "
              f"{'bit-equal' if same else 'MISMATCH'}", flush=True)


def section_d(ctx, gen, runs=3):
    p, L = ctx.modulus, ctx.n_limbs

    def case(d):
        X, Y, R, P, Q = (rnd(ctx, gen, d, d) for _ in range(5))
        XY, PQ = linalg.matmul(ctx, X, Y), linalg.matmul(ctx, P, Q)
        dX, dY, dP, dQ, dPQ, dRt = (deal(ctx, gen, v) for v in (X, Y, P, Q, PQ, R))
        dR2 = deal(ctx, gen, R, degree=2)
        # the element-wise route: x[i][l][j] = X[i][l], y[i][l][j] = Y[l][j], one scalar triple a product
        ex = [v.unsqueeze(2).expand(d, d, d, L).reshape(-1, L).contiguous() for v in dX]
        ey = [v.unsqueeze(0).expand(d, d, d, L).reshape(-1, L).contiguous() for v in dY]
        tp, tq = rnd(ctx, gen, d * d * d), rnd(ctx, gen, d * d * d)
        dtp, dtq, dtpq = (deal(ctx, gen, v) for v in (tp, tq, sa.mul(ctx, tp, tq)))

        async def ds(co, i):
            return await linalg.double_sharing_matmul(co, dX[i], dY[i], dRt[i], dR2[i])

        async def bv(co, i):
            return await linalg.beaver_matmul(co, dX[i], dY[i], (dP[i], dQ[i], dPQ[i]))

        async def ew(co, i):
            return await sa.beaver_multiply_arrays(co, ex[i], ey[i], (dtp[i], dtq[i], dtpq[i]))

        def opened(body):
            async def run(co, i):
                return await co.open_share_array((await body(co, i)).view(-1, L))

            return run

        ok = {}
        for nm, body in (("ds", ds), ("bv", bv)):
            ok[nm] = all(bool(torch.equal(r.view(d, d, L), XY)) for r in run_parties(p, opened(body))[1])
        want = sa.mul(ctx, X.unsqueeze(2).expand(d, d, d, L).reshape(-1, L).contiguous(), Y.unsqueeze(0).expand(d, d, d, L).reshape(-1, L).contiguous())
        ok["ew"] = all(bool(torch.equal(r, want)) for r in run_parties(p, opened(ew))[1])
        return {"ds": ds, "bv": bv, "ew": ew}, ok

    bodies, _ = case(8)
    for body in bodies.values():
        run_parties(p, body)
    d = 64
    bodies, ok = case(d)
    secs = {}
    for nm, label, method in (("ds", "double_sharing_matmul", linalg.DOUBLE_SHARING), ("bv", "beaver_matmul", linalg.BEAVER),
                              ("ew", "beaver_multiply_arrays (expanded)", linalg.ELEMENTWISE)):
        ts = [run_parties(p, bodies[nm])[0] for _ in range(runs)]
        secs[nm] = float(np.median(ts))
        print(f"(d) {label:34s} 64 x 64 x 64  n = {N}, t = {T}  {linalg.count_opens(method, d, d, d):7d} opened elements, {linalg.count_triples(method, d, d, d):7d} scalar triples   "
              f"{np.median(ts) * 1e3:9.1f} ms ({min(ts) * 1e3:.1f} .. {max(ts) * 1e3:.1f}), all four parties   {'opens to X Y' if ok[nm] else 'MISMATCH'}", flush=True)
    print(f"(d) element-wise / double sharing = {secs['ew'] / secs['ds']:6.2f}   element-wise / matrix Beaver = {secs['ew'] / secs['bv']:6.2f}", flush=True)


def main():
    args = sys.argv[1:]
    if not torch.cuda.is_available():
        raise SystemExit("scratch/time_linalg.py needs the GPU")
    reps = max(20, int(args[0])) if args and args[0].isdigit() else 20
    label = args[args.index("--label") + 1] if "--label" in args else "working tree"
    print(f"# scratch/time_linalg.py, {reps} runs a figure: median (min .. max); {torch.cuda.get_device_name(0)} on {socket.gethostname()}; {label}")
    print(f"# tile {linalg.TILE_M} x {linalg.TILE_N} x {linalg.TILE_K}, L = {linalg.LAZY_L}, split when at most {linalg.SPLIT_MAX_WORKGROUPS} workgroups and k >= {linalg.SPLIT_MIN_K}")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(31)
    fields = (("BLS", Context.get(BLS)), ("2^64-59", Context.get(P64)))
    for section in (section_a, section_b, section_c):
        for name, ctx in fields:
            section(ctx, gen, name, reps)
    section_d(fields[0][1], gen)


main()

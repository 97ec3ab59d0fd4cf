"""The Jubjub kernels timed on the device:
   python scratch/time_jubjub.py [reps] [--label TEXT] [--level-only | --scalar-only | --protocol-only | --kernels | --steps] > profiles/jubjub.txt

(a) One level of shared additions, LOCAL launches only (no open: what a stage wrote is handed to the next as if it had been opened --
the timing of the arithmetic, not of the protocol): fused = add_mask, add_stage1, add_stage2, add_stage3, add_finish of
honeybadgermpc_amd.progs.jubjub (6 launches); composed = the same addition line by line as SharedPoint.add reads, from
share_arithmetic's sub / beaver_combine / mul / add / inv (the local halves of beaver_multiply_arrays and divide_share_arrays).
m = 2^10, 2^16, 2^20 pairs, BLS12-381 Fr and 2^64 - 59.  HIP events around one level, `reps` levels after a warm-up, the two versions
ALTERNATED call by call in one run; median (min .. max).  The operands are random field elements, not curve points: the kernels do
field arithmetic and never ask.

(b) scalar_mul at 2^10, 2^16, 2^20 elements with random 255-bit (64-bit) scalars, a scalar and a point per element; also as field
multiplications a second.  The products are COUNTED, from the code of hb_jj.hip and fp29.hpp and from the scalars of the run: 8 a
doubling for each of the 32 NW rounds, 9 an addition for each set bit of each scalar (the bits are counted on the host), fp_inv's
29 NL squarings and popcount(p - 2) products, 4 before the loop (two conversions, x y, d x y) and 2 after it (X / Z, Y / Z).  Lanes of
a wave whose bits differ wait for one another's additions: that idle time is in the denominator, not in the count.

(c) Protocol: n = 4, t = 1, every party in this process over an in-process transport, B = 2^10 clients: wall time (host clock ending
in a synchronise) of a whole share_mul(K = 32) and of a whole mimc_decrypt (share_mul, then 161 rounds over 3 blocks a client).
Opens, Python and the event loop included: it is NOT kernel time.

--kernels runs two levels of each version at 2^20 over BLS12-381 and one scalar_mul at 2^16, and nothing else (for a kernel trace).
--steps times every entry point alone at both widths (the stages at m = 2^20, scalar_mul and double_table at 2^16), HIP events around
one launch with the host kept ahead of the device; run it against two builds of the library (HBMPC_HIP_LIB) in one visit to compare them.
No GPU: fails (there is nothing to fall back to)."""
import asyncio
import socket
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from honeybadgermpc_amd import share_arithmetic as sa  # noqa: E402
from honeybadgermpc_amd._capi import Context  # noqa: E402
from honeybadgermpc_amd.elliptic_curve import Jubjub  # noqa: E402
from honeybadgermpc_amd.open_coalescer import OpenCoalescer  # noqa: E402
from honeybadgermpc_amd.progs import jubjub, mimc, mimc_jubjub_pkc as pkc  # noqa: E402

BLS = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
P64 = (1 << 64) - 59
MAD_RATE = 34.0e12          # profiles/r01_mad_issue_rate_vs_occupancy.txt, as scratch/time_mimc.py
MADS = {4: 162, 1: 18}


def rnd(ctx, gen, count):
    return ctx.reduce_(torch.randint(-(1 << 63), (1 << 63) - 1, (count, ctx.n_limbs), dtype=torch.int64, device="cuda", generator=gen))


def fmt(ts):
    return f"{np.median(ts):9.1f} us ({min(ts):.1f} .. {max(ts):.1f})"


def curve_of(p):
    return Jubjub() if p == BLS else Jubjub(-1, 2, p)


def fused_level(ctx, curve, P, Q, trip, rs):
    a = jubjub.add_mask(ctx, P, Q, trip)
    b = jubjub.add_stage1(ctx, a, trip, rs)
    uv, c = jubjub.add_stage2(ctx, b, trip, rs, curve)
    d = jubjub.add_stage3(ctx, c, trip)
    return jubjub.add_finish(ctx, d, uv, check=False)[0]


def composed_level(ctx, curve, P, Q, trip, rs):
    """SharedPoint.add line by line; every product is the local part of beaver_multiply_arrays (two sub, one beaver_combine), every
    division the local part of divide_share_arrays (a product, an inversion, a scaling, a product).  Triples by the fused index."""
    (x1, y1), (x2, y2) = P, Q
    tp, tq, tpq = trip

    def product(x, y, k):
        return sa.beaver_combine(ctx, sa.sub(ctx, x, tp[k]), sa.sub(ctx, y, tq[k]), tp[k], tq[k], tpq[k])

    def divide(num, den, r, k_inv, k_mul):
        sig = product(den, r, k_inv)
        inv, _ = sa.inv(ctx, sig, check=False)
        return product(num, sa.mul(ctx, r, inv), k_mul)

    xp, yp = product(x1, x2, 0), product(y1, y2, 1)
    d_prod = sa.mul(ctx, product(xp, yp, 4), curve.d)
    nx = sa.add(ctx, product(x1, y2, 2), product(y1, x2, 3))
    x3 = divide(nx, sa.add(ctx, d_prod, 1), rs[0], 7, 5)
    y3 = divide(sa.add(ctx, yp, xp), sa.add(ctx, sa.neg(ctx, d_prod), 1), rs[1], 8, 6)
    return x3, y3


def time_level(reps):
    print("# (a) one level of shared additions, local launches only: fused = 6 launches (hb_jj.hip); composed = SharedPoint.add line by line from "
          "share_arithmetic (37 calls of its functions, one launch each, counted from composed_level; --kernels under a kernel trace shows them)")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    for name, p in (("BLS12-381 Fr", BLS), ("2^64 - 59", P64)):
        ctx = Context.get(p)
        curve = curve_of(p)
        for n in (10, 16, 20):
            m = 1 << n
            P, Q = (rnd(ctx, gen, m), rnd(ctx, gen, m)), (rnd(ctx, gen, m), rnd(ctx, gen, m))
            trip = tuple(rnd(ctx, gen, 9 * m).reshape(9, m, ctx.n_limbs) for _ in range(3))
            rs = rnd(ctx, gen, 2 * m).reshape(2, m, ctx.n_limbs)
            for _ in range(2):
                fused_level(ctx, curve, P, Q, trip, rs); composed_level(ctx, curve, P, Q, trip, rs)
            torch.cuda.synchronize()
            evs = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(reps)]
            for e3 in evs:
                for ev in e3:
                    ev.record()
            torch.cuda.synchronize()
            for e3 in evs:
                e3[0].record()
                fused_level(ctx, curve, P, Q, trip, rs)
                e3[1].record()
                composed_level(ctx, curve, P, Q, trip, rs)
                e3[2].record()
            torch.cuda.synchronize()
            tf = [e3[0].elapsed_time(e3[1]) * 1e3 for e3 in evs]
            tc = [e3[1].elapsed_time(e3[2]) * 1e3 for e3 in evs]
            print(f"{name:13s} m = 2^{n:<2d}   fused {fmt(tf)}   composed {fmt(tc)}   composed / fused = {np.median(tc) / np.median(tf):5.2f}", flush=True)
            del P, Q, trip, rs
            torch.cuda.empty_cache()


def some_points(ctx, curve, gen, count):
    """`count` points of the curve: random multiples of a base point, by the kernel under test (its results are checked by the tests)"""
    p = curve.p
    if p == BLS:
        base = pkc.GP
    else:
        from honeybadgermpc_amd.elliptic_curve import Point

        x = 2
        while True:
            y2 = (1 + x * x) * pow(1 - curve.d * x * x, -1, p) % p
            if pow(y2, (p - 1) // 2, p) == 1:
                break
            x += 1
        v = pow(2 * y2, (p - 5) // 8, p)
        base = Point(x, y2 * v * (2 * y2 * v * v - 1) % p, curve)
    return jubjub.scalar_mul(ctx, rnd(ctx, gen, count), base)


def time_scalar(reps):
    print("# (b) scalar_mul, a scalar and a point per element; G mul/s = counted products / median: 8 a doubling x 32 NW rounds + 9 an addition x the set bits of "
          "the run's scalars + fp_inv (29 NL squarings + popcount(p - 2)) + 6 around the loop; estimate = what 34.0e12 v_mad_u64_u32 a second allow at "
          "162 (9 digits) or 18 (3 digits) of them a product -- an estimate of the bound, not a target")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    for name, p in (("BLS12-381 Fr", BLS), ("2^64 - 59", P64)):
        ctx = Context.get(p)
        curve = curve_of(p)
        rounds, nl = 64 * ctx.n_limbs, 9 if ctx.n_limbs == 4 else 3
        fixed = 8 * rounds + 29 * nl + bin(p - 2).count("1") + 6
        for n in (10, 16, 20):
            count = 1 << n
            pts = some_points(ctx, curve, gen, count)
            ns = rnd(ctx, gen, count)
            set_bits = int(np.unpackbits(ns.cpu().numpy().view(np.uint8)).sum())
            muls = fixed * count + 9 * set_bits
            out = (ctx.empty(count), ctx.empty(count))
            jubjub.scalar_mul(ctx, ns, pts, curve, out=out)
            torch.cuda.synchronize()
            evs = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(reps)]
            for e2 in evs:
                e2[0].record()
                jubjub.scalar_mul(ctx, ns, pts, curve, out=out)
                e2[1].record()
            torch.cuda.synchronize()
            ts = [e2[0].elapsed_time(e2[1]) * 1e3 for e2 in evs]
            rate = muls / (np.median(ts) * 1e-6)
            bound = MAD_RATE / MADS[ctx.n_limbs]
            print(f"{name:13s} count = 2^{n:<2d}   {fmt(ts)}   {np.median(ts) * 1e-6 / count * 1e9:8.1f} ns a point   {muls / count:.1f} products an element ({set_bits / count:.1f} set bits): "
                  f"{rate / 1e9:7.1f} G mul/s ({rate / bound * 100:4.1f}% of the estimate {bound / 1e9:.0f} G)", flush=True)
            del pts, ns, out
            torch.cuda.empty_cache()


class Net:
    def __init__(self, n):
        self.q = [dict() for _ in range(n)]

    def _queue(self, party, tag):
        return self.q[party].setdefault(tag, asyncio.Queue())

    def get_send_recv(self, i):
        def factory(tag):
            def send(dest, msg):
                self._queue(dest, tag).put_nowait((i, msg))

            return send, self._queue(i, tag).get

        return factory


def time_protocol(reps):
    print("# (c) whole protocols, n = 4, t = 1, four parties in one process over an in-process transport, B = 2^10 clients, K = 32 bits: wall time (host clock "
          "ending in a synchronise); opens, Python and the event loop included -- not kernel time")
    p, n, t, K, B, blocks = BLS, 4, 1, 32, 1 << 10, 3
    ctx = Context.get(p)
    L = ctx.n_limbs
    curve = curve_of(p)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9)

    def deal(secret):
        r = rnd(ctx, gen, secret.shape[0])
        return [sa.add(ctx, secret, sa.mul(ctx, r, i + 1)) for i in range(n)]

    bit_values = (torch.randint(0, 2, (K * B, 1), device="cuda", generator=gen, dtype=torch.int64) * torch.tensor([[1] + [0] * (L - 1)], device="cuda")).contiguous()
    bits = deal(bit_values)
    pairs = (K - 1) * B
    a, b = rnd(ctx, gen, 9 * pairs), rnd(ctx, gen, 9 * pairs)
    trip = [deal(v) for v in (a, b, sa.mul(ctx, a, b))]
    rs = deal(rnd(ctx, gen, 2 * pairs))
    r = rnd(ctx, gen, mimc.ROUND * B * blocks)
    r2 = sa.mul(ctx, r, r)
    cubes = [deal(v) for v in (r, r2, sa.mul(ctx, r2, r))]
    pts = some_points(ctx, curve, gen, B)
    cs = rnd(ctx, gen, B * blocks).reshape(B, blocks, L)

    async def run(what):
        net = Net(n)

        async def party(i):
            co = OpenCoalescer(p, n, t, i, net.get_send_recv(i))
            tr = tuple(c[i].reshape(9, pairs, L) for c in trip)
            bi = bits[i].reshape(K, B, L)
            if what == "share_mul":
                out = await jubjub.share_mul(co, bi, pts, tr, rs[i].reshape(2, pairs, L))
                return co.batches, out
            cu = tuple(c[i].reshape(mimc.ROUND, B * blocks, L) for c in cubes)
            return co.batches, await pkc.mimc_decrypt(co, bi, (cs, pts), tr, rs[i].reshape(2, pairs, L), cu)

        return await asyncio.gather(*[party(i) for i in range(n)])

    for what in ("share_mul", "mimc_decrypt"):
        times = []
        for rep in range(reps + 1):                                      # the first pass warms up and is not counted
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = asyncio.run(run(what))
            torch.cuda.synchronize()
            if rep:
                times.append(time.perf_counter() - t0)
        print(f"{what:13s} B = 2^10, K = {K}" + (f", {blocks} blocks a client, {mimc.ROUND} rounds" if what == "mimc_decrypt" else "") +
              f": {res[0][0]} batches   {np.median(times):8.3f} s ({min(times):.3f} .. {max(times):.3f}), {reps} timed runs", flush=True)


def one_launch(reps, fn, pad):
    """HIP events around ONE call with the host kept ahead of the device: the device is still clearing `pad` when the call is enqueued"""
    fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in evs:
        pad.zero_()
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) * 1e3 for e0, e1 in evs]


def time_steps(reps):
    """--steps: every entry point of csrc/hb_jj.hip alone, both widths: the stages of the shared addition at m = 2^20, scalar_mul and
    double_table (8 rows) at 2^16 points.  add_finish and double_table are their row's launch and the batched inversion behind it."""
    pad = torch.empty(1 << 29, dtype=torch.uint8, device="cuda")
    for p, name in ((BLS, "<9, 8>"), (P64, "<3, 2>")):
        ctx, curve = Context.get(p), curve_of(p)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(11)
        m, small = 1 << 20, 1 << 16
        P, Q = (rnd(ctx, gen, m), rnd(ctx, gen, m)), (rnd(ctx, gen, m), rnd(ctx, gen, m))
        trip = tuple(rnd(ctx, gen, 9 * m).reshape(9, m, ctx.n_limbs) for _ in range(3))
        rs = rnd(ctx, gen, 2 * m).reshape(2, m, ctx.n_limbs)
        A, B, C, D, uv = (rnd(ctx, gen, k * m) for k in (8, 6, 4, 2, 2))
        pts, ns = some_points(ctx, curve, gen, small), rnd(ctx, gen, small)
        steps = (("JjMaskRow", lambda: jubjub.add_mask(ctx, P, Q, trip)), ("JjStage1Row", lambda: jubjub.add_stage1(ctx, A, trip, rs)),
                 ("JjStage2Row", lambda: jubjub.add_stage2(ctx, B, trip, rs, curve)), ("JjStage3Row", lambda: jubjub.add_stage3(ctx, C, trip)),
                 ("add_finish (JjScaleRow)", lambda: jubjub.add_finish(ctx, D, uv, check=False)),
                 ("JjScalarMulRow", lambda: jubjub.scalar_mul(ctx, ns, pts, curve)),
                 ("double_table (JjDoubleTableRow)", lambda: jubjub.double_table(ctx, pts, 8, curve)))
        for step, fn in steps:
            print(f"step {step + ' ' + name:40s} {fmt(one_launch(reps, fn, pad))}", flush=True)
        del P, Q, trip, rs, A, B, C, D, uv, pts, ns, steps
        torch.cuda.empty_cache()


def main():
    args = sys.argv[1:]
    if not torch.cuda.is_available():
        raise SystemExit("scratch/time_jubjub.py needs the GPU")
    reps = int(args[0]) if args and args[0].isdigit() else 20
    label = args[args.index("--label") + 1] if "--label" in args else "working tree"
    if "--steps" in args:
        print(f"# scratch/time_jubjub.py --steps, {reps} runs a figure, HIP events around one launch: median (min .. max); {label}")
        return time_steps(reps)
    if "--kernels" in args:
        ctx = Context.get(BLS)
        curve = curve_of(BLS)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(7)
        m = 1 << 20
        P, Q = (rnd(ctx, gen, m), rnd(ctx, gen, m)), (rnd(ctx, gen, m), rnd(ctx, gen, m))
        trip = tuple(rnd(ctx, gen, 9 * m).reshape(9, m, ctx.n_limbs) for _ in range(3))
        rs = rnd(ctx, gen, 2 * m).reshape(2, m, ctx.n_limbs)
        for _ in range(2):
            fused_level(ctx, curve, P, Q, trip, rs)
            composed_level(ctx, curve, P, Q, trip, rs)
        jubjub.scalar_mul(ctx, rnd(ctx, gen, 1 << 16), pkc.GP)
        torch.cuda.synchronize()
        return
    print(f"# scratch/time_jubjub.py, {reps} calls a figure: median (min .. max); {torch.cuda.get_device_name(0)} on {socket.gethostname()}; {label}")
    only = [a for a in args if a.endswith("-only")]
    if not only or "--level-only" in only:
        time_level(reps)
    if not only or "--scalar-only" in only:
        time_scalar(reps)
    if not only or "--protocol-only" in only:
        time_protocol(3)


main()

"""local_power_sums of honeybadgermpc_amd.power_mixing timed call by call (HIP events) at M = k in {256, 1024, 4096} over BLS12-381's
scalar field, both paths; beside it the same result composed only from calls the package exported before (share_arithmetic.mul /
add, hb_fft_batch_evaluate), and at k = 256 the route through Python ints (the binomial formula through field.py):
   python scratch/time_power_mixing.py [reps] [--label TEXT] [--sizes 256,1024] [--crossover] > profiles/power_mixing.txt
--crossover adds the curve HB_PM_AUTO's constant is read from (M = k from 8 to 512, both paths).
--kernels runs each path three times at M = k = 1024 and nothing else (for a kernel trace).
Every figure: warm-up, then `reps` calls, each between its own pair of events recorded once before the timed region; median and
the spread (min .. max) are printed."""
import socket
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from honeybadgermpc_amd import power_mixing as pm  # noqa: E402
from honeybadgermpc_amd import share_arithmetic as sa  # noqa: E402
from honeybadgermpc_amd._capi import Context, np_ptr  # noqa: E402
from honeybadgermpc_amd.field import GF  # noqa: E402
from honeybadgermpc_amd.polynomial import get_omega  # noqa: E402

BLS = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def timed(call, reps, warm=2):
    """-> (median, min, max) microseconds of a call"""
    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in evs:
        a.record(); b.record()
    torch.cuda.synchronize()
    for a, b in evs:
        a.record()
        call()
        b.record()
    torch.cuda.synchronize()
    ts = [a.elapsed_time(b) * 1e3 for a, b in evs]
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def fmt(t):
    return f"{t[0]:11.1f} us ({t[1]:.1f} .. {t[2]:.1f})"


class Composed:
    """S_1 .. S_k from share_arithmetic.mul / add and hb_fft_batch_evaluate alone; tables of constants made once, as the library caches its own"""

    def __init__(self, ctx, m, k):
        p = ctx.modulus
        self.ctx, self.m, self.k, self.n = ctx, m, k, pm.transform_order(k)
        fact = [1]
        for i in range(1, k + 1):
            fact.append(fact[-1] * i % p)
        ifact = [pow(f, -1, p) for f in fact]
        self.ifact_u = ctx.upload_ints(ifact[1:]).repeat(m, 1)                       # (m k, limbs): 1 / j!, j = 1 .. k, a row a client
        self.ifact_v = ctx.upload_ints(ifact).repeat(m, 1)                           # (m (k + 1), limbs)
        ninv = pow(self.n, -1, p)
        self.scale = ctx.upload_ints([fact[i] * ninv % p for i in range(1, k + 1)])
        om = int(get_omega(GF(p), self.n, seed=0).value)
        self.omega, self.omega_inv = ctx.host_elems([om]), ctx.host_elems([pow(om, -1, p)])
        self.one = ctx.upload_ints([1])

    def fft(self, omega, x, rows, d):
        ctx = self.ctx
        out = ctx.empty(rows * self.n)
        ctx.check(ctx.lib.hb_fft_batch_evaluate(ctx.h, np_ptr(omega), self.n, ctx.ptr(x), rows, d, self.n, ctx.ptr(out), ctx.stream()), "fft")
        return out

    def __call__(self, c, powers):
        ctx, m, k, L = self.ctx, self.m, self.k, self.ctx.n_limbs
        # u = (1, powers / j!)
        scaled = sa.mul(ctx, powers.reshape(m * k, L), self.ifact_u).reshape(m, k, L)
        u = torch.cat([self.one.expand(m, L).reshape(m, 1, L), scaled], dim=1).contiguous()
        # c^i by doubling: cp[:, h : 2h] = cp[:, : h] * c^h
        cp = torch.cat([self.one.expand(m, L).reshape(m, 1, L), c.reshape(m, 1, L)], dim=1).contiguous()
        ch = sa.mul(ctx, c, c)                                                       # c^2
        while cp.shape[1] < k + 1:
            h = cp.shape[1]
            nxt = sa.mul(ctx, cp.reshape(m * h, L), ch.reshape(m, 1, L).expand(m, h, L).contiguous().reshape(m * h, L)).reshape(m, h, L)
            cp = torch.cat([cp, nxt], dim=1)
            ch = sa.mul(ctx, ch, ch)
        v = sa.mul(ctx, cp[:, : k + 1].contiguous().reshape(m * (k + 1), L), self.ifact_v)
        big_u = self.fft(self.omega, u.reshape(m * (k + 1), L), m, k + 1)
        big_v = self.fft(self.omega, v, m, k + 1)
        w = sa.mul(ctx, big_u, big_v, out=big_u).reshape(m, self.n, L)
        rows = m
        while rows > 1:                                                              # halving tree over the client axis
            half = rows // 2
            sa.add(ctx, w[:half].reshape(half * self.n, L), w[rows - half:rows].reshape(half * self.n, L), out=w[:half].reshape(half * self.n, L))
            rows -= half
        back = self.fft(self.omega_inv, w[0].contiguous(), 1, self.n)
        return sa.mul(ctx, back[1: k + 1].contiguous(), self.scale)


def python_ints(ctx, c, powers, k):
    p = ctx.modulus
    f = GF(p)
    cs = ctx.download_ints(c)
    flat = ctx.download_ints(powers.reshape(-1, ctx.n_limbs))
    sums = [f(0)] * k
    binom, row = [], [1]
    for _ in range(k):
        row = [1] + [(row[i] + row[i + 1]) % p for i in range(len(row) - 1)] + [1]
        binom.append(row)
    for ci in range(len(cs)):
        b = [f(1)] + [f(x) for x in flat[ci * k:(ci + 1) * k]]
        cp = [f(1)]
        for _ in range(k):
            cp.append(cp[-1] * f(cs[ci]))
        for m in range(1, k + 1):
            acc = f(0)
            for j in range(m + 1):
                acc = acc + cp[m - j] * b[j] * binom[m - 1][j]
            sums[m - 1] = sums[m - 1] + acc
    return ctx.upload_ints([int(s.value) for s in sums])


def main():
    args = sys.argv[1:]
    reps = int(args[0]) if args and args[0].isdigit() else 20
    label = args[args.index("--label") + 1] if "--label" in args else "working tree"
    sizes = [int(x) for x in args[args.index("--sizes") + 1].split(",")] if "--sizes" in args else [256, 1024, 4096]
    ctx = Context.get(BLS)
    L = ctx.n_limbs
    gen = torch.Generator(device="cuda")
    gen.manual_seed(77)

    def rnd(count):
        return ctx.reduce_(torch.randint(-(1 << 63), (1 << 63) - 1, (count, L), dtype=torch.int64, device="cuda", generator=gen))

    if "--kernels" in args:
        k = m = 1024
        c, powers = rnd(m), rnd(m * k).reshape(m, k, L)
        for _ in range(3):
            pm.local_power_sums(ctx, c, powers, method="direct")
            pm.local_power_sums(ctx, c, powers, method="ntt")
        torch.cuda.synchronize()
        return
    print(f"# scratch/time_power_mixing.py, {reps} calls a figure: median (min .. max); {torch.cuda.get_device_name(0)} on {socket.gethostname()}; {label}")
    print("# BLS12-381 Fr, M = k clients and powers; local_power_sums between HIP events; MAC/s = M k (k + 1) / 2 field multiply-accumulates over the direct path's time")
    for k in sizes:
        m = k
        c, powers = rnd(m), rnd(m * k).reshape(m, k, L)
        heavy = reps
        t_d = timed(lambda: pm.local_power_sums(ctx, c, powers, method="direct"), heavy)
        t_n = timed(lambda: pm.local_power_sums(ctx, c, powers, method="ntt"), heavy)
        comp = Composed(ctx, m, k)
        t_c = timed(lambda: comp(c, powers), heavy)
        fused, direct, composed = pm.local_power_sums(ctx, c, powers, method="ntt"), pm.local_power_sums(ctx, c, powers, method="direct"), comp(c, powers)
        same = bool(torch.equal(fused, composed)) and bool(torch.equal(fused, direct))
        macs = m * k * (k + 1) / 2
        print(f"M = k = {k:5d}  N = {pm.transform_order(k):6d}   direct {fmt(t_d)}  {macs / t_d[0] / 1e3:8.2f} G MAC/s   ntt {fmt(t_n)}   "
              f"composed from exported calls {fmt(t_c)} = {t_c[0] / t_n[0]:5.2f}x the fused NTT path ({'all three bit-equal' if same else 'MISMATCH'})", flush=True)
        if k == 256:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = python_ints(ctx, c, powers, k)
            torch.cuda.synchronize()
            host_s = time.perf_counter() - t0
            ok = bool(torch.equal(host, fused))
            print(f"M = k = {k:5d}  through Python ints (download_ints, the binomial formula through field.py, upload_ints): {host_s:8.2f} s; "
                  f"{host_s / (min(t_d[0], t_n[0]) * 1e-6):9.0f}x the faster device path ({'same values' if ok else 'MISMATCH'})", flush=True)
        del comp, fused, direct, composed
        torch.cuda.empty_cache()
    if "--crossover" in args:
        print("# crossover of HB_PM_AUTO: M = k, both paths")
        for k in (16, 64, 128, 256, 320, 384, 448, 512, 640, 768, 896, 1023):
            m = k
            c, powers = rnd(m), rnd(m * k).reshape(m, k, L)
            t_d = timed(lambda: pm.local_power_sums(ctx, c, powers, method="direct"), reps)
            t_n = timed(lambda: pm.local_power_sums(ctx, c, powers, method="ntt"), reps)
            print(f"M = k = {k:5d}  N = {pm.transform_order(k):6d}   direct {fmt(t_d)}   ntt {fmt(t_n)}   direct / ntt = {t_d[0] / t_n[0]:5.2f}", flush=True)


main()

"""The fixed-point kernels timed on the device:
   python scratch/time_fixedpoint.py [reps] [--label TEXT] > profiles/fixedpoint.txt

BLS12-381 Fr, (k, kappa) = (64, 32), count = 2^16 and 2^20, two groups of launches, each beside the same steps composed from
share_arithmetic calls (what the package exported before):

(a) truncation: trunc_mask + trunc_pr_finish with m = 32 (2 launches) | composed: Horner over the 96 planes (2 adds a plane), the
    scaling of r2, the three additions, and after the "open" sub, add, mul by 2^-m (the low bits of c are taken with torch).
(b) one ltz's launches, m = 63: ltl_leaves, every level's carry_mask and carry_combine, div2m_finish (1 + 2 * 6 + 1 launches; the
    trunc_mask in front is group (a)'s) | composed: the reference's leaf formulas (6 launches a bit, the public bit as an
    array), a level as 2 subs, beaver_combine and an add a triple, the finish as 8 launches.  What a level "opens" is what its
    mask wrote (degree-0 shares): no open is timed.

Each figure: HIP events around one group, `reps` (at least 20) runs after a warm-up, the two versions alternated run by run;
median (min .. max).  Outputs are compared bit for bit.  No GPU: fails (there is nothing to fall back to)."""
import socket
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from honeybadgermpc_amd import share_arithmetic as sa  # noqa: E402
from honeybadgermpc_amd._capi import Context  # noqa: E402
from honeybadgermpc_amd.progs import fixedpoint as fx  # noqa: E402

BLS = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
K, KAPPA = 64, 32


def rnd(ctx, gen, count, rows=None):
    n = count if rows is None else rows * count
    t = ctx.reduce_(torch.randint(-(1 << 63), (1 << 63) - 1, (n, ctx.n_limbs), dtype=torch.int64, device="cuda", generator=gen))
    return t if rows is None else t.view(rows, count, ctx.n_limbs)


def fmt(ts):
    return f"{np.median(ts):10.1f} us ({min(ts):.1f} .. {max(ts):.1f})"


def low_bits(ctx, c, m):
    out = c.clone()
    for j in range(ctx.n_limbs):
        rem = m - 64 * j
        if rem <= 0:
            out[:, j] = 0
        elif rem < 64:
            out[:, j] &= (1 << rem) - 1
    return out


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


def main():
    args = sys.argv[1:]
    if not torch.cuda.is_available():
        raise SystemExit("scratch/time_fixedpoint.py needs the GPU")
    reps = max(20, int(args[0])) if args and args[0].isdigit() else 20
    label = args[args.index("--label") + 1] if "--label" in args else "working tree"
    print(f"# scratch/time_fixedpoint.py, {reps} runs a figure: median (min .. max); {torch.cuda.get_device_name(0)} on {socket.gethostname()}; {label}")
    p = BLS
    ctx = Context.get(p)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(13)
    for logc in (16, 20):
        count = 1 << logc
        x, c, carry = rnd(ctx, gen, count), rnd(ctx, gen, count), rnd(ctx, gen, count)
        bits = rnd(ctx, gen, count, rows=K + KAPPA)
        # ---- (a)
        m = 32
        inv = pow(2, -m, p)
        c2 = low_bits(ctx, c, m)

        def fused_a():
            masked, r1 = fx.trunc_mask(ctx, x, bits, K, m, KAPPA)
            return masked, fx.trunc_pr_finish(ctx, x, c, r1, m)

        def composed_a():
            hi, lo = torch.zeros_like(x), torch.zeros_like(x)
            for i in range(K + KAPPA - 1, -1, -1):
                acc = hi if i >= m else lo
                sa.add(ctx, sa.add(ctx, acc, acc, out=acc), bits[i], out=acc)
            masked = sa.add(ctx, sa.add(ctx, sa.add(ctx, x, pow(2, K - 1, p)), lo), sa.mul(ctx, hi, pow(2, m, p)))
            return masked, sa.mul(ctx, sa.add(ctx, sa.sub(ctx, x, c2), lo), inv)

        same = all(bool(torch.equal(a, b)) for a, b in zip(fused_a(), composed_a()))
        tf, tc = alternate(reps, fused_a, composed_a)
        print(f"(a) mask + trunc_pr_finish, m = {m}   count = 2^{logc:<2d}  fused (2 launches) {fmt(tf)}   composed ({2 * (K + KAPPA) + 7} launches) {fmt(tc)}   "
              f"composed / fused = {np.median(tc) / np.median(tf):5.2f}   {'bit-equal' if same else 'MISMATCH'}", flush=True)
        # ---- (b)
        m = K - 1
        inv = pow(2, -m, p)
        r1 = rnd(ctx, gen, count)
        n_tr = fx.carry_triples(m)
        ta, tb = rnd(ctx, gen, count, rows=n_tr), rnd(ctx, gen, count, rows=n_tr)
        tab = rnd(ctx, gen, count, rows=n_tr)
        c2 = low_bits(ctx, c, m)
        abits = []
        for i in range(m):
            a = torch.zeros_like(c)
            a[:, 0] = (c[:, i // 64] >> (i % 64)) & 1
            abits.append(a)
        one, zero = ctx.upload_ints([1] * count), ctx.upload_ints([0] * count)

        def fused_b():
            g, q = fx.ltl_leaves(ctx, c, bits, m)
            nodes, off = m + 1, 0
            while True:
                root = nodes == 2
                n = 1 if root else 2 * (nodes // 2)
                masked = fx.carry_mask(ctx, g, q, ta[off:off + n], tb[off:off + n], root=root)
                res = fx.carry_combine(ctx, masked, g, q, ta[off:off + n], tb[off:off + n], tab[off:off + n], root=root)
                if root:
                    return fx.div2m_finish(ctx, x, c, r1, res, m, fx.NEG_TRUNC)
                (g, q), nodes, off = res, (nodes + 1) // 2, off + n

        def composed_b():
            g, q = [], []
            for j in range(m):
                a, nb = abits[m - 1 - j], sa.add(ctx, sa.neg(ctx, bits[m - 1 - j]), 1)
                cy = sa.mul(ctx, a, nb)
                g.append(cy)
                q.append(sa.sub(ctx, sa.add(ctx, a, nb), sa.mul(ctx, cy, 2)))
            g.append(one)
            q.append(zero)
            off = 0
            while len(g) > 1:
                root = len(g) == 2
                g2, q2 = [], []
                for j in range(len(g) // 2):
                    t = off + (j if root else 2 * j)
                    d, e = sa.sub(ctx, q[2 * j], ta[t]), sa.sub(ctx, g[2 * j + 1], tb[t])
                    g2.append(sa.add(ctx, g[2 * j], sa.beaver_combine(ctx, d, e, ta[t], tb[t], tab[t])))
                    if not root:
                        d, e = sa.sub(ctx, q[2 * j], ta[t + 1]), sa.sub(ctx, q[2 * j + 1], tb[t + 1])
                        q2.append(sa.beaver_combine(ctx, d, e, ta[t + 1], tb[t + 1], tab[t + 1]))
                if len(g) & 1:
                    g2.append(g[-1])
                    q2.append(q[-1])
                off += 1 if root else 2 * (len(g) // 2)
                g, q = g2, q2
            a2 = sa.add(ctx, sa.sub(ctx, c2, r1), sa.mul(ctx, sa.add(ctx, sa.neg(ctx, g[0]), 1), pow(2, m, p)))
            return sa.neg(ctx, sa.mul(ctx, sa.sub(ctx, x, a2), inv))

        same = bool(torch.equal(fused_b(), composed_b()))
        tf, tc = alternate(reps, fused_b, composed_b)
        levels = fx.carry_levels(m)
        print(f"(b) one ltz after its mask, m = {m}  count = 2^{logc:<2d}  fused ({2 + 2 * levels} launches) {fmt(tf)}   composed ({6 * m + 4 * m + 3 * (m - 1) + 8} launches) {fmt(tc)}   "
              f"composed / fused = {np.median(tc) / np.median(tf):5.2f}   {'bit-equal' if same else 'MISMATCH'}", flush=True)
        del bits, ta, tb, tab, abits
        torch.cuda.empty_cache()


main()

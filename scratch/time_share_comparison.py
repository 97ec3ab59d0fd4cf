"""The equality kernels timed on the device:
   python scratch/time_share_comparison.py [reps] [--label TEXT] > profiles/share_comparison.txt

BLS12-381 Fr.

(a) hb_legendre at 2^20 and 2^24 elements beside hb_sqrt_mod on the same array (the bit-by-bit chain of hb_sqrt.hip plus
    Tonelli-Shanks for the residues), alternated.  Legendre >= 0 must agree with sqrt's `ok`.  Field multiplications a second are
    reported with the chain's own count (254 squarings, the schedule's products, 4 for the table, 1 conversion), to be read beside
    MiMC's figure in profiles/mimc.txt -- the same kind of dependent chain.
(b) the three glue launches (eq_mask1, eq_mid, eq_cshare) and eq_finish at kappa = 32, count = 2^16, each group beside the same
    steps composed from share_arithmetic calls.  What a step "opens" is what the step before wrote (degree-0 shares): no open is timed.

Each figure: HIP events around one group, `reps` (at least 20) runs after a warm-up, the two versions alternated run by run;
median (min .. max).  Outputs are compared bit for bit.  No GPU: fails (there is nothing to fall back to).

With --steps instead: every entry point alone at both widths (BLS12-381 Fr and 2^64 - 59), 2^20 elements (rows = 4 at count = 2^18),
HIP events around one launch with the host kept ahead of the device.  Run it against two builds of the library (HBMPC_HIP_LIB)
in one visit to compare them."""
import socket
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from honeybadgermpc_amd import share_arithmetic as sa  # noqa: E402
from honeybadgermpc_amd import share_comparison as sc  # noqa: E402
from honeybadgermpc_amd._capi import Context  # noqa: E402

BLS = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
P64 = (1 << 64) - 59
KAPPA = 32


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


def chain_multiplications(p):
    """field multiplications of one Legendre chain: the sliding window of csrc/hb_eq.hip (window 3) walked over (p - 1) / 2"""
    e, sq, mul = (p - 1) // 2, 0, 0
    i, first = e.bit_length() - 1, True
    while i >= 0:
        if not (e >> i) & 1:
            sq, i = sq + 1, i - 1
            continue
        lo = max(i - 2, 0)
        while not (e >> lo) & 1:
            lo += 1
        if not first:
            sq, mul = sq + (i - lo + 1), mul + 1
        first, i = False, lo - 1
    return sq + mul + 4 + 1


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
    """--steps: every entry point of csrc/hb_eq.hip alone, both widths: 2^20 elements, rows = 4 at count = 2^18"""
    pad = torch.empty(1 << 29, dtype=torch.uint8, device="cuda")
    rows, count = 4, 1 << 18
    for p, name in ((BLS, "<9, 8>"), (P64, "<3, 2>")):
        ctx = Context.get(p)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(19)
        nr = sc.smallest_nonresidue(p)
        a, x, y = rnd(ctx, gen, rows * count), rnd(ctx, gen, count), rnd(ctx, gen, count)
        r, rp, bits, dr, c = (rnd(ctx, gen, count, rows) for _ in range(5))
        ta, tb, tc = (tuple(rnd(ctx, gen, count, rows) for _ in range(3)) for _ in range(3))
        o4, o2 = rnd(ctx, gen, 4 * rows * count), rnd(ctx, gen, 2 * rows * count)
        steps = (("EqLegendreRow", lambda: sc.legendre(ctx, a)),
                 ("EqMask1Row<true>", lambda: sc.eq_mask1(ctx, x, y, r, rp, ta[0], ta[1], tb[0], tb[1])),
                 ("EqMask1Row<false>", lambda: sc.eq_mask1(ctx, x, None, r, rp, ta[0], ta[1], tb[0], tb[1])),
                 ("EqMidRow", lambda: sc.eq_mid(ctx, o4, ta, tb, bits, tc[0], tc[1], nr)),
                 ("EqCshareRow", lambda: sc.eq_cshare(ctx, o2, dr, tc)),
                 ("EqFinishRow BIT", lambda: sc.eq_finish(ctx, c, bits, sc.BIT, nr)),
                 ("EqFinishRow REFERENCE", lambda: sc.eq_finish(ctx, c, bits, sc.REFERENCE, nr)))
        for step, fn in steps:
            print(f"step {step + ' ' + name:30s} {fmt(one_launch(reps, fn, pad))}", flush=True)
        del a, x, y, r, rp, bits, dr, c, ta, tb, tc, o4, o2, steps
        torch.cuda.empty_cache()


def main():
    args = sys.argv[1:]
    if not torch.cuda.is_available():
        raise SystemExit("scratch/time_share_comparison.py needs the GPU")
    reps = max(20, int(args[0])) if args and args[0].isdigit() else 20
    label = args[args.index("--label") + 1] if "--label" in args else "working tree"
    if "--steps" in args:
        print(f"# scratch/time_share_comparison.py --steps, {reps} runs a figure, HIP events around one launch: median (min .. max); {label}")
        return time_steps(reps)
    print(f"# scratch/time_share_comparison.py, {reps} runs a figure: median (min .. max); {torch.cuda.get_device_name(0)} on {socket.gethostname()}; {label}")
    p = BLS
    ctx = Context.get(p)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(17)
    nmul = chain_multiplications(p)
    # ---- (a)
    for logc in (20, 24):
        count = 1 << logc
        a = rnd(ctx, gen, count)
        root, ok = ctx.empty(count), torch.zeros(count, dtype=torch.uint8, device="cuda")
        got = []

        def fused_a():
            got[:] = [sc.legendre(ctx, a)]

        def composed_a():
            ctx.check(ctx.lib.hb_sqrt_mod(ctx.h, ctx.ptr(a), count, ctx.ptr(root), ctx.ptr(ok), ctx.stream()), "hb_sqrt_mod")

        tf, tc = alternate(reps, fused_a, composed_a)
        same = bool(torch.equal(got[0] >= 0, ok.bool()))
        print(f"(a) legendre   count = 2^{logc:<2d}  hb_legendre {fmt(tf)}   hb_sqrt_mod {fmt(tc)}   sqrt / legendre = {np.median(tc) / np.median(tf):5.2f}   "
              f"{nmul} multiplications a chain: {count * nmul / np.median(tf) / 1e3:7.1f} G mul/s   {'agrees with ok' if same else 'MISMATCH'}", flush=True)
        del a, root, ok
        torch.cuda.empty_cache()
    # ---- (b)
    rows, count, nr = KAPPA, 1 << 16, 5
    g = (nr - 1) * pow(2, -1, p) % p
    x, y = rnd(ctx, gen, count), rnd(ctx, gen, count)
    r, rp = rnd(ctx, gen, count, rows), rnd(ctx, gen, count, rows)
    bits = torch.zeros((rows, count, ctx.n_limbs), dtype=torch.int64, device="cuda")
    bits[:, :, 0] = torch.randint(0, 2, (rows, count), device="cuda", generator=gen)
    ta, tb, tc_ = (tuple(rnd(ctx, gen, count, rows) for _ in range(3)) for _ in range(3))
    flat = lambda t: t.reshape(-1, ctx.n_limbs)                                                 # noqa: E731
    nrs, g1s, gs = (ctx.upload_ints([v]).expand(rows * count, ctx.n_limbs).contiguous() for v in (nr, g + 1, g))
    ones, zeros = ctx.upload_ints([1]).expand(rows * count, ctx.n_limbs).contiguous(), torch.zeros((rows * count, ctx.n_limbs), dtype=torch.int64, device="cuda")

    def fused_b():
        masked = sc.eq_mask1(ctx, x, y, r, rp, ta[0], ta[1], tb[0], tb[1])
        masked2, dr = sc.eq_mid(ctx, masked, ta, tb, bits, tc_[0], tc_[1], nr)
        return masked, masked2, sc.eq_cshare(ctx, masked2, dr, tc_)

    def composed_b():
        diff = sa.sub(ctx, x, y).unsqueeze(0).expand(rows, count, ctx.n_limbs).contiguous()
        m = [sa.sub(ctx, flat(u), flat(v)) for u, v in ((diff, ta[0]), (r, ta[1]), (rp, tb[0]), (rp, tb[1]))]
        dr = sa.beaver_combine(ctx, m[0], m[1], *(flat(v) for v in ta))
        rp2 = sa.beaver_combine(ctx, m[2], m[3], *(flat(v) for v in tb))
        _b = sa.sub(ctx, nrs, sa.mul(ctx, flat(bits), nr - 1))
        m2 = [sa.sub(ctx, _b, flat(tc_[0])), sa.sub(ctx, rp2, flat(tc_[1]))]
        c = sa.add(ctx, dr, sa.beaver_combine(ctx, m2[0], m2[1], *(flat(v) for v in tc_)))
        return torch.cat(m), torch.cat(m2), c

    same = all(bool(torch.equal(flat(u), v)) for u, v in zip(fused_b(), composed_b()))
    tf, tc = alternate(reps, fused_b, composed_b)
    print(f"(b) mask1 + mid + cshare, kappa = {rows}  count = 2^16  fused (3 launches) {fmt(tf)}   composed (15 launches and 3 copies) {fmt(tc)}   "
          f"composed / fused = {np.median(tc) / np.median(tf):5.2f}   {'bit-equal' if same else 'MISMATCH'}", flush=True)
    c = rnd(ctx, gen, count, rows)
    for mode, name in ((sc.BIT, "BIT"), (sc.REFERENCE, "REFERENCE")):
        def fused_c():
            return sc.eq_finish(ctx, c, bits, mode, nr)[0]

        def composed_c():
            leg = sc.legendre(ctx, c).view(rows * count, 1)
            b = flat(bits)
            if mode == sc.BIT:
                pos, neg = b, sa.sub(ctx, ones, b)
            else:
                gb = sa.mul(ctx, b, g)
                pos, neg = sa.sub(ctx, g1s, gb), sa.sub(ctx, gb, gs)
            return torch.where(leg > 0, pos, torch.where(leg < 0, neg, zeros))

        same = bool(torch.equal(flat(fused_c()), composed_c()))
        tf, tc = alternate(reps, fused_c, composed_c)
        print(f"(b) finish {name:9s}, kappa = {rows}  count = 2^16  fused (1 launch) {fmt(tf)}   composed (legendre + {2 if mode == sc.BIT else 4} launches and 2 selects) {fmt(tc)}   "
              f"composed / fused = {np.median(tc) / np.median(tf):5.2f}   {'bit-equal' if same else 'MISMATCH'}   {rows * count * nmul / np.median(tf) / 1e3:7.1f} G mul/s", flush=True)


if __name__ == "__main__":
    main()

"""mul, beaver_combine and inv of honeybadgermpc_amd.share_arithmetic timed call by call (HIP events), at 2^20 and 2^24 elements over
BLS12-381's scalar field (32-byte elements) and over 2^64 - 59 (8-byte elements); the six-launch composition beside the fused Beaver
step; and the route a user had before these kernels (download_ints, the list comprehension on Python ints, upload_ints) at 2^20:
   python scratch/time_share_arith.py [reps] [--label TEXT] > profiles/ew_share_arith.txt
Every call of a timed loop works on the next of a rotation of operand sets that together exceed 1 GiB (the chip's 256 MB of cache
holds none of them by the time its turn comes again); every event object is recorded once before the timed region.

With --steps instead: every binary op and the Beaver step alone at both widths (BLS12-381 Fr and 2^64 - 59), 2^20 elements, HIP events around one launch
with the host kept ahead of the device (one_launch of scratch/time_share_comparison.py).  Run it against two builds of the library
(HBMPC_HIP_LIB) in one visit to compare them."""
import socket
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from honeybadgermpc_amd import share_arithmetic as sa  # noqa: E402
from honeybadgermpc_amd._capi import Context  # noqa: E402

BLS = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
P64 = (1 << 64) - 59
HBM_BYTES_PER_S = 8e12


def timed(calls, reps):
    """calls: one closure per operand set; -> median microseconds of a call"""
    for c in calls:
        c()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in evs:
        a.record(); b.record()
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(evs):
        a.record()
        calls[k % len(calls)]()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in evs])) * 1e3


def time_steps(reps, label):
    """--steps: every binary op (b an array, b one element for all) and the Beaver step alone, both widths, 2^20 elements"""
    from time_share_comparison import fmt as band, one_launch, rnd as draw

    print(f"# scratch/time_share_arith.py --steps, {reps} runs a figure, HIP events around one launch: median (min .. max); {label}")
    pad = torch.empty(1 << 29, dtype=torch.uint8, device="cuda")
    count = 1 << 20
    for p, width in ((BLS, "<9, 8>"), (P64, "<3, 2>")):
        ctx = Context.get(p)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(19)
        a, b, d, e, tp, tq, tpq = (draw(ctx, gen, count) for _ in range(7))
        out = ctx.empty(count)
        steps = []
        for name, fn in (("ADD", sa.add), ("SUB", sa.sub), ("MUL", sa.mul)):
            steps.append((f"EwBinaryRow {name}", lambda fn=fn: fn(ctx, a, b, out=out)))
            steps.append((f"EwBinaryRow {name} broadcast", lambda fn=fn: fn(ctx, a, 0x1234567, out=out)))
        steps.append(("EwBinaryRow NEG", lambda: sa.neg(ctx, a, out=out)))
        steps.append(("EwBeaverRow", lambda: sa.beaver_combine(ctx, d, e, tp, tq, tpq, out=out)))
        for step, fn in steps:
            print(f"step {step + ' ' + width:34s} {band(one_launch(reps, fn, pad))}", flush=True)
        del steps
        torch.cuda.empty_cache()


def main():
    args = sys.argv[1:]
    reps = int(args[0]) if args and args[0].isdigit() else 40
    label = args[args.index("--label") + 1] if "--label" in args else "working tree"
    if "--steps" in args:
        return time_steps(max(20, reps), label)
    print(f"# scratch/time_share_arith.py, {reps} calls a figure (medians); {torch.cuda.get_device_name(0)} on {socket.gethostname()}; {label}")
    print("# us = microseconds a call between HIP events; rotation = operand sets cycled through (together > 1 GiB)")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2024)
    for name, p, nl in (("BLS12-381 Fr", BLS, 4), ("2^64 - 59", P64, 1)):
        ctx = Context.get(p, 0, nl)
        eb = 8 * nl
        for lg in (20, 24):
            count = 1 << lg
            set_bytes = 6 * eb * count
            nsets = max(2, -(-(1 << 30) // set_bytes))

            def rnd():
                return ctx.reduce_(torch.randint(-(1 << 63), (1 << 63) - 1, (count, nl), dtype=torch.int64, device="cuda", generator=gen))

            sets = [[rnd() for _ in range(5)] + [ctx.empty(count)] for _ in range(nsets)]
            t_mul = timed([lambda s=s: sa.mul(ctx, s[0], s[1], out=s[5]) for s in sets], reps)
            t_bv = timed([lambda s=s: sa.beaver_combine(ctx, s[0], s[1], s[2], s[3], s[4], out=s[5]) for s in sets], reps)
            tmp = [ctx.empty(count), ctx.empty(count)]

            def six(s):
                sa.mul(ctx, s[0], s[1], out=tmp[0])
                sa.mul(ctx, s[0], s[3], out=tmp[1])
                sa.add(ctx, tmp[0], tmp[1], out=tmp[0])
                sa.mul(ctx, s[1], s[2], out=tmp[1])
                sa.add(ctx, tmp[0], tmp[1], out=tmp[0])
                sa.add(ctx, tmp[0], s[4], out=s[5])

            t_six = timed([lambda s=s: six(s) for s in sets], reps)
            t_inv = timed([lambda s=s: sa.inv(ctx, s[0], check=False, out=s[5]) for s in sets], max(reps // 4, 8))
            fused = sa.beaver_combine(ctx, *sets[0][:5])
            six(sets[0])
            same = bool(torch.equal(fused, sets[0][5]))
            moved = 6 * eb * count
            print(f"{name:13s} 2^{lg} rotation {nsets:3d}   mul {t_mul:9.1f} us {count / t_mul / 1e3:7.2f} G el/s   "
                  f"beaver_combine {t_bv:9.1f} us {count / t_bv / 1e3:7.2f} G el/s  {moved / (t_bv * 1e-6) / 1e12:5.2f} TB/s = {moved / (t_bv * 1e-6) / HBM_BYTES_PER_S:5.1%} of 8 TB/s   "
                  f"six launches {t_six:9.1f} us ({t_six / t_bv:4.2f}x fused, {'bit-equal' if same else 'MISMATCH'})   "
                  f"inv {t_inv:9.1f} us {count / t_inv / 1e3:7.3f} G el/s", flush=True)
            if p == BLS and lg == 20:
                # what the package offered before: every operand through Python ints and back
                s = sets[0]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                d, e, pp, q, pq = (ctx.download_ints(v) for v in s[:5])
                xy = [(dd * ee + dd * qq + ee * ppp + pqq) % p for (ppp, qq, pqq, dd, ee) in zip(pp, q, pq, d, e)]
                back = ctx.upload_ints(xy)
                torch.cuda.synchronize()
                host_s = time.perf_counter() - t0
                ok = bool(torch.equal(back, fused))
                print(f"{name:13s} 2^{lg} through Python ints (download_ints x 5, list comprehension, upload_ints): {host_s:7.3f} s = {count / host_s / 1e6:5.2f} M el/s; "
                      f"beaver_combine is {host_s / (t_bv * 1e-6):9.0f}x faster ({'same values' if ok else 'MISMATCH'})", flush=True)
                del d, e, pp, q, pq, xy, back
            del sets, tmp, fused
            torch.cuda.empty_cache()


main()

"""Host-side cost of one call of hb_lt_mid and hb_fxp_carry_combine at count = 256, BLS12-381 scalar field:
   HBMPC_HIP_LIB=<a build> python scratch/time_rows_host_side.py

A call returns after the enqueue.  The clock (perf_counter_ns) ticks in about 10 ns here, a few tenths of a per cent of a call, so a
call is not timed alone: a GROUP of 50 calls is, the device is synchronised outside the timed region after every group, and a group's
figure is its time / 50.  Median (p10 .. p90) of GROUPS groups after WARM, i.e. 5000 timed calls a step, and the clock's tick as
measured.  Run it against two builds (HBMPC_HIP_LIB), alternated, several times each: the parent's run-to-run band is the yardstick.
Prints one JSON line.  No GPU: fails."""
import json
import os
import sys
import time

sys.path.insert(0, ".")
from honeybadgermpc_amd._capi import Context  # noqa: E402

BLS = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
COUNT, GROUP, GROUPS, WARM = 256, 50, 100, 10


def carve(ctx, rows_list):
    eb = 8 * ctx.n_limbs
    buf = ctx.torch.zeros(sum(r * COUNT * eb for r in rows_list), dtype=ctx.torch.uint8, device=ctx.tdev)
    ptrs, at = [], buf.data_ptr()
    for r in rows_list:
        ptrs.append(at)
        at += r * COUNT * eb
    return buf, ptrs


def timed(ctx, call):
    ts = []
    for g in range(WARM + GROUPS):
        t0 = time.perf_counter_ns()
        for _ in range(GROUP):
            rc = call()
        t1 = time.perf_counter_ns()
        assert rc == 0, (rc, ctx.lib.hb_last_error(ctx.h))
        ctx.torch.cuda.synchronize()
        if g >= WARM:
            ts.append((t1 - t0) / GROUP)
    ts.sort()
    return {"median_us": round(ts[len(ts) // 2] / 1e3, 4), "p10_us": round(ts[len(ts) // 10] / 1e3, 4), "p90_us": round(ts[9 * len(ts) // 10] / 1e3, 4)}


def tick_ns():
    seen = set()
    for _ in range(20000):
        a = time.perf_counter_ns()
        b = time.perf_counter_ns()
        if b > a:
            seen.add(b - a)
    return min(seen)


def main():
    ctx = Context.get(BLS)
    lib, h, L = ctx.lib, ctx.h, BLS.bit_length()
    # hb_lt_mid: opened (5), u, s_bits (L), pa qa pqa pb qb pqb pc qc, v, d0, masked (2)
    keep1, p = carve(ctx, [5, 1, L] + [1] * 8 + [1, 1, 2])
    lt_mid = lambda: lib.hb_lt_mid(h, p[0], p[1], p[2], L, *p[3:11], p[11], p[12], p[13], COUNT, None)  # noqa: E731
    # hb_fxp_carry_combine at nodes = 257: opened (512), g p (257), ta tb tab (256), g_out p_out (129)
    keep2, q = carve(ctx, [512, 257, 257, 256, 256, 256, 129, 129])
    combine = lambda: lib.hb_fxp_carry_combine(h, q[0], q[1], q[2], 257, 0, q[3], q[4], q[5], q[6], q[7], COUNT, None)  # noqa: E731
    print(json.dumps({"lib": os.environ.get("HBMPC_HIP_LIB", "tree"), "tick_ns": tick_ns(), "hb_lt_mid": timed(ctx, lt_mid),
                      "hb_fxp_carry_combine": timed(ctx, combine)}))


main()

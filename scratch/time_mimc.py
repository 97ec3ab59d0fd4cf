"""The MiMC kernels timed on the device:
   python scratch/time_mimc.py [reps] [--label TEXT] [--round-only | --protocol-only | --plain-only | --kernels] > profiles/mimc.txt

(a) Round: cube_round of honeybadgermpc_amd.progs.mimc (one launch) beside the same round composed from what the package
exported before, in its cheapest grouping -- Horner, y (y (y + 3 r) + 3 r2) + r3 + (key + c + 1) - r_next: mul 3, add, mul, mul 3,
add, mul, add, add const, sub: 9 launches of hb_ew_op, the constants one-element broadcast operands that are already on the
device.  BLS12-381 Fr and 2^64 - 59, count = 2^10, 2^16, 2^20.  Each figure: HIP events around one round, `reps` rounds after a
warm-up, the two versions ALTERNATED call by call in one run, operand sets rotated (as many sets as pass 512 MiB, at most 8: at
2^20 no set is in the 256 MiB last-level cache when it is read again; at 2^10 all of them are, and the figure is launch time);
median (min .. max).  "need" = the 6 elements a block the algorithm reads and writes, over the median, as a share of 8 TB/s.
Outputs are compared bit for bit at every timed size.

(b) Protocol: n = 4, t = 1, every party in this process over an in-process transport, count = 2^10 and 2^16, 161 rounds: wall
time of a whole mimc_mpc_batch (host clock, ending in a synchronise), fused and composed.  Opens, Python and the event loop
included: it is NOT kernel time.

(c) Cleartext: mimc_keystream (counters, a key for all) and mimc_plain_device (array, a key per element) at 2^16 and 2^20 blocks,
both widths, one and two elements a thread, alternated; also as field multiplications a second, counting the 2 a round of the
chain (2 * rounds an element; the three conversions are not counted).

--kernels runs three rounds of each version at 2^20 over BLS12-381 and two cleartext launches, and nothing else (for a kernel trace).
No GPU: fails (there is nothing to fall back to).

With --steps instead: the first mask and the cubing round alone at both widths (BLS12-381 Fr and 2^64 - 59), 2^20 elements, HIP events around one launch
with the host kept ahead of the device (one_launch of scratch/time_share_comparison.py).  Run it against two builds of the library
(HBMPC_HIP_LIB) in one visit to compare them."""
import asyncio
import socket
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from honeybadgermpc_amd import share_arithmetic as sa  # noqa: E402
from honeybadgermpc_amd._capi import HB_EW_ADD, HB_EW_MUL, Context  # noqa: E402
from honeybadgermpc_amd.open_coalescer import OpenCoalescer  # noqa: E402
from honeybadgermpc_amd.progs import mimc  # noqa: E402

BLS = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
P64 = (1 << 64) - 59
PEAK = 8e12
# profiles/r01_mad_issue_rate_vs_occupancy.txt: 34.0e12 v_mad_u64_u32 lane-operations a second at 8 waves a SIMD.  A 9-digit Montgomery
# product is 81 of them for the product and 81 for REDC (its 9 quotient digits are 32-bit multiplies, not counted); 3 digits: 9 + 9.
MAD_RATE = 34.0e12
MADS = {4: 162, 1: 18}


def rnd(ctx, gen, count):
    return ctx.reduce_(torch.randint(-(1 << 63), (1 << 63) - 1, (count, ctx.n_limbs), dtype=torch.int64, device="cuda", generator=gen))


def fmt(ts):
    return f"{np.median(ts):9.1f} us ({min(ts):.1f} .. {max(ts):.1f})"


class Composed:
    """the round from calls the package exported before this module; its constants are uploaded once"""

    def __init__(self, ctx, key):
        self.ctx, self.key = ctx, key
        self.three = ctx.upload_ints([3])
        self.consts = {}

    def const(self, v):
        c = self.consts.get(v)
        if c is None:
            c = self.consts[v] = self.ctx.upload_ints([v % self.ctx.modulus])
        return c

    def bc(self, op, a, c, out):
        ctx = self.ctx
        ctx.check(ctx.lib.hb_ew_op(ctx.h, op, ctx.ptr(a), ctx.ptr(c), 1, ctx.ptr(out), a.shape[0], ctx.stream()), "hb_ew_op")
        return out

    def first(self, x, r0):
        ctx = self.ctx
        t = self.bc(HB_EW_ADD, x, self.const(self.key), ctx.empty(x.shape[0]))
        return sa.sub(ctx, t, r0, out=t)

    def round(self, y, r, r2, r3, ctr, r_next):
        ctx = self.ctx
        s = self.bc(HB_EW_MUL, r, self.three, ctx.empty(y.shape[0]))
        sa.add(ctx, s, y, out=s)
        sa.mul(ctx, y, s, out=s)
        w = self.bc(HB_EW_MUL, r2, self.three, ctx.empty(y.shape[0]))
        sa.add(ctx, w, s, out=w)
        sa.mul(ctx, y, w, out=w)
        sa.add(ctx, w, r3, out=w)
        if r_next is None:
            return self.bc(HB_EW_ADD, w, self.const(self.key), w)
        self.bc(HB_EW_ADD, w, self.const(self.key + ctr + 1), w)
        return sa.sub(ctx, w, r_next, out=w)


def time_round(reps):
    print("# (a) one round: fused = cube_round (1 launch); composed = 9 launches of hb_ew_op; need = 6 elements a block / median, of 8 TB/s")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    ctr = 80
    for name, p in (("BLS12-381 Fr", BLS), ("2^64 - 59", P64)):
        ctx = Context.get(p)
        key = 0x1234567 % p
        key_dev = ctx.upload_ints([key])
        comp = Composed(ctx, key)
        comp.const(key + ctr + 1)
        for n in (10, 16, 20):
            count = 1 << n
            set_bytes = 6 * count * ctx.nbytes
            n_sets = min(8, max(2, -(-(512 << 20) // set_bytes)))
            sets = [{w: rnd(ctx, gen, count) for w in ("y", "r", "r2", "r3", "rn", "out")} for _ in range(n_sets)]

            def fused(s):
                return mimc.cube_round(ctx, s["y"], s["r"], s["r2"], s["r3"], key_dev, ctr, r_next=s["rn"], out=s["out"])

            def composed(s):
                return comp.round(s["y"], s["r"], s["r2"], s["r3"], ctr, s["rn"])

            s0 = sets[0]
            same = bool(torch.equal(fused(s0), composed(s0)))
            same = same and bool(torch.equal(mimc.cube_round(ctx, s0["y"], s0["r"], s0["r2"], s0["r3"], key_dev, ctr), comp.round(s0["y"], s0["r"], s0["r2"], s0["r3"], ctr, None)))
            for s in sets:
                fused(s); composed(s)
            torch.cuda.synchronize()
            evs = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(reps)]
            for e3 in evs:
                for ev in e3:
                    ev.record()
            torch.cuda.synchronize()
            for i, e3 in enumerate(evs):
                s = sets[i % n_sets]
                e3[0].record()
                fused(s)
                e3[1].record()
                composed(s)
                e3[2].record()
            torch.cuda.synchronize()
            tf = [e3[0].elapsed_time(e3[1]) * 1e3 for e3 in evs]
            tc = [e3[1].elapsed_time(e3[2]) * 1e3 for e3 in evs]
            need = 6 * count * ctx.nbytes
            print(f"{name:13s} count = 2^{n:<2d} sets {n_sets}   fused {fmt(tf)}  need {need / (np.median(tf) * 1e-6) / PEAK * 100:5.1f}% of 8 TB/s   "
                  f"composed {fmt(tc)}   composed / fused = {np.median(tc) / np.median(tf):5.2f}   {'bit-equal' if same else 'MISMATCH'}", flush=True)
            del sets
            torch.cuda.empty_cache()


# ---- the whole protocol ---------------------------------------------------------------------------------------------
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


async def composed_batch(co, xs, key, cubes, rounds):
    comp = Composed(co.ctx, key)
    r, r2, r3 = cubes
    cur = comp.first(xs, r[0])
    for c in range(rounds):
        y = await co.open_share_array(cur)
        cur = comp.round(y, r[c], r2[c], r3[c], c, r[c + 1] if c + 1 < rounds else None)
    return cur


def time_protocol(reps):
    print("# (b) whole mimc_mpc_batch, 161 rounds, n = 4, t = 1, four parties in one process over an in-process transport: wall time (host clock ending in a "
          "synchronise); opens, Python and the event loop included -- not kernel time")
    p, n, t, rounds = BLS, 4, 1, mimc.ROUND
    ctx = Context.get(p)
    L = ctx.n_limbs
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9)
    key = 0x1234567
    for logc in (10, 16):
        count = 1 << logc

        def deal(secret):
            """degree-1 sharings made on the device: share of party i = s + r (i + 1)"""
            r = rnd(ctx, gen, secret.shape[0])
            return [sa.add(ctx, secret, sa.mul(ctx, r, i + 1)) for i in range(n)]

        rs = rnd(ctx, gen, rounds * count)
        rs2 = sa.mul(ctx, rs, rs)
        dealt = {"x": deal(rnd(ctx, gen, count)), "r": deal(rs), "r2": deal(rs2), "r3": deal(sa.mul(ctx, rs2, rs))}
        del rs, rs2

        async def run(mode):
            net = Net(n)

            async def party(i):
                co = OpenCoalescer(p, n, t, i, net.get_send_recv(i))
                cubes = tuple(dealt[w][i].reshape(rounds, count, L) for w in ("r", "r2", "r3"))
                if mode == "composed":
                    shares = await composed_batch(co, dealt["x"][i], key, cubes, rounds)
                else:
                    shares = await mimc.mimc_mpc_batch(co, dealt["x"][i], key, cubes)
                return shares, await co.open_share_array(shares)

            return await asyncio.gather(*[party(i) for i in range(n)])

        modes = ("composed", "fused")
        times = {m: [] for m in modes}
        outs = {}
        nrep = reps if logc <= 10 else 2
        for rep in range(nrep + 1):                                      # the first pass warms up and is not counted
            for m in modes:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = asyncio.run(run(m))
                torch.cuda.synchronize()
                if rep:
                    times[m].append(time.perf_counter() - t0)
                outs[m] = res[0]
        same = bool(torch.equal(outs["fused"][0], outs["composed"][0])) and bool(torch.equal(outs["fused"][1], outs["composed"][1]))
        line = "   ".join(f"{m} {np.median(times[m]):8.3f} s ({min(times[m]):.3f} .. {max(times[m]):.3f})" for m in modes)
        print(f"count = 2^{logc:<2d} {rounds} rounds, {nrep} timed run(s) a mode, alternated:   {line}   per round: " +
              " / ".join(f"{np.median(times[m]) / rounds * 1e3:.2f}" for m in modes) + f" ms   composed / fused = "
              f"{np.median(times['composed']) / np.median(times['fused']):.2f}   ({'bit-equal' if same else 'MISMATCH'})", flush=True)
        del dealt, outs
        torch.cuda.empty_cache()


def time_plain(reps):
    print("# (c) the cleartext cipher, full rounds: keystream = counters and a key for all, array = x and a key per element from memory; one | pair = elements a "
          "thread; G mul/s = 2 * rounds * count / median; estimate = what 34.0e12 v_mad_u64_u32 a second (profiles/r01_mad_issue_rate_vs_occupancy.txt) allow at "
          "162 (9 digits) or 18 (3 digits) of them a product -- an estimate of the bound, not a target")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    for name, p in (("BLS12-381 Fr", BLS), ("2^64 - 59", P64)):
        ctx = Context.get(p)
        rounds = mimc.rounds_for(p)
        key = 0x1234567 % p
        key_dev = ctx.upload_ints([key])
        for n in (16, 20):
            count = 1 << n
            xs, ks, out = rnd(ctx, gen, count), rnd(ctx, gen, count), ctx.empty(count)
            start = ctx.host_elems([5])

            def keystream(pair):
                ctx.check(ctx.lib.hb_mimc_plain(ctx.h, None, start.ctypes.data, ctx.ptr(key_dev), 1, None, 2 if pair else 0, rounds, ctx.ptr(out), count, ctx.stream()), "hb_mimc_plain")
                return out

            def array(pair):
                return mimc.mimc_plain_device(ctx, xs, ks, out=out, pair=pair)

            for what, fn in (("keystream", keystream), ("array    ", array)):
                same = bool(torch.equal(fn(False).clone(), fn(True)))
                torch.cuda.synchronize()
                evs = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(reps)]
                for e3 in evs:
                    for ev in e3:
                        ev.record()
                torch.cuda.synchronize()
                for e3 in evs:
                    e3[0].record()
                    fn(False)
                    e3[1].record()
                    fn(True)
                    e3[2].record()
                torch.cuda.synchronize()
                t1 = [e3[0].elapsed_time(e3[1]) * 1e3 for e3 in evs]
                t2 = [e3[1].elapsed_time(e3[2]) * 1e3 for e3 in evs]
                muls = 2 * rounds * count
                bound = MAD_RATE / MADS[ctx.n_limbs]
                print(f"{name:13s} {what} count = 2^{n:<2d} {rounds} rounds   one {fmt(t1)} {muls / (np.median(t1) * 1e-6) / 1e9:8.1f} G mul/s ({muls / (np.median(t1) * 1e-6) / bound * 100:4.1f}% of the "
                      f"estimate {bound / 1e9:.0f} G)   pair {fmt(t2)} {muls / (np.median(t2) * 1e-6) / 1e9:8.1f} G mul/s   pair / one = {np.median(t2) / np.median(t1):5.2f}   "
                      f"{'bit-equal' if same else 'MISMATCH'}", flush=True)
            del xs, ks, out
            torch.cuda.empty_cache()


def time_steps(reps, label):
    """--steps: the first mask and the cubing round alone (last and not, a key for all and a key an element), both widths, 2^20 elements"""
    from time_share_comparison import fmt as band, one_launch, rnd as draw

    print(f"# scratch/time_mimc.py --steps, {reps} runs a figure, HIP events around one launch: median (min .. max); {label}")
    pad = torch.empty(1 << 29, dtype=torch.uint8, device="cuda")
    count = 1 << 20
    for p, width in ((BLS, "<9, 8>"), (P64, "<3, 2>")):
        ctx = Context.get(p)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(19)
        x, r0, y, r, r2, r3, rn, keys = (draw(ctx, gen, count) for _ in range(8))
        key, out = ctx.upload_ints([0x1234567]), ctx.empty(count)
        steps = []
        for k, kname in ((key, "key for all"), (keys, "key an element")):
            steps.append((f"MimcFirstRow {kname}", lambda k=k: mimc.first_mask(ctx, x, k, r0, out=out)))
            steps.append((f"MimcFirstRow counters, {kname}", lambda k=k: mimc.first_mask(ctx, None, k, r0, start=5, out=out)))
            steps.append((f"MimcRoundRow {kname}", lambda k=k: mimc.cube_round(ctx, y, r, r2, r3, k, 80, r_next=rn, out=out)))
            steps.append((f"MimcRoundRow last, {kname}", lambda k=k: mimc.cube_round(ctx, y, r, r2, r3, k, 160, out=out)))
        for step, fn in steps:
            print(f"step {step + ' ' + width:46s} {band(one_launch(reps, fn, pad))}", flush=True)
        del steps
        torch.cuda.empty_cache()


def main():
    args = sys.argv[1:]
    if not torch.cuda.is_available():
        raise SystemExit("scratch/time_mimc.py needs the GPU")
    reps = int(args[0]) if args and args[0].isdigit() else 20
    label = args[args.index("--label") + 1] if "--label" in args else "working tree"
    if "--steps" in args:
        return time_steps(max(20, reps), label)
    if "--kernels" in args:
        ctx = Context.get(BLS)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(7)
        count, ctr = 1 << 20, 80
        y, r, r2, r3, rn = (rnd(ctx, gen, count) for _ in range(5))
        key_dev = ctx.upload_ints([0x1234567])
        comp = Composed(ctx, 0x1234567)
        for _ in range(3):
            mimc.cube_round(ctx, y, r, r2, r3, key_dev, ctr, r_next=rn)
            comp.round(y, r, r2, r3, ctr, rn)
        for pair in (False, True):
            mimc.mimc_keystream(ctx, key_dev, count, pair=pair)
        torch.cuda.synchronize()
        return
    print(f"# scratch/time_mimc.py, {reps} calls a figure: median (min .. max); {torch.cuda.get_device_name(0)} on {socket.gethostname()}; {label}")
    only = [a for a in args if a.endswith("-only")]
    if not only or "--round-only" in only:
        time_round(reps)
    if not only or "--plain-only" in only:
        time_plain(reps)
    if not only or "--protocol-only" in only:
        time_protocol(3)


main()

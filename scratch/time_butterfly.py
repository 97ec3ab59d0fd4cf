"""One layer of the butterfly network, and the whole network, timed on the device:
   python scratch/time_butterfly.py [reps] [--label TEXT] [--layers-only | --network-only | --kernels] > profiles/butterfly_network.txt

Layer: mask_layer + switch_layer of honeybadgermpc_amd.butterfly_network (two launches) beside the same layer composed from what
the package exported before -- two torch.index_select, three sub, beaver_combine, add, add, sub, two products by 1/2 (hb_ew_op with
a one-element broadcast operand that is already on the device) and torch.stack: 13 launches.  BLS12-381 Fr and 2^64 - 59,
k = 2^10, 2^16, 2^20, strides 1, 2^5, k / 2.  Each figure: HIP events around one layer, `reps` layers after a warm-up, the two
versions ALTERNATED call by call in one run, operand sets rotated (as many sets as pass 512 MiB, at most 8: at k = 2^20 no set is
in the 256 MiB last-level cache when it is read again; at k = 2^10 all of them are, and the figure is launch time); median
(min .. max).  "need" = the 16 elements a switch the algorithm reads and writes, over the median, as a share of 8 TB/s.  Outputs
are compared bit for bit at every timed size.

Network: n = 4, t = 1, every party in this process over an in-process transport, k = 2^10 and 2^16: wall time of a whole shuffle
(host clock, ending in a synchronise) for the composition, the fused "per_layer" mode and "upfront".  Opens, Python and the event
loop included: it is NOT kernel time.

--kernels runs three layers of each version at k = 2^20 over BLS12-381 and nothing else (for a kernel trace).
No GPU: fails (there is nothing to fall back to).

With --steps instead: the mask and the switch of a layer alone at both widths (BLS12-381 Fr and 2^64 - 59), k = 2^21 (2^20 switches), HIP events around one launch
with the host kept ahead of the device (one_launch of scratch/time_share_comparison.py).  Run it against two builds of the library
(HBMPC_HIP_LIB) in one visit to compare them."""
import asyncio
import socket
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from honeybadgermpc_amd import butterfly_network as bn  # noqa: E402
from honeybadgermpc_amd import share_arithmetic as sa  # noqa: E402
from honeybadgermpc_amd._capi import HB_EW_MUL, Context  # noqa: E402
from honeybadgermpc_amd.open_coalescer import OpenCoalescer  # noqa: E402

BLS = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
P64 = (1 << 64) - 59
PEAK = 8e12


def rnd(ctx, gen, count):
    return ctx.reduce_(torch.randint(-(1 << 63), (1 << 63) - 1, (count, ctx.n_limbs), dtype=torch.int64, device="cuda", generator=gen))


class Composed:
    """the layer from calls the package exported before this module"""

    def __init__(self, ctx, k, a):
        self.ctx, self.k = ctx, k
        j = torch.arange(k // 2, device="cuda")
        self.xi = ((j >> a) << (a + 1)) | (j & ((1 << a) - 1))
        self.yi = self.xi | (1 << a)
        self.inv2 = ctx.upload_ints([pow(2, -1, ctx.modulus)])

    def halve(self, v):
        ctx = self.ctx
        ctx.check(ctx.lib.hb_ew_op(ctx.h, HB_EW_MUL, ctx.ptr(v), ctx.ptr(self.inv2), 1, ctx.ptr(v), v.shape[0], ctx.stream()), "hb_ew_op")
        return v

    def mask(self, x, bits, p, q):
        ctx = self.ctx
        self.xs, self.ys = x.index_select(0, self.xi), x.index_select(0, self.yi)
        return sa.sub(ctx, bits, p), sa.sub(ctx, sa.sub(ctx, self.xs, self.ys), q)

    def switch(self, d, e, p, q, pq):
        ctx = self.ctx
        m = sa.beaver_combine(ctx, d, e, p, q, pq)
        s = sa.add(ctx, self.xs, self.ys)
        return torch.stack([self.halve(sa.add(ctx, s, m)), self.halve(sa.sub(ctx, s, m))], dim=1).reshape(self.k, ctx.n_limbs)


def fmt(ts):
    return f"{np.median(ts):9.1f} us ({min(ts):.1f} .. {max(ts):.1f})"


def time_layers(reps):
    print("# one layer: fused = mask_layer + switch_layer (2 launches); composed = 13 launches of calls exported before; need = 16 elements a switch / median, of 8 TB/s")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    for name, p in (("BLS12-381 Fr", BLS), ("2^64 - 59", P64)):
        ctx = Context.get(p)
        for n in (10, 16, 20):
            k = 1 << n
            half = k // 2
            set_bytes = (k * 3 + half * 6) * ctx.nbytes
            n_sets = min(8, max(2, -(-(512 << 20) // set_bytes)))
            sets = []
            for _ in range(n_sets):
                s = {"x": rnd(ctx, gen, k), "masked": ctx.empty(k), "out": ctx.empty(k)}
                for w in ("bits", "p", "q", "pq", "d", "e"):
                    s[w] = rnd(ctx, gen, half)
                sets.append(s)
            for a in (0, 5, n - 1):
                comp = Composed(ctx, k, a)

                def fused(s):
                    bn.mask_layer(ctx, s["x"], s["bits"], s["p"], s["q"], a, out=s["masked"])
                    return bn.switch_layer(ctx, s["x"], s["d"], s["e"], s["p"], s["q"], s["pq"], a, out=s["out"])

                def composed(s):
                    comp.mask(s["x"], s["bits"], s["p"], s["q"])
                    return comp.switch(s["d"], s["e"], s["p"], s["q"], s["pq"])

                # bit-equality at this size: the mask halves, and the switch outputs
                s0 = sets[0]
                mb, me = comp.mask(s0["x"], s0["bits"], s0["p"], s0["q"])
                same = bool(torch.equal(fused(s0), composed(s0))) and bool(torch.equal(s0["masked"][:half], mb)) and bool(torch.equal(s0["masked"][half:], me))
                for s in sets:
                    fused(s); composed(s)
                torch.cuda.synchronize()
                evs = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(reps)]
                for e3 in evs:
                    for ev in e3:
                        ev.record()
                torch.cuda.synchronize()
                for r, e3 in enumerate(evs):
                    s = sets[r % n_sets]
                    e3[0].record()
                    fused(s)
                    e3[1].record()
                    composed(s)
                    e3[2].record()
                torch.cuda.synchronize()
                tf = [e3[0].elapsed_time(e3[1]) * 1e3 for e3 in evs]
                tc = [e3[1].elapsed_time(e3[2]) * 1e3 for e3 in evs]
                need = 16 * half * ctx.nbytes
                print(f"{name:13s} k = 2^{n:<2d} stride 2^{a:<2d} sets {n_sets}   fused {fmt(tf)}  need {need / (np.median(tf) * 1e-6) / PEAK * 100:5.1f}% of 8 TB/s   "
                      f"composed {fmt(tc)}   composed / fused = {np.median(tc) / np.median(tf):5.2f}   {'bit-equal' if same else 'MISMATCH'}", flush=True)
                del comp
            del sets
            torch.cuda.empty_cache()


# ---- the whole network ----------------------------------------------------------------------------------------------
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


async def composed_network(co, inputs, bits, triples):
    ctx = co.ctx
    k = inputs.shape[0]
    p, q, pq = triples
    cur = inputs
    comps = {}
    for l, a in enumerate(bn.layers(k)):
        comp = comps.setdefault(a, Composed(ctx, k, a))
        mb, me = comp.mask(cur, bits[l], p[l], q[l])
        f, g = co.open_share_array(mb), co.open_share_array(me)
        d = await f
        e = await g
        cur = comp.switch(d, e, p[l], q[l], pq[l])
    return cur


def time_network(reps):
    print("# whole network, n = 4, t = 1, four parties in one process over an in-process transport: wall time of a shuffle (host clock ending in a synchronise); "
          "opens, Python and the event loop included -- not kernel time")
    p, n, t = BLS, 4, 1
    ctx = Context.get(p)
    L = ctx.n_limbs
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9)
    for logk in (10, 16):
        k = 1 << logk
        half, n_layers = k // 2, logk * logk
        rows = n_layers * half

        def deal(secret):
            """degree-1 sharings made on the device: share of party i = s + r (i + 1)"""
            r = rnd(ctx, gen, secret.shape[0])
            return [sa.add(ctx, secret, sa.mul(ctx, r, i + 1)) for i in range(n)]

        plus_minus = ctx.upload_ints([1, p - 1])
        signs = plus_minus.index_select(0, torch.randint(0, 2, (rows,), device="cuda", generator=gen))
        tp, tq = rnd(ctx, gen, rows), rnd(ctx, gen, rows)
        msgs = rnd(ctx, gen, k)
        dealt = {w: deal(v) for w, v in (("in", msgs), ("bits", signs), ("p", tp), ("q", tq), ("pq", sa.mul(ctx, tp, tq)))}
        del signs, tp, tq

        def shaped(w, i):
            return dealt[w][i].reshape(n_layers, half, L)

        async def run(mode):
            net = Net(n)

            async def party(i):
                co = OpenCoalescer(p, n, t, i, net.get_send_recv(i))
                tr = (shaped("p", i), shaped("q", i), shaped("pq", i))
                if mode == "composed":
                    shares = await composed_network(co, dealt["in"][i], shaped("bits", i), tr)
                else:
                    shares = await bn.iterated_butterfly_network(co, dealt["in"][i], shaped("bits", i), tr, open_bits=mode)
                return shares, await co.open_share_array(shares)

            return await asyncio.gather(*[party(i) for i in range(n)])

        modes = ("composed", "per_layer", "upfront")
        times = {m: [] for m in modes}
        outs = {}
        nrep = reps if logk <= 10 else 1
        for rep in range(nrep + 1):                                      # the first pass warms up and is not counted
            for m in modes:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = asyncio.run(run(m))
                torch.cuda.synchronize()
                if rep:
                    times[m].append(time.perf_counter() - t0)
                outs[m] = res[0]
        same = all(torch.equal(outs[m][0], outs["composed"][0]) and torch.equal(outs[m][1], outs["composed"][1]) for m in modes)
        perm_ok = bool(torch.equal(torch.sort(outs["per_layer"][1].reshape(k, L)[:, 0]).values, torch.sort(msgs[:, 0]).values))
        line = "   ".join(f"{m} {np.median(times[m]):8.3f} s ({min(times[m]):.3f} .. {max(times[m]):.3f})" for m in modes)
        print(f"k = 2^{logk:<2d} {n_layers:3d} layers, {nrep} timed run(s) a mode, alternated:   {line}   per layer: " +
              " / ".join(f"{np.median(times[m]) / n_layers * 1e3:.2f}" for m in modes) + f" ms   "
              f"({'all three bit-equal' if same else 'MISMATCH'}; {'opened output is a permutation of the messages' if perm_ok else 'NOT A PERMUTATION'})", flush=True)
        del dealt, outs
        torch.cuda.empty_cache()


def time_steps(reps, label):
    """--steps: the mask (with and without the signs) and the switch of one layer alone, both widths, k = 2^21 (2^20 switches), strides
    1 (in the 8-byte width: the instantiation that takes a switch's two inputs in one access), 2^5 and k / 2"""
    from time_share_comparison import fmt as band, one_launch, rnd as draw

    print(f"# scratch/time_butterfly.py --steps, {reps} runs a figure, HIP events around one launch: median (min .. max); {label}")
    pad = torch.empty(1 << 29, dtype=torch.uint8, device="cuda")
    k = 1 << 21
    for p, width in ((BLS, "<9, 8>"), (P64, "<3, 2>")):
        ctx = Context.get(p)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(19)
        x, (bits, tp, tq, tpq, d, e) = draw(ctx, gen, k), [draw(ctx, gen, k // 2) for _ in range(6)]
        out = ctx.empty(k)
        steps = []
        for a in (0, 5, 20):
            steps.append((f"BfMaskRow<true> stride 2^{a}", lambda a=a: bn.mask_layer(ctx, x, bits, tp, tq, a, out=out)))
            steps.append((f"BfMaskRow<false> stride 2^{a}", lambda a=a: bn.mask_layer(ctx, x, None, None, tq, a, out=out[:k // 2])))
            steps.append((f"BfSwitchRow stride 2^{a}", lambda a=a: bn.switch_layer(ctx, x, d, e, tp, tq, tpq, a, out=out)))
        for step, fn in steps:
            print(f"step {step + ' ' + width:34s} {band(one_launch(reps, fn, pad))}", flush=True)
        del steps
        torch.cuda.empty_cache()


def main():
    args = sys.argv[1:]
    if not torch.cuda.is_available():
        raise SystemExit("scratch/time_butterfly.py needs the GPU")
    reps = int(args[0]) if args and args[0].isdigit() else 20
    label = args[args.index("--label") + 1] if "--label" in args else "working tree"
    if "--steps" in args:
        return time_steps(max(20, reps), label)
    if "--kernels" in args:
        ctx = Context.get(BLS)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(7)
        k, a = 1 << 20, 5
        x, (bits, p, q, pq, d, e) = rnd(ctx, gen, k), [rnd(ctx, gen, k // 2) for _ in range(6)]
        comp = Composed(ctx, k, a)
        for _ in range(3):
            bn.mask_layer(ctx, x, bits, p, q, a)
            bn.switch_layer(ctx, x, d, e, p, q, pq, a)
            comp.mask(x, bits, p, q)
            comp.switch(d, e, p, q, pq)
        torch.cuda.synchronize()
        return
    print(f"# scratch/time_butterfly.py, {reps} layers a figure: median (min .. max); {torch.cuda.get_device_name(0)} on {socket.gethostname()}; {label}")
    if "--network-only" not in args:
        time_layers(reps)
    if "--layers-only" not in args:
        time_network(3)


main()

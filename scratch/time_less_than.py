"""The less-than kernels and protocol timed on the device:
   python scratch/time_less_than.py [reps] [--label TEXT] > profiles/less_than.txt

BLS12-381 Fr, L = 255.

(a) lt_leaves at count = 2^16, both modes, beside the same planes composed from share_arithmetic calls and selects (the public bits
    of c are made into a mask before the clock starts, which favours the composition).  HIP events around one group, `reps` (at
    least 20) runs after a warm-up, the two versions alternated run by run; median (min .. max).  Outputs are compared bit for bit.
(b) one whole less_than (DIRECT, then REFERENCE) at count = 2^16 beside progs.fixedpoint.lt at k = 64, kappa = 32 on the same number
    of pairs: four parties (t = 1) in one process over an in-memory network, every party's coroutine on the one device, wall clock
    from the first coroutine's start to the last one's end with the device synchronised, `runs` = 3 after a warm-up at count = 256.
    The dealing is not timed.  The two compare different things (any residues below (p - 1) / 2 against signed 64-bit values) and spend
    different preprocessing (508 | 510 triples and 255 | 510 bit shares against 125 triples and 96 bit shares an element); the figure
    says what the wider comparison costs.  Every opened result is checked against a < b.

With --steps instead: every entry point alone at both widths (BLS12-381 Fr and 2^64 - 59), 2^20 elements (lt_leaves: L planes at
2^16), HIP events around one launch with the host kept ahead of the device.  Run it against two builds of the library
(HBMPC_HIP_LIB) in one visit to compare them.

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
from honeybadgermpc_amd import share_comparison as sc  # noqa: E402
from honeybadgermpc_amd._capi import Context  # noqa: E402
from honeybadgermpc_amd.open_coalescer import OpenCoalescer  # noqa: E402
from honeybadgermpc_amd.progs import fixedpoint as fx  # noqa: E402

BLS = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
P64 = (1 << 64) - 59
N, T = 4, 1


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


def bit_planes(ctx, t, nbits):
    out = torch.zeros((nbits, t.shape[0], ctx.n_limbs), dtype=torch.int64, device="cuda")
    for i in range(nbits):
        out[i, :, 0] = (t[:, i // 64] >> (i % 64)) & 1
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


def triples(ctx, gen, rows, count):
    tp, tq = rnd(ctx, gen, count, rows), rnd(ctx, gen, count, rows)
    tpq = sa.mul(ctx, tp.view(-1, ctx.n_limbs), tq.view(-1, ctx.n_limbs)).view(tp.shape)
    return [deal(ctx, gen, v) for v in (tp, tq, tpq)]


def time_less_than(ctx, gen, count, mode, runs):
    p, L = ctx.modulus, ctx.modulus.bit_length()
    py = random.Random(count + mode)
    half = (p - 1) // 2
    a = [py.randrange(half) for _ in range(count)]
    b = [a[i] if i % 4 == 0 else py.randrange(half) for i in range(count)]
    want = [1 if x < y else 0 for x, y in zip(a, b)]
    r, s = rnd(ctx, gen, count), rnd(ctx, gen, count)
    da, db, dr, drb = deal(ctx, gen, ctx.upload_ints(a)), deal(ctx, gen, ctx.upload_ints(b)), deal(ctx, gen, r), deal(ctx, gen, bit_planes(ctx, r, L))
    ds, dsb = (deal(ctx, gen, s), deal(ctx, gen, bit_planes(ctx, s, L))) if mode == sc.REFERENCE else ([None] * N, [None] * N)
    dtrip = triples(ctx, gen, sc.less_than_triples(L, mode), count)

    async def body(co, i):
        return await sc.less_than(co, da[i], db[i], dr[i], drb[i], tuple(v[i] for v in dtrip), ds[i], dsb[i], mode)

    async def opened(co, i):
        return ctx.download_ints(await co.open_share_array(await body(co, i)))

    ok = all(got == want for got in run_parties(p, opened)[1])
    return [run_parties(p, body)[0] for _ in range(runs)], ok


def time_fixedpoint_lt(ctx, gen, count, runs, k=64, kappa=32):
    p = ctx.modulus
    py = random.Random(count)
    a = [py.randrange(-(1 << (k - 2)), 1 << (k - 2)) for _ in range(count)]
    b = [a[i] if i % 4 == 0 else py.randrange(-(1 << (k - 2)), 1 << (k - 2)) for i in range(count)]
    want = [1 if x < y else 0 for x, y in zip(a, b)]
    bits = torch.zeros((k + kappa, count, ctx.n_limbs), dtype=torch.int64, device="cuda")
    bits[:, :, 0] = torch.randint(0, 2, (k + kappa, count), device="cuda", generator=gen)
    da, db, dbits = deal(ctx, gen, ctx.upload_ints([v % p for v in a])), deal(ctx, gen, ctx.upload_ints([v % p for v in b])), deal(ctx, gen, bits)
    dtrip = triples(ctx, gen, fx.carry_triples(k - 1), count)

    async def body(co, i):
        return await fx.lt(co, da[i], db[i], dbits[i], tuple(v[i] for v in dtrip), k, kappa)

    async def opened(co, i):
        return ctx.download_ints(await co.open_share_array(await body(co, i)))

    ok = all(got == want for got in run_parties(p, opened)[1])
    return [run_parties(p, body)[0] for _ in range(runs)], ok


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
    """--steps: every entry point of csrc/hb_lt.hip alone, both widths: 2^20 elements (lt_leaves: L planes at 2^16)"""
    pad = torch.empty(1 << 29, dtype=torch.uint8, device="cuda")
    for p, name in ((BLS, "<9, 8>"), (P64, "<3, 2>")):
        ctx = Context.get(p)
        L = p.bit_length()
        gen = torch.Generator(device="cuda")
        gen.manual_seed(29)
        count = 1 << 20
        a, b, r, c, w, x, s, u, v = (rnd(ctx, gen, count) for _ in range(9))
        ta, tb, tc = (tuple(rnd(ctx, gen, count) for _ in range(3)) for _ in range(3))
        s_bits = torch.zeros((L, count, ctx.n_limbs), dtype=torch.int64, device="cuda")           # planes 0, L - 1, L - 2 are read
        o5, o2 = rnd(ctx, gen, count, 5), rnd(ctx, gen, count, 2)
        small = 1 << 16
        c16, bits16 = rnd(ctx, gen, small), rnd(ctx, gen, small, L)
        steps = (("LtMaskRow<true>", lambda: sc.lt_mask(ctx, a, b, r)), ("LtMaskRow<false>", lambda: sc.lt_mask(ctx, a, None, r)),
                 ("LtLeavesRow DIRECT", lambda: sc.lt_leaves(ctx, c16, bits16, sc.DIRECT)), ("LtLeavesRow REFERENCE", lambda: sc.lt_leaves(ctx, c16, bits16, sc.REFERENCE)),
                 ("LtXorMaskRow", lambda: sc.lt_xor_mask(ctx, c, r, w, ta[0], ta[1])),
                 ("LtDmaskRow", lambda: sc.lt_dmask(ctx, c, r, x, s, s_bits, ta[0], ta[1], tb[0], tb[1])),
                 ("LtMidRow", lambda: sc.lt_mid(ctx, o5, u, s_bits, ta, tb, tc[0], tc[1])),
                 ("LtXorFinishRow", lambda: sc.lt_xor_finish(ctx, o2, u, v, tc)))
        for step, fn in steps:
            print(f"step {step + ' ' + name:30s} {fmt(one_launch(reps, fn, pad))}", flush=True)
        del a, b, r, c, w, x, s, u, v, ta, tb, tc, s_bits, o5, o2, c16, bits16, steps
        torch.cuda.empty_cache()


def main():
    args = sys.argv[1:]
    if not torch.cuda.is_available():
        raise SystemExit("scratch/time_less_than.py needs the GPU")
    reps = max(20, int(args[0])) if args and args[0].isdigit() else 20
    label = args[args.index("--label") + 1] if "--label" in args else "working tree"
    if "--steps" in args:
        print(f"# scratch/time_less_than.py --steps, {reps} runs a figure, HIP events around one launch: median (min .. max); {label}")
        return time_steps(reps)
    print(f"# scratch/time_less_than.py, {reps} runs a figure: median (min .. max); {torch.cuda.get_device_name(0)} on {socket.gethostname()}; {label}")
    p = BLS
    ctx = Context.get(p)
    L = p.bit_length()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(23)
    # ---- (a)
    count = 1 << 16
    c, r_bits = rnd(ctx, gen, count), rnd(ctx, gen, count, L)
    msb_first = r_bits.flip(0).reshape(-1, ctx.n_limbs).contiguous()
    mask = torch.cat([(((c[:, i // 64] >> (i % 64)) & 1) != 0) for i in range(L - 1, -1, -1)]).unsqueeze(1)
    zeros = torch.zeros_like(msb_first)
    ones, twos = (ctx.upload_ints([v]).expand(L * count, ctx.n_limbs).contiguous() for v in (1, 2))
    for mode, name in ((sc.DIRECT, "DIRECT"), (sc.REFERENCE, "REFERENCE")):
        def fused():
            return sc.lt_leaves(ctx, c, r_bits, mode)

        def composed():
            g = torch.where(mask, zeros, msb_first)
            if mode == sc.DIRECT:
                return g, torch.where(mask, msb_first, sa.sub(ctx, ones, msb_first))
            return g, torch.where(mask, sa.sub(ctx, twos, msb_first), sa.add(ctx, msb_first, 1))

        same = all(bool(torch.equal(u.reshape(-1, ctx.n_limbs), v)) for u, v in zip(fused(), composed()))
        tf, tc = alternate(reps, fused, composed)
        nbytes = 3 * L * count * 8 * ctx.n_limbs
        print(f"(a) lt_leaves {name:9s} L = {L}  count = 2^16  fused (1 launch) {fmt(tf)}   composed ({1 if mode == sc.DIRECT else 2} launches and 2 selects) {fmt(tc)}   "
              f"composed / fused = {np.median(tc) / np.median(tf):5.2f}   {nbytes / np.median(tf) / 1e3:7.1f} GB/s read + written   {'bit-equal' if same else 'MISMATCH'}", flush=True)
    del c, r_bits, msb_first, mask, zeros, ones, twos
    torch.cuda.empty_cache()
    # ---- (b)
    runs = 3
    for mode in (sc.DIRECT, sc.REFERENCE):
        time_less_than(ctx, gen, 256, mode, 1)
    time_fixedpoint_lt(ctx, gen, 256, 1)
    torch.cuda.empty_cache()
    secs = {}
    for mode, name in ((sc.DIRECT, "DIRECT"), (sc.REFERENCE, "REFERENCE")):
        ts, ok = time_less_than(ctx, gen, count, mode, runs)
        secs[name] = float(np.median(ts))
        print(f"(b) less_than {name:9s} count = 2^16  n = {N}, t = {T}  {sc.less_than_opens(L, mode)} opens, {sc.less_than_triples(L, mode)} triples an element   "
              f"{np.median(ts) * 1e3:9.1f} ms ({min(ts) * 1e3:.1f} .. {max(ts) * 1e3:.1f}), all four parties   {'opens to a < b' if ok else 'MISMATCH'}", flush=True)
        torch.cuda.empty_cache()
    ts, ok = time_fixedpoint_lt(ctx, gen, count, runs)
    print(f"(b) fixedpoint.lt k = 64  count = 2^16  n = {N}, t = {T}  {1 + fx.carry_levels(63)} opens, {fx.carry_triples(63)} triples an element   "
          f"{np.median(ts) * 1e3:9.1f} ms ({min(ts) * 1e3:.1f} .. {max(ts) * 1e3:.1f}), all four parties   {'opens to a < b' if ok else 'MISMATCH'}   "
          f"less_than DIRECT / fixedpoint.lt = {secs['DIRECT'] / np.median(ts):5.2f}", flush=True)


main()

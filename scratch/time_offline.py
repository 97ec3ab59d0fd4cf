"""The offline phase's kernels and protocol timed on the device:
   python scratch/time_offline.py [reps] [--label TEXT] [--out PATH]        (PATH defaults to profiles/offline.txt)

(a) each kernel of csrc/hb_off.hip beside the same result composed from entry points that were there before it, at 2^16 and 2^20
    elements over BLS12-381 Fr and 2^16 over Goldilocks:
      mul_add         against share_arithmetic.mul then add (in place)
      invsqrt_scale   PM1 against hb_sqrt_mod, share_arithmetic.inv, mul; ZERO_ONE against those and add 1, mul (p + 1) / 2
      degree_check    (one inverse mat-vec + one launch + one read-back) against HyperInvertible.check of both sharings and a
                      comparison of the constants, n = 4, t = 1 and n = 16, t = 5, k = 2^16 columns (BLS12-381)
    HIP events around one call of each, `reps` (at least 30) runs after a warm-up, the two versions alternated run by run; median
    (min .. max).  Outputs are compared bit for bit.  "kept": the fused median is below the composed median by more than the composed
    route's own spread (max - min).
(b) one whole generate_triples and one whole generate_bits at k = 2^16, four parties (t = 1) in one process over an in-memory network,
    every party's coroutine on the one device: wall clock from the first coroutine's start to the last one's end with the device
    synchronised, 3 runs after a warm-up at k = 256.  Context, not judged against anything.

No GPU: fails (there is nothing to fall back to).

With --steps instead: mul_add alone at both widths (BLS12-381 Fr and 2^64 - 59), 2^20 elements, HIP events around one launch
with the host kept ahead of the device (one_launch of scratch/time_share_comparison.py).  Run it against two builds of the library
(HBMPC_HIP_LIB) in one visit to compare them."""
import asyncio
import os
import socket
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from honeybadgermpc_amd import offline  # noqa: E402
from honeybadgermpc_amd import share_arithmetic as sa  # noqa: E402
from honeybadgermpc_amd._capi import Context  # noqa: E402
from honeybadgermpc_amd.open_coalescer import OpenCoalescer  # noqa: E402

BLS = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
GOLDILOCKS = 0xFFFFFFFF00000001
N, T = 4, 1
LINES = []


def say(line):
    LINES.append(line)
    print(line, flush=True)


def rnd(ctx, gen, count):
    return ctx.reduce_(torch.randint(-(1 << 63), (1 << 63) - 1, (count, ctx.n_limbs), dtype=torch.int64, device="cuda", generator=gen))


def fmt(ts):
    return f"{np.median(ts):10.1f} us ({min(ts):.1f} .. {max(ts):.1f})"


def alternate(reps, fused, composed):
    for _ in range(3):
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


def report(what, shape, tf, tc, same, note=""):
    kept = np.median(tf) < np.median(tc) - (max(tc) - min(tc))
    say(f"(a) {what:24s} {shape:34s} fused {fmt(tf)}   composed {fmt(tc)}   composed / fused = {np.median(tc) / np.median(tf):6.2f}   "
        f"{'kept' if kept else 'NOT beyond the spread'}   {'bit-equal' if same else 'MISMATCH'}{note}")


def kernels(ctx, gen, name, count, reps):
    p, half = ctx.modulus, (ctx.modulus + 1) // 2
    shape = f"{name}  count = 2^{count.bit_length() - 1}"
    a, b, c = (rnd(ctx, gen, count) for _ in range(3))

    def fused():
        return offline.mul_add(ctx, a, b, c)

    def composed():
        prod = sa.mul(ctx, a, b)
        return sa.add(ctx, prod, c, out=prod)

    same = bool(torch.equal(fused(), composed()))
    tf, tc = alternate(reps, fused, composed)
    report("mul_add", shape, tf, tc, same, f"   {4 * count * 8 * ctx.n_limbs / np.median(tf) / 1e3:7.1f} GB/s read + written")
    u = rnd(ctx, gen, count)
    x = sa.mul(ctx, u, u)                                             # squares: every element has a root (a zero has probability count / p)
    roots, ok = ctx.empty(count), torch.zeros(count, dtype=torch.uint8, device="cuda")
    for mode, label in ((offline.PM1, "PM1"), (offline.ZERO_ONE, "ZERO_ONE")):
        def fused():
            return offline.invsqrt_scale(ctx, x, u, mode, check=False)[0]

        def composed():
            ctx.check(ctx.lib.hb_sqrt_mod(ctx.h, ctx.ptr(x), count, ctx.ptr(roots), ctx.ptr(ok), ctx.stream()), "hb_sqrt_mod")
            w, _ = sa.inv(ctx, roots, check=False)
            out = sa.mul(ctx, u, w, out=w)
            if mode == offline.ZERO_ONE:
                out = sa.mul(ctx, sa.add(ctx, out, 1, out=out), half, out=out)
            return out

        same = bool(torch.equal(fused(), composed()))
        tf, tc = alternate(reps, fused, composed)
        report(f"invsqrt_scale {label}", shape, tf, tc, same)


def degree_checks(ctx, gen, n, t, k, reps):
    codec = offline._Codec.get(ctx, n, t, k)
    secrets = rnd(ctx, gen, k)
    shares_t, _ = codec.deal_t.deal_secrets(secrets, gen)
    shares_2t, _ = codec.deal_2t.deal_secrets(secrets, gen)
    block = torch.cat((shares_t.view(n, k, -1), shares_2t.view(n, k, -1)), dim=1).contiguous().view(n * 2 * k, -1)

    def fused():
        return offline.degree_check(ctx, codec.interpolate(block, 2 * k), n, t) == (0, 0, 0)

    def composed():
        ok_t, s_t = codec.hyper.check(shares_t, t)
        ok_2t, s_2t = codec.hyper.check(shares_2t, 2 * t)
        return ok_t and ok_2t and bool(torch.equal(s_t, s_2t))

    same = fused() is True and composed() is True
    tf, tc = alternate(reps, fused, composed)
    report("degree_check + interpolate", f"BLS12-381  n = {n}, t = {t}  k = 2^{k.bit_length() - 1}", tf, tc, same)


class Net:
    def __init__(self, n):
        self.q = [dict() for _ in range(n)]

    def get_send_recv(self, i):
        def factory(tag):
            def send(dest, msg):
                self.q[dest].setdefault(tag, asyncio.Queue()).put_nowait((i, msg))

            return send, self.q[i].setdefault(tag, asyncio.Queue()).get

        return factory


def run_parties(p, body):
    async def main():
        net = Net(N)
        return await asyncio.gather(*[body(OpenCoalescer(p, N, T, i, net.get_send_recv(i)), i) for i in range(N)])

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = asyncio.run(main())
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res


def protocol(ctx, k, runs):
    p = ctx.modulus
    gens = [torch.Generator(device="cuda") for _ in range(N)]
    for i, g in enumerate(gens):
        g.manual_seed(77 + i)

    async def triples(co, i):
        return await offline.generate_triples(co, k, generator=gens[i])

    async def bits(co, i):
        return await offline.generate_bits(co, k, offline.ZERO_ONE, generator=gens[i])

    async def triples_opened(co, i):
        a, b, ab = await triples(co, i)
        h = [co.open_share_array(v) for v in (a, b, ab)]
        a, b, ab = [await v for v in h]
        return bool(torch.equal(sa.mul(ctx, a, b), ab))

    async def bits_opened(co, i):
        v = await co.open_share_array(await bits(co, i))
        return bool(((v[:, 0] == 0) | (v[:, 0] == 1)).all()) and not bool(v[:, 1:].any())

    out = []
    for name, body, check in (("generate_triples", triples, triples_opened), ("generate_bits ZERO_ONE", bits, bits_opened)):
        ok = all(run_parties(p, check)[1])
        ts = [run_parties(p, body)[0] for _ in range(runs)]
        out.append((name, ts, ok))
    return out


def time_steps(reps, label):
    """--steps: mul_add alone (a b + c, and the square a a + c written over c), both widths, 2^20 elements"""
    from time_share_comparison import fmt as band, one_launch, rnd as draw

    print(f"# scratch/time_offline.py --steps, {reps} runs a figure, HIP events around one launch: median (min .. max); {label}")
    pad = torch.empty(1 << 29, dtype=torch.uint8, device="cuda")
    count = 1 << 20
    for p, width in ((BLS, "<9, 8>"), ((1 << 64) - 59, "<3, 2>")):
        ctx = Context.get(p)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(19)
        a, b, c = (draw(ctx, gen, count) for _ in range(3))
        out = ctx.empty(count)
        steps = [("OffMulAddRow", lambda: offline.mul_add(ctx, a, b, c, out=out)), ("OffMulAddRow square, out = c", lambda: offline.mul_add(ctx, a, a, c, out=c))]
        for step, fn in steps:
            print(f"step {step + ' ' + width:34s} {band(one_launch(reps, fn, pad))}", flush=True)
        del steps
        torch.cuda.empty_cache()


def main():
    args = sys.argv[1:]
    if not torch.cuda.is_available():
        raise SystemExit("scratch/time_offline.py needs the GPU")
    reps = max(30, int(args[0])) if args and args[0].isdigit() else 30
    label = args[args.index("--label") + 1] if "--label" in args else "working tree"
    if "--steps" in args:
        return time_steps(max(20, int(args[0])) if args and args[0].isdigit() else 20, label)
    path = args[args.index("--out") + 1] if "--out" in args else os.path.join("profiles", "offline.txt")
    say(f"# scratch/time_offline.py, {reps} runs a figure: median (min .. max); {torch.cuda.get_device_name(0)} on {socket.gethostname()}; {label}")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(29)
    bls, gold = Context.get(BLS), Context.get(GOLDILOCKS)
    for ctx, name, count in ((bls, "BLS12-381", 1 << 16), (bls, "BLS12-381", 1 << 20), (gold, "Goldilocks", 1 << 16)):
        kernels(ctx, gen, name, count, reps)
        torch.cuda.empty_cache()
    for n, t in ((4, 1), (16, 5)):
        degree_checks(bls, gen, n, t, 1 << 16, reps)
        torch.cuda.empty_cache()
    protocol(bls, 256, 1)
    for name, ts, ok in protocol(bls, 1 << 16, 3):
        say(f"(b) {name:24s} k = 2^16  n = {N}, t = {T}  {np.median(ts) * 1e3:9.1f} ms ({min(ts) * 1e3:.1f} .. {max(ts) * 1e3:.1f}), all four parties   "
            f"{'opens as it should' if ok else 'MISMATCH'}")
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(LINES) + "\n")


main()

"""The shared powers and cubes of the offline phase timed on the device:
   python scratch/time_offline_powers.py [reps] [--label TEXT] [--out PATH] [--skip-protocol]     (PATH defaults to profiles/offline_powers.txt)

(a) one doubling level as the two fused launches of csrc/hb_offpow.hip: offline.pow_mask over the item-major (count, k) powers array,
    then offline.pow_finish with a fixed array standing for what the open returns;
(b) the same level composed from entry points that were there before those kernels: a torch gather of each factor into contiguous
    arrays, offline.mul_add, share_arithmetic.sub, and a strided copy of the differences into the powers array.
    Shapes: count = k = 1024 at level (512, 512) -- the last and largest level of generate_powers(co, 1024, 1024) -- and count = 64,
    k = 16 at level (8, 8), where a level is launch-bound (two launches against six), over BLS12-381 Fr.  HIP events around one level
    of each, `reps` (at least 30) runs after a warm-up, the two routes alternated run by run; median (min .. max).  The masked arrays
    and the powers arrays of the two routes are compared bit for bit.  "kept": the fused median is below the composed median by
    more than the composed route's own spread (max - min).
(c) one whole generate_powers(co, 1024, 1024) and one whole generate_cubes(co, 161, 4096) (what a MiMC encryption of 4096 blocks over
    BLS12-381 takes: 161 rounds), four parties (t = 1) in one process over an in-memory network, every party's coroutine on the one
    device: wall clock from the first coroutine's start to the last one's end with the device synchronised, 3 runs after a warm-up at
    a small size.  Context, not judged against anything.

The file is rewritten after every figure, so a run that is cut short leaves what it measured.  No GPU: fails (there is nothing to fall
back to)."""
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
N, T = 4, 1
LINES = []
PATH = [None]


def say(line):
    LINES.append(line)
    print(line, flush=True)
    os.makedirs(os.path.dirname(PATH[0]) or ".", exist_ok=True)
    with open(PATH[0], "w") as f:
        f.write("\n".join(LINES) + "\n")


def rnd(ctx, gen, count):
    return ctx.reduce_(torch.randint(-(1 << 63), (1 << 63) - 1, (count, ctx.n_limbs), dtype=torch.int64, device="cuda", generator=gen))


def fmt(ts):
    return f"{np.median(ts):9.1f} us ({min(ts):.1f} .. {max(ts):.1f})"


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


def level(ctx, gen, count, k, m, w, reps):
    L = ctx.n_limbs
    powers = rnd(ctx, gen, count * k).view(count, k, L)
    r2t, rt, opened = (rnd(ctx, gen, count * w) for _ in range(3))
    pf, pc = powers.clone(), powers.clone()
    masked_f, masked_c = ctx.empty(count * w), ctx.empty(count * w)
    diff = ctx.empty(count * w)

    def fused():
        offline.pow_mask(ctx, pf, r2t, m, w, out=masked_f)
        offline.pow_finish(ctx, opened, rt, pf, m, w)

    def composed():
        a = pc[:, m - 1:m].expand(count, w, L).reshape(count * w, L)      # gathers: the factors as contiguous arrays
        b = pc[:, :w].reshape(count * w, L)
        offline.mul_add(ctx, a, b, r2t, out=masked_c)
        sa.sub(ctx, opened, rt, out=diff)
        pc[:, m:m + w] = diff.view(count, w, L)                            # scatter

    fused(); composed()
    same = bool(torch.equal(masked_f, masked_c)) and bool(torch.equal(pf, pc)) and not bool(torch.equal(pf, powers))
    tf, tc = alternate(reps, fused, composed)
    kept = np.median(tf) < np.median(tc) - (max(tc) - min(tc))
    moved = (3 + 3) * count * w * 8 * L                                   # the fused pair: 3 + 1 element moves for the mask (the shared factor not counted), 2 + 1 for the finish
    say(f"(a, b) one level  count = {count}, k = {k}, (m, w) = ({m}, {w})  BLS12-381   fused (a) {fmt(tf)}   composed (b) {fmt(tc)}   "
        f"composed / fused = {np.median(tc) / np.median(tf):5.2f}   {'kept' if kept else 'NOT beyond the spread'}   "
        f"{'bit-equal' if same else 'MISMATCH'}   fused: {moved / np.median(tf) / 1e3:7.1f} GB/s of its 6 element moves a product")


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


def protocol(ctx, name, make, check, runs):
    p = ctx.modulus
    gens = [torch.Generator(device="cuda") for _ in range(N)]
    for i, g in enumerate(gens):
        g.manual_seed(91 + i)

    async def plain(co, i):
        await make(co, gens[i])
        return co.batches

    async def checked(co, i):
        return await check(co, await make(co, gens[i]))

    ok = all(run_parties(p, checked)[1])
    ts, batches = [], None
    for _ in range(runs):
        dt, res = run_parties(p, plain)
        ts.append(dt)
        batches = res[0]
    return ts, ok, batches


def main():
    args = sys.argv[1:]
    if not torch.cuda.is_available():
        raise SystemExit("scratch/time_offline_powers.py needs the GPU")
    reps = max(30, int(args[0])) if args and args[0].isdigit() else 30
    label = args[args.index("--label") + 1] if "--label" in args else "working tree"
    PATH[0] = args[args.index("--out") + 1] if "--out" in args else os.path.join("profiles", "offline_powers.txt")
    say(f"# scratch/time_offline_powers.py, {reps} runs a figure: median (min .. max); {torch.cuda.get_device_name(0)} on {socket.gethostname()}; {label}")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(31)
    ctx = Context.get(BLS)
    L = ctx.n_limbs
    level(ctx, gen, 1024, 1024, 512, 512, reps)
    level(ctx, gen, 64, 16, 8, 8, reps)
    torch.cuda.empty_cache()
    if "--skip-protocol" in args:
        say("(c) generate_powers(co, 1024, 1024), generate_cubes(co, 161, 4096): not taken yet")
        return

    async def powers_ok(co, powers):
        count, k = powers.shape[0], powers.shape[1]
        v = await co.open_share_array(powers.view(count * k, L))
        return bool(torch.equal(sa.mul(ctx, v.view(count, k, L)[:, :-1].reshape(-1, L), v.view(count, k, L)[:, :1].expand(count, k - 1, L).reshape(-1, L)),
                                v.view(count, k, L)[:, 1:].reshape(-1, L)))

    async def cubes_ok(co, cubes):
        h = [co.open_share_array(v.reshape(-1, L)) for v in cubes]
        r, r2, r3 = [await v for v in h]
        return bool(torch.equal(sa.mul(ctx, r, r), r2)) and bool(torch.equal(sa.mul(ctx, r2, r), r3))

    for name, small, full, check in (
        ("generate_powers(co, 1024, 1024)", lambda co, g: offline.generate_powers(co, 16, 16, generator=g), lambda co, g: offline.generate_powers(co, 1024, 1024, generator=g), powers_ok),
        ("generate_cubes(co, 161, 4096)", lambda co, g: offline.generate_cubes(co, 3, 16, generator=g), lambda co, g: offline.generate_cubes(co, 161, 4096, generator=g), cubes_ok),
    ):
        protocol(ctx, name, small, check, 1)
        ts, ok, batches = protocol(ctx, name, full, check, 3)
        say(f"(c) {name:32s} n = {N}, t = {T}  BLS12-381  {np.median(ts) * 1e3:9.1f} ms ({min(ts) * 1e3:.1f} .. {max(ts) * 1e3:.1f}), all four parties, "
            f"{batches} opens a party   {'opens as it should' if ok else 'MISMATCH'}")
        torch.cuda.empty_cache()


main()

"""The share bits of the offline phase timed on the device:
   python scratch/time_offline_share_bits.py [reps] [--label TEXT] [--out PATH] [--skip-protocol]     (PATH defaults to profiles/offline_share_bits.txt)

(a) the leaves of [r > p - 1] over m candidates as the one fused launch of csrc/hb_offsb.hip (offline.sb_leaves: the bound held by value)
    against the composition that was there before it: an (m, limbs) array holding p - 1 in every element, made for the call, plus
    share_comparison.lt_leaves in mode DIRECT;
(b) the finish over the kept candidates (offline.sb_finish: gather of the kept planes and composition of r in one pass) against torch's
    index_select of the planes plus linalg.matmul of the (1, L) row of powers of two with the kept (L, kept) planes.  The index is
    torch.nonzero of a random verdict that keeps a candidate with probability p / 2^L.
    m = 2^12 and 2^16 candidates over BLS12-381 Fr and over 2^64 - 59.  HIP events around one call of each, `reps` (at least 30) runs
    after a warm-up, the two routes alternated run by run; median (min .. max).  The results of the two routes are compared bit for bit.
    "fused faster": the fused median is below the composed median by more than the composed route's own spread (max - min).
(c) one whole generate_share_bits(co, 1024), four parties (t = 1) in one process over an in-memory network, every party's coroutine on
    the one device: wall clock from the first coroutine's start to the last one's end with the device synchronised, 3 runs after a
    warm-up at a small size; and, as runs of their own over the candidates of its first round, its parts: the bit source, the triple
    source, leaves + tree + the verdicts' open, and the finish (HIP events in party 0, the other parties' work on the device included).
    Context, not judged against anything.

The file is rewritten after every figure, so a run that is cut short leaves what it measured.  No GPU: fails (there is nothing to fall
back to)."""
import asyncio
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from honeybadgermpc_amd import linalg, offline  # noqa: E402
from honeybadgermpc_amd import share_comparison as sc  # noqa: E402
from honeybadgermpc_amd._capi import Context  # noqa: E402
from honeybadgermpc_amd.open_coalescer import OpenCoalescer  # noqa: E402
from honeybadgermpc_amd.progs.fixedpoint import carry_tree  # noqa: E402

BLS = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
P64 = (1 << 64) - 59
NAMES = {BLS: "BLS12-381", P64: "2^64-59"}
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


def verdict(tf, tc):
    if np.median(tf) < np.median(tc) - (max(tc) - min(tc)):
        return "fused faster"
    if np.median(tc) < np.median(tf) - (max(tf) - min(tf)):
        return "fused SLOWER"
    return "within the spread"


def kernels(ctx, gen, m, reps):
    p, nl, L = ctx.modulus, ctx.n_limbs, ctx.modulus.bit_length()
    bits = rnd(ctx, gen, L * m).view(L, m, nl)
    bound = ctx.upload_ints([p - 1])
    out = {}

    def fused_leaves():
        out["f"] = offline.sb_leaves(ctx, bits)

    def composed_leaves():
        out["c"] = sc.lt_leaves(ctx, bound.repeat(m, 1), bits, sc.DIRECT)

    fused_leaves(); composed_leaves()
    same = all(bool(torch.equal(a, b)) for a, b in zip(out["f"], out["c"]))
    tf, tc = alternate(reps, fused_leaves, composed_leaves)
    moved = 3 * L * m * 8 * nl                                            # a plane element read, two written
    say(f"(a) leaves   m = {m:6d}  {NAMES[p]:10s} fused {fmt(tf)}   composed {fmt(tc)}   composed / fused = {np.median(tc) / np.median(tf):5.2f}   "
        f"{verdict(tf, tc)}   {'bit-equal' if same else 'MISMATCH'}   fused: {moved / np.median(tf) / 1e3:7.1f} GB/s of its 3 element moves a leaf")
    out.clear()

    keep = torch.rand(m, device="cuda", generator=gen) < p / 2 ** L
    index = torch.nonzero(keep).view(-1)
    k = int(index.shape[0])
    pow2 = ctx.upload_ints([pow(2, q, p) for q in range(L)]).view(1, L, nl)

    def fused_finish():
        out["f"] = offline.sb_finish(ctx, bits, index, check=False)

    def composed_finish():
        planes = bits.index_select(1, index)
        out["c"] = (linalg.matmul(ctx, pow2, planes).view(k, nl), planes)

    fused_finish(); composed_finish()
    same = all(bool(torch.equal(a, b)) for a, b in zip(out["f"], out["c"]))
    tf, tc = alternate(reps, fused_finish, composed_finish)
    moved = (2 * L + 1) * k * 8 * nl                                      # a plane element read and written, r written
    say(f"(b) finish   m = {m:6d}  {NAMES[p]:10s} fused {fmt(tf)}   composed {fmt(tc)}   composed / fused = {np.median(tc) / np.median(tf):5.2f}   "
        f"{verdict(tf, tc)}   {'bit-equal' if same else 'MISMATCH'}   kept {k}   fused: {moved / np.median(tf) / 1e3:7.1f} GB/s of its 2 L + 1 element moves a slot")
    out.clear()
    del bits
    torch.cuda.empty_cache()


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


def ms(ts):
    return f"{np.median(ts) * 1e3:9.1f} ms ({min(ts) * 1e3:.1f} .. {max(ts) * 1e3:.1f})"


def protocol(ctx, count, runs):
    p, nl, L = ctx.modulus, ctx.n_limbs, ctx.modulus.bit_length()
    gens = [torch.Generator(device="cuda") for _ in range(N)]
    for i, g in enumerate(gens):
        g.manual_seed(91 + i)
    m, rows = offline.share_bits_candidates(p, count), 2 * L - 3

    async def whole(co, i, k=count):
        r, r_bits = await offline.generate_share_bits(co, k, generator=gens[i])
        return r, r_bits, co.batches

    async def checked(co, i):
        r, r_bits, _ = await whole(co, i, 16)
        opened = await co.open_share_array(torch.cat((r, r_bits.view(-1, nl))))
        v, planes = opened[:16], opened[16:].view(L, 16, nl)
        pow2 = ctx.upload_ints([pow(2, q, p) for q in range(L)]).view(1, L, nl)
        is_bit = ((planes[..., 1:] == 0).all(dim=-1) & ((planes[..., 0] == 0) | (planes[..., 0] == 1))).all()
        return bool(is_bit) and bool(torch.equal(linalg.matmul(ctx, pow2, planes).view(16, nl), v))

    ok = all(run_parties(p, checked)[1])                                   # the warm-up, checked: planes of bits that compose their r
    ts, batches = [], None
    for _ in range(runs):
        dt, res = run_parties(p, whole)
        ts.append(dt)
        batches = res[0][2]
    say(f"(c) generate_share_bits(co, {count})  n = {N}, t = {T}  {NAMES[p]}  {ms(ts)}, all four parties, {m} candidates in the first round, "
        f"{batches} opens a party   {'opens as it should' if ok else 'MISMATCH'}")

    material = [None] * N

    async def bit_source(co, i):
        material[i] = [(await offline.generate_bits(co, L * m, encoding=offline.ZERO_ONE, generator=gens[i])).view(L, m, nl), None]

    async def triple_source(co, i):
        material[i][1] = tuple(v.view(rows, m, nl) for v in await offline.generate_triples(co, rows * m, generator=gens[i]))

    finish_us = []

    async def tree(co, i):
        bits, trip = material[i]
        g, q = offline.sb_leaves(ctx, bits)
        w = await co.open_share_array(await carry_tree(co, g, q, trip))
        index = torch.nonzero((w == 0).all(dim=1)).view(-1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        offline.sb_finish(ctx, bits, index, check=False)
        e1.record()
        if i == 0:
            torch.cuda.synchronize()
            finish_us.append(e0.elapsed_time(e1) * 1e3)

    for name, body in (("bit source: generate_bits of L m bits", bit_source), ("triple source: generate_triples of (2 L - 3) m", triple_source),
                       ("leaves, tree, the verdicts' open (and the finish)", tree)):
        ts = [run_parties(p, body)[0] for _ in range(runs)]
        say(f"    {name:52s} {ms(ts)}, all four parties, run on its own")
    say(f"    finish: sb_finish over the kept of {m} candidates, party 0     {fmt(finish_us)}")


def main():
    args = sys.argv[1:]
    if not torch.cuda.is_available():
        raise SystemExit("scratch/time_offline_share_bits.py needs the GPU")
    reps = max(30, int(args[0])) if args and args[0].isdigit() else 30
    label = args[args.index("--label") + 1] if "--label" in args else "working tree"
    PATH[0] = args[args.index("--out") + 1] if "--out" in args else os.path.join("profiles", "offline_share_bits.txt")
    say(f"# scratch/time_offline_share_bits.py, {reps} runs a figure: median (min .. max); {torch.cuda.get_device_name(0)}; {label}")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(31)
    for p in (BLS, P64):
        for m in (1 << 12, 1 << 16):
            kernels(Context.get(p), gen, m, reps)
    if "--skip-protocol" in args:
        say("(c) generate_share_bits(co, 1024): not taken yet")
        return
    protocol(Context.get(BLS), 1024, 3)


main()

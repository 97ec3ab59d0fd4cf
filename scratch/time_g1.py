"""The G1 kernels (csrc/hb_g1.hip): what the compiler made of them, and their timing on the device.  Writes profiles/g1.txt, one section a mode;
a mode rewrites its own section and keeps the other.

   python scratch/time_g1.py --resources        no GPU needed: compiles hb_g1.hip for gfx950 with -Rpass-analysis=kernel-resource-usage and
                                                 reads the code size of every function from the device code object (llvm-readelf)
   python scratch/time_g1.py [reps]             needs the GPU (fails without: there is nothing to fall back to)

Timing: scalar_mul (a scalar and a point an element, random 255-bit scalars), commit at window 4 and 8, eval_commitments and verify at
t = 21, i = 64, each at 2^12 and 2^16 items; HIP events around one call, `reps` calls after a warm-up of the same shape, median (min .. max).
Beside verify, the SAME verification done the reference's way (poly_commit_lin.py:24-29): every commitment raised to i^j mod R by scalar_mul,
the t + 1 powers of an item added up by `add`, the right side from commit, the two sides compared -- the schedule, from this package's own
kernels, for scale; the reference's Rust group arithmetic itself cannot be built here.  The inputs are honest: commitments of random
polynomials, their shares and witnesses at i (the run asserts that verify rejects nothing), so every lane walks the ordinary path.
Field products an item are COUNTED from hb_g1.hip: 7 a doubling, 11 a mixed and 16 a general addition, 8 the compare, 3 an on-curve check,
2 a loaded point; fq_inv 384 squarings + popcount(Q - 2) products."""
import os
import re
import socket
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "profiles", "g1.txt")
HEADS = {"resources": "## resources", "timing": "## timing"}
T, INDEX = 21, 64


def write_section(which, lines):
    sections = {"resources": ["## resources", "not recorded yet"], "timing": ["## timing", "timings not taken yet"]}
    if os.path.exists(OUT):
        cur = None
        for line in open(OUT).read().splitlines():
            for k, h in HEADS.items():
                if line.startswith(h):
                    cur = k
                    sections[k] = []
            if cur:
                sections[cur].append(line)
    sections[which] = [HEADS[which]] + lines
    with open(OUT, "w") as f:
        f.write("# profiles/g1.txt -- written by scratch/time_g1.py\n")
        for k in ("resources", "timing"):
            f.write("\n".join(sections[k]).rstrip() + "\n\n")


def resources():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(REPO, "honeybadgermpc_amd", "csrc", "hb_g1.hip")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "--no-gpu-bundle-output", "-c", src]
    with tempfile.TemporaryDirectory() as tmp:
        obj = os.path.join(tmp, "hb_g1.co")
        r = subprocess.run([hipcc] + flags + ["-Rpass-analysis=kernel-resource-usage", "-o", obj], capture_output=True, text=True, check=True)
        readelf = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "llvm-readelf")
        if not os.path.exists(readelf):
            readelf = "/opt/rocm/llvm/bin/llvm-readelf"
        syms = subprocess.run([readelf, "-s", "--wide", "--demangle", obj], capture_output=True, text=True, check=True).stdout
    sizes = {}
    for line in syms.splitlines():
        m = re.match(r"\s*\d+:\s+[0-9a-f]+\s+(\d+)\s+FUNC\s+\S+\s+\S+\s+\S+\s+(.*)", line)
        if m:
            sizes[re.sub(r"\(.*", "", m.group(2)).replace("hb::", "")] = int(m.group(1))
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?)\s*\[-Rpass", line)
        if not m:
            continue
        key, _, val = m.group(1).partition(":")
        if key.strip() == "Function Name":
            name = subprocess.run(["c++filt", val.strip()], capture_output=True, text=True).stdout.strip() or val.strip()
            cur = {"name": re.sub(r"\(.*", "", name).replace("hb::", "")}
            rows.append(cur)
        elif cur is not None:
            cur[key.strip()] = val.strip()
    lines = ["hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage on csrc/hb_g1.hip; code size: the function's bytes in the device code object.",
             "mont_mul<14> is one function (fq_mul_call), called, not inlined: its bytes are its own row and in no kernel's.",
             f"{'function':18s} {'VGPRs':>6s} {'AGPRs':>6s} {'SGPRs':>6s} {'scratch B/lane':>15s} {'waves/SIMD':>11s} {'LDS B':>6s} {'code bytes':>11s}"]
    for c in rows:
        lines.append(f"{c['name']:18s} {c.get('VGPRs', '?'):>6s} {c.get('AGPRs', '?'):>6s} {c.get('TotalSGPRs', c.get('SGPRs', '?')):>6s} "
                     f"{c.get('ScratchSize [bytes/lane]', '?'):>15s} {c.get('Occupancy [waves/SIMD]', '?'):>11s} {c.get('LDS Size [bytes/block]', '?'):>6s} "
                     f"{sizes.get(c['name'], 0):>11d}")
    for name, size in sizes.items():
        if not any(c["name"] == name for c in rows):
            lines.append(f"{name:18s} {'':>6s} {'':>6s} {'':>6s} {'':>15s} {'':>11s} {'':>6s} {size:>11d}   (called by every kernel)")
    assert all(c.get("ScratchSize [bytes/lane]") == "0" for c in rows), "a G1 kernel uses scratch memory"
    write_section("resources", lines)
    print("\n".join(lines))


def fmt(ts):
    return f"{np.median(ts):10.1f} us ({min(ts):.1f} .. {max(ts):.1f})"


def timed(torch, reps, fn):
    fn()
    torch.cuda.synchronize()
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(reps)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e3 for a, b in evs]


def timing(reps):
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("scratch/time_g1.py needs the GPU")
    from honeybadgermpc_amd import g1, share_arithmetic as sa
    from honeybadgermpc_amd._capi import Context
    from honeybadgermpc_amd.bls12_381 import G1, Q, R

    ctx = Context.get(R)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(13)                                      # timing inputs only: NOT how a dealer draws its blinding

    def rnd(count):
        return ctx.reduce_(torch.randint(-(1 << 63), (1 << 63) - 1, (count, 4), dtype=torch.int64, device="cuda", generator=gen))

    g, h = G1.generator(), G1.rand("h")
    tabs = {c: (g1.FixedBase(ctx, g, c), g1.FixedBase(ctx, h, c)) for c in (4, 8)}
    inv = 384 + bin(Q - 2).count("1")
    dbl, mixed, general, load, store = 7, 11, 16, 2, inv + 5
    log_i, pop_i = INDEX.bit_length() - 1, bin(INDEX).count("1")
    horner = T * (log_i * dbl + (pop_i - 1) * general + mixed) + (T + 1) * load
    lines = [f"{reps} calls a figure after a warm-up: median (min .. max); {torch.cuda.get_device_name(0)} on {socket.gethostname()}; t = {T}, i = {INDEX}",
             "products an item: counted from hb_g1.hip (see the head of scratch/time_g1.py); a non-zero window digit is assumed in every window",
             "2^16 items are 1024 waves, ONE a SIMD of the device: up to there a call lasts as long as one wave's serial chain, whatever the count;",
             "the reference's schedule at 2^16 is a launch of 22 x 2^16 lanes and shows the rate of a full device"]
    for n in (12, 16):
        B = 1 << n
        ks, pts = rnd(B), g1.scalar_mul(ctx, rnd(B), g)
        out = torch.empty((B, 2, 6), dtype=torch.int64, device="cuda")
        ts = timed(torch, reps, lambda: g1.scalar_mul(ctx, ks, pts, out=out))
        bits = int(np.unpackbits(ks.cpu().numpy().view(np.uint8)).sum()) / B
        muls = 255 * dbl + bits * mixed + load + store
        lines.append(f"scalar_mul        2^{n} items  {fmt(ts)}  {muls:8.0f} products an item  {muls * B / np.median(ts) / 1e3:7.1f} G products/s")
        a, b = rnd(B), rnd(B)
        for c in (4, 8):
            ts = timed(torch, reps, lambda: g1.commit(ctx, *tabs[c], a, b, out=out))
            muls = 2 * (256 // c) * mixed + store
            lines.append(f"commit c = {c}      2^{n} items  {fmt(ts)}  {muls:8.0f} products an item  {muls * B / np.median(ts) / 1e3:7.1f} G products/s")
        # honest items: B polynomials of degree T, their commitments, and share and witness at INDEX
        coef, hat = rnd(B * (T + 1)).reshape(B, T + 1, 4), rnd(B * (T + 1)).reshape(B, T + 1, 4)
        cs = g1.commit(ctx, *tabs[8], coef.reshape(-1, 4), hat.reshape(-1, 4)).reshape(B, T + 1, 2, 6)

        def at_index(co):
            acc = co[:, T].contiguous()
            for j in range(T - 1, -1, -1):
                acc = sa.add(ctx, sa.mul(ctx, acc, INDEX), co[:, j].contiguous())
            return acc

        sh, wi = at_index(coef), at_index(hat)
        ts = timed(torch, reps, lambda: g1.eval_commitments(ctx, cs, INDEX, out=out))
        muls = horner + store
        lines.append(f"eval_commitments  2^{n} items  {fmt(ts)}  {muls:8.0f} products an item  {muls * B / np.median(ts) / 1e3:7.1f} G products/s")
        verdict, counter = g1.verify(ctx, *tabs[8], cs, INDEX, sh, wi)
        assert int(counter.item()) == 0 and bool(verdict.all()), "honest items were rejected"
        ts_v = timed(torch, reps, lambda: g1.verify(ctx, *tabs[8], cs, INDEX, sh, wi))
        muls = horner + 3 * (T + 1) + 2 * 32 * mixed + 8
        lines.append(f"verify c = 8      2^{n} items  {fmt(ts_v)}  {muls:8.0f} products an item  {muls * B / np.median(ts_v) / 1e3:7.1f} G products/s")
        # the reference's schedule: cs[b][j] ^ (i^j mod R) for every j, their product, == g^s h^w
        exps = ctx.upload_ints([pow(INDEX, j, R) for j in range(T + 1)]).repeat_interleave(B, dim=0)
        cs_rows = cs.transpose(0, 1).contiguous()             # (t + 1, B): the powers of one j are one contiguous batch
        powers = torch.empty((T + 1, B, 2, 6), dtype=torch.int64, device="cuda")
        lhs, rhs = torch.empty_like(out), torch.empty_like(out)

        def reference_way():
            g1.scalar_mul(ctx, exps, cs_rows.reshape(-1, 2, 6), out=powers)
            g1.add(ctx, powers[0], powers[1], out=lhs)
            for j in range(2, T + 1):
                g1.add(ctx, lhs, powers[j], out=lhs)
            g1.commit(ctx, *tabs[8], sh, wi, out=rhs)
            return (lhs == rhs).reshape(B, -1).all(dim=1)

        assert bool(reference_way().all()), "the reference's schedule disagrees"
        ts_r = timed(torch, max(reps // 4, 3), reference_way)
        lines.append(f"verify, the reference's schedule (t + 1 = {T + 1} full-width powers an item, {T} additions, commit, compare: {T + 3} launches)")
        lines.append(f"                  2^{n} items  {fmt(ts_r)}  = {np.median(ts_r) / np.median(ts_v):6.1f} x verify")
        del cs, cs_rows, powers, exps, coef, hat
        torch.cuda.empty_cache()
    write_section("timing", lines)
    print("\n".join(lines))


def main():
    args = sys.argv[1:]
    if "--resources" in args:
        return resources()
    timing(int(args[0]) if args and args[0].isdigit() else 20)


main()

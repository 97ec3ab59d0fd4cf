"""The MSM kernels (csrc/hb_msm.hip): what the compiler made of them, and their timing on the device.  Writes profiles/g1_msm.txt, one section
a mode; a mode rewrites its own section and keeps the other (the form of scratch/time_g1.py and profiles/g1.txt).

   python scratch/time_g1_msm.py --resources    no GPU needed: compiles hb_msm.hip for gfx950 with -Rpass-analysis=kernel-resource-usage and
                                                 reads the code size of every function from the device code object (llvm-readelf)
   python scratch/time_g1_msm.py [reps]         needs the GPU (fails without: there is nothing to fall back to)

Timing: g1.msm with method "direct" and "bucket", and beside them the COMPOSED schedule on the same inputs -- what a caller did before msm
existed: scalar_mul on the operands expanded to M K pairs, then g1.add over halves of the term axis until one point a row is left
(ceil(log2 K) launches; K - 1 calls of add in a row would only be slower).  HIP events around one call, `reps` calls after a warm-up of the
same shape, median (min .. max).  Shapes: M = 64 rows of K in {22, 256, 1024, 4096} over shared bases with random 255-bit scalars; M = 1 with
K in {2^12, 2^16, 2^20}; and M = 64, K = 4096 with ALL scalars equal (every window of every chunk one bucket of 4096 entries: the
heavy-bucket path) next to the uniform input.  The run asserts that the three agree on every shape.
The last lines name the crossover g1.MSM_CROSSOVER is taken from: the smallest K of the M = 64 rows at which bucket beats direct."""
import os
import re
import socket
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "profiles", "g1_msm.txt")
HEADS = {"resources": "## resources", "timing": "## timing"}


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
        f.write("# profiles/g1_msm.txt -- written by scratch/time_g1_msm.py\n")
        for k in ("resources", "timing"):
            f.write("\n".join(sections[k]).rstrip() + "\n\n")


def resources():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(REPO, "honeybadgermpc_amd", "csrc", "hb_msm.hip")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "--no-gpu-bundle-output", "-c", src]
    with tempfile.TemporaryDirectory() as tmp:
        obj = os.path.join(tmp, "hb_msm.co")
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
    lines = ["hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage on csrc/hb_msm.hip; code size: the function's bytes in the device code object.",
             "mont_mul<14> is one function (fq_mul_call), called, not inlined: its bytes are its own row and in no kernel's.",
             "LDS: the tree's 256 nodes of 43 words (44 032 B); k_msm_bucket adds 64 parked heavy sums, the 4096-entry list and the counters.",
             f"{'function':18s} {'VGPRs':>6s} {'AGPRs':>6s} {'SGPRs':>6s} {'scratch B/lane':>15s} {'waves/SIMD':>11s} {'LDS B':>6s} {'code bytes':>11s}"]
    for c in rows:
        lines.append(f"{c['name']:18s} {c.get('VGPRs', '?'):>6s} {c.get('AGPRs', '?'):>6s} {c.get('TotalSGPRs', c.get('SGPRs', '?')):>6s} "
                     f"{c.get('ScratchSize [bytes/lane]', '?'):>15s} {c.get('Occupancy [waves/SIMD]', '?'):>11s} {c.get('LDS Size [bytes/block]', '?'):>6s} "
                     f"{sizes.get(c['name'], 0):>11d}")
    for name, size in sizes.items():
        if not any(c["name"] == name for c in rows):
            lines.append(f"{name:18s} {'':>6s} {'':>6s} {'':>6s} {'':>15s} {'':>11s} {'':>6s} {size:>11d}   (called by every kernel)")
    assert all(c.get("ScratchSize [bytes/lane]") == "0" for c in rows), "an MSM kernel uses scratch memory"
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
        raise SystemExit("scratch/time_g1_msm.py needs the GPU")
    from honeybadgermpc_amd import g1
    from honeybadgermpc_amd._capi import Context
    from honeybadgermpc_amd.bls12_381 import G1, R

    ctx = Context.get(R)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(17)

    def rnd(count):
        return ctx.reduce_(torch.randint(-(1 << 63), (1 << 63) - 1, (count, 4), dtype=torch.int64, device="cuda", generator=gen))

    def composed(sc, pts, M, K, terms):
        """scalar_mul on M K pairs, laid out term-major so that the halves of the term axis are contiguous batches; then add by halves"""
        g1.scalar_mul(ctx, sc, pts, out=terms)
        n = K
        while n > 1:
            h = n // 2
            g1.add(ctx, terms[:h * M], terms[h * M:2 * h * M], out=terms[:h * M])
            if n & 1:
                g1.add(ctx, terms[:M], terms[2 * h * M:n * M], out=terms[:M])
            n = h
        return terms[:M]

    g = G1.generator()
    lines = [f"{reps} calls a figure after a warm-up: median (min .. max); {torch.cuda.get_device_name(0)} on {socket.gethostname()}",
             "composed: scalar_mul on the M K expanded pairs + g1.add by halves of the term axis (1 + about log2 K launches), same inputs, same commit",
             "every call ends in one lane a row: 248 dependent doublings on the bucket path, so about one scalar_mul chain (profiles/g1.txt: 7.8 ms) is the floor"]
    shapes = [(64, 22, False), (64, 256, False), (64, 1024, False), (64, 4096, False), (64, 4096, True), (1, 1 << 12, False), (1, 1 << 16, False), (1, 1 << 20, False)]
    bases = g1.scalar_mul(ctx, rnd(1 << 20), g)
    cross = {}
    for M, K, equal in shapes:
        pts = bases[:K].contiguous()
        sc = rnd(M * K).reshape(M, K, 4)
        if equal:
            sc = sc[:1, :1].expand(M, K, 4).contiguous()
        out = torch.empty((M, 2, 6), dtype=torch.int64, device="cuda")
        # the composed schedule's operands: pair (k, m) at k M + m
        sc_t = sc.transpose(0, 1).contiguous().reshape(K * M, 4)
        pts_t = pts.unsqueeze(1).expand(K, M, 2, 6).contiguous().reshape(K * M, 2, 6)
        terms = torch.empty((K * M, 2, 6), dtype=torch.int64, device="cuda")
        ref = composed(sc_t, pts_t, M, K, terms).clone()
        res = {}
        for method in ("direct", "bucket"):
            assert torch.equal(g1.msm(ctx, sc, pts, method=method), ref), f"{method} disagrees with the composed schedule at M = {M}, K = {K}"
            res[method] = timed(torch, reps, lambda: g1.msm(ctx, sc, pts, out=out, method=method))
        res["composed"] = timed(torch, reps, lambda: composed(sc_t, pts_t, M, K, terms))
        tag = f"M = {M:2d}  K = {K:7d}  {'equal scalars ' if equal else 'random scalars'}"
        for name in ("direct", "bucket", "composed"):
            lines.append(f"{tag}  {name:9s} {fmt(res[name])}" + (f"  = {np.median(res['composed']) / np.median(res[name]):5.2f} x composed" if name != "composed" else ""))
        if M == 64 and not equal:
            cross[K] = np.median(res["bucket"]) < np.median(res["direct"])
        del sc_t, pts_t, terms
        torch.cuda.empty_cache()
    wins = [K for K in sorted(cross) if cross[K]]
    lines.append(f"crossover (g1.MSM_CROSSOVER, hb_msm.hip MSM_AUTO_TERMS): the smallest K of the M = 64 rows at which bucket beats direct: "
                 f"{wins[0] if wins else 'none: direct wins at every measured K'}")
    write_section("timing", lines)
    print("\n".join(lines))


def main():
    args = sys.argv[1:]
    if "--resources" in args:
        return resources()
    timing(int(args[0]) if args and args[0].isdigit() else 20)


main()

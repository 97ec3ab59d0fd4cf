"""The pairing kernel (csrc/hb_pair.hip): what the compiler made of it, and its timing on the device.  Writes profiles/pairing.txt, one section
a mode; a mode rewrites its own section and keeps the other (the form of scratch/time_g1_crs.py and profiles/g1_crs.txt).

   python scratch/time_pairing.py --resources    no GPU needed: compiles hb_pair.hip for gfx950 with -Rpass-analysis=kernel-resource-usage and
                                                  reads the registers, scratch and code size of every function from the device assembly
   python scratch/time_pairing.py [reps]         needs the GPU (fails without: there is nothing to fall back to)

Timing, at 2^12, 2^16 and 2^18 items:
   product_is_one     K = 2: two Miller loops that share their squarings, one final exponentiation, the verdict
   verify_batch       PolyCommitConst at t = 21, ONE index (64) for the batch: the G1 left side (msm_fixed over gs[0] and hs[0], scalar_mul by the
                      index, add, sub, neg) and product_is_one; the left side alone is timed beside it
   yardstick          time a product of Fq: product_is_one's time / (items x PRODUCTS_K2) against k_g1_verify's at the parent commit,
                      2^16 items x 1 935 products in 3.0 ms (profiles/g1.txt)
HIP events around one call, `reps` calls a figure after a warm-up; median (min .. max)."""
import os
import re
import socket
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "profiles", "pairing.txt")
HEADS = {"resources": "## resources", "timing": "## timing"}
# products of Fq an item at K = 2 (the head of csrc/hb_pair.hip counts them): the loop 2 924 K + 2 232, the final exponentiation about 8 350
PRODUCTS_K2 = 2 * 2924 + 2232 + 8350
G1_VERIFY_NS_A_PRODUCT = 3.0e6 / (65536 * 1935)


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
        f.write("# profiles/pairing.txt -- written by scratch/time_pairing.py\n")
        for k in ("resources", "timing"):
            f.write("\n".join(sections[k]).rstrip() + "\n\n")


def resources():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(REPO, "honeybadgermpc_amd", "csrc", "hb_pair.hip")
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "hb_pair.s")
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", src, "-Rpass-analysis=kernel-resource-usage", "-o", asm],
                           capture_output=True, text=True, check=True)
        text = open(asm).read()
    kernel = {}
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?)\s*\[-Rpass", line)
        if m:
            key, _, val = m.group(1).partition(":")
            kernel[key.strip()] = val.strip()
    demangle = lambda n: subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip() or n
    short = lambda n: re.sub(r"\(.*", "", demangle(n)).replace("hb::", "").replace("void ", "")
    lines = ["hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage on csrc/hb_pair.hip.  The kernel's figures include everything it calls;",
             "the functions' own figures are read from the device assembly (a function's registers include its callees').",
             f"{'function':28s} {'VGPRs':>6s} {'AGPRs':>6s} {'scratch B/lane':>15s} {'code bytes':>11s}"]
    for m in re.finditer(r"^(_Z\w+):.*?\n; codeLenInByte = (\d+).*?; NumVgprs: (\d+)\n; NumAgprs: (\d+).*?; ScratchSize: (\d+)", text, re.S | re.M):
        lines.append(f"{short(m.group(1)):28s} {m.group(3):>6s} {m.group(4):>6s} {m.group(5):>15s} {m.group(2):>11s}")
    lines.append(f"k_pair_product as launched: VGPRs {kernel.get('VGPRs')}, AGPRs {kernel.get('AGPRs')}, SGPRs {kernel.get('TotalSGPRs')}, scratch "
                 f"{kernel.get('ScratchSize [bytes/lane]')} B/lane, VGPR spills {kernel.get('VGPRs Spill')}, LDS {kernel.get('LDS Size [bytes/block]')} B, "
                 f"occupancy {kernel.get('Occupancy [waves/SIMD]')} wave(s)/SIMD")
    write_section("resources", lines)
    print("\n".join(lines))


def fmt(ts):
    return f"{np.median(ts) / 1e3:10.2f} ms ({min(ts) / 1e3:.2f} .. {max(ts) / 1e3:.2f})"


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


def timing(reps, sizes):
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("scratch/time_pairing.py needs the GPU")
    from honeybadgermpc_amd import g1, pairing
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd._capi import Context
    from honeybadgermpc_amd.bls12_381 import G1, R
    from honeybadgermpc_amd.bls12_381_pairing import G2
    from honeybadgermpc_amd.poly_commit_const import PolyCommitConst

    ctx = Context.get(R)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(29)

    def rnd(*shape):
        return ctx.reduce_(torch.randint(-(1 << 63), (1 << 63) - 1, (*shape, 4), dtype=torch.int64, device="cuda", generator=gen))

    t, index = 21, 64
    g = G1.generator()
    alpha = 0x5A17C0FFEE5EED0123456789ABCDEF0FEDCBA98765432100112233445566778 % R
    lam = 0x0123456789ABCDEF00112233445566778899AABBCCDDEEFF0F1E2D3C4B5A6978 % R
    powers = ctx.upload_ints([pow(alpha, j, R) for j in range(t + 1)])
    gs, hs = g1.download(g1.scalar_mul(ctx, powers, g)), g1.download(g1.scalar_mul(ctx, powers, g ** lam))
    ghat = G2.generator()
    pc = PolyCommitConst([gs, [ghat, ghat ** alpha], hs], ctx=ctx)
    pc.preprocess_verifier()
    _, _, p0, p1 = pc._verifier_state()
    lines = []

    def emit(text):
        lines.append(text)
        print(text, flush=True)

    emit(f"{reps} calls a figure after a warm-up: median (min .. max); {torch.cuda.get_device_name(0)} on {socket.gethostname()}")
    emit(f"yardstick: k_g1_verify at the parent commit, 2^16 items x 1 935 products of Fq in 3.0 ms = {G1_VERIFY_NS_A_PRODUCT * 1e3:.2f} ps a product")
    for n in sizes:
        # honest openings of the trapdoor CRS: c = (s + lam a + (alpha - i) k) g, w = k g for random s, a, k
        s, a, k = rnd(n), rnd(n), rnd(n)
        e = sa.add(ctx, sa.add(ctx, s, sa.mul(ctx, a, lam)), sa.mul(ctx, k, (alpha - index) % R))
        c, w = g1.scalar_mul(ctx, e, g), g1.scalar_mul(ctx, k, g)
        lhs, nw = pc.verify_lhs(c, index, s, a, w)
        ok, counter = pairing.product_is_one(ctx, [(lhs, p0), (nw, p1)])
        assert bool(ok.all().item()) and int(counter.item()) == 0, "honest openings were rejected"
        bad = s.clone()
        bad[n // 2, 0] ^= 1
        assert pc.verify_batch(c, index, bad, a, w).sum().item() == n - 1, "a wrong share was accepted"
        tp = timed(torch, reps, lambda: pairing.product_is_one(ctx, [(lhs, p0), (nw, p1)]))
        tl = timed(torch, reps, lambda: pc.verify_lhs(c, index, s, a, w))
        tv = timed(torch, reps, lambda: pc.verify_batch(c, index, s, a, w))
        ns = np.median(tp) * 1e3 / (n * PRODUCTS_K2)
        emit(f"items = {n:7d}  product_is_one, K = 2        {fmt(tp)}   {ns * 1e3:8.2f} ps a product of Fq ({PRODUCTS_K2} an item) = "
             f"{ns / G1_VERIFY_NS_A_PRODUCT:5.2f} x k_g1_verify's")
        emit(f"items = {n:7d}  G1 left side, composed       {fmt(tl)}   {np.median(tl) / np.median(tp):6.3f} of product_is_one")
        emit(f"items = {n:7d}  verify_batch, t = 21, i = 64 {fmt(tv)}")
        del s, a, k, e, c, w, lhs, nw
        torch.cuda.empty_cache()
    write_section("timing", lines)


def main():
    args = sys.argv[1:]
    if "--resources" in args:
        return resources()
    nums = [int(a) for a in args if a.isdigit()]
    reps = nums[0] if nums else 5
    sizes = [1 << b for b in nums[1:]] or [1 << 12, 1 << 16, 1 << 18]
    timing(max(reps, 3), sizes)


main()

"""The KZG prover's kernels (csrc/hb_crs.hip): what the compiler made of them, and their timing on the device.  Writes profiles/g1_crs.txt, one
section a mode; a mode rewrites its own section and keeps the other (the form of scratch/time_g1_msm.py and profiles/g1_msm.txt).

   python scratch/time_g1_crs.py --resources    no GPU needed: compiles hb_crs.hip for gfx950 with -Rpass-analysis=kernel-resource-usage and
                                                 reads the code size of every function from the device code object (llvm-readelf)
   python scratch/time_g1_crs.py [reps]         needs the GPU (fails without: there is nothing to fall back to)

Timing, at the dealer's shapes of HbAvssBatch (t = 21, n = 64, B in {16, 1024}), windows 4 and 8:
   commit      rows = B, K = 22 terms a family, two families               g1.msm_fixed against the baseline
   witnesses   rows = B n, K = 21 terms a family, two families            g1.msm_fixed against the baseline; the quotients beside them
   baseline    what the parent commit can do for the same sums: g1.msm over the shared points [gs | hs] with the scalars concatenated,
               method "auto".  For the witnesses the parent has no quotient kernel: the synthetic division in Python ints on the host (its
               upload not counted), timed separately and less often (it takes seconds).
   sweep       split S in {1, 4, 16, 64, 256} and the library's rule (split 0), every shape and window.
HIP events around one call, `reps` >= 10 calls a figure after a warm-up; the table side and the baseline run ALTERNATELY in one process;
median (min .. max).  The run asserts that both sides return the same words on every shape."""
import os
import re
import socket
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "profiles", "g1_crs.txt")
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
        f.write("# profiles/g1_crs.txt -- written by scratch/time_g1_crs.py\n")
        for k in ("resources", "timing"):
            f.write("\n".join(sections[k]).rstrip() + "\n\n")


def resources():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(REPO, "honeybadgermpc_amd", "csrc", "hb_crs.hip")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "--no-gpu-bundle-output", "-c", src]
    with tempfile.TemporaryDirectory() as tmp:
        obj = os.path.join(tmp, "hb_crs.co")
        r = subprocess.run([hipcc] + flags + ["-Rpass-analysis=kernel-resource-usage", "-o", obj], capture_output=True, text=True, check=True)
        readelf = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "llvm-readelf")
        if not os.path.exists(readelf):
            readelf = "/opt/rocm/llvm/bin/llvm-readelf"
        syms = subprocess.run([readelf, "-s", "--wide", "--demangle", obj], capture_output=True, text=True, check=True).stdout
    short = lambda name: re.sub(r"\(.*", "", name).replace("hb::", "").replace("void ", "")
    sizes = {}
    for line in syms.splitlines():
        m = re.match(r"\s*\d+:\s+[0-9a-f]+\s+(\d+)\s+FUNC\s+\S+\s+\S+\s+\S+\s+(.*)", line)
        if m:
            sizes[short(m.group(2))] = int(m.group(1))
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?)\s*\[-Rpass", line)
        if not m:
            continue
        key, _, val = m.group(1).partition(":")
        if key.strip() == "Function Name":
            name = subprocess.run(["c++filt", val.strip()], capture_output=True, text=True).stdout.strip() or val.strip()
            cur = {"name": short(name)}
            rows.append(cur)
        elif cur is not None:
            cur[key.strip()] = val.strip()
    lines = ["hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage on csrc/hb_crs.hip; code size: the function's bytes in the device code object.",
             "mont_mul<14> is one function (fq_mul_call), called, not inlined: its bytes are its own row and in no kernel's.",
             "k_g1_crs_msm<false> is split 1 (no LDS); <true> the split path: the tree's 256 nodes of 43 words (44 032 B).",
             f"{'function':22s} {'VGPRs':>6s} {'AGPRs':>6s} {'SGPRs':>6s} {'scratch B/lane':>15s} {'waves/SIMD':>11s} {'LDS B':>6s} {'code bytes':>11s}"]
    for c in rows:
        lines.append(f"{c['name']:22s} {c.get('VGPRs', '?'):>6s} {c.get('AGPRs', '?'):>6s} {c.get('TotalSGPRs', c.get('SGPRs', '?')):>6s} "
                     f"{c.get('ScratchSize [bytes/lane]', '?'):>15s} {c.get('Occupancy [waves/SIMD]', '?'):>11s} {c.get('LDS Size [bytes/block]', '?'):>6s} "
                     f"{sizes.get(c['name'], 0):>11d}")
    for name, size in sizes.items():
        if not any(c["name"] == name for c in rows):
            lines.append(f"{name:22s} {'':>6s} {'':>6s} {'':>6s} {'':>15s} {'':>11s} {'':>6s} {size:>11d}   (called by every G1 kernel)")
    assert rows and all(c.get("ScratchSize [bytes/lane]") == "0" for c in rows), "a kernel of hb_crs.hip uses scratch memory"
    lines.append("no kernel of hb_crs.hip uses scratch (private) memory")
    write_section("resources", lines)
    print("\n".join(lines))


def fmt(ts):
    return f"{np.median(ts):11.1f} us ({min(ts):.1f} .. {max(ts):.1f})"


def timed(torch, reps, *fns):
    """the functions run alternately: `reps` rounds of one call each -> a list of microseconds a function"""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    evs = [[[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in fns] for _ in range(reps)]
    for rnd in evs:
        for (a, b), fn in zip(rnd, fns):
            a.record()
            fn()
            b.record()
    torch.cuda.synchronize()
    return [[rnd[k][0].elapsed_time(rnd[k][1]) * 1e3 for rnd in evs] for k in range(len(fns))]


def host_quotients(R, phis, xs):
    out = []
    for phi in phis:
        for x in xs:
            acc, q = phi[-1], [0] * (len(phi) - 1)
            for j in range(len(phi) - 2, -1, -1):
                q[j] = acc
                acc = (phi[j] + x * acc) % R
            out.append((q, acc))
    return out


def timing(reps):
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("scratch/time_g1_crs.py needs the GPU")
    from honeybadgermpc_amd import g1
    from honeybadgermpc_amd._capi import Context
    from honeybadgermpc_amd.bls12_381 import G1, R

    reps = max(reps, 10)
    ctx = Context.get(R)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(23)

    def rnd(*shape):
        return ctx.reduce_(torch.randint(-(1 << 63), (1 << 63) - 1, (*shape, 4), dtype=torch.int64, device="cuda", generator=gen))

    t, n = 21, 64
    g = G1.generator()
    alpha = 0x5A17C0FFEE5EED0123456789ABCDEF0FEDCBA98765432100112233445566778 % R
    powers = ctx.upload_ints([pow(alpha, j, R) for j in range(t + 1)])
    gs_dev, hs_dev = g1.scalar_mul(ctx, powers, g), g1.scalar_mul(ctx, powers, G1.rand("h"))
    gs, hs = g1.download(gs_dev), g1.download(hs_dev)
    lines = []

    def emit(text):
        lines.append(text)
        print(text, flush=True)

    for text in [f"{reps} calls a figure after a warm-up, table side and baseline alternately: median (min .. max); {torch.cuda.get_device_name(0)} on {socket.gethostname()}",
             f"t = {t}, n = {n}; commit: rows = B, K = {t + 1}, two families; witnesses: rows = B n, K = {t}, two families",
                 "baseline: g1.msm(method='auto') over the shared points [gs | hs], scalars concatenated (what the parent commit has for these sums);",
                 "  it does not depend on the window: measured alternately with the window 8 tables, and those figures stand beside window 4 too"]:
        emit(text)
    verdict, baseline = [], {}
    inputs = {B: (rnd(B, t + 1), rnd(B, t + 1)) for B in (16, 1024)}
    for window in (8, 4):
        t0 = time.perf_counter()
        tg, th = g1.FixedBases(ctx, gs, window), g1.FixedBases(ctx, hs, window)
        torch.cuda.synchronize()
        emit(f"window {window}: tables of 2 x {t + 1} bases built in {(time.perf_counter() - t0) * 1e3:.1f} ms (two launches), {2 * tg.tables.numel() * 8 / 2 ** 20:.1f} MiB")
        for B in (16, 1024):
            phi, hat = inputs[B]
            xs = ctx.upload_ints(list(range(1, n + 1)))
            (tq,) = timed(torch, reps, lambda: (g1.kzg_quotients(ctx, phi, xs), g1.kzg_quotients(ctx, hat, xs)))
            q, _ = g1.kzg_quotients(ctx, phi, xs)
            qh, _ = g1.kzg_quotients(ctx, hat, xs)
            if window == 8:
                phis = [ctx.download_ints(phi[b]) for b in range(B)]
                hq = []
                for _ in range(3 if B == 16 else 1):
                    t0 = time.perf_counter()
                    ref = host_quotients(R, phis, list(range(1, n + 1)))
                    hq.append((time.perf_counter() - t0) * 1e6)
                assert [v for qq, _ in ref for v in qq] == ctx.download_ints(q.reshape(-1, 4)), "device and host quotients differ"
                emit(f"B = {B:4d}  quotients of phi and hat, two launches      {fmt(tq)}")
                emit(f"B = {B:4d}  baseline quotients: Python ints on the host, ONE polynomial family, {len(hq)} run(s): {min(hq):.0f} us at best (twice that for phi and hat)")
            for what, a, b, K in (("commit   ", phi, hat, t + 1), ("witnesses", q.reshape(B * n, t, 4), qh.reshape(B * n, t, 4), t)):
                rows = int(a.shape[0])
                pts = torch.cat([gs_dev[:K], hs_dev[:K]]).contiguous()
                sc = torch.cat([a, b], dim=1).contiguous()
                out_t = torch.empty((rows, 2, 6), dtype=torch.int64, device="cuda")
                if (B, what) not in baseline:
                    out_b = torch.empty((rows, 2, 6), dtype=torch.int64, device="cuda")
                    tt, tb = timed(torch, reps, lambda: g1.msm_fixed(ctx, tg, a, th, b, out=out_t), lambda: g1.msm(ctx, sc, pts, out=out_b))
                    baseline[(B, what)] = (tb, out_b)
                else:
                    (tt,) = timed(torch, reps, lambda: g1.msm_fixed(ctx, tg, a, th, b, out=out_t))
                    tb, out_b = baseline[(B, what)]
                assert torch.equal(out_t, out_b), f"tables and g1.msm disagree at window {window}, B = {B}, {what}"
                tag = f"window {window}  B = {B:4d}  {what} rows = {rows:6d}"
                emit(f"{tag}  tables (split 0) {fmt(tt)}")
                emit(f"{tag}  baseline g1.msm  {fmt(tb)}  = {np.median(tb) / np.median(tt):7.1f} x tables")
                ok = max(tt) < min(tb)
                verdict.append((tag, ok))
                best = None
                for S in (1, 4, 16, 64, 256):
                    (ts,) = timed(torch, reps, lambda: g1.msm_fixed(ctx, tg, a, th, b, out=out_t, split=S))
                    assert torch.equal(out_t, out_b), f"split {S} disagrees at window {window}, B = {B}, {what}"
                    emit(f"{tag}  split {S:3d}        {fmt(ts)}")
                    if best is None or np.median(ts) < best[1]:
                        best = (S, np.median(ts))
                emit(f"{tag}  best split {best[0]} ({best[1]:.1f} us); the rule's run is {np.median(tt) / best[1]:.2f} x that")
                del out_t, sc
                torch.cuda.empty_cache()
        del tg, th
        torch.cuda.empty_cache()
    emit("check (the tables' slowest run against the baseline's fastest, a shape):")
    for tag, ok in verdict:
        emit(f"  {tag}: {'tables faster in every run' if ok else 'TABLES NOT FASTER IN EVERY RUN'}")
    for text in ['split 0 (hb_crs.hip, CRS_FILL_LANES): the smallest power of two S with rows S >= 262 144 lanes, S <= U and S <= 256.  The starting point was', '  65 536 lanes, one wave a SIMD of the device; under it rows = 1 024 ran at S = 64 and rows = 65 536 at S = 1.  The sweep above has its best', '  split at 256 for 16 and 1 024 rows and at 4 for 65 536 rows, at both windows: 262 144 lanes, the two waves a SIMD these kernels run at,', '  twice over.  The "best split" lines hold the rule against the sweep of the run that wrote this file.']:
        emit(text)
    write_section("timing", lines)


def main():
    args = sys.argv[1:]
    if "--resources" in args:
        return resources()
    timing(int(args[0]) if args and args[0].isdigit() else 10)


main()

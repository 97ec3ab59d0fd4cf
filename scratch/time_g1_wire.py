"""The wire kernels of G1 (csrc/hb_g1_wire.hip): what the compiler made of them, and their timing on the device.  Writes profiles/g1_wire.txt,
one section a mode; a mode rewrites its own section and keeps the other (the form of scratch/time_g1_crs.py and profiles/g1_crs.txt).

   python scratch/time_g1_wire.py --resources    no GPU needed: compiles hb_g1_wire.hip for gfx950 with -Rpass-analysis=kernel-resource-usage and
                                                  reads the code size of every function from the device code object (llvm-readelf)
   python scratch/time_g1_wire.py [reps]         needs the GPU (fails without: there is nothing to fall back to)

Timing, at 2^16 points (the crate's 1000 valid vectors, repeated):
   decompress          g1.decompress with and without check_subgroup, device bytes in
   compress            g1.compress
   in_subgroup         method "order" against method "endomorphism" on the same points, alternately
   baseline            what the parent commit has for bytes from the wire: the host loop bls12_381.G1.decompress over 256 of the encodings and
                       g1.upload of the result, a host clock around each (upload ends in a synchronise), SCALED by 2^16 / 256 -- an estimate,
                       stated as one, not a measurement at 2^16
HIP events around one call, `reps` >= 10 calls a figure after a warm-up, the sides of a comparison ALTERNATELY in one process; median
(min .. max).  The run asserts that compress(decompress(v)) == v, that both methods return the same flags and that every status is 0."""
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
OUT = os.path.join(REPO, "profiles", "g1_wire.txt")
HEADS = {"resources": "## resources", "timing": "## timing"}
# field products an item, counted from hb_g1_wire.hip and hb_g1_elem.hpp
SQRT = 4 + 377 + 106 + 1                                  # the table, the squarings, the products of the schedule, the test
MEMBER = 2 * (63 * 7 + 5 * 16) + 6                        # two passes of 63 doublings and 5 additions, the comparison
DECOMPRESS = 1 + 2 + SQRT + 1 + 2                         # to Montgomery form, x^3, the root, y back for the sign, x and y back for the store
ON_CURVE = 2 + 3                                          # the point to Montgomery form, y^2 and x^3
ORDER = 3805 + ON_CURVE                                   # scalar_mul by R with its inversion (profiles/g1.txt), then on_curve


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
        f.write("# profiles/g1_wire.txt -- written by scratch/time_g1_wire.py\n")
        for k in ("resources", "timing"):
            f.write("\n".join(sections[k]).rstrip() + "\n\n")


def resources():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(REPO, "honeybadgermpc_amd", "csrc", "hb_g1_wire.hip")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "--no-gpu-bundle-output", "-c", src]
    with tempfile.TemporaryDirectory() as tmp:
        obj = os.path.join(tmp, "hb_g1_wire.co")
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
    lines = ["hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage on csrc/hb_g1_wire.hip; code size: the function's bytes in the device code object.",
             "mont_mul<14> is one function (fq_mul_call), called, not inlined: its bytes are its own row and in no kernel's.",
             "VGPRs and AGPRs share one file of 512 a lane: above 256 together a SIMD holds ONE wave of the kernel (the AGPRs hold values the",
             "compiler moved out of the VGPRs: no memory traffic).  The complete Jacobian addition inside the two passes over x is the peak:",
             "with g1_add in place of g1_add_base both long kernels held 256 VGPRs and 7 / 63 AGPRs, one wave a SIMD each.",
             f"{'function':22s} {'VGPRs':>6s} {'AGPRs':>6s} {'SGPRs':>6s} {'scratch B/lane':>15s} {'waves/SIMD':>11s} {'LDS B':>6s} {'code bytes':>11s}"]
    for c in rows:
        lines.append(f"{c['name']:22s} {c.get('VGPRs', '?'):>6s} {c.get('AGPRs', '?'):>6s} {c.get('TotalSGPRs', c.get('SGPRs', '?')):>6s} "
                     f"{c.get('ScratchSize [bytes/lane]', '?'):>15s} {c.get('Occupancy [waves/SIMD]', '?'):>11s} {c.get('LDS Size [bytes/block]', '?'):>6s} "
                     f"{sizes.get(c['name'], 0):>11d}")
    for name, size in sizes.items():
        if not any(c["name"] == name for c in rows):
            lines.append(f"{name:22s} {'':>6s} {'':>6s} {'':>6s} {'':>15s} {'':>11s} {'':>6s} {size:>11d}   (called by every G1 kernel)")
    assert rows and all(c.get("ScratchSize [bytes/lane]") == "0" for c in rows), "a kernel of hb_g1_wire.hip uses scratch memory"
    lines.append("no kernel of hb_g1_wire.hip uses scratch (private) memory")
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


def timing(reps):
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("scratch/time_g1_wire.py needs the GPU")
    from honeybadgermpc_amd import g1
    from honeybadgermpc_amd._capi import Context
    from honeybadgermpc_amd.bls12_381 import G1, R

    reps = max(reps, 10)
    ctx = Context.get(R)
    with open(os.path.join(REPO, "tests", "golden", "g1_compressed_valid_test_vectors.dat"), "rb") as f:
        vectors = f.read()
    N, HOST = 1 << 16, 256
    data = (vectors * (N // 1000 + 1))[:48 * N]
    enc = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(ctx.tdev).reshape(N, 48)
    lines = []

    def emit(text):
        lines.append(text)
        print(text, flush=True)

    emit(f"{reps} calls a figure after a warm-up, the sides of a comparison alternately: median (min .. max); {torch.cuda.get_device_name(0)} on {socket.gethostname()}")
    emit(f"2^16 points: the crate's 1000 valid vectors repeated; 2^16 items are 1024 waves, ONE a SIMD of the device (profiles/g1.txt)")
    emit("products an item: counted from hb_g1_wire.hip (see the head of scratch/time_g1_wire.py)")
    out = torch.empty((N, 2, 6), dtype=torch.int64, device=ctx.tdev)
    t_plain, t_check = timed(torch, reps, lambda: g1.decompress(ctx, enc, out=out), lambda: g1.decompress(ctx, enc, check_subgroup=True, out=out))
    pts, status, rejected = g1.decompress(ctx, enc, check_subgroup=True)
    assert int(rejected.item()) == 0 and not status.any().item(), "a valid vector was rejected"
    back = torch.empty((N, 48), dtype=torch.uint8, device=ctx.tdev)
    (t_comp,) = timed(torch, reps, lambda: g1.compress(ctx, pts, out=back))
    assert torch.equal(back, enc), "compress(decompress(v)) != v"
    t_endo, t_order = timed(torch, reps, lambda: g1.in_subgroup(ctx, pts, method="endomorphism"), lambda: g1.in_subgroup(ctx, pts, method="order"))
    assert torch.equal(g1.in_subgroup(ctx, pts, method="endomorphism"), g1.in_subgroup(ctx, pts, method="order")), "the two methods disagree"
    rate = lambda products, ts: f"{products:5d} products an item  {products * N / np.median(ts) / 1e3:6.1f} G products/s"
    emit(f"decompress                   2^16 items {fmt(t_plain)}  {rate(DECOMPRESS, t_plain)}")
    emit(f"decompress, check_subgroup   2^16 items {fmt(t_check)}  {rate(DECOMPRESS + MEMBER, t_check)}")
    emit(f"compress                     2^16 items {fmt(t_comp)}  no field product: {N * 144 / np.median(t_comp) / 1e3:.1f} GB/s of points in and bytes out")
    emit(f"in_subgroup, endomorphism    2^16 items {fmt(t_endo)}  {rate(ON_CURVE + MEMBER, t_endo)}")
    emit(f"in_subgroup, order           2^16 items {fmt(t_order)}  {rate(ORDER, t_order)}  (scalar_mul, on_curve and the comparison in torch)")
    emit(f"in_subgroup: order / endomorphism = {np.median(t_order) / np.median(t_endo):.2f} x by the medians; "
         + ("endomorphism faster in EVERY run" if max(t_endo) < min(t_order) else "ENDOMORPHISM NOT FASTER IN EVERY RUN"))
    # the parent commit's way, on the host
    some = [data[48 * k:48 * k + 48] for k in range(1, HOST + 1)]
    host = {}
    for name, check in (("G1.decompress", False), ("G1.decompress, check_subgroup", True)):
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            hp = [G1.decompress(v, check_subgroup=check) for v in some]
            ts.append((time.perf_counter() - t0) * 1e6)
        host[name] = ts
    up = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g1.upload(hp, ctx)
        torch.cuda.synchronize()
        up.append((time.perf_counter() - t0) * 1e6)
    emit(f"baseline, the parent commit's way, on the HOST over {HOST} encodings, three runs each, a host clock around the loop (upload: to the synchronise):")
    for name, ts in host.items():
        emit(f"  {name:32s} {np.median(ts) / HOST:9.1f} us a point ({min(ts) / HOST:.1f} .. {max(ts) / HOST:.1f})")
    emit(f"  {'g1.upload':32s} {np.median(up) / HOST:9.1f} us a point ({min(up) / HOST:.1f} .. {max(up) / HOST:.1f})")
    for name, dev in (("G1.decompress", t_plain), ("G1.decompress, check_subgroup", t_check)):
        est = (np.median(host[name]) + np.median(up)) / HOST * N
        emit(f"  SCALED to 2^16 points (an estimate: {HOST} points measured): {name} + upload = {est / 1e6:.1f} s = {est / np.median(dev):.0f} x the device call")
    write_section("timing", lines)


def main():
    args = sys.argv[1:]
    if "--resources" in args:
        return resources()
    timing(int(args[0]) if args and args[0].isdigit() else 10)


main()

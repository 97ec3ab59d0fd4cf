"""The root finder timed on the device:
   python scratch/time_solver.py [reps] [--label TEXT]          (writes profiles/solver.txt)

BLS12-381 Fr, k = 64, 256, 1024 random distinct roots.  One child process a k, each under its own time limit; the first one that fails
or runs out of time ends the script, and nothing is tried again.  For each k:

  roots     solver.roots on the device polynomial: a host clock around the call, which ends in a stream synchronise (hb_rf_roots
            waits once a level and once before it returns), `reps` (at least 5) calls after a warm-up: median (min .. max).  The final
            host sort of solver.roots is inside the figure.
  counts    levels of the split tree, kernel launches and stream waits of one call (hb_debug_rf_stats)
  split     one more call in profile mode (a wait after every stage, so the stages can be charged): chains, GCDs, waits for the degrees
  newton    solver.newton_coefficients_device, HIP events around one launch, 20 runs: median (min .. max); beside it
            power_mixing.newton_coefficients on the host, one run, and whether the two are bit-equal

No GPU: fails (there is nothing to fall back to)."""
import os
import random
import socket
import subprocess
import sys
import time

BLS = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
KS = (64, 256, 1024)
LIMIT_S = {64: 120, 256: 150, 1024: 240}


def fmt(ts, unit="ms"):
    ts = sorted(ts)
    return f"{ts[len(ts) // 2]:10.3f} {unit} ({ts[0]:.3f} .. {ts[-1]:.3f})"


def one(k, reps):
    import numpy as np
    import torch

    sys.path.insert(0, ".")
    from honeybadgermpc_amd import power_mixing, solver
    from honeybadgermpc_amd._capi import Context, np_ptr

    if not torch.cuda.is_available():
        raise SystemExit("scratch/time_solver.py needs the GPU")
    ctx = Context.get(BLS)
    rnd = random.Random(k)
    want = sorted(rnd.sample(range(BLS), k))
    cur, sums = [1] * k, []
    for _ in range(k):
        cur = [c * r % BLS for c, r in zip(cur, want)]
        sums.append(sum(cur) % BLS)
    sums_dev = ctx.upload_ints(sums)
    # ---- Newton
    coeffs = solver.newton_coefficients_device(ctx, sums_dev)
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
    for a, b in evs:
        a.record()
        solver.newton_coefficients_device(ctx, sums_dev)
        b.record()
    torch.cuda.synchronize()
    t_dev = [a.elapsed_time(b) for a, b in evs]
    t0 = time.perf_counter()
    host = power_mixing.newton_coefficients(sums, BLS)
    t_host = (time.perf_counter() - t0) * 1e3
    same = ctx.download_ints(coeffs) == host
    # ---- roots
    stats = np.zeros(8, dtype=np.int64)
    got = solver.roots(ctx, coeffs)                                    # warm-up (code objects, scratch)
    ok = got is not None and ctx.download_ints(got) == want
    ts = []
    for r in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        solver.roots(ctx, coeffs, seed=r)
        ts.append((time.perf_counter() - t0) * 1e3)
    solver.roots(ctx, coeffs)
    ctx.lib.hb_debug_rf_stats(np_ptr(stats))
    levels, launches, waits, rounds = (int(x) for x in stats[:4])
    ctx.lib.hb_debug_rf_profile(1)
    try:
        solver.roots(ctx, coeffs)
        ctx.lib.hb_debug_rf_stats(np_ptr(stats))
    finally:
        ctx.lib.hb_debug_rf_profile(0)
    print(f"k = {k:4d}  roots {fmt(ts)}   {'roots as drawn' if ok else 'MISMATCH'}")
    print(f"          levels {levels}, launches {launches}, stream waits {waits}, rounds of the repeated-root loop {rounds}, nodes over all levels {int(stats[7])}")
    print(f"          profile mode: chains {stats[4] / 1e3:.3f} ms, GCDs and divisions {stats[5] / 1e3:.3f} ms, waits for the degrees {stats[6] / 1e3:.3f} ms")
    print(f"          newton on the device {fmt(t_dev)}   on the host {t_host:.3f} ms   host / device = {t_host / sorted(t_dev)[len(t_dev) // 2]:.1f}   "
          f"{'bit-equal' if same else 'MISMATCH'}", flush=True)
    if not (ok and same):
        raise SystemExit(1)


def main():
    args = sys.argv[1:]
    if "--one" in args:
        return one(int(args[args.index("--one") + 1]), int(args[args.index("--reps") + 1]))
    reps = max(5, int(args[0])) if args and args[0].isdigit() else 5
    label = args[args.index("--label") + 1] if "--label" in args else "working tree"
    lines = [f"# scratch/time_solver.py, BLS12-381 Fr, random distinct roots, {reps} calls a roots figure: median (min .. max); {socket.gethostname()}; {label}"]
    os.makedirs("profiles", exist_ok=True)
    for k in KS:
        try:
            r = subprocess.run([sys.executable, sys.argv[0], "--one", str(k), "--reps", str(reps)], capture_output=True, text=True, timeout=LIMIT_S[k])
        except subprocess.TimeoutExpired:
            lines.append(f"k = {k}: no result within {LIMIT_S[k]} s; stopped here")
            break
        lines += r.stdout.rstrip().splitlines()
        if r.returncode != 0:
            lines.append(f"k = {k}: exit status {r.returncode}; stopped here")
            lines += r.stderr.rstrip().splitlines()[-5:]
            break
    text = "\n".join(lines) + "\n"
    with open("profiles/solver.txt", "w") as f:
        f.write(text)
    sys.stdout.write(text)
    if "stopped here" in text:
        raise SystemExit(1)


main()

"""Times the fused launches of csrc/hb_fxexp.hip beside the same steps composed from what the package had, at BLS12-381, (64, 32, 32),
g = 8 and g = 4, with 2^12 and 2^16 elements, alternating fused and composed in one process; and one whole exp2 of 2^12 elements among
four parties in one process.  Writes profiles/fixedpoint_exp.txt.

    python scratch/time_fixedpoint_exp.py [reps] [--label TEXT] [--out PATH]

finish_lookup_mask: the last level of the widest fraction group ((4, 4) at g = 8, (2, 2) at g = 4) against demux_finish + demux.lookup
+ share_arithmetic.sub, with the bytes the algorithm needs (PQ once, the opened rows and the triple's factors once, the kept factor and
its masked row) over the kernel time as a share of the 8 TB/s HBM peak.  products_trunc: against beaver_combine + trunc_mask a product.
tree_step: against trunc_pr_finish + sub a value.  Medians and the spread (min .. max) of `reps` timings by device events."""
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))

BLS = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
HBM_PEAK = 8.0e12


def timed(torch, fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return out


def alternate(torch, fused, composed, reps):
    fused(), composed()
    f, c = [], []
    for _ in range(reps):
        f += timed(torch, fused, 1)
        c += timed(torch, composed, 1)
    fmt = lambda v: f"{statistics.median(v):9.1f} us ({min(v):.1f} .. {max(v):.1f})"
    return statistics.median(f), f"fused {fmt(f)}   composed {fmt(c)}   composed / fused {statistics.median(c) / statistics.median(f):5.2f}"


def main():
    import bitdec_cases as bc
    import exp_cases as ec

    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd._capi import Context
    from honeybadgermpc_amd.progs import demux as dx
    from honeybadgermpc_amd.progs import fixedpoint as fx
    from honeybadgermpc_amd.progs import fixedpoint_exp as fe

    reps = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 15
    label = sys.argv[sys.argv.index("--label") + 1] if "--label" in sys.argv else ""
    ctx = Context.get(BLS)
    torch, L, p = ctx.torch, ctx.n_limbs, BLS
    k, f, kappa = 64, 32, 32
    width, s = fe.exp2_width(k), k + fe.GUARD_BITS
    nb = width + kappa
    lines = [f"fixed-point exponential, BLS12-381, (k, f, kappa) = ({k}, {f}, {kappa}), {reps} alternating repetitions {label}".rstrip()]
    for g in (8, 4):
        w = fe.exp2_groups(k, f, g)[-1][1]
        _, wl, wh = dx.demux_plan(w)[-1].merges[0]
        table = fe.exp2_tables(k, f, g)[-2]
        tdev, _ = fe.table_rows(ctx, [table])
        for count in (1 << 12, 1 << 16):
            rows, entries = (1 << wl) + (1 << wh), 1 << w
            opened, ta, tab = bc.random_tensor(ctx, 1, count, rows=rows), bc.random_tensor(ctx, 2, count, rows=rows), bc.random_tensor(ctx, 3, count, rows=entries)
            nxt = (bc.random_tensor(ctx, 4, count, rows=1), bc.random_tensor(ctx, 5, count, rows=1))
            store = dx.demux_groups(ctx, w, count)
            masked, kept = torch.empty((2, count, L), dtype=torch.int64, device=ctx.tdev), torch.empty((1, count, L), dtype=torch.int64, device=ctx.tdev)
            level = dx.demux_levels(w) - 1
            fused = lambda: fe.finish_lookup_mask(ctx, [(wl, wh, 0, 0, 0, 0)], tdev, 1, 1, count, opened=opened, ta=ta, tab=tab, nxt=nxt, out=masked, kept_out=kept)
            cols = [[t] for t in table]

            def composed():
                onehot = dx.demux_finish(ctx, opened, store, level, ta, tab)
                return sa.sub(ctx, dx.lookup(ctx, onehot, cols)[0], nxt[0][0])

            assert torch.equal(fused()[0][0], composed())
            med, text = alternate(torch, fused, composed, reps)
            need = 32 * count * (entries + 2 * rows + 1 + 2)
            lines.append(f"finish_lookup_mask g = {g} ({wl}, {wh}) count 2^{count.bit_length() - 1}: {text}   {need / 1e6:.1f} MB needed, {need / (med * 1e-6) / HBM_PEAK:.1%} of the HBM peak")
            for products in (1, 2, 4):
                o2, a, b, ab = bc.random_tensor(ctx, 6, count, rows=2 * products), *(bc.random_tensor(ctx, 7 + i, count, rows=products) for i in range(3))
                planes = bc.random_tensor(ctx, 10, count, rows=products * nb)
                fused = lambda: fe.products_trunc(ctx, o2, a, b, ab, planes, width, s, kappa)

                def composed():
                    out = []
                    for r in range(products):
                        v = sa.beaver_combine(ctx, o2[2 * r], o2[2 * r + 1], a[r], b[r], ab[r])
                        out.append(fx.trunc_mask(ctx, v, planes[r * nb:(r + 1) * nb], width, s, kappa)[0])
                    return out

                assert torch.equal(fused()[0][products - 1], composed()[-1])
                lines.append(f"products_trunc {products} product(s) count 2^{count.bit_length() - 1}: {alternate(torch, fused, composed, reps)[1]}")
                sv, zero = bc.random_tensor(ctx, 11, count, rows=products), ctx.upload_ints([0] * count)
                carry = bc.random_tensor(ctx, 12, count)
                pairs = (products + 1) // 2
                fused = lambda: fe.tree_step(ctx, o2[:products], sv, s, a[:pairs], b[:pairs], carry=carry if products & 1 else None)

                def composed():
                    vals = [fx.trunc_pr_finish(ctx, sv[j], o2[j], zero, s) for j in range(products)] + ([carry] if products & 1 else [])
                    return [sa.sub(ctx, v, (a if i % 2 == 0 else b)[i // 2]) for i, v in enumerate(vals)]

                assert torch.equal(fused()[0][0], composed()[0])
                lines.append(f"tree_step {products} row(s) count 2^{count.bit_length() - 1}: {alternate(torch, fused, composed, reps)[1]}")
    # one whole exp2 among four parties
    n, t, count, g = 4, 1, 1 << 12, 8
    rnd = random.Random(5)
    lay = fe.exp2_layout(k, f, kappa, g)
    widths = [w for _, w in lay["groups"]] + [(k - 3).bit_length() + 1]
    xs = [rnd.randrange(-(40 << f), 29 << f) for _ in range(count)]
    bit_rows = [[rnd.getrandbits(1) for _ in range(count)] for _ in range(lay["n_planes"])]
    starts = ec.truncation_planes(lay, kappa)
    r1s = [[sum(bit_rows[st + i][e] << i for i in range(s)) for st in starts] for e in range(count)]
    ta, tb = ([[rnd.randrange(p) for _ in range(count)] for _ in range(lay["n_triples"])] for _ in range(2))
    tab = [[x * y % p for x, y in zip(ra, rb)] for ra, rb in zip(ta, tb)]
    bits = bc.deal_planes(ctx, rnd, p, n, t, bit_rows)
    trip = [bc.deal_planes(ctx, rnd, p, n, t, v) for v in (ta, tb, tab)]
    demux_prep = ec.deal_demux_triples(ctx, fe, dx, rnd, p, n, t, lay, widths, count)
    vals = bc.deal_planes(ctx, rnd, p, n, t, [[x % p for x in xs]])
    took = []

    async def body(co, i):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = await fe.exp2(co, vals[i][0], bits[i], tuple(tr[i] for tr in trip), demux_prep[i], f, k, kappa, g)
        torch.cuda.synchronize()
        took.append(time.perf_counter() - t0)
        return ctx.download_ints(await co.open_share_array(out))

    results = bc.run_parties(p, n, t, set(), rnd, body)
    assert results[0] == [fe.exp2_model(xs[e], p, k, f, r1s[e], g) for e in range(count)]
    lines.append(f"exp2 of 2^12 elements among four parties in one process, g = 8, {lay['opens']} opens: {max(took):.2f} s (opens to exp2_model)")
    text = "\n".join(lines) + "\n"
    print(text)
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "fixedpoint_exp.txt")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()

"""Times the fused launches of csrc/hb_fxtrig.hip beside the same steps composed from what the package had, at BLS12-381, (64, 32, 32),
with 2^12, 2^16 and 2^20 elements, alternating the variants in one process; the lookup at every lane split, and beside
hb_fxexp_finish_lookup_mask on ONE table of the same merge (the yardstick for "two tables for little more than one"); and one whole
sincos_turns of 2^12 elements among four parties in one process.  Writes profiles/fixedpoint_trig.txt.

    python scratch/time_fixedpoint_trig.py [reps] [--label TEXT] [--out PATH] [--counts 12,16,20]

finish_lookup_mask: the last level of a group of g = 8 bits ((4, 4), 256 entries a table) and of g = 4 bits ((2, 2)) against demux_finish +
two demux.lookup + the subs of the three masked rows, with the bytes the algorithm needs (PQ once, the opened rows and the triple's
factors once, two kept rows, three masked rows and their triples) over the time as a share of the 8 TB/s HBM peak.  cproducts_trunc:
against three beaver_combine, the subs and two trunc_mask a product.  tree_step: against trunc_pr_finish and the adds and subs of the
masked rows a value.  Medians and the spread (min .. max) of `reps` timings between device events around the Python call; every
compared pair is checked bit-equal first."""
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))

BLS = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
HBM_PEAK = 8.0e12


def timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def alternate(torch, variants, reps):
    """variants: {name: callable}, run in turn `reps` times after one warm-up each -> ({name: median us}, text)"""
    for fn in variants.values():
        fn()
    took = {name: [] for name in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            took[name].append(timed(torch, fn))
    med = {name: statistics.median(v) for name, v in took.items()}
    first = next(iter(variants))
    text = "   ".join(f"{name} {med[name]:9.1f} us ({min(v):.1f} .. {max(v):.1f})" + ("" if name == first else f" [{med[name] / med[first]:5.2f} x {first}]") for name, v in took.items())
    return med, text


def device_rows(ctx, seed, rows, count):
    """canonical residues made on the device: three full limbs and a top limb below 2^62, below the 255-bit modulus"""
    torch = ctx.torch
    gen = torch.Generator(device=ctx.tdev)
    gen.manual_seed(seed)
    return torch.randint(0, 1 << 62, (rows, count, ctx.n_limbs), dtype=torch.int64, device=ctx.tdev, generator=gen)


def main():
    import bitdec_cases as bc
    import exp_cases as ec
    import trig_cases as tc

    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd._capi import Context
    from honeybadgermpc_amd.progs import demux as dx
    from honeybadgermpc_amd.progs import fixedpoint as fx
    from honeybadgermpc_amd.progs import fixedpoint_exp as fe
    from honeybadgermpc_amd.progs import fixedpoint_trig as ft

    reps = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 11
    label = sys.argv[sys.argv.index("--label") + 1] if "--label" in sys.argv else ""
    logs = [int(v) for v in sys.argv[sys.argv.index("--counts") + 1].split(",")] if "--counts" in sys.argv else [12, 16, 20]
    ctx = Context.get(BLS)
    torch, L, p = ctx.torch, ctx.n_limbs, BLS
    k, f, kappa = 64, 32, 32
    width, s = ft.trig_width(k, f), f + ft.TRIG_GUARD
    nb = width + kappa
    lines = [f"fixed-point sine and cosine, BLS12-381, (k, f, kappa) = ({k}, {f}, {kappa}), {reps} alternating repetitions {label}".rstrip()]
    for g in (8, 4):
        o, w = ft.trig_groups(k, f, g)[-1]                                   # the top group: signed entries
        _, wl, wh = dx.demux_plan(w)[-1].merges[0]
        ctab, stab = ft.trig_tables(k, f, g)[-1]
        tdev, _ = fe.table_rows(ctx, [ctab + stab])
        cdev, _ = fe.table_rows(ctx, [ctab])
        ccols, scols = [[t % p] for t in ctab], [[t % p] for t in stab]
        level = dx.demux_levels(w) - 1
        for log in logs:
            count = 1 << log
            rows, entries = (1 << wl) + (1 << wh), 1 << w
            opened, ta, tab = device_rows(ctx, 1, rows, count), device_rows(ctx, 2, rows, count), device_rows(ctx, 3, entries, count)
            nxt = (device_rows(ctx, 4, 3, count), device_rows(ctx, 5, 3, count))
            store = dx.demux_groups(ctx, w, count)
            masked, kept = torch.empty((6, count, L), dtype=torch.int64, device=ctx.tdev), torch.empty((2, count, L), dtype=torch.int64, device=ctx.tdev)
            m1, k1 = torch.empty((2, count, L), dtype=torch.int64, device=ctx.tdev), torch.empty((1, count, L), dtype=torch.int64, device=ctx.tdev)
            desc = [(wl, wh, 0, 0, 0, 0)]

            def composed():
                onehot = dx.demux_finish(ctx, opened, store, level, ta, tab)
                re, im = dx.lookup(ctx, onehot, ccols)[0], dx.lookup(ctx, onehot, scols)[0]
                return [sa.sub(ctx, re, nxt[0][0]), sa.sub(ctx, im, nxt[0][1]), sa.sub(ctx, sa.add(ctx, re, im), nxt[0][2])], re, im

            variants = {f"split {sp}": (lambda sp=sp: ft.finish_lookup_mask(ctx, desc, tdev, 1, 1, count, split=sp, opened=opened, ta=ta, tab=tab, nxt=nxt, out=masked, kept_out=kept))
                        for sp in ft.SPLITS}
            cm, cre, cim = composed()
            for name, fn in variants.items():                                   # every compared pair bit-equal
                mk, kp = fn()
                assert torch.equal(kp[0], cre) and torch.equal(kp[1], cim) and all(torch.equal(mk[2 * t], cm[t]) for t in range(3)), name
            one = lambda: fe.finish_lookup_mask(ctx, desc, cdev, 1, 1, count, opened=opened, ta=ta, tab=tab, nxt=(nxt[0][:1], nxt[1][:1]), out=m1, kept_out=k1)
            assert torch.equal(one()[1][0], cre)
            variants["composed"] = composed
            variants["fxexp, one table"] = one
            med, text = alternate(torch, variants, reps)
            best = min(ft.SPLITS, key=lambda sp: med[f"split {sp}"])
            need = 32 * count * (entries + 2 * rows + 2 + 3 + 3)
            lines.append(f"finish_lookup_mask g = {g} ({wl}, {wh}) count 2^{log}: {text}   best split {best}; {need / 1e6:.1f} MB needed, "
                         f"{need / (med[f'split {best}'] * 1e-6) / HBM_PEAK:.1%} of the HBM peak at it; the rule's split here is {ft.lookup_split(count)}")
            del opened, ta, tab, store, cm, cre, cim
            if g == 4:
                continue
            for products in (1, 2, 4):
                o6, a, b, ab = device_rows(ctx, 6, 6 * products, count), *(device_rows(ctx, 7 + i, 3 * products, count) for i in range(3))
                planes = bc.random_tensor(ctx, 10, count, rows=1).expand(2 * products * nb, count, L).contiguous() if log > 16 else bc.random_tensor(ctx, 10, count, rows=2 * products * nb)
                fused = lambda: ft.cproducts_trunc(ctx, products, ft.MODE_BOTH, o6, a, b, ab, planes, width, s, kappa)

                def composed():
                    out = []
                    for q in range(products):
                        pr = [sa.beaver_combine(ctx, o6[2 * r], o6[2 * r + 1], a[r], b[r], ab[r]) for r in range(3 * q, 3 * q + 3)]
                        for c, v in enumerate((sa.sub(ctx, pr[0], pr[1]), sa.sub(ctx, sa.sub(ctx, pr[2], pr[0]), pr[1]))):
                            out.append(fx.trunc_mask(ctx, v, planes[(2 * q + c) * nb:(2 * q + c + 1) * nb], width, s, kappa)[0])
                    return out

                got, want = fused()[0], composed()
                assert all(torch.equal(got[r], want[r]) for r in range(2 * products))
                lines.append(f"cproducts_trunc {products} product(s) count 2^{log}: {alternate(torch, {'fused': fused, 'composed': composed}, reps)[1]}")
                sv, zero = device_rows(ctx, 11, 2 * products, count), ctx.upload_ints([0] * count)
                carry = device_rows(ctx, 12, 2, count)
                values = products + (products & 1)
                pairs = values // 2
                fused = lambda: ft.tree_step(ctx, o6[:2 * products], sv, s, mode=ft.MODE_BOTH, ta=a[:3 * pairs], tb=b[:3 * pairs], carry=carry if products & 1 else None)

                def composed():
                    t = [fx.trunc_pr_finish(ctx, sv[j], o6[j], zero, s) for j in range(2 * products)]
                    vals = [(t[2 * u], t[2 * u + 1]) for u in range(products)] + ([(carry[0], carry[1])] if products & 1 else [])
                    out = []
                    for u, (re, im) in enumerate(vals):
                        trip = b if u & 1 else a
                        out += [sa.sub(ctx, v, trip[3 * (u >> 1) + i]) for i, v in enumerate((re, im, sa.add(ctx, re, im)))]
                    return out

                got, want = fused()[0], composed()
                assert all(torch.equal(got[2 * (3 * (u >> 1) + i) + (u & 1)], want[3 * u + i]) for u in range(values) for i in range(3))
                lines.append(f"tree_step {products} complex value(s) count 2^{log}: {alternate(torch, {'fused': fused, 'composed': composed}, reps)[1]}")
                del o6, a, b, ab, planes, sv, carry
    # one whole sincos_turns among four parties
    n, t, count, g = 4, 1, 1 << 12, 8
    rnd = random.Random(5)
    lay = ft.trig_layout(k, f, kappa, g)
    limits = ft.trig_shifts(k, f, g)
    xs = [rnd.randrange(-(1 << (k - 1)), 1 << (k - 1)) for _ in range(count)]
    bit_rows = [[rnd.getrandbits(1) for _ in range(count)] for _ in range(lay["n_planes"])]
    starts = [st for st, _ in tc.truncation_planes(lay, kappa)]
    r1s = [[sum(bit_rows[st + i][e] << i for i in range(m)) for st, m in zip(starts, limits)] for e in range(count)]
    ta, tb = ([[rnd.randrange(p) for _ in range(count)] for _ in range(lay["n_triples"])] for _ in range(2))
    tab = [[x * y % p for x, y in zip(ra, rb)] for ra, rb in zip(ta, tb)]
    bits = bc.deal_planes(ctx, rnd, p, n, t, bit_rows)
    trip = [bc.deal_planes(ctx, rnd, p, n, t, v) for v in (ta, tb, tab)]
    demux_prep = ec.deal_demux_triples(ctx, ft, dx, rnd, p, n, t, lay, [w for _, w in lay["groups"]], count)
    vals = bc.deal_planes(ctx, rnd, p, n, t, [[x % p for x in xs]])
    took = []

    async def body(co, i):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = await ft.sincos_turns(co, vals[i][0], bits[i], tuple(tr[i] for tr in trip), demux_prep[i], f, k, kappa, g)
        torch.cuda.synchronize()
        took.append(time.perf_counter() - t0)
        return [ctx.download_ints(await co.open_share_array(v)) for v in out]

    results = bc.run_parties(p, n, t, set(), rnd, body)
    assert list(zip(*results[0])) == [ft.sincos_turns_model(xs[e], p, k, f, r1s[e], g) for e in range(count)]
    lines.append(f"sincos_turns of 2^12 elements among four parties in one process, g = 8, {lay['opens']} opens: {max(took):.2f} s (opens to sincos_turns_model)")
    text = "\n".join(lines) + "\n"
    print(text)
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "fixedpoint_trig.txt")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()

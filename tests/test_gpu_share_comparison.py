"""GPU: honeybadgermpc_amd.share_comparison -- the kernels of csrc/hb_eq.hip against Python ints, against the `ok` flag of the
Tonelli-Shanks kernel behind ntl.sqrt_mod and, bit for bit, against the same steps composed from share_arithmetic, and the whole
protocol over an OpenCoalescer: equal and is_zero open to the host model's value in the stated number of batches, in both modes, the
reference's recorded runs among them, and a zero c is drawn again from the spare rows.  Exact equality everywhere."""
import asyncio
import json
import os
import random

import numpy as np
import pytest

from conftest import BLS, REPO

pytestmark = pytest.mark.gpu

GOLDILOCKS = 0xFFFFFFFF00000001
P64 = (1 << 64) - 59
P256 = (1 << 256) - 189
FIELDS = [BLS, P256, P64, GOLDILOCKS]
FIELD_IDS = ["bls", "2^256-189", "2^64-59", "goldilocks"]
COUNTS = (0, 1, 255, 256, 257, 5000)
ROWS = (1, 3, 32)


def _ctx(p):
    from honeybadgermpc_amd._capi import Context

    return Context.get(p)


def _random_tensor(ctx, seed, count, rows=None):
    """uniform canonical residues made on the device side (numpy limbs, reduced by hb_reduce)"""
    g = np.random.default_rng(seed)
    n = count if rows is None else rows * count
    limbs = g.integers(-(1 << 63), (1 << 63) - 1, size=(n, ctx.n_limbs), dtype=np.int64, endpoint=True)
    t = ctx.reduce_(ctx.to_device(limbs))
    return t if rows is None else t.view(rows, count, ctx.n_limbs)


def _bit_tensor(ctx, seed, rows, count):
    g = np.random.default_rng(seed)
    limbs = np.zeros((rows * count, ctx.n_limbs), dtype=np.int64)
    limbs[:, 0] = g.integers(0, 2, size=rows * count)
    return ctx.to_device(limbs).view(rows, count, ctx.n_limbs)


def _ints(ctx, t):
    return ctx.download_ints(t.reshape(-1, ctx.n_limbs))


def _rows(ctx, t):
    """(rows, count, limbs) -> [row][element] ints"""
    flat, count = _ints(ctx, t), t.shape[1]
    return [flat[r * count:(r + 1) * count] for r in range(t.shape[0])]


def _sample(count):
    return list(range(count)) if count <= 257 else sorted({0, 1, 2, 3, 4, 255, 256, 257, count - 1} | set(random.Random(count).sample(range(count), 40)))


def _const(ctx, v, like):
    """the residue v in every element of a tensor shaped like `like`"""
    return ctx.upload_ints([v % ctx.modulus]).expand(like.numel() // ctx.n_limbs, ctx.n_limbs).contiguous().view(like.shape)


# ---- the kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", FIELDS, ids=FIELD_IDS)
def test_legendre_kernel(p):
    from honeybadgermpc_amd import share_comparison as sc

    ctx = _ctx(p)
    torch = ctx.torch
    nr = sc.smallest_nonresidue(p)
    corners = [0, 1, p - 1, nr, nr * nr % p]
    for count in COUNTS:
        a = _random_tensor(ctx, 7 + count, count)
        if count >= 255:
            a[:5] = ctx.upload_ints(corners)
        keep = a.clone()
        got = sc.legendre(ctx, a)
        assert got.dtype == torch.int8 and tuple(got.shape) == (count,) and torch.equal(a, keep)
        if not count:
            continue
        sel = torch.tensor(_sample(count), device=ctx.tdev)
        assert got.index_select(0, sel).tolist() == [sc.legendre_mod_p(v, p) for v in ctx.download_ints(a.index_select(0, sel))], count
        if count >= 255:
            assert got[:5].tolist() == [0, 1, sc.legendre_mod_p(p - 1, p), -1, 1]
        # the whole array against code that is independent and already on the device: Tonelli-Shanks says `ok` for 1 and 0
        root, ok = ctx.empty(count), torch.zeros(count, dtype=torch.uint8, device=ctx.tdev)
        ctx.check(ctx.lib.hb_sqrt_mod(ctx.h, ctx.ptr(a), count, ctx.ptr(root), ctx.ptr(ok), ctx.stream()), "hb_sqrt_mod")
        assert torch.equal(got >= 0, ok.bool()) and set(got.tolist()) <= {-1, 0, 1}, count
        assert torch.equal(got == 0, (a == 0).all(dim=1))


@pytest.mark.parametrize("p", FIELDS, ids=FIELD_IDS)
def test_fused_kernels_equal_their_compositions(p):
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd import share_comparison as sc

    ctx = _ctx(p)
    torch = ctx.torch
    nr = sc.smallest_nonresidue(p)
    g = (nr - 1) * pow(2, -1, p) % p
    for rows in ROWS:
        for count in COUNTS:
            s = 100 * rows + count
            x, y = _random_tensor(ctx, s, count), _random_tensor(ctx, s + 1, count)
            if count >= 255:
                y[:3] = x[:3]
            r, rp, bits = _random_tensor(ctx, s + 2, count, rows), _random_tensor(ctx, s + 3, count, rows), _bit_tensor(ctx, s + 4, rows, count)
            ta, tb, tc = (tuple(_random_tensor(ctx, s + 5 + 3 * k + j, count, rows) for j in range(3)) for k in range(3))
            inputs = [x, y, r, rp, bits, *ta, *tb, *tc]
            keep = [v.clone() for v in inputs]
            flat = lambda t: t.reshape(-1, ctx.n_limbs)                                     # noqa: E731
            for yy in (y, None):
                diff = sa.sub(ctx, x, y) if yy is not None else x
                drows = diff.unsqueeze(0).expand(rows, count, ctx.n_limbs).contiguous()
                masked = sc.eq_mask1(ctx, x, yy, r, rp, ta[0], ta[1], tb[0], tb[1])
                assert tuple(masked.shape) == (4, rows, count, ctx.n_limbs)
                want = [sa.sub(ctx, flat(a), flat(b)) for a, b in ((drows, ta[0]), (r, ta[1]), (rp, tb[0]), (rp, tb[1]))]
                assert torch.equal(flat(masked), torch.cat(want)), (rows, count, yy is None)
            opened = _random_tensor(ctx, s + 20, count, 4 * rows).view(4, rows, count, ctx.n_limbs)
            masked2, dr = sc.eq_mid(ctx, opened, ta, tb, bits, tc[0], tc[1], nr)
            want_dr = sa.beaver_combine(ctx, flat(opened[0]), flat(opened[1]), *(flat(v) for v in ta))
            rp2 = sa.beaver_combine(ctx, flat(opened[2]), flat(opened[3]), *(flat(v) for v in tb))
            _b = sa.sub(ctx, _const(ctx, nr, flat(bits)), sa.mul(ctx, flat(bits), nr - 1))
            assert torch.equal(flat(dr), want_dr) and tuple(dr.shape) == (rows, count, ctx.n_limbs)
            assert torch.equal(flat(masked2), torch.cat((sa.sub(ctx, _b, flat(tc[0])), sa.sub(ctx, rp2, flat(tc[1]))))), (rows, count)
            opened2 = _random_tensor(ctx, s + 21, count, 2 * rows).view(2, rows, count, ctx.n_limbs)
            c_share = sc.eq_cshare(ctx, opened2, dr, tc)
            assert torch.equal(flat(c_share), sa.add(ctx, want_dr, sa.beaver_combine(ctx, flat(opened2[0]), flat(opened2[1]), *(flat(v) for v in tc)))), (rows, count)
            # the finish: c any residue, the corners in front, a zero in the last row too
            c = _random_tensor(ctx, s + 22, count, rows)
            want_zero = [0] * rows
            if count >= 255:
                c[0, :3] = ctx.upload_ints([0, 1, p - 1])
                c[rows - 1, 200] = 0
                want_zero[0] = want_zero[rows - 1] = 1
            leg = sc.legendre(ctx, c).view(rows * count, 1)
            b = flat(bits)
            zero, one = _const(ctx, 0, b), _const(ctx, 1, b)
            for mode in (sc.BIT, sc.REFERENCE):
                if mode == sc.BIT:
                    pos, neg = b, sa.sub(ctx, one, b)
                else:
                    gb = sa.mul(ctx, b, g)
                    pos, neg = sa.sub(ctx, _const(ctx, g + 1, b), gb), sa.sub(ctx, gb, _const(ctx, g, b))
                got, zero_rows = sc.eq_finish(ctx, c, bits, mode, nr)
                assert torch.equal(flat(got), torch.where(leg > 0, pos, torch.where(leg < 0, neg, zero))), (rows, count, mode)
                assert zero_rows.dtype == torch.int32 and zero_rows.tolist() == want_zero
            if count:
                sel = _sample(count)
                cs, bs, fs = _rows(ctx, c), _rows(ctx, bits), _rows(ctx, got)
                for e in sel[:12]:
                    L = sc.legendre_mod_p(cs[rows - 1][e], p)
                    assert fs[rows - 1][e] == (0 if L == 0 else L * (nr + L) * pow(2, -1, p) - L * g * bs[rows - 1][e]) % p
            assert all(torch.equal(a, b) for a, b in zip(inputs, keep)), "inputs were written"


def test_arguments_are_checked():
    from honeybadgermpc_amd import share_comparison as sc

    ctx = _ctx(BLS)
    rows, count = 3, 9
    x = _random_tensor(ctx, 1, count)
    pl = [_random_tensor(ctx, 2 + k, count, rows) for k in range(6)]
    with pytest.raises(ValueError):
        sc.eq_mask1(ctx, x[:4], None, *pl)
    with pytest.raises(ValueError):
        sc.eq_mask1(ctx, x, x, pl[0], pl[1][:2], *pl[2:])
    with pytest.raises(ValueError):
        sc.eq_mid(ctx, _random_tensor(ctx, 9, count, 4 * rows), tuple(pl[:3]), tuple(pl[3:]), pl[0], pl[1], pl[2], nr=4)       # a square
    with pytest.raises(ValueError):
        sc.eq_mid(ctx, _random_tensor(ctx, 9, count, 3 * rows), tuple(pl[:3]), tuple(pl[3:]), pl[0], pl[1], pl[2])
    with pytest.raises(ValueError):
        sc.eq_cshare(ctx, _random_tensor(ctx, 9, count, 2 * rows), pl[0], (pl[1], pl[2]))
    with pytest.raises(ValueError):
        sc.eq_finish(ctx, pl[0], pl[1], mode=2)
    with pytest.raises(TypeError):
        sc.legendre(ctx, x.cpu().numpy())
    st, P = ctx.stream(), ctx.ptr
    out = ctx.torch.zeros(count, dtype=ctx.torch.int8, device=ctx.tdev)
    assert ctx.lib.hb_legendre(ctx.h, None, P(out), count, st) == 2 and ctx.lib.hb_legendre(ctx.h, P(x), P(out), -1, st) == 2
    assert ctx.lib.hb_legendre(ctx.h, None, None, 0, st) == 0
    buf = ctx.torch.zeros((rows, count, ctx.n_limbs), dtype=ctx.torch.int64, device=ctx.tdev)
    zr = ctx.torch.zeros(rows, dtype=ctx.torch.int32, device=ctx.tdev)
    assert ctx.lib.hb_eq_finish(ctx.h, P(pl[0]), P(pl[1]), 7, None, P(buf), P(zr), rows, count, st) == 2
    assert ctx.lib.hb_eq_finish(ctx.h, P(pl[0]), P(pl[1]), sc.BIT, None, P(buf), P(zr), 0, count, st) == 2
    assert ctx.lib.hb_eq_cshare(ctx.h, P(pl[0]), P(pl[1]), P(pl[2]), P(pl[3]), P(pl[4]), P(pl[2]), 1, count, st) == 2         # c over an input
    ctx.torch.cuda.synchronize()
    assert not buf.any()


# ---- the protocol, end to end over the in-process tagged network of tests/test_gpu_fixedpoint.py (restated) ----------------
class _TaggedNet:
    def __init__(self, n):
        self.n, self.q = n, [dict() for _ in range(n)]

    def _queue(self, party, tag):
        return self.q[party].setdefault(tag, asyncio.Queue())

    def get_send_recv(self, i):
        def factory(tag):
            def send(dest, msg):
                self._queue(dest, tag).put_nowait((i, msg))

            return send, self._queue(i, tag).get

        return factory


def _run_parties(p, n, t, body):
    from honeybadgermpc_amd.open_coalescer import OpenCoalescer

    async def party(i, net):
        return await body(OpenCoalescer(p, n, t, i, net.get_send_recv(i)), i)

    async def main():
        net = _TaggedNet(n)
        return await asyncio.gather(*[party(i, net) for i in range(n)])

    results = asyncio.run(main())
    _ctx(p).torch.cuda.synchronize()
    return results


def _deal(ctx, seed, values, n):
    """degree-1 Shamir shares of a tensor of values at the points 1..n, dealt on the device: value + point * slope"""
    from honeybadgermpc_amd import share_arithmetic as sa

    flat = values.reshape(-1, ctx.n_limbs)
    slope = _random_tensor(ctx, seed, flat.shape[0])
    return [sa.add(ctx, flat, sa.mul(ctx, slope, i + 1)).view(values.shape) for i in range(n)]


def _preprocessing(ctx, seed, kappa, count, spare=0, rows_from=None):
    """-> (values, dealt): bits, rands and the triple planes for kappa test bits, `spare` spare test bits and the tree.
    rows_from: {"bits": [[...]], "rands": [[...]]} fixes the first rows (the reference's recorded draws)."""
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd import share_comparison as sc

    nb, nr_, nt = kappa + spare, 2 * kappa + 2 * spare, sc.equality_triples(kappa) + 3 * spare
    bits, rands = _bit_tensor(ctx, seed, nb, count), _random_tensor(ctx, seed + 1, count, nr_)
    if rows_from:
        bits[:kappa] = ctx.upload_ints([v for row in rows_from["bits"] for v in row]).view(kappa, count, ctx.n_limbs)
        rands[:2 * kappa] = ctx.upload_ints([v for row in rows_from["rands"] for v in row]).view(2 * kappa, count, ctx.n_limbs)
    tp, tq = _random_tensor(ctx, seed + 2, count, nt), _random_tensor(ctx, seed + 3, count, nt)
    tpq = sa.mul(ctx, tp.view(-1, ctx.n_limbs), tq.view(-1, ctx.n_limbs)).view(tp.shape)
    return bits, rands, (tp, tq, tpq)


def _model(ctx, sc, xs, ys, bits, rands, kappa, nr, mode, rows=None, stop_at_zero=False):
    """equal_model for every element from the dealt values; rows: which plane each test bit uses (default 0..kappa-1)"""
    p = ctx.modulus
    b, r = _rows(ctx, bits), _rows(ctx, rands)
    rows = rows or [(j, j, kappa + j) for j in range(kappa)]
    out = []
    for e, (x, y) in enumerate(zip(xs, ys)):
        acc = 1
        for jb, jr, jrp in rows:
            _, f = sc.test_bit_model((x - y) % p, b[jb][e], r[jr][e], r[jrp][e], p, nr, mode)
            assert f is not None
            acc = acc * f % p
            if stop_at_zero and acc == 0:
                break
        out.append(acc)
    return out


def _protocol(p, kappa, count, seed, modes, n=4, t=1, against_zero=False):
    from honeybadgermpc_amd import share_comparison as sc

    ctx = _ctx(p)
    nr = sc.smallest_nonresidue(p)
    x, y = _random_tensor(ctx, seed, count), _random_tensor(ctx, seed + 1, count)
    if against_zero:
        y = ctx.torch.zeros_like(x)
        x[::2] = 0
    else:
        y[::2] = x[::2]                                                 # equal and unequal pairs mixed; element 0 is an equal pair
    bits, rands, trip = _preprocessing(ctx, seed + 2, kappa, count)
    xs, ys = ctx.download_ints(x), ctx.download_ints(y)
    dx, dy, dbits, drands = (_deal(ctx, seed + 10 + k, v, n) for k, v in enumerate((x, y, bits, rands)))
    dtrip = [_deal(ctx, seed + 20 + k, v, n) for k, v in enumerate(trip)]

    async def body(co, i):
        got = {}
        keep = (dx[i].clone(), dbits[i].clone(), drands[i].clone(), dtrip[i][2].clone()) if i == 0 else None
        for mode in modes:
            before = co.batches
            tr = tuple(v[i] for v in dtrip)
            if against_zero:
                shares = await sc.is_zero(co, dx[i], dbits[i], drands[i], tr, kappa, None, mode)
            else:
                shares = await sc.equal(co, dx[i], dy[i], dbits[i], drands[i], tr, kappa, nr, mode)
            batches = co.batches - before
            got[mode] = (ctx.download_ints(await co.open_share_array(shares)), batches)
        if keep:
            assert all(ctx.torch.equal(a, b) for a, b in zip(keep, (dx[i], dbits[i], drands[i], dtrip[i][2])))
        return got

    results = _run_parties(p, n, t, body)
    for mode in modes:
        want = _model(ctx, sc, xs, ys, bits, rands, kappa, nr, mode)
        for got in results:
            assert got[mode] == (want, sc.equality_opens(kappa)), (kappa, count, mode)
        if mode == sc.BIT:
            assert all(w == 1 for w, a, b in zip(want, xs, ys) if a == b) and set(want) <= {0, 1}


@pytest.mark.parametrize("kappa", (1, 2, 3, 5, 32))
@pytest.mark.parametrize("count", (1, 257))
def test_equal_opens_to_the_model(kappa, count):
    from honeybadgermpc_amd import share_comparison as sc

    _protocol(BLS, kappa, count, 1000 * kappa + count, (sc.BIT, sc.REFERENCE))


@pytest.mark.parametrize("kappa, count", [(1, 1), (3, 257), (32, 1)])
def test_equal_narrow_field_and_is_zero(kappa, count):
    from honeybadgermpc_amd import share_comparison as sc

    _protocol(P64, kappa, count, 64 + kappa, (sc.BIT, sc.REFERENCE))
    _protocol(P64 if kappa == 3 else BLS, kappa, count, 99 + kappa, (sc.BIT,), against_zero=True)


def test_equal_is_one_and_unequal_is_zero_at_kappa_32():
    """5000 pairs, BIT mode.  The seed is one for which the host model alone gives 1 for every equal pair and 0 for every unequal
    one (an unequal pair survives kappa = 32 test bits with probability 2^-32): asserted here before the device is asked."""
    from honeybadgermpc_amd import share_comparison as sc

    p, kappa, count, n, seed = BLS, 32, 5000, 4, 5032
    ctx = _ctx(p)
    x, y = _random_tensor(ctx, seed, count), _random_tensor(ctx, seed + 1, count)
    y[::4] = x[::4]
    bits, rands, trip = _preprocessing(ctx, seed + 2, kappa, count)
    xs, ys = ctx.download_ints(x), ctx.download_ints(y)
    want = _model(ctx, sc, xs, ys, bits, rands, kappa, 5, sc.BIT, stop_at_zero=True)
    assert want == [1 if a == b else 0 for a, b in zip(xs, ys)] and sum(want) == 1250
    dx, dy, dbits, drands = (_deal(ctx, seed + 10 + k, v, n) for k, v in enumerate((x, y, bits, rands)))
    dtrip = [_deal(ctx, seed + 20 + k, v, n) for k, v in enumerate(trip)]

    async def body(co, i):
        shares = await sc.equal(co, dx[i], dy[i], dbits[i], drands[i], tuple(v[i] for v in dtrip))
        return ctx.download_ints(await co.open_share_array(shares)), co.batches

    for got in _run_parties(p, n, 1, body):
        assert got == (want, sc.equality_opens(kappa) + 1)


def test_reference_runs_are_replayed():
    """the reference's recorded _prog runs, their draws shared out freshly: REFERENCE mode opens to the reference's result"""
    from honeybadgermpc_amd import share_comparison as sc

    with open(os.path.join(REPO, "tests", "golden", "share_comparison.json")) as f:
        cases = json.load(f)["equal"]
    p, n = BLS, 4
    ctx = _ctx(p)
    for kappa in (1, 2, 3, 5, 32):
        group = [c for c in cases if c["kappa"] == kappa]
        count = len(group)
        assert count >= 4
        x, y = ctx.upload_ints([int(c["x"]) for c in group]), ctx.upload_ints([int(c["y"]) for c in group])
        rows_from = {"bits": [[int(c["bits"][j]) for c in group] for j in range(kappa)],
                     "rands": [[int(c["rs"][j]) for c in group] for j in range(kappa)] + [[int(c["rps"][j]) for c in group] for j in range(kappa)]}
        bits, rands, trip = _preprocessing(ctx, 300 + kappa, kappa, count, rows_from=rows_from)
        dx, dy, dbits, drands = (_deal(ctx, 310 + k, v, n) for k, v in enumerate((x, y, bits, rands)))
        dtrip = [_deal(ctx, 320 + k, v, n) for k, v in enumerate(trip)]

        async def body(co, i):
            shares = await sc.equal(co, dx[i], dy[i], dbits[i], drands[i], tuple(v[i] for v in dtrip), kappa, 5, sc.REFERENCE)
            return ctx.download_ints(await co.open_share_array(shares))

        for got in _run_parties(p, n, 1, body):
            assert got == [int(c["out"]) for c in group], kappa


def test_a_zero_c_is_drawn_again_from_the_spare_rows():
    """crafted preprocessing: diff = 0 and rp = 0 for one element in row 1, so that c opens to 0 there -- ordinary data"""
    from honeybadgermpc_amd import share_comparison as sc
    from honeybadgermpc_amd.exceptions import PreprocessingExhausted

    p, kappa, count, n, e = BLS, 3, 5, 4, 2
    ctx = _ctx(p)
    for mode in (sc.BIT, sc.REFERENCE):
        x, y = _random_tensor(ctx, 70, count), _random_tensor(ctx, 71, count)
        y[e] = x[e]
        bits, rands, trip = _preprocessing(ctx, 72, kappa, count, spare=1)
        rands[kappa + 1, e] = 0                                          # rp of test bit 1
        xs, ys = ctx.download_ints(x), ctx.download_ints(y)
        assert sc.test_bit_model(0, 1, 5, 0, p, 5, mode) == (0, None)
        # the spare test bit: bits row kappa, r = rands row 2 kappa, rp = rands row 2 kappa + 1, in the place of test bit 1
        want = _model(ctx, sc, xs, ys, bits, rands, kappa, 5, mode, rows=[(0, 0, kappa), (kappa, 2 * kappa, 2 * kappa + 1), (2, 2, kappa + 2)])
        dx, dy, dbits, drands = (_deal(ctx, 80 + k, v, n) for k, v in enumerate((x, y, bits, rands)))
        dtrip = [_deal(ctx, 90 + k, v, n) for k, v in enumerate(trip)]

        async def body(co, i):
            tr = tuple(v[i] for v in dtrip)
            shares = await sc.equal(co, dx[i], dy[i], dbits[i], drands[i], tr, kappa, 5, mode)
            batches = co.batches
            opened = ctx.download_ints(await co.open_share_array(shares))
            short = (dbits[i][:kappa], drands[i], tr) if i % 2 else (dbits[i], drands[i], tuple(v[:sc.equality_triples(kappa) + 2] for v in tr))
            with pytest.raises(PreprocessingExhausted, match=r"\[1\]"):
                await sc.equal(co, dx[i], dy[i], short[0], short[1], short[2], kappa, 5, mode)
            return opened, batches

        for got in _run_parties(p, n, 1, body):
            assert got == (want, sc.equality_opens(kappa) + 3), mode


@pytest.mark.parametrize("count", (1, 257))
@pytest.mark.parametrize("p", (BLS, P64), ids=("bls", "2^64-59"))
def test_every_step_equals_the_host_self_test(p, count):
    """One row body: for every step of csrc/hb_eq.hip the device's output equals, bit for bit, what hb_selftest_eq computes on the host
    from the same random inputs -- the self test runs the rows the kernels run, addressing included.  rows = 3, so a plane (rows *
    count) and a row (count) are different offsets; the first mask with and without y; the c share into a fresh array and into dr;
    the finish in both modes with one c of the middle row forced to 0: zero_rows = [0, 1, 0] and that element's factor is 0.
    count 1 is one partial workgroup, 257 a second workgroup that holds one element."""
    import selftest_cases as stc
    from honeybadgermpc_amd import share_comparison as sc

    ctx = _ctx(p)
    torch, nl, rows = ctx.torch, ctx.n_limbs, 3
    LEGENDRE, MASK1, MID, CSHARE, FINISH = range(5)
    nr = sc.smallest_nonresidue(p)
    seeds = iter(range(600, 700))

    def rnd(n_rows=None):
        return _random_tensor(ctx, next(seeds), count, n_rows)

    def host(what, operands, out_rows, mode=sc.BIT):
        rc, outs = stc.run_eq(p, nl, what, [o if o is None or isinstance(o, list) else _ints(ctx, o) for o in operands], rows, mode, out_rows, count)
        assert rc == 0
        return outs

    def same(dev, want):
        return torch.equal(dev.reshape(-1, nl), ctx.upload_ints(want))

    x, y = rnd(), rnd()
    assert sc.legendre(ctx, x).tolist() == host(LEGENDRE, [x], ["i8"])[0]
    r, rp, bits = rnd(rows), rnd(rows), rnd(rows)
    ta, tb, tc = ((rnd(rows), rnd(rows), rnd(rows)) for _ in range(3))
    for yy in (y, None):
        assert same(sc.eq_mask1(ctx, x, yy, r, rp, ta[0], ta[1], tb[0], tb[1]), host(MASK1, [x, yy, r, rp, ta[0], ta[1], tb[0], tb[1]], [4 * rows])[0])
    opened = rnd(4 * rows)
    masked2, dr = sc.eq_mid(ctx, opened, ta, tb, bits, tc[0], tc[1], nr)
    h = host(MID, [opened, *ta, *tb, bits, tc[0], tc[1], [nr]], [2 * rows, rows])
    assert same(masked2, h[0]) and same(dr, h[1])
    opened2 = rnd(2 * rows)
    want = host(CSHARE, [opened2, dr, *tc], [rows])[0]
    assert same(sc.eq_cshare(ctx, opened2, dr, tc), want)
    in_place = dr.clone()                                                 # c = dr, the permitted alias
    ctx.check(ctx.lib.hb_eq_cshare(ctx.h, ctx.ptr(opened2.view(-1, nl)), ctx.ptr(in_place), *(ctx.ptr(t) for t in tc), ctx.ptr(in_place), rows, count, ctx.stream()),
              "hb_eq_cshare")
    assert same(in_place, want)
    c = rnd(rows)
    c[1, count // 2] = 0
    for mode in (sc.BIT, sc.REFERENCE):
        factor, zero_rows = sc.eq_finish(ctx, c, bits, mode, nr)
        h = host(FINISH, [c, bits, [nr]], [rows, "zr"], mode)
        assert same(factor, h[0]) and zero_rows.tolist() == h[1] == [0, 1, 0], mode
        assert _ints(ctx, factor[1, count // 2]) == [0]

"""GPU: honeybadgermpc_amd.progs.sorting -- the three kernels of csrc/hb_sort.hip bit for bit against the host self test of the same
rows (hb_selftest_sort) and against the same steps composed from index_select, share_arithmetic and fixedpoint calls (what a caller
had to write before), and the whole sort among four parties over an OpenCoalescer against sort_model: keys and payload columns, the
number of batches, the sizes of the preprocessing.  Exact equality everywhere."""
import asyncio
import random

import numpy as np
import pytest

import sort_cases as sc
from conftest import BLS

pytestmark = pytest.mark.gpu

GOLDILOCKS = 0xFFFFFFFF00000001
P64 = (1 << 64) - 59
P256 = (1 << 256) - 189
FIELDS = [BLS, P256, P64, GOLDILOCKS]                 # the four fields of test_gpu_fixedpoint.py
FIELD_IDS = ["bls", "2^256-189", "2^64-59", "goldilocks"]
# (n, layer, batch): 0, 1, 255, 256 and 257 slots -- one partial workgroup, a full one, a second one that holds one slot -- reached
# with batch over a small n, then layers of n = 13 with a = 3, 1, 0, r = 0 and r = p and counts 5, 3, 6
KERNEL_CASES = [(2, (0, 0, 1, 0), 1), (2, (0, 0, 1, 1), 1), (5, (0, 1, 3, 1), 255), (5, (1, 0, 2, 2), 128), (5, (1, 2, 2, 1), 257),
                (13, (3, 0, 8, 5), 3), (13, (1, 2, 6, 3), 2), (13, (0, 1, 1, 6), 3)]


def _ctx(p):
    from honeybadgermpc_amd._capi import Context

    return Context.get(p)


def _random_tensor(ctx, seed, count, rows=None):
    """uniform canonical residues made on the device side (numpy limbs, reduced by hb_reduce)"""
    g = np.random.default_rng(seed)
    n = count if rows is None else rows * count
    limbs = g.integers(-(1 << 63), (1 << 63) - 1, size=(n, ctx.n_limbs), dtype=np.int64, endpoint=True)
    t = ctx.reduce_(ctx.to_device(limbs)) if n else ctx.empty(0)
    return t if rows is None else t.view(rows, count, ctx.n_limbs)


def _ints(ctx, t):
    return ctx.download_ints(t.reshape(-1, ctx.n_limbs))


def test_kernel_cases_are_layers_of_the_network():
    from honeybadgermpc_amd.progs import sorting as so

    for n, layer, _ in KERNEL_CASES:
        assert layer in so.layers(n) or (layer[3] == 0 and layer[:3] + (1,) in so.layers(n))


@pytest.mark.parametrize("width", (1, 3))
@pytest.mark.parametrize("p", FIELDS, ids=FIELD_IDS)
def test_kernels_equal_the_self_test_rows_and_the_composition(p, width):
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd.progs import fixedpoint as fx
    from honeybadgermpc_amd.progs import sorting as so

    ctx = _ctx(p)
    torch, nl = ctx.torch, ctx.n_limbs
    k, kappa = (64, 32) if p >> 64 else (16, 16)
    m = k - 1
    for case, (n, layer, batch) in enumerate(KERNEL_CASES):
        slots, plane, seed = batch * layer[3], batch * n, 1000 * case + 10 * width
        table, bits = _random_tensor(ctx, seed, plane, rows=width), _random_tensor(ctx, seed + 1, slots, rows=k + kappa)
        c, carry = _random_tensor(ctx, seed + 2, slots), _random_tensor(ctx, seed + 3, slots)
        tp, tq, tpq = (_random_tensor(ctx, seed + 4 + s, slots, rows=width) for s in range(3))
        opened = _random_tensor(ctx, seed + 7, slots, rows=2 * width)
        ops = [table, bits, c, carry, tp, tq, tpq, opened]
        keep = [t.clone() for t in ops]
        ti, args = sc.unflat(_ints(ctx, table), width), (n, batch, width, layer, k, kappa)

        def host(what, operands, outs):
            rc, res = sc.run_sort(p, nl, what, operands, *args, outs)
            assert rc == 0
            return res

        # before the first open
        masked, r1 = so.cmp_mask(ctx, table, layer, n, batch, bits, k, kappa)
        assert tuple(masked.shape) == tuple(r1.shape) == (slots, nl)
        h = host(sc.CMP_MASK, [_ints(ctx, table), _ints(ctx, bits)], [slots, slots])
        assert _ints(ctx, masked) == h[0] and _ints(ctx, r1) == h[1], (n, layer, batch)
        # after the tree's root
        out = so.swap_mask(ctx, table, layer, n, batch, c, r1, carry, tp, tq, k)
        assert tuple(out.shape) == (2 * width, slots, nl)
        h = host(sc.SWAP_MASK, [_ints(ctx, table), _ints(ctx, c), _ints(ctx, r1), _ints(ctx, carry), _ints(ctx, tp), _ints(ctx, tq), [pow(2, -m, p)]], [2 * width * slots])
        assert _ints(ctx, out) == h[0], (n, layer, batch)
        # after the second open: in place
        work = table.clone()
        assert so.swap_finish(ctx, work, layer, n, batch, opened, tp, tq, tpq) is work
        h = host(sc.SWAP_FINISH, [_ints(ctx, opened), _ints(ctx, tp), _ints(ctx, tq), _ints(ctx, tpq)], [_ints(ctx, table)])
        assert _ints(ctx, work) == h[0], (n, layer, batch)
        assert all(torch.equal(t, cp) for t, cp in zip(ops, keep))
        if not slots:
            assert torch.equal(work, table)
            continue
        # the composition a caller had to write: two gathers, sub, the lt pipeline's steps, the affine map, a Beaver product a column, two scatters
        rows = [sc.slot_rows(s, n, layer) for s in range(slots)]
        lo, hi = (torch.tensor([r[j] for r in rows], device=ctx.tdev) for j in (0, 1))
        diffs = [sa.sub(ctx, table[w].index_select(0, lo), table[w].index_select(0, hi)) for w in range(width)]
        want_masked, want_r1 = fx.trunc_mask(ctx, diffs[0], bits, k, m, kappa)
        assert torch.equal(masked, want_masked) and torch.equal(r1, want_r1), (n, layer, batch)
        u = sa.add(ctx, sa.neg(ctx, fx.div2m_finish(ctx, diffs[0], c, r1, carry, m, fx.NEG_TRUNC)), 1)
        for w in range(width):
            assert torch.equal(out[2 * w], sa.sub(ctx, u, tp[w])) and torch.equal(out[2 * w + 1], sa.sub(ctx, diffs[w], tq[w])), (n, layer, batch, w)
            prod = sa.beaver_combine(ctx, opened[2 * w], opened[2 * w + 1], tp[w], tq[w], tpq[w])
            col = table[w].clone()
            col.index_copy_(0, lo, sa.sub(ctx, table[w].index_select(0, lo), prod))
            col.index_copy_(0, hi, sa.add(ctx, table[w].index_select(0, hi), prod))
            assert torch.equal(work[w], col), (n, layer, batch, w)
        # the formulas on Python ints, at a sample of the slots
        want = sc.swap_finish_model(p, ti, sc.unflat(_ints(ctx, opened), 2 * width), *(sc.unflat(_ints(ctx, v), width) for v in (tp, tq, tpq)), n, batch, layer)
        assert _ints(ctx, work) == sc.flat(want)


def test_out_given_arguments_checked_and_streams():
    from honeybadgermpc_amd._capi import HB_ERR_BAD_ARG
    from honeybadgermpc_amd.progs import sorting as so

    p, n, batch, width, k, kappa = BLS, 13, 40, 2, 64, 32
    layer = (1, 0, 2, 6)
    assert layer in so.layers(n)
    ctx = _ctx(p)
    torch, nl = ctx.torch, ctx.n_limbs
    slots, plane = batch * layer[3], batch * n
    table, bits = _random_tensor(ctx, 1, plane, rows=width), _random_tensor(ctx, 2, slots, rows=k + kappa + 1)     # a plane more than needed is fine
    c, carry = _random_tensor(ctx, 3, slots), _random_tensor(ctx, 4, slots)
    tp, tq, tpq = (_random_tensor(ctx, 5 + s, slots, rows=width) for s in range(3))
    opened = _random_tensor(ctx, 8, slots, rows=2 * width)
    masked, r1 = so.cmp_mask(ctx, table, layer, n, batch, bits, k, kappa)
    out = so.swap_mask(ctx, table, layer, n, batch, c, r1, carry, tp, tq, k)
    done = so.swap_finish(ctx, table.clone(), layer, n, batch, opened.view(-1, nl), tp, tq, tpq)                   # opened flat, as an open returns it
    # out given: written where asked, and handed back; on a side stream
    b1, b2, b3 = ctx.empty(slots), ctx.empty(slots), torch.empty_like(out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = so.cmp_mask(ctx, table, layer, n, batch, bits, k, kappa, out=b1, r1_out=b2)
        got3 = so.swap_mask(ctx, table, layer, n, batch, c, b2, carry, tp, tq, k, out=b3)
        work = so.swap_finish(ctx, table.clone(), layer, n, batch, opened, tp, tq, tpq)
    side.synchronize()
    assert got[0] is b1 and got[1] is b2 and torch.equal(b1, masked) and torch.equal(b2, r1)
    assert got3.data_ptr() == b3.data_ptr() and torch.equal(b3, out) and torch.equal(work, done)
    # a strided table is read as its values; in place it is refused
    wide = torch.zeros((width, plane, 2, nl), dtype=torch.int64, device=ctx.tdev)
    wide[:, :, 0] = table
    assert torch.equal(so.cmp_mask(ctx, wide[:, :, 0], layer, n, batch, bits, k, kappa)[0], masked)
    seven = b1.fill_(7).clone()
    bad_calls = [
        lambda: so.cmp_mask(ctx, table, (0, 0, 2, 1), n, batch, bits, k, kappa, out=b1),                      # d is no odd multiple of 2^a
        lambda: so.cmp_mask(ctx, table, (1, 0, 2, 7), n, batch, bits, k, kappa, out=b1),                      # a comparator too many
        lambda: so.cmp_mask(ctx, table, (1, 1, 2, 6), n, batch, bits, k, kappa, out=b1),
        lambda: so.cmp_mask(ctx, table, layer[:3], n, batch, bits, k, kappa, out=b1),
        lambda: so.cmp_mask(ctx, table, layer, n, batch + 1, bits, k, kappa, out=b1),
        lambda: so.cmp_mask(ctx, table[:, :-1], layer, n, batch, bits, k, kappa, out=b1),
        lambda: so.cmp_mask(ctx, table[0], layer, n, batch, bits, k, kappa, out=b1),
        lambda: so.cmp_mask(ctx, table, layer, n, batch, bits[:k + kappa - 1], k, kappa, out=b1),
        lambda: so.cmp_mask(ctx, table, layer, n, batch, bits[:, :-1], k, kappa, out=b1),
        lambda: so.cmp_mask(ctx, table, layer, n, batch, bits, 222, kappa, out=b1),                           # would wrap
        lambda: so.cmp_mask(ctx, table, layer, n, batch, bits, 1, kappa, out=b1),
        lambda: so.cmp_mask(ctx, table, layer, n, batch, bits, k, kappa, out=b1, r1_out=b1),
        lambda: so.cmp_mask(ctx, table, layer, n, batch, bits, k, kappa, out=b1[:-1]),
        lambda: so.cmp_mask(ctx, table.cpu(), layer, n, batch, bits, k, kappa, out=b1),
        lambda: so.swap_mask(ctx, table, layer, n, batch, c[:-1], r1, carry, tp, tq, k, out=b3),
        lambda: so.swap_mask(ctx, table, layer, n, batch, c, r1, carry, tp[:1], tq, k, out=b3),
        lambda: so.swap_mask(ctx, table, layer, n, batch, c, r1, carry, tp, tq[:, :-1], k, out=b3),
        lambda: so.swap_mask(ctx, table, layer, n, batch, c, r1, carry, tp, tq, k, out=b3[:-1]),
        lambda: so.swap_finish(ctx, wide[:, :, 0], layer, n, batch, opened, tp, tq, tpq),                     # not contiguous: cannot be updated in place
        lambda: so.swap_finish(ctx, table, layer, n, batch, opened[:-1], tp, tq, tpq),
        lambda: so.swap_finish(ctx, table, layer, n, batch, opened, tp, tq, tpq[:, :-1]),
        lambda: so.swap_finish(ctx, table, (1, 0, 2, 7), n, batch, opened, tp, tq, tpq),
    ]
    keep = table.clone()
    for i, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"bad call {i} was accepted")
    with pytest.raises(TypeError):
        so.cmp_mask(ctx, table.to(torch.int32), layer, n, batch, bits, k, kappa)
    # ... and the C ABI refuses what gets past Python
    lib, st, P = ctx.lib, ctx.stream(), ctx.ptr
    a, r, d, cnt = layer
    inv = ctx.host_elems([pow(2, -(k - 1), p)])
    big = ctx.host_elems([0])
    big[:] = np.frombuffer(int(p).to_bytes(32, "little"), dtype=np.uint64)
    assert lib.hb_sort_cmp_mask(ctx.h, P(table), n, batch, a, r, d, cnt, P(bits), k, kappa, P(b1), P(b2), st) == 0
    assert torch.equal(b1, masked)
    b1.fill_(7)
    assert lib.hb_sort_cmp_mask(ctx.h, P(table), n, batch, a, r, d, cnt + 1, P(bits), k, kappa, P(b1), P(b2), st) == HB_ERR_BAD_ARG
    assert lib.hb_sort_cmp_mask(ctx.h, P(table), n, batch, a, r, 4, cnt, P(bits), k, kappa, P(b1), P(b2), st) == HB_ERR_BAD_ARG
    assert lib.hb_sort_cmp_mask(ctx.h, P(table), n, 0, a, r, d, cnt, P(bits), k, kappa, P(b1), P(b2), st) == HB_ERR_BAD_ARG
    assert lib.hb_sort_cmp_mask(ctx.h, P(table), 1, batch, a, r, d, cnt, P(bits), k, kappa, P(b1), P(b2), st) == HB_ERR_BAD_ARG
    assert lib.hb_sort_cmp_mask(ctx.h, P(table), n, batch, a, r, d, cnt, P(bits), k, 190, P(b1), P(b2), st) == HB_ERR_BAD_ARG
    assert lib.hb_sort_cmp_mask(ctx.h, P(table), n, batch, a, r, d, cnt, None, k, kappa, P(b1), P(b2), st) == HB_ERR_BAD_ARG
    assert lib.hb_sort_cmp_mask(ctx.h, P(table), n, batch, a, r, d, cnt, P(bits), k, kappa, P(b1), P(b1), st) == HB_ERR_BAD_ARG
    assert lib.hb_sort_cmp_mask(ctx.h, P(table), n, batch, a, r, d, cnt, P(bits), k, kappa, P(table), P(b2), st) == HB_ERR_BAD_ARG      # masked over the table
    assert lib.hb_sort_cmp_mask(ctx.h, P(table), n, batch, a, r, d, cnt, P(bits), k, kappa, P(b1), P(bits), st) == HB_ERR_BAD_ARG
    sm = [P(c), P(r1), P(carry), P(tp), P(tq)]
    assert lib.hb_sort_swap_mask(ctx.h, P(table), 0, n, batch, a, r, d, cnt, *sm, k, inv.ctypes.data, P(b3), st) == HB_ERR_BAD_ARG
    assert lib.hb_sort_swap_mask(ctx.h, P(table), 257, n, batch, a, r, d, cnt, *sm, k, inv.ctypes.data, P(b3), st) == HB_ERR_BAD_ARG
    assert lib.hb_sort_swap_mask(ctx.h, P(table), width, n, batch, a, r, d, cnt, *sm, k, None, P(b3), st) == HB_ERR_BAD_ARG
    assert lib.hb_sort_swap_mask(ctx.h, P(table), width, n, batch, a, r, d, cnt, *sm, k, big.ctypes.data, P(b3), st) == HB_ERR_BAD_ARG
    assert lib.hb_sort_swap_mask(ctx.h, P(table), width, n, batch, a, r, d, cnt, *sm, k, inv.ctypes.data, P(tp), st) == HB_ERR_BAD_ARG  # out over an operand
    assert lib.hb_sort_swap_mask(ctx.h, P(table), width, n, batch, a, r, d, cnt, *sm, k, inv.ctypes.data, P(table), st) == HB_ERR_BAD_ARG
    assert lib.hb_sort_swap_mask(ctx.h, P(table), width, n, batch, a, r, d, cnt, *sm[:4], None, k, inv.ctypes.data, P(b3), st) == HB_ERR_BAD_ARG
    sf = [P(opened), P(tp), P(tq), P(tpq)]
    assert lib.hb_sort_swap_finish(ctx.h, None, width, n, batch, a, r, d, cnt, *sf, st) == HB_ERR_BAD_ARG
    assert lib.hb_sort_swap_finish(ctx.h, P(table), width, n, batch, a, r, d, cnt, P(table), *sf[1:], st) == HB_ERR_BAD_ARG           # the table over an operand
    assert lib.hb_sort_swap_finish(ctx.h, P(table), width, n, batch, a, 1, d, cnt, *sf, st) == HB_ERR_BAD_ARG
    assert lib.hb_sort_swap_finish(ctx.h, P(table), width, n, batch, a, r, d, 0, *sf, st) == 0                                         # no slot: nothing launched
    torch.cuda.synchronize()
    assert torch.equal(b1, seven) and torch.equal(table, keep)


# ---- the protocol, end to end over the in-process tagged network of tests/test_gpu_fixedpoint.py (restated) ------------------
class _TaggedNet:
    def __init__(self, n):
        self.n, self.q = n, [dict() for _ in range(n)]

    def _queue(self, party, tag):
        return self.q[party].setdefault(tag, asyncio.Queue())

    def get_send_recv(self, i, tamper=None):
        def factory(tag):
            def send(dest, msg):
                self._queue(dest, tag).put_nowait((i, tamper(msg) if tamper else msg))

            return send, self._queue(i, tag).get

        return factory


def _deal(ctx, rnd, p, n, degree, values):
    """-> [party] (len(values), limbs) tensors: Shamir shares of the values at the points 1..n"""
    out = [[0] * len(values) for _ in range(n)]
    for j, v in enumerate(values):
        coeffs = [rnd.randrange(p) for _ in range(degree)]
        for i in range(n):
            acc = 0
            for co in reversed(coeffs):
                acc = (acc + co) * (i + 1) % p
            out[i][j] = (acc + v) % p
    return [ctx.upload_ints(d) if d else ctx.empty(0) for d in out]


def _run_parties(p, n, t, bad, rnd, body):
    from honeybadgermpc_amd import wire
    from honeybadgermpc_amd.open_coalescer import OpenCoalescer

    def garble(msg):
        tag, blob = msg
        count = wire.unpack_limbs(blob).shape[0]
        return (tag, wire.pack_ints([rnd.randrange(p) for _ in range(count)], p))

    async def party(i, net):
        co = OpenCoalescer(p, n, t, i, net.get_send_recv(i, garble if i in bad else None))
        return await body(co, i)

    async def main():
        net = _TaggedNet(n)
        return await asyncio.gather(*[party(i, net) for i in range(n)])

    results = asyncio.run(main())
    _ctx(p).torch.cuda.synchronize()
    return results


def _dealt_sort(p, n, batch, width, k, kappa, seed, parties=4, t=1):
    """a plan, a cleartext table with duplicate keys and both ends of the allowed range, and every party's table and preprocessing"""
    from honeybadgermpc_amd.progs import sorting as so

    ctx = _ctx(p)
    rnd = random.Random(seed)
    plan = so.SortPlan(n, batch, width, k, kappa)
    lim, rows = 1 << (k - 2), batch * n
    pool = [-lim, lim - 1, -lim, lim - 1, 0, 0, 1, -1, 3, 3]
    keys = [pool[i] if i < len(pool) else rnd.randrange(-lim, lim) for i in range(rows)]
    rnd.shuffle(keys)
    clear = [keys] + [[rnd.randrange(p) for _ in range(rows)] for _ in range(width - 1)]
    tables = [d.view(width, rows, ctx.n_limbs) for d in _deal(ctx, rnd, p, parties, t, [v % p for col in clear for v in col])]
    bits = _deal(ctx, rnd, p, parties, t, [rnd.getrandbits(1) for _ in range(plan.size("bits"))])

    def triples(kind):
        a, b = ([rnd.randrange(p) for _ in range(plan.size(kind))] for _ in range(2))
        dealt = [_deal(ctx, rnd, p, parties, t, v) for v in (a, b, [x * y % p for x, y in zip(a, b)])]
        return [tuple(d[i] for d in dealt) for i in range(parties)]

    return ctx, rnd, plan, clear, tables, bits, triples("carry"), triples("swap")


@pytest.mark.parametrize("n, width, batch, p, k, kappa, liars", [
    (13, 3, 1, BLS, 8, 8, 0), (5, 1, 3, BLS, 8, 8, 0), (8, 2, 2, BLS, 8, 8, 0), (2, 1, 1, BLS, 8, 8, 0), (1, 2, 1, BLS, 8, 8, 0), (3, 1, 1, BLS, 64, 32, 0),
    (5, 2, 1, P64, 8, 8, 0), (5, 2, 1, BLS, 8, 8, 1)],
    ids=["13x3", "5x1-batch3", "8x2-batch2", "2x1", "1x2", "3x1-k64", "5x2-2^64-59", "5x2-one-party-sends-garbage"])
def test_sort_opens_to_the_model(n, width, batch, p, k, kappa, liars):
    from honeybadgermpc_amd.progs import fixedpoint as fx
    from honeybadgermpc_amd.progs import sorting as so

    parties, t = 4, 1
    ctx, rnd, plan, clear, tables, bits, carry, swap = _dealt_sort(p, n, batch, width, k, kappa, 100 * n + 10 * width + batch + liars)
    bad = set(rnd.sample(range(parties), liars))
    want = so.sort_model(clear, n, k)
    assert plan.opens == plan.n_layers * (2 + fx.carry_levels(k - 1)) and plan.opens <= 50
    for i in range(parties):                                                    # the preprocessing has exactly the plan's sizes
        assert tuple(bits[i].shape) == (plan.size("bits"), ctx.n_limbs) == ((k + kappa) * plan.total_slots, ctx.n_limbs)
        assert all(tuple(v.shape) == ((2 * k - 3) * plan.total_slots, ctx.n_limbs) for v in carry[i])
        assert all(tuple(v.shape) == (width * plan.total_slots, ctx.n_limbs) for v in swap[i])

    async def body(co, i):
        prep = [bits[i], *carry[i], *swap[i]]
        keep = [v.clone() for v in prep]
        before = co.batches
        out = await so.sort(co, tables[i], plan, bits[i], carry[i], swap[i])
        batches = co.batches - before
        assert out.data_ptr() == tables[i].data_ptr() and tuple(out.shape) == (width, batch * n, ctx.n_limbs)      # in place
        assert all(ctx.torch.equal(v, cp) for v, cp in zip(prep, keep))
        return ctx.download_ints(await co.open_share_array(out.view(-1, ctx.n_limbs))), batches

    for i, (got, batches) in enumerate(_run_parties(p, parties, t, bad, rnd, body)):
        if i in bad:
            continue
        assert sc.unflat(got, width) == [[v % p for v in col] for col in want], i
        assert batches == plan.opens, i
    assert [v for b in range(batch) for v in want[0][b * n:(b + 1) * n]] == [v for b in range(batch) for v in sorted(clear[0][b * n:(b + 1) * n])]


def test_layer_by_layer_fixed_point_array_and_refusals():
    """compare_exchange_layer run layer after layer is sort; FixedPointArray.sort wraps it and leaves its inputs alone; preprocessing
    of another size is refused before anything is opened"""
    from honeybadgermpc_amd.progs import fixedpoint as fx
    from honeybadgermpc_amd.progs import sorting as so

    p, n, width, batch, k, kappa = BLS, 5, 2, 1, 8, 8
    ctx, rnd, plan, clear, tables, bits, carry, swap = _dealt_sort(p, n, batch, width, k, kappa, 77)
    want = [[v % p for v in col] for col in so.sort_model(clear, n, k)]

    async def body(co, i):
        torch, table = ctx.torch, tables[i]
        longer = torch.cat([bits[i], bits[i][:1]])
        for call in (lambda: so.sort(co, table, plan, longer, carry[i], swap[i]), lambda: so.sort(co, table, plan, bits[i][:-1], carry[i], swap[i]),
                     lambda: so.sort(co, table, plan, bits[i], carry[i][:2], swap[i]), lambda: so.sort(co, table, plan, bits[i], carry[i], (swap[i][0], swap[i][1], swap[i][2][:-1])),
                     lambda: so.sort(co, table, plan, bits[i], swap[i], carry[i]), lambda: so.sort(co, table[:1], plan, bits[i], carry[i], swap[i]),
                     lambda: so.sort(co, table, so.SortPlan(n, batch, width, 222, kappa), bits[i], carry[i], swap[i]),
                     lambda: so.sort(co, table, None, bits[i], carry[i], swap[i]), lambda: so.compare_exchange_layer(co, table, plan, plan.n_layers, bits[i], carry[i], swap[i]),
                     lambda: fx.FixedPointArray(co, table[0], 2, k, kappa).sort(plan, bits[i], carry[i], swap[i]),                     # the plan wants a payload column
                     lambda: fx.FixedPointArray(co, table[0], 2, k + 1, kappa).sort(plan, bits[i], carry[i], swap[i], payload=table[1:])):
            with pytest.raises(ValueError):
                await call()
        assert co.batches == 0                                                   # nothing was opened
        keep = table.clone()
        arr, payload = await fx.FixedPointArray(co, table[0], 2, k, kappa).sort(plan, bits[i], carry[i], swap[i], payload=table[1:])
        assert torch.equal(table, keep) and co.batches == plan.opens
        wrapped = [ctx.download_ints(await co.open_share_array(arr.shares)), ctx.download_ints(await co.open_share_array(payload.reshape(-1, ctx.n_limbs)))]
        floats = await arr.open()
        for l in range(plan.n_layers):
            assert (await so.compare_exchange_layer(co, table, plan, l, bits[i], carry[i], swap[i])).data_ptr() == table.data_ptr()
        return wrapped, floats, sc.unflat(ctx.download_ints(await co.open_share_array(table.view(-1, ctx.n_limbs))), width)

    for wrapped, floats, layered in _run_parties(p, 4, 1, set(), rnd, body):
        assert wrapped == want and layered == want
        assert floats == [v / 4 for v in sorted(clear[0])] and floats[::-1] == sorted(floats, reverse=True)      # descending: a flip

"""GPU: honeybadgermpc_amd.butterfly_network -- the kernels of csrc/hb_bf.hip through mask_layer / switch_layer against Python
ints and against the same layer composed from share_arithmetic, and the whole network over an OpenCoalescer against the
permutation the reference applies for the same signs (tests/golden/butterfly_network.json).  Exact equality everywhere."""
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
FIELDS = [BLS, (1 << 256) - 189, P64, GOLDILOCKS]
FIELD_IDS = ["bls", "2^256-189", "2^64-59", "goldilocks"]


def _ctx(p):
    from honeybadgermpc_amd._capi import Context

    return Context.get(p)


def _random_tensor(ctx, seed, count):
    """`count` uniform canonical residues made on the device side (numpy limbs, reduced by hb_reduce)"""
    g = np.random.default_rng(seed)
    limbs = g.integers(-(1 << 63), (1 << 63) - 1, size=(count, ctx.n_limbs), dtype=np.int64, endpoint=True)
    return ctx.reduce_(ctx.to_device(limbs))


def _draw(rnd, p, count):
    return [rnd.choice([0, 1, p - 1, rnd.randrange(p), rnd.randrange(p), rnd.randrange(p)]) for _ in range(count)]


def _mask_ref(p, xs, bits, ps, qs, xi, yi):
    return [(b - pp) % p for b, pp in zip(bits, ps)] + [(xs[i] - xs[j] - q) % p for i, j, q in zip(xi, yi, qs)]


def _switch_ref(p, xs, d, e, ps, qs, pqs, xi, yi, switches=None):
    inv2 = pow(2, -1, p)
    out = []
    for j in (range(len(xi)) if switches is None else switches):
        m = (d[j] * e[j] + d[j] * qs[j] + e[j] * ps[j] + pqs[j]) % p
        x, y = xs[xi[j]], xs[yi[j]]
        out += [(x + y + m) * inv2 % p, (x + y - m) * inv2 % p]
    return out


def _composed_layer(ctx, x, bits, p, q, pq, a, opened=None):
    """the same layer from torch.index_select, share_arithmetic and torch.stack alone -> (masked, out); `opened` stands for the
    open of masked (default: masked itself)"""
    from honeybadgermpc_amd import butterfly_network as bn
    from honeybadgermpc_amd import share_arithmetic as sa

    torch = ctx.torch
    k = x.shape[0]
    half = k // 2
    j = torch.arange(half, device=ctx.tdev)
    xi = ((j >> a) << (a + 1)) | (j & ((1 << a) - 1))
    if k <= 1024:
        assert xi.tolist() == bn.switch_indices(k, a)[0]
    xs, ys = x.index_select(0, xi), x.index_select(0, xi | (1 << a))
    masked = torch.cat([sa.sub(ctx, bits, p), sa.sub(ctx, sa.sub(ctx, xs, ys), q)], dim=0)
    opened = masked if opened is None else opened
    m = sa.beaver_combine(ctx, opened[:half], opened[half:], p, q, pq)
    s = sa.add(ctx, xs, ys)
    inv2 = pow(2, -1, ctx.modulus)
    t1, t2 = sa.mul(ctx, sa.add(ctx, s, m), inv2), sa.mul(ctx, sa.sub(ctx, s, m), inv2)
    return masked, torch.stack([t1, t2], dim=1).reshape(k, ctx.n_limbs)


@pytest.mark.parametrize("p", FIELDS, ids=FIELD_IDS)
def test_layers_equal_python_ints_every_stride(p):
    from honeybadgermpc_amd import butterfly_network as bn

    ctx = _ctx(p)
    rnd = random.Random(p % 997)
    for n in (1, 2, 3, 6, 9, 10, 16):
        k = 1 << n
        half = k // 2
        draw = (lambda c: _draw(rnd, p, c)) if n < 16 else (lambda c: [rnd.randrange(p) for _ in range(c)])
        xs = draw(k)
        bits, ps, qs, pqs, d, e = (draw(half) for _ in range(6))
        x_dev = ctx.upload_ints(xs)
        b_dev, p_dev, q_dev, pq_dev, d_dev, e_dev = (ctx.upload_ints(v) for v in (bits, ps, qs, pqs, d, e))
        for a in range(n):
            xi, yi = bn.switch_indices(k, a)
            want = _mask_ref(p, xs, bits, ps, qs, xi, yi)
            masked = bn.mask_layer(ctx, x_dev, b_dev, p_dev, q_dev, a)
            assert tuple(masked.shape) == (k, ctx.n_limbs) and ctx.download_ints(masked) == want, (k, a)
            e_only = bn.mask_layer(ctx, x_dev, None, None, q_dev, a)
            assert tuple(e_only.shape) == (half, ctx.n_limbs) and ctx.torch.equal(e_only, masked[half:]), (k, a)
            out = bn.switch_layer(ctx, x_dev, d_dev, e_dev, p_dev, q_dev, pq_dev, a)
            assert tuple(out.shape) == (k, ctx.n_limbs)
            assert ctx.download_ints(out) == _switch_ref(p, xs, d, e, ps, qs, pqs, xi, yi), (k, a)
            # ... and as a layer of the protocol runs them: the switch fed with the mask's own output
            out2 = bn.switch_layer(ctx, x_dev, masked[:half], masked[half:], p_dev, q_dev, pq_dev, a)
            _, comp = _composed_layer(ctx, x_dev, b_dev, p_dev, q_dev, pq_dev, a)
            assert ctx.torch.equal(out2, comp), (k, a)


@pytest.mark.parametrize("p", [BLS, P64], ids=["bls", "2^64-59"])
def test_one_layer_of_a_million_inputs(p):
    from honeybadgermpc_amd import butterfly_network as bn

    ctx = _ctx(p)
    k = 1 << 20
    half = k // 2
    x = _random_tensor(ctx, 1, k)
    bits, ps, qs, pqs = (_random_tensor(ctx, 2 + i, half) for i in range(4))
    rnd = random.Random(20)
    for a in (0, 7, 19):
        masked = bn.mask_layer(ctx, x, bits, ps, qs, a)
        out = bn.switch_layer(ctx, x, masked[:half], masked[half:], ps, qs, pqs, a)
        c_masked, c_out = _composed_layer(ctx, x, bits, ps, qs, pqs, a)
        assert ctx.torch.equal(masked, c_masked) and ctx.torch.equal(out, c_out), a
        assert ctx.torch.equal(bn.mask_layer(ctx, x, None, None, qs, a), masked[half:])
        # a sample of switches against Python ints: the ends, a block boundary of the stride, random ones
        sw = sorted({0, 1, half - 1, half - 2, (1 << a) % half, ((1 << a) - 1) % half} | {rnd.randrange(half) for _ in range(200)})
        idx = ctx.torch.tensor(sw, device=ctx.tdev)
        xi = [((j >> a) << (a + 1)) | (j & ((1 << a) - 1)) for j in sw]
        yi = [v | (1 << a) for v in xi]
        pick = lambda t, rows: ctx.download_ints(t.index_select(0, ctx.torch.tensor(rows, device=ctx.tdev)))  # noqa: E731
        xv, yv = pick(x, xi), pick(x, yi)
        bv, pv, qv, pqv = (ctx.download_ints(t.index_select(0, idx)) for t in (bits, ps, qs, pqs))
        xs_small = [v for pr in zip(xv, yv) for v in pr]                 # switch i of the sample reads 2i, 2i + 1
        pairs = (list(range(0, 2 * len(sw), 2)), list(range(1, 2 * len(sw), 2)))
        want_masked = _mask_ref(p, xs_small, bv, pv, qv, *pairs)
        assert ctx.download_ints(masked.index_select(0, idx)) == want_masked[:len(sw)]
        assert ctx.download_ints(masked.index_select(0, idx + half)) == want_masked[len(sw):]
        want_out = _switch_ref(p, xs_small, want_masked[:len(sw)], want_masked[len(sw):], pv, qv, pqv, *pairs)
        got = ctx.download_ints(out.reshape(half, 2, ctx.n_limbs).index_select(0, idx).reshape(-1, ctx.n_limbs))
        assert got == want_out, a


def test_inputs_untouched_out_given_arguments_checked_and_asynchronous():
    from honeybadgermpc_amd import butterfly_network as bn
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd._capi import HB_ERR_BAD_ARG

    p, k, a = BLS, 512, 3
    half = k // 2
    ctx = _ctx(p)
    torch = ctx.torch
    rnd = random.Random(4)
    xs = _draw(rnd, p, k)
    bits, ps, qs, pqs, d, e = (_draw(rnd, p, half) for _ in range(6))
    x_dev = ctx.upload_ints(xs)
    b_dev, p_dev, q_dev, pq_dev, d_dev, e_dev = (ctx.upload_ints(v) for v in (bits, ps, qs, pqs, d, e))
    ops = (x_dev, b_dev, p_dev, q_dev, pq_dev, d_dev, e_dev)
    copies = [t.clone() for t in ops]
    xi, yi = bn.switch_indices(k, a)
    want_m = _mask_ref(p, xs, bits, ps, qs, xi, yi)
    want_o = _switch_ref(p, xs, d, e, ps, qs, pqs, xi, yi)
    # results consumed on the current stream without a synchronise, through another kernel of the library
    masked = bn.mask_layer(ctx, x_dev, b_dev, p_dev, q_dev, a)
    out = bn.switch_layer(ctx, x_dev, d_dev, e_dev, p_dev, q_dev, pq_dev, a)
    assert ctx.download_ints(sa.neg(ctx, masked)) == [-v % p for v in want_m]
    assert ctx.download_ints(sa.add(ctx, out, out)) == [2 * v % p for v in want_o]
    # on a side stream as well
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        o2 = bn.switch_layer(ctx, x_dev, d_dev, e_dev, p_dev, q_dev, pq_dev, a)
        twice = sa.add(ctx, o2, o2)
    side.synchronize()
    assert ctx.download_ints(twice) == [2 * v % p for v in want_o]
    # out given: written where asked, and handed back
    buf = ctx.empty(k)
    assert bn.switch_layer(ctx, x_dev, d_dev, e_dev, p_dev, q_dev, pq_dev, a, out=buf) is buf and ctx.download_ints(buf) == want_o
    assert bn.mask_layer(ctx, x_dev, b_dev, p_dev, q_dev, a, out=buf) is buf and ctx.download_ints(buf) == want_m
    hbuf = ctx.empty(half)
    assert bn.mask_layer(ctx, x_dev, None, None, q_dev, a, out=hbuf) is hbuf and ctx.download_ints(hbuf) == want_m[half:]
    assert all(torch.equal(t, c) for t, c in zip(ops, copies))
    assert out.data_ptr() != x_dev.data_ptr() and masked.data_ptr() != x_dev.data_ptr()
    # a strided view of the inputs is taken as its values
    wide = torch.zeros((k, 2, ctx.n_limbs), dtype=torch.int64, device=ctx.tdev)
    wide[:, 0] = x_dev
    assert ctx.download_ints(bn.switch_layer(ctx, wide[:, 0], d_dev, e_dev, p_dev, q_dev, pq_dev, a)) == want_o
    # 8-byte elements behind an odd element offset (a buffer that is not 16-byte aligned) at stride 1
    small = _ctx(P64)
    xs8 = _draw(rnd, P64, 65)
    h8 = [_draw(rnd, P64, 32) for _ in range(6)]
    x8 = small.upload_ints(xs8)[1:]
    t8 = [small.upload_ints(v) for v in h8]
    o8 = small.empty(65)[1:]
    assert x8.data_ptr() % 16 == 8 and o8.data_ptr() % 16 == 8
    i8 = bn.switch_indices(64, 0)
    assert small.download_ints(bn.switch_layer(small, x8, t8[4], t8[5], t8[1], t8[2], t8[3], 0, out=o8)) == _switch_ref(P64, xs8[1:], h8[4], h8[5], h8[1], h8[2], h8[3], *i8)
    assert small.download_ints(bn.mask_layer(small, x8, t8[0], t8[1], t8[2], 0)) == _mask_ref(P64, xs8[1:], h8[0], h8[1], h8[2], *i8)
    # argument checks raise before C and nothing is launched: the output buffer keeps its contents
    buf.fill_(7)
    seven = buf.clone()
    bad_calls = [
        lambda: bn.switch_layer(ctx, x_dev, d_dev, e_dev, p_dev, q_dev, pq_dev, 9, out=buf),            # stride == k
        lambda: bn.switch_layer(ctx, x_dev, d_dev, e_dev, p_dev, q_dev, pq_dev, -1, out=buf),
        lambda: bn.switch_layer(ctx, x_dev, d_dev, e_dev, p_dev, q_dev, pq_dev, 1.0, out=buf),
        lambda: bn.switch_layer(ctx, x_dev[:500], d_dev[:250], e_dev[:250], p_dev[:250], q_dev[:250], pq_dev[:250], 0, out=buf[:500]),  # k not a power of two
        lambda: bn.switch_layer(ctx, x_dev[:1], d_dev[:0], e_dev[:0], p_dev[:0], q_dev[:0], pq_dev[:0], 0, out=buf[:1]),
        lambda: bn.switch_layer(ctx, x_dev, d_dev[:-1], e_dev, p_dev, q_dev, pq_dev, a, out=buf),       # a short operand
        lambda: bn.switch_layer(ctx, x_dev, d_dev, e_dev, p_dev, q_dev, x_dev, a, out=buf),             # a long one
        lambda: bn.switch_layer(ctx, x_dev, d_dev, e_dev, p_dev, q_dev, pq_dev, a, out=buf[:half]),     # a short out
        lambda: bn.mask_layer(ctx, x_dev, b_dev, p_dev, q_dev, a, out=buf[:half]),
        lambda: bn.mask_layer(ctx, x_dev, None, None, q_dev, a, out=buf),                                # (k / 2 expected)
        lambda: bn.mask_layer(ctx, x_dev, b_dev[:3], p_dev, q_dev, a, out=buf),
        lambda: bn.switch_layer(ctx, x_dev.cpu(), d_dev, e_dev, p_dev, q_dev, pq_dev, a, out=buf),
    ]
    for call in bad_calls:
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TypeError):
        bn.switch_layer(ctx, x_dev.to(torch.int32), d_dev, e_dev, p_dev, q_dev, pq_dev, a, out=buf)
    assert torch.equal(buf, seven)
    # a layer is not in place: out may not be, or overlap, the inputs
    both = ctx.empty(k + half)
    both[:k] = x_dev
    keep = both.clone()
    for o in (both[:k], both[half:]):
        with pytest.raises(ValueError):
            bn.switch_layer(ctx, both[:k], d_dev, e_dev, p_dev, q_dev, pq_dev, a, out=o)
        with pytest.raises(ValueError):
            bn.mask_layer(ctx, both[:k], b_dev, p_dev, q_dev, a, out=o)
    assert torch.equal(both, keep)
    # ... and the C ABI refuses what gets past Python
    lib, st = ctx.lib, ctx.stream()
    P = ctx.ptr
    good = (P(x_dev), P(d_dev), P(e_dev), P(p_dev), P(q_dev), P(pq_dev))
    assert lib.hb_bf_switch(ctx.h, *good, k, 9, P(buf), st) == HB_ERR_BAD_ARG
    assert lib.hb_bf_switch(ctx.h, *good, k, -1, P(buf), st) == HB_ERR_BAD_ARG
    assert lib.hb_bf_switch(ctx.h, *good, 500, 0, P(buf), st) == HB_ERR_BAD_ARG
    assert lib.hb_bf_switch(ctx.h, *good, 1, 0, P(buf), st) == HB_ERR_BAD_ARG
    assert lib.hb_bf_switch(ctx.h, *good, 0, 0, P(buf), st) == HB_ERR_BAD_ARG
    assert lib.hb_bf_switch(ctx.h, *good, k, a, P(x_dev), st) == HB_ERR_BAD_ARG
    assert lib.hb_bf_switch(ctx.h, *good, k, a, None, st) == HB_ERR_BAD_ARG
    for i in range(6):
        args = list(good)
        args[i] = None
        assert lib.hb_bf_switch(ctx.h, *args, k, a, P(buf), st) == HB_ERR_BAD_ARG
    assert lib.hb_bf_mask(ctx.h, P(x_dev), P(b_dev), P(p_dev), P(q_dev), k, 9, P(buf), st) == HB_ERR_BAD_ARG
    assert lib.hb_bf_mask(ctx.h, P(x_dev), P(b_dev), P(p_dev), P(q_dev), 6, 0, P(buf), st) == HB_ERR_BAD_ARG
    assert lib.hb_bf_mask(ctx.h, P(x_dev), P(b_dev), None, P(q_dev), k, a, P(buf), st) == HB_ERR_BAD_ARG
    assert lib.hb_bf_mask(ctx.h, None, P(b_dev), P(p_dev), P(q_dev), k, a, P(buf), st) == HB_ERR_BAD_ARG
    assert lib.hb_bf_mask(ctx.h, P(x_dev), P(b_dev), P(p_dev), None, k, a, P(buf), st) == HB_ERR_BAD_ARG
    assert lib.hb_bf_mask(ctx.h, P(x_dev), P(b_dev), P(p_dev), P(q_dev), k, a, None, st) == HB_ERR_BAD_ARG
    assert lib.hb_bf_mask(ctx.h, P(x_dev), P(b_dev), P(p_dev), P(q_dev), k, a, P(x_dev), st) == HB_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert torch.equal(buf, seven) and all(torch.equal(t, c) for t, c in zip(ops, copies))
    assert lib.hb_bf_mask(ctx.h, P(x_dev), None, None, P(q_dev), k, a, P(hbuf), st) == 0
    assert ctx.download_ints(hbuf) == want_m[half:]


# ---- the protocol, end to end over the in-process tagged network of tests/test_gpu_power_mixing.py -------------------------
class _TaggedNet:
    """get_send_recv(tag) -> (send, recv) for party i, as the runtime hands out per-share-id channels (mpc.py:196-205)"""

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


def _deal(rnd, p, n, degree, values):
    """-> [party][k]: Shamir shares of values[k] at the points 1..n"""
    polys = [[v] + [rnd.randrange(p) for _ in range(degree)] for v in values]
    return [[sum(co * pow(x, e, p) for e, co in enumerate(poly)) % p for poly in polys] for x in range(1, n + 1)]


def _run_network(p, n, t, bad, msgs, signs, rnd, slab_bytes=None):
    """every party runs shuffle_and_open in both modes -> {mode: [(shares tensor, opened ints) per party]}, coalescer batches"""
    from honeybadgermpc_amd import butterfly_network as bn
    from honeybadgermpc_amd import wire
    from honeybadgermpc_amd.open_coalescer import OpenCoalescer

    ctx = _ctx(p)
    k = len(msgs)
    half, n_layers = k // 2, len(signs)
    flat_signs = [b % p for row in signs for b in row]
    tp = [rnd.randrange(p) for _ in flat_signs]
    tq = [rnd.randrange(p) for _ in flat_signs]
    dealt = [_deal(rnd, p, n, t, v) for v in (msgs, flat_signs, tp, tq, [a * b % p for a, b in zip(tp, tq)])]

    def rows(values):
        return ctx.upload_ints(values).reshape(n_layers, half, ctx.n_limbs)

    def garble(msg):
        tag, blob = msg
        count = wire.unpack_limbs(blob).shape[0]
        return (tag, wire.pack_ints([rnd.randrange(p) for _ in range(count)], p))

    batches = {}

    async def party(i, net, mode):
        co = OpenCoalescer(p, n, t, i, net.get_send_recv(i, garble if i in bad else None))
        inputs = ctx.upload_ints(dealt[0][i])
        before = inputs.clone()
        kw = {} if slab_bytes is None else {"slab_bytes": slab_bytes}
        shares, opened = await bn.shuffle_and_open(co, inputs, rows(dealt[1][i]), tuple(rows(dealt[j][i]) for j in (2, 3, 4)), open_bits=mode, **kw)
        assert ctx.torch.equal(inputs, before) and shares.data_ptr() != inputs.data_ptr()
        batches.setdefault(mode, set()).add(co.batches)
        return shares, ctx.download_ints(opened)

    async def main(mode):
        net = _TaggedNet(n)
        return await asyncio.gather(*[party(i, net, mode) for i in range(n)])

    results = {mode: asyncio.run(main(mode)) for mode in ("per_layer", "upfront")}
    ctx.torch.cuda.synchronize()
    return results, batches


@pytest.mark.parametrize("n, t, liars", [(4, 1, 0), (7, 2, 0), (4, 1, 1), (7, 2, 2)])
@pytest.mark.parametrize("k", [32, 256])
def test_network_end_to_end(n, t, liars, k):
    from honeybadgermpc_amd import butterfly_network as bn

    p = BLS
    ctx = _ctx(p)
    rnd = random.Random(1000 * n + 10 * k + liars)
    msgs = [rnd.randrange(p) for _ in range(k)]
    msgs[0], msgs[1] = 0, p - 1
    n_layers = len(bn.layers(k))
    signs = [[rnd.choice((1, -1)) for _ in range(k // 2)] for _ in range(n_layers)]
    bad = set(rnd.sample(range(n), liars))
    # k = 32: sign differences opened three layers a slab (25 layers: nine slabs, the last one ragged); k = 256: one slab
    slab = 3 * (k // 2) * ctx.nbytes if k == 32 else None
    results, batches = _run_network(p, n, t, bad, msgs, signs, rnd, slab_bytes=slab)
    want = [msgs[i] for i in bn.permutation(k, signs)]
    assert sorted(want) == sorted(msgs)
    for i in range(n):
        if i in bad:
            continue
        for mode in ("per_layer", "upfront"):
            assert results[mode][i][1] == want, (i, mode)
        assert ctx.torch.equal(results["per_layer"][i][0], results["upfront"][i][0]), i
    # one open a layer and one for the result; the sign differences travel ahead: one batch more, none a later slab
    assert batches["per_layer"] == {n_layers + 1} and batches["upfront"] == {n_layers + 2}


def test_golden_signs_give_the_reference_output():
    with open(os.path.join(REPO, "tests", "golden", "butterfly_network.json")) as f:
        g = json.load(f)
    p = int(g["modulus"])
    assert p == BLS
    for c in g["cases"]:
        msgs, want = [int(v) for v in c["inputs"]], [int(v) for v in c["output"]]
        results, _ = _run_network(p, 4, 1, set(), msgs, c["signs"], random.Random(c["k"]))
        for mode in ("per_layer", "upfront"):
            for i in range(4):
                assert results[mode][i][1] == want, (c["k"], mode, i)


@pytest.mark.parametrize("k, strides", [(2, (0,)), (4, (0, 1)), (1024, (0, 5, 9))], ids=["k2", "k4", "k1024"])
@pytest.mark.parametrize("p", (BLS, P64), ids=("bls", "2^64-59"))
def test_mask_and_switch_equal_the_host_self_test(p, k, strides):
    """One row body: the device's mask (with and without the signs) and switch of a layer equal, bit for bit, what hb_selftest_bf
    computes on the host from the same inputs: the self test runs the rows the kernels run, addressing included.  Both instantiations;
    every stride of 2 and 4 inputs, the first, a middle and the last of 1024 (512 switches: two workgroups).  At stride 1 in the 8-byte
    width `inputs` is given once 16-byte aligned and once as a view that starts 8 bytes off, so the instantiation that takes a
    switch's two inputs in one access and the general one both run."""
    import selftest_cases as stc
    from honeybadgermpc_amd import butterfly_network as bn

    MASK, SWITCH = 0, 1
    ctx = _ctx(p)
    torch, nl, half = ctx.torch, ctx.n_limbs, k // 2
    rnd = random.Random(k + nl)

    def draw(count, shift):
        xs = [rnd.randrange(p) for _ in range(count)]
        for i, v in enumerate((0, 1, p - 1)):
            xs[(shift + i) % count] = v
        return xs

    xs = draw(k, 0)
    bits, ps, qs, pqs, d, e = (draw(half, i) for i in range(6))
    aligned = ctx.upload_ints(xs)
    off_by_one = ctx.upload_ints([0] + xs)[1:]
    assert aligned.data_ptr() % 16 == 0 and off_by_one.data_ptr() % 16 == 8 * nl % 16
    up = ctx.upload_ints
    for a in strides:
        for x in (aligned, off_by_one) if (nl == 1 and a == 0) else (aligned,):
            rc, want = stc.run_bf(p, nl, MASK, [xs, bits, ps, qs], k, a, k)
            assert rc == 0 and torch.equal(bn.mask_layer(ctx, x, up(bits), up(ps), up(qs), a), up(want)), (a, x.data_ptr() % 16)
            rc, want = stc.run_bf(p, nl, MASK, [xs, None, None, qs], k, a, half)
            assert rc == 0 and torch.equal(bn.mask_layer(ctx, x, None, None, up(qs), a), up(want)), (a, x.data_ptr() % 16)
            rc, want = stc.run_bf(p, nl, SWITCH, [xs, d, e, ps, qs, pqs], k, a, k)
            assert rc == 0 and torch.equal(bn.switch_layer(ctx, x, up(d), up(e), up(ps), up(qs), up(pqs), a), up(want)), (a, x.data_ptr() % 16)
    torch.cuda.synchronize()

"""GPU: the offline phase of honeybadgermpc_amd.offline.  The three kernels of csrc/hb_off.hip through their wrappers, bit for bit
against the Python-int models and against the same results composed from entry points that were there before (mul then add; sqrt_mod,
inv, mul); and the protocol -- randousha, generate_triples, generate_bits -- with n parties in one process over an in-process tagged
network, checked by its invariants on Python ints: degrees, equal constants, the refinement recomputed from the recorded messages, the
abort paths, products, bits.  Exact equality everywhere."""
import asyncio
import random

import numpy as np
import pytest

from conftest import BLS

pytestmark = pytest.mark.gpu

GOLDILOCKS = 0xFFFFFFFF00000001
P64 = (1 << 64) - 59
P256 = (1 << 256) - 189
FIELDS = [BLS, P256, P64, GOLDILOCKS, 13]
FIELD_IDS = ["bls", "2^256-189", "2^64-59", "goldilocks", "13"]
COUNTS = (0, 1, 255, 256, 257, 5000)


def _ctx(p):
    from honeybadgermpc_amd._capi import Context

    return Context.get(p)


def _random_tensor(ctx, seed, count):
    g = np.random.default_rng(seed)
    limbs = g.integers(-(1 << 63), (1 << 63) - 1, size=(count, ctx.n_limbs), dtype=np.int64, endpoint=True)
    return ctx.reduce_(ctx.to_device(limbs))


def _sample(count):
    return list(range(count)) if count <= 257 else sorted({0, 1, 2, 62, 63, 64, 65, 255, 256, 257, count - 1} | set(random.Random(count).sample(range(count), 40)))


def _generator(seed):
    import torch

    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return g


# ---- the kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", FIELDS, ids=FIELD_IDS)
def test_mul_add_equals_mul_then_add(p):
    from honeybadgermpc_amd import offline
    from honeybadgermpc_amd import share_arithmetic as sa

    ctx = _ctx(p)
    torch = ctx.torch
    corners = [(x, y, z) for x in (0, 1, p - 1) for y in (0, 1, p - 1) for z in (0, 1, p - 1)]
    for count in COUNTS:
        a, b, c = (_random_tensor(ctx, 100 + 3 * count + i, count) for i in range(3))
        if count >= 255:
            for i, t in enumerate((a, b, c)):
                t[:len(corners)] = ctx.upload_ints([r[i] for r in corners])
        keep = [v.clone() for v in (a, b, c)]
        got = offline.mul_add(ctx, a, b, c)
        assert tuple(got.shape) == (count, ctx.n_limbs) and torch.equal(got, sa.add(ctx, sa.mul(ctx, a, b), c)), count
        idx = _sample(count)
        if idx:
            ai, bi, ci, gi = (ctx.download_ints(v[idx]) for v in (a, b, c, got))
            assert gi == [(x * y + z) % p for x, y, z in zip(ai, bi, ci)], count
        square = offline.mul_add(ctx, a, a, c)
        assert torch.equal(square, sa.add(ctx, sa.mul(ctx, a, a), c)), count
        for which in range(3):                                           # out over each input
            ops = [v.clone() for v in keep]
            assert offline.mul_add(ctx, *ops, out=ops[which]) is ops[which] and torch.equal(ops[which], got), (count, which)
        x = keep[0].clone()
        assert torch.equal(offline.mul_add(ctx, x, x, c, out=x), square)
        assert all(torch.equal(v, w) for v, w in zip((a, b, c), keep)), "inputs were written"
    with pytest.raises(ValueError):
        offline.mul_add(ctx, a, b[:7], c)
    with pytest.raises(ValueError):
        offline.mul_add(ctx, a, b, c, out=ctx.empty(3))
    with pytest.raises(TypeError):
        offline.mul_add(ctx, a.cpu().numpy(), b, c)
    st, P = ctx.stream(), ctx.ptr
    assert ctx.lib.hb_off_mul_add(ctx.h, P(a), None, P(c), P(b), 5, st) == 2 and ctx.lib.hb_off_mul_add(ctx.h, P(a), P(b), P(c), P(b), -1, st) == 2
    assert ctx.lib.hb_off_mul_add(ctx.h, None, None, None, None, 0, st) == 0


def _invsqrt_inputs(p, count, rnd):
    """as tests/test_offline_host.py: squares of corner and random values, every 2-power order of x^q where s is large, zeros and
    non-residues at the first, the last and the wave- and workgroup-edge positions"""
    from honeybadgermpc_amd import offline

    q, s, g = offline._tonelli_constants(p)
    nonres = [v for v in range(2, 200) if pow(v, (p - 1) // 2, p) == p - 1][:4]
    xs = [v * v % p for v in (1, p - 1, 2, p - 2, (p - 1) // 2, (p + 1) // 2)]
    if s >= 8:
        xs += [pow(g, 1 << j, p) for j in range(1, s + 1)]
        xs += [pow(g, 1 << j, p) * pow(rnd.randrange(2, p), 2 << s, p) % p for j in range(1, s)]
    xs += [pow(rnd.randrange(1, p), 2, p) for _ in range(count)]
    xs = xs[:count]
    for pos, v in ((0, 0), (64, 0), (256, 0), (count - 1, nonres[0]), (63, nonres[-1]), (255, nonres[1]), (257, nonres[2])):
        if 0 <= pos < count and (count > 2 or pos == 0):
            xs[pos] = v % p
    return xs


@pytest.mark.parametrize("p", FIELDS, ids=FIELD_IDS)
def test_invsqrt_scale_equals_the_model_and_the_composed_route(p):
    from honeybadgermpc_amd import ntl, offline
    from honeybadgermpc_amd import share_arithmetic as sa

    ctx = _ctx(p)
    torch = ctx.torch
    rnd = random.Random(p % 1021)
    half = (p + 1) // 2
    for count in COUNTS:
        xi = _invsqrt_inputs(p, count, rnd)
        x, u = ctx.upload_ints(xi), _random_tensor(ctx, 500 + count, count)
        keep = (x.clone(), u.clone())
        residue = [v != 0 and pow(v, (p - 1) // 2, p) == 1 for v in xi]
        want_status = [sum(v == 0 for v in xi), sum(v != 0 and not ok for v, ok in zip(xi, residue))]
        if count >= 255:
            assert want_status[0] >= 2 and want_status[1] >= 2
        outs = {}
        for name, args in (("w", (None, offline.PM1)), ("pm1", (u, offline.PM1)), ("b01", (u, offline.ZERO_ONE))):
            out, status = offline.invsqrt_scale(ctx, x, args[0], args[1], check=False)
            assert tuple(out.shape) == (count, ctx.n_limbs) and [int(v) for v in status.tolist()] == want_status, (count, name)
            outs[name] = out
            if want_status != [0, 0]:
                with pytest.raises(AssertionError):
                    offline.invsqrt_scale(ctx, x, args[0], args[1])
        # the composed route over the residues (a 1 stands where there is none): sqrt_mod, inv, mul; zeros where the fused launch writes zeros
        if count:
            mask = torch.tensor(residue, device=ctx.tdev).unsqueeze(1)
            zero = torch.zeros_like(x)
            roots = ctx.upload_ints(ntl.sqrt_mod_batch([v if ok else 1 for v, ok in zip(xi, residue)], p))
            w = sa.inv(ctx, roots)
            assert torch.equal(outs["w"], torch.where(mask, w, zero)), count
            uw = sa.mul(ctx, u, w)
            assert torch.equal(outs["pm1"], torch.where(mask, uw, zero)), count
            assert torch.equal(outs["b01"], torch.where(mask, sa.mul(ctx, sa.add(ctx, uw, 1), half), zero)), count
        # the model on Python ints
        idx = _sample(count)
        if idx:
            ui = ctx.download_ints(u[idx])
            got = {name: ctx.download_ints(out[idx]) for name, out in outs.items()}
            for e, i in enumerate(idx):
                w, st = offline.invsqrt_model(xi[i], p)
                assert st == (0 if residue[i] else (1 if xi[i] == 0 else 2))
                assert got["w"][e] == w and (st or w * w * xi[i] % p == 1), (count, i)
                assert got["pm1"][e] == (0 if st else ui[e] * w % p) and got["b01"][e] == (0 if st else (ui[e] * w + 1) * half % p), (count, i)
        if count and want_status == [0, 0]:
            y = x.clone()
            assert offline.invsqrt_scale(ctx, y, u, out=y) is y and torch.equal(y, outs["pm1"])
        assert torch.equal(x, keep[0]) and torch.equal(u, keep[1]), "inputs were written"
    with pytest.raises(ValueError):
        offline.invsqrt_scale(ctx, x, u, mode=2)
    with pytest.raises(ValueError):
        offline.invsqrt_scale(ctx, x, u[:3])
    st, P = ctx.stream(), ctx.ptr
    status = torch.zeros(2, dtype=torch.int32, device=ctx.tdev)
    assert ctx.lib.hb_off_invsqrt_scale(ctx.h, P(x), P(u), 2, P(u), 5, P(status), st) == 2
    assert ctx.lib.hb_off_invsqrt_scale(ctx.h, P(x), P(u), 0, P(u), 5, None, st) == 2 and ctx.lib.hb_off_invsqrt_scale(ctx.h, None, None, 0, None, 0, None, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(u, keep[1]) and not status.any()


KINDS = ("exact", "lead_zero", "stray_top", "only_top", "stray_next", "const_top_limb", "zero")


def _crafted_block(p, n, k, t, rnd):
    """as tests/test_offline_host.py: [n][2k] coefficients, column j of kind KINDS[j % 7] -> (flat list, kinds)"""
    assert 2 * t < n - 1
    L = p.bit_length()
    cols = [[0] * n for _ in range(2 * k)]
    kinds = [KINDS[j % len(KINDS)] for j in range(k)]
    for j, kind in enumerate(kinds):
        secret = rnd.randrange(1 << (L - 3))
        for col, deg in ((j, t), (k + j, 2 * t)):
            poly = [secret] + [rnd.randrange(p) for _ in range(deg - 1)] + [rnd.randrange(1, p)] + [0] * (n - 1 - deg)
            if kind == "lead_zero":
                poly[deg] = 0
            elif kind == "stray_top":
                poly[n - 1] = 1
            elif kind == "only_top":
                poly = [0] * (n - 1) + [rnd.randrange(1, p)]
            elif kind == "stray_next":
                poly[deg + 1] = p - 1
            elif kind == "zero":
                poly = [0] * n
            cols[col] = poly
        if kind == "const_top_limb":
            cols[k + j][0] = secret + (1 << (L - 2))
    return [cols[c][e] for e in range(n) for c in range(2 * k)], kinds


@pytest.mark.parametrize("p", FIELDS, ids=FIELD_IDS)
def test_degree_check_on_crafted_columns(p):
    from honeybadgermpc_amd import offline

    ctx = _ctx(p)
    rnd = random.Random(p % 1031)
    for n, t in ((4, 1), (7, 2), (16, 5)):
        for k in (1, 64, 65, 255, 256, 257) + ((5000,) if n == 4 else ()):
            coeffs, kinds = _crafted_block(p, n, k, t, rnd)
            bad = sum(kind in ("lead_zero", "stray_top", "only_top", "stray_next", "zero") for kind in kinds)
            want = (bad, bad, sum(kind == "const_top_limb" for kind in kinds))
            if k <= 257:
                assert tuple(offline.degree_check_model(coeffs, n, k, t)) == want
            dev = ctx.upload_ints(coeffs)
            assert offline.degree_check(ctx, dev, n, t) == want, (n, t, k)
            assert tuple(int(v) for v in offline.degree_check(ctx, dev.view(n, 2 * k, ctx.n_limbs), n, t, check=False).tolist()) == want
        coeffs, _ = _crafted_block(p, n, 1, t, rnd)                      # one column of exact degrees: nothing is counted
        assert offline.degree_check(ctx, ctx.upload_ints(coeffs), n, t) == (0, 0, 0)
        coeffs[2 * t * 2] = 5                                            # the t-sharing alone: a stray coefficient where the other's leading one is
        assert offline.degree_check(ctx, ctx.upload_ints(coeffs), n, t) == (1, 0, 0)
    with pytest.raises(ValueError):
        offline.degree_check(ctx, ctx.upload_ints([0] * 9), 4, 1)
    with pytest.raises(ValueError):
        offline.degree_check(ctx, ctx.upload_ints([0] * 8), 4, 2)
    dev = ctx.upload_ints([0] * 8)
    assert ctx.lib.hb_off_degree_check(ctx.h, ctx.ptr(dev), 4, 1, 2, None, ctx.stream()) == 2 and ctx.lib.hb_off_degree_check(ctx.h, ctx.ptr(dev), 4, 1, 1, None, ctx.stream()) == 2
    assert ctx.lib.hb_off_degree_check(ctx.h, None, 4, 0, 1, None, ctx.stream()) == 0


# ---- the protocol over the in-process tagged network ------------------------------------------------------------------------
class _TaggedNet:
    """get_send_recv(i)(tag) -> (send, recv) for party i; hook(sender, tag, dest, msg) -> the message that travels (tampering, recording)"""

    def __init__(self, n, hook=None):
        self.n, self.q, self.hook = n, [dict() for _ in range(n)], hook

    def _queue(self, party, tag):
        return self.q[party].setdefault(tag, asyncio.Queue())

    def get_send_recv(self, i):
        def factory(tag):
            def send(dest, msg):
                self._queue(dest, tag).put_nowait((i, self.hook(i, tag, dest, msg) if self.hook else msg))

            return send, self._queue(i, tag).get

        return factory


def _run_parties(p, n, t, body, hook=None, return_exceptions=False):
    from honeybadgermpc_amd.open_coalescer import OpenCoalescer

    async def main():
        net = _TaggedNet(n, hook)
        work = asyncio.gather(*[body(OpenCoalescer(p, n, t, i, net.get_send_recv(i)), i) for i in range(n)], return_exceptions=return_exceptions)
        return await asyncio.wait_for(work, 20)

    results = asyncio.run(main())
    _ctx(p).torch.cuda.synchronize()
    return results


def _coefficients(ys, p):
    """the polynomial of degree < n through (1, ys[0]) .. (n, ys[n-1]) on Python ints -> n coefficients"""
    n = len(ys)
    out = [0] * n
    for i in range(n):
        num, den = [1], 1
        for j in range(n):
            if j != i:
                num = [(a - (j + 1) * b) % p for a, b in zip([0] + num, num + [0])]
                den = den * (i - j) % p
        scale = ys[i] * pow(den, -1, p) % p
        for e in range(n):
            out[e] = (out[e] + scale * num[e]) % p
    return out


def _check_sharings(p, n, t, per_party_t, per_party_2t=None):
    """every column of per_party_t ([party][index] ints) is a sharing of degree <= t, of per_party_2t of degree <= 2t with the same
    constant -> the constants"""
    secrets = []
    for idx in range(len(per_party_t[0])):
        ct = _coefficients([per_party_t[i][idx] for i in range(n)], p)
        assert not any(ct[t + 1:]), idx
        if per_party_2t is not None:
            c2 = _coefficients([per_party_2t[i][idx] for i in range(n)], p)
            assert not any(c2[2 * t + 1:]) and c2[0] == ct[0], idx
        secrets.append(ct[0])
    return secrets


@pytest.mark.parametrize("p, n, t, k", [(BLS, 4, 1, 1), (BLS, 4, 1, 10), (BLS, 7, 2, 5), (BLS, 16, 5, 3), (P64, 4, 1, 10)],
                         ids=["4-1-1", "4-1-10", "7-2-5", "16-5-3", "4-1-10-2^64-59"])
def test_randousha_invariants(p, n, t, k):
    from honeybadgermpc_amd import offline, wire

    ctx = _ctx(p)
    sent = {}

    def record(sender, tag, dest, msg):
        if tag[-1] == "H1":
            sent[(sender, dest)] = msg
        return msg

    async def body(co, i):
        r_t, r_2t = await offline.randousha(co, k, generator=_generator(900 + i))
        assert tuple(r_t.shape) == tuple(r_2t.shape) == ((n - 2 * t) * k, ctx.n_limbs) and co.batches == 0
        return ctx.download_ints(r_t), ctx.download_ints(r_2t)

    results = _run_parties(p, n, t, body, record)
    good = n - 2 * t
    secrets = _check_sharings(p, n, t, [r[0] for r in results], [r[1] for r in results])
    assert len(secrets) == good * k and len(set(secrets)) == good * k
    # the refinement recomputed from what travelled: element j (n - 2t) + i = sum_s received[s][j] (i + 1)^s
    assert len(sent) == n * n
    for me in range(n):
        received = [wire.unpack_ints(sent[(s, me)]) for s in range(n)]
        assert all(len(row) == 2 * k for row in received)
        for j in range(k):
            for i in range(good):
                assert results[me][0][j * good + i] == sum(received[s][j] * pow(i + 1, s, p) for s in range(n)) % p
                assert results[me][1][j * good + i] == sum(received[s][k + j] * pow(i + 1, s, p) for s in range(n)) % p


def _repack(blob, p, change):
    from honeybadgermpc_amd import wire

    values = wire.unpack_ints(blob)
    change(values)
    return wire.pack_ints([v % p for v in values], p)


@pytest.mark.parametrize("case", ["perturbed_share", "two_secrets", "checker_aborts", "truncated_blob", "truncated_for_one"])
def test_randousha_aborts(case):
    """every party raises HoneyBadgerMPCError, and none waits for a message that will not come"""
    from honeybadgermpc_amd import offline
    from honeybadgermpc_amd.exceptions import HoneyBadgerMPCError

    p, n, t, k = BLS, 7, 2, 4

    def bump(positions):
        def change(values):
            for e in positions:
                values[e] += 1

        return change

    def hook(sender, tag, dest, msg):
        if case == "perturbed_share" and tag[-1] == "H1" and sender == 1 and dest == 2:
            return _repack(msg, p, bump([0]))                             # one recipient's t-share of the first value
        if case == "two_secrets" and tag[-1] == "H1" and sender == 1:
            return _repack(msg, p, bump(range(k, 2 * k)))                 # every 2t-share + 1: consistent sharings of secret + 1
        if case == "checker_aborts" and tag[-1] == "H3" and sender == n - 1:
            return "A"
        if case == "truncated_blob" and tag[-1] == "H1" and sender == 3:
            return msg[:-3]
        if case == "truncated_for_one" and tag[-1] == "H1" and sender == 3 and dest == 0:
            return msg[:-3]
        return msg

    async def body(co, i):
        return await offline.randousha(co, k, generator=_generator(40 + i))

    results = _run_parties(p, n, t, body, hook, return_exceptions=True)
    assert all(isinstance(r, HoneyBadgerMPCError) for r in results), results


def test_randousha_refuses_non_bytes_messages():
    from honeybadgermpc_amd import offline
    from honeybadgermpc_amd.exceptions import HoneyBadgerMPCError

    def hook(sender, tag, dest, msg):
        return [1, 2, 3] if tag[-1] == "H2" and sender == 0 else msg

    async def body(co, i):
        return await offline.randousha(co, 2, generator=_generator(70 + i))

    results = _run_parties(BLS, 4, 1, body, hook, return_exceptions=True)
    assert all(isinstance(r, HoneyBadgerMPCError) for r in results), results


@pytest.mark.parametrize("n, t, k", [(4, 1, 1), (4, 1, 7), (7, 2, 20)])
def test_generate_triples(n, t, k):
    from honeybadgermpc_amd import offline
    from honeybadgermpc_amd import share_arithmetic as sa

    p = BLS
    ctx = _ctx(p)
    rnd = random.Random(n + k)
    xs, ys = [rnd.randrange(p) for _ in range(k)], [rnd.randrange(p) for _ in range(k)]
    slopes = [[rnd.randrange(p) for _ in range(k)] for _ in range(2)]

    async def body(co, i):
        a, b, ab = await offline.generate_triples(co, k, generator=_generator(300 + i))
        assert tuple(a.shape) == tuple(b.shape) == tuple(ab.shape) == (k, ctx.n_limbs) and co.batches == 1
        opened = [co.open_share_array(v) for v in (a, b, ab)]
        out = [ctx.download_ints(v) for v in (a, b, ab)] + [ctx.download_ints(await h) for h in opened]
        if k == 20:                                                       # end to end: the triples multiply two dealt arrays
            x = ctx.upload_ints([(v + (i + 1) * s) % p for v, s in zip(xs, slopes[0])])
            y = ctx.upload_ints([(v + (i + 1) * s) % p for v, s in zip(ys, slopes[1])])
            out.append(ctx.download_ints(await co.open_share_array(await sa.beaver_multiply_arrays(co, x, y, (a, b, ab)))))
        return out

    results = _run_parties(p, n, t, body)
    for part in range(3):
        assert _check_sharings(p, n, t, [r[part] for r in results]) == results[0][3 + part]
    for r in results:
        assert r[3:6] == results[0][3:6] and r[5] == [x * y % p for x, y in zip(r[3], r[4])]
        if k == 20:
            assert r[6] == [x * y % p for x, y in zip(xs, ys)]
    assert len(set(results[0][3] + results[0][4])) == 2 * k


@pytest.mark.parametrize("n, t, k", [(4, 1, 10), (7, 2, 33)])
def test_generate_bits(n, t, k):
    from honeybadgermpc_amd import offline

    p = BLS
    ctx = _ctx(p)

    async def body(co, i):
        out = []
        for enc, seed in ((offline.PM1, 500), (offline.ZERO_ONE, 600)):
            before = co.batches
            bits = await offline.generate_bits(co, k, enc, tag=("bits", enc), generator=_generator(seed + i))
            assert tuple(bits.shape) == (k, ctx.n_limbs) and co.batches - before == 2
            out += [ctx.download_ints(bits), ctx.download_ints(await co.open_share_array(bits))]
        return out

    results = _run_parties(p, n, t, body)
    for which, allowed in ((0, {1, p - 1}), (2, {0, 1})):
        opened = results[0][which + 1]
        assert _check_sharings(p, n, t, [r[which] for r in results]) == opened and all(r[which + 1] == opened for r in results)
        assert set(opened) <= allowed
        if k == 33:
            assert set(opened) == allowed                                 # both values occur: 2^-32 that they would not


def test_generate_bits_finish_refuses_what_has_no_root():
    """the second open's result is public: a zero or a non-residue among it raises AssertionError, as the reference's sqrt does"""
    from honeybadgermpc_amd import offline

    p = BLS
    ctx = _ctx(p)
    nonres = next(v for v in range(2, 50) if pow(v, (p - 1) // 2, p) == p - 1)
    u = _random_tensor(ctx, 9, 300)
    good = [pow(v + 2, 2, p) for v in range(300)]
    assert ctx.download_ints(offline.invsqrt_scale(ctx, ctx.upload_ints(good), u, offline.ZERO_ONE))[:1] == [
        (ctx.download_ints(u[:1])[0] * offline.invsqrt_model(good[0], p)[0] + 1) * ((p + 1) // 2) % p]
    for pos, v in ((0, nonres), (299, nonres), (64, 0)):
        x = list(good)
        x[pos] = v
        for mode in (offline.PM1, offline.ZERO_ONE):
            with pytest.raises(AssertionError):
                offline.invsqrt_scale(ctx, ctx.upload_ints(x), u, mode)


@pytest.mark.parametrize("count", (1, 255, 256, 257, 513))
@pytest.mark.parametrize("p", (BLS, P64), ids=("bls", "2^64-59"))
def test_mul_add_equals_the_host_self_test(p, count):
    """One row body: the device's a b + c -- plain, with b the array a itself (the square) and written over c -- equals, bit for bit,
    what hb_selftest_off computes on the host from the same inputs: the self test runs the row the kernel runs, addressing included.
    Both instantiations; one lane, a full workgroup, one lane into a second, a ragged third."""
    import selftest_cases as stc
    from honeybadgermpc_amd import offline

    ctx = _ctx(p)
    nl = ctx.n_limbs
    rnd = random.Random(count)
    cols = []
    for shift in range(3):
        xs = [rnd.randrange(p) for _ in range(count)]
        for k, v in enumerate((0, 1, p - 1)):
            xs[(shift + k) % count] = v
        cols.append(xs)

    def same(dev, host):
        rc, want = host
        return rc == 0 and tuple(dev.shape) == (count, nl) and ctx.torch.equal(dev, ctx.upload_ints(want))

    a, b, c = (ctx.upload_ints(v) for v in cols)
    assert same(offline.mul_add(ctx, a, b, c), stc.run_off_mul_add(p, nl, *cols))
    assert same(offline.mul_add(ctx, a, a, c), stc.run_off_mul_add(p, nl, *cols, b_is_a=True))
    assert offline.mul_add(ctx, a, b, c, out=c) is c and same(c, stc.run_off_mul_add(p, nl, *cols, out_is=2))
    c = ctx.upload_ints(cols[2])
    assert offline.mul_add(ctx, a, a, c, out=c) is c and same(c, stc.run_off_mul_add(p, nl, *cols, b_is_a=True, out_is=2))
    ctx.torch.cuda.synchronize()

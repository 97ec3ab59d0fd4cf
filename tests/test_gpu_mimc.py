"""GPU: honeybadgermpc_amd.progs.mimc -- the kernels of csrc/hb_mimc.hip against tests/golden/mimc.json (the reference's own
mimc_plain), against Python ints and against the same round composed from share_arithmetic, and the whole protocol over an
OpenCoalescer (a shared x under a public key, public counters under a shared key, mimc_decrypt of mimc_encrypt).  Exact equality
everywhere."""
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


def _ctx(p):
    from honeybadgermpc_amd._capi import Context

    return Context.get(p)


def _golden():
    with open(os.path.join(REPO, "tests", "golden", "mimc.json")) as f:
        g = json.load(f)
    assert int(g["modulus"]) == BLS and g["ROUND"] == 161
    return [(int(c["x"]), int(c["k"]), int(c["out"])) for c in g["cases"]]


def _random_tensor(ctx, seed, count):
    """`count` uniform canonical residues made on the device side (numpy limbs, reduced by hb_reduce)"""
    g = np.random.default_rng(seed)
    limbs = g.integers(-(1 << 63), (1 << 63) - 1, size=(count, ctx.n_limbs), dtype=np.int64, endpoint=True)
    return ctx.reduce_(ctx.to_device(limbs))


def _draw(rnd, p, count):
    return [rnd.choice([0, 1, p - 1, rnd.randrange(p), rnd.randrange(p), rnd.randrange(p)]) for _ in range(count)]


def _round_ref(p, y, r, r2, r3, key, ctr, r_next):
    x3 = (y ** 3 + 3 * y * y * r + 3 * y * r2 + r3) % p
    return (x3 + key) % p if r_next is None else (x3 + key + ctr + 1 - r_next) % p


def _composed_round(ctx, y, r, r2, r3, key, ctr, r_next):
    """the same round from share_arithmetic alone (what the package offered before): key an int"""
    from honeybadgermpc_amd import share_arithmetic as sa

    y2 = sa.mul(ctx, y, y)
    x3 = sa.add(ctx, sa.add(ctx, sa.add(ctx, sa.mul(ctx, y2, y), sa.mul(ctx, sa.mul(ctx, y2, r), 3)), sa.mul(ctx, sa.mul(ctx, y, r2), 3)), r3)
    if r_next is None:
        return sa.add(ctx, x3, key)
    return sa.sub(ctx, sa.add(ctx, x3, (key + ctr + 1) % ctx.modulus), r_next)


# ---- the cleartext kernel -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [False, True], ids=["one", "pair"])
def test_plain_kernel_equals_the_golden_file(pair):
    from honeybadgermpc_amd.progs import mimc

    ctx = _ctx(BLS)
    cases = _golden()
    xs, ks, outs = ([c[i] for c in cases] for i in range(3))
    x_dev, k_dev = ctx.upload_ints(xs), ctx.upload_ints(ks)
    assert ctx.download_ints(mimc.mimc_plain_device(ctx, x_dev, k_dev, pair=pair)) == outs
    assert ctx.download_ints(mimc.mimc_plain_device(ctx, x_dev, k_dev, rounds=161, pair=pair)) == outs
    for x, k, out in cases[:3] + cases[-3:]:
        assert ctx.download_ints(mimc.mimc_plain_device(ctx, ctx.upload_ints([x] * 3), k, pair=pair)) == [out] * 3          # an int key
        assert ctx.download_ints(mimc.mimc_keystream(ctx, ctx.upload_ints([k]), 1, start=x, pair=pair)) == [out]           # a one-element key


@pytest.mark.parametrize("pair", [False, True], ids=["one", "pair"])
@pytest.mark.parametrize("p", FIELDS, ids=FIELD_IDS)
def test_plain_kernel_equals_python_ints_every_count(p, pair):
    from honeybadgermpc_amd.progs import mimc

    ctx = _ctx(p)
    rnd = random.Random(p % 997 + pair)
    rounds = mimc.rounds_for(p)
    for count in (0, 1, 255, 256, 257, 511, 513, 1 << 16):
        if count < 1 << 16:
            xs, ks = _draw(rnd, p, count), _draw(rnd, p, count)
            x_dev, k_dev = ctx.upload_ints(xs), ctx.upload_ints(ks)
            check = list(range(count))
        else:
            x_dev, k_dev = _random_tensor(ctx, 5, count), _random_tensor(ctx, 6, count)
            xs, ks = ctx.download_ints(x_dev), ctx.download_ints(k_dev)
            check = sorted({0, 1, 255, 256, 511, 512, count - 257, count - 256, count - 2, count - 1} | {rnd.randrange(count) for _ in range(300)})
        got = mimc.mimc_plain_device(ctx, x_dev, k_dev, pair=pair)
        assert tuple(got.shape) == (count, ctx.n_limbs)
        got = ctx.download_ints(got)
        assert [got[i] for i in check] == [mimc.mimc_plain(xs[i], ks[i], p, rounds) for i in check], count
        key = ks[0] if count else 5
        one = ctx.download_ints(mimc.mimc_plain_device(ctx, x_dev, key, pair=pair))
        assert [one[i] for i in check[:64]] == [mimc.mimc_plain(xs[i], key, p, rounds) for i in check[:64]], count
    # fewer rounds than the default
    xs, ks = _draw(rnd, p, 70), _draw(rnd, p, 70)
    for rounds in (1, 2, 7):
        got = ctx.download_ints(mimc.mimc_plain_device(ctx, ctx.upload_ints(xs), ctx.upload_ints(ks), rounds=rounds, pair=pair))
        assert got == [mimc.mimc_plain(x, k, p, rounds) for x, k in zip(xs, ks)], rounds


@pytest.mark.parametrize("p", [BLS, P64], ids=["bls", "2^64-59"])
def test_a_million_blocks(p):
    from honeybadgermpc_amd.progs import mimc

    ctx = _ctx(p)
    count = 1 << 20
    rnd = random.Random(20)
    key, start = rnd.randrange(p), p - 12345                      # the counters wrap past p inside the batch
    ms = _random_tensor(ctx, 9, count)
    stream = mimc.mimc_keystream(ctx, key, count, start=start)
    paired = mimc.mimc_keystream(ctx, key, count, start=start, pair=True)
    cs = mimc.mimc_encrypt(ctx, key, ms, start=start)
    assert ctx.torch.equal(stream, paired)
    sample = sorted({0, 1, 12344, 12345, 12346, count - 2, count - 1} | {rnd.randrange(count) for _ in range(1024)})
    assert len(sample) >= 1024
    idx = ctx.torch.tensor(sample, device=ctx.tdev)
    want = [mimc.mimc_plain((start + i) % p, key, p) for i in sample]
    assert ctx.download_ints(stream.index_select(0, idx)) == want
    m = ctx.download_ints(ms.index_select(0, idx))
    assert ctx.download_ints(cs.index_select(0, idx)) == [(a + b) % p for a, b in zip(m, want)]
    assert ctx.torch.equal(mimc.mimc_decrypt_plain(ctx, key, cs, start=start), ms)
    # x from an array, a key per element
    xs, ks = _random_tensor(ctx, 10, count), _random_tensor(ctx, 11, count)
    got = mimc.mimc_plain_device(ctx, xs, ks)
    xv, kv = ctx.download_ints(xs.index_select(0, idx)), ctx.download_ints(ks.index_select(0, idx))
    assert ctx.download_ints(got.index_select(0, idx)) == [mimc.mimc_plain(x, k, p) for x, k in zip(xv, kv)]
    assert ctx.torch.equal(mimc.mimc_plain_device(ctx, xs, ks, pair=True), got)


@pytest.mark.parametrize("p", FIELDS, ids=FIELD_IDS)
def test_keystream_encrypt_and_cleartext_decrypt(p):
    from honeybadgermpc_amd.progs import mimc

    ctx = _ctx(p)
    rnd = random.Random(p % 991)
    for count in (1, 100, 700):
        ms = _draw(rnd, p, count)
        m_dev = ctx.upload_ints(ms)
        keep = m_dev.clone()
        for key, start in ((rnd.randrange(p), 0), (p - 1, p - 3), (0, rnd.randrange(p))):
            f = [mimc.mimc_plain((start + i) % p, key, p) for i in range(count)]
            for pair in (False, True):
                assert ctx.download_ints(mimc.mimc_keystream(ctx, key, count, start=start, pair=pair)) == f
                cs = mimc.mimc_encrypt(ctx, key, m_dev, start=start, pair=pair)
                assert ctx.download_ints(cs) == [(m + v) % p for m, v in zip(ms, f)]
                assert ctx.torch.equal(mimc.mimc_decrypt_plain(ctx, key, cs, start=start, pair=pair), m_dev)
            # the reference's mimc_encrypt counts from 0; a start beyond the modulus is taken mod p
            assert ctx.torch.equal(mimc.mimc_encrypt(ctx, key, m_dev, start=start + p), cs)
        # a key per element, and in place
        ks = _draw(rnd, p, count)
        buf = m_dev.clone()
        assert mimc.mimc_encrypt(ctx, ctx.upload_ints(ks), buf, start=7 % p, out=buf) is buf
        assert ctx.download_ints(buf) == [(m + mimc.mimc_plain((7 + i) % p, k, p)) % p for i, (m, k) in enumerate(zip(ms, ks))]
        assert ctx.torch.equal(m_dev, keep)
    assert tuple(mimc.mimc_keystream(ctx, 3, 0).shape) == (0, ctx.n_limbs)


# ---- the round kernels --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", FIELDS, ids=FIELD_IDS)
def test_round_and_first_mask_equal_python_ints_and_the_composition(p):
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd.progs import mimc

    ctx = _ctx(p)
    rnd = random.Random(p % 983)
    for count in (1, 255, 256, 257, 5000):
        y, r, r2, r3, rn, ks, xs = (_draw(rnd, p, count) for _ in range(7))
        if count == 257:
            y, r, r2, r3, rn, ks = ([p - 1] * count for _ in range(6))                      # the largest operands
        d = {w: ctx.upload_ints(v) for w, v in (("y", y), ("r", r), ("r2", r2), ("r3", r3), ("rn", rn), ("k", ks), ("x", xs))}
        key = ks[0]
        for ctr in (0, 7, 159, 160):
            for r_next, rnv in ((d["rn"], rn), (None, [None] * count)):
                got = mimc.cube_round(ctx, d["y"], d["r"], d["r2"], d["r3"], key, ctr, r_next=r_next)
                assert tuple(got.shape) == (count, ctx.n_limbs)
                assert ctx.download_ints(got) == [_round_ref(p, *t, key, ctr, n) for *t, n in zip(y, r, r2, r3, rnv)], (count, ctr)
                assert ctx.torch.equal(got, _composed_round(ctx, d["y"], d["r"], d["r2"], d["r3"], key, ctr, r_next)), (count, ctr)
                per = mimc.cube_round(ctx, d["y"], d["r"], d["r2"], d["r3"], d["k"], ctr, r_next=r_next)
                assert ctx.download_ints(per) == [_round_ref(p, *t, k, ctr, n) for *t, k, n in zip(y, r, r2, r3, ks, rnv)], (count, ctr)
        first = mimc.first_mask(ctx, d["x"], key, d["r"])
        assert ctx.download_ints(first) == [(a + key - b) % p for a, b in zip(xs, r)]
        assert ctx.torch.equal(first, sa.sub(ctx, sa.add(ctx, d["x"], key), d["r"]))
        assert ctx.download_ints(mimc.first_mask(ctx, d["x"], d["k"], d["r"])) == [(a + k - b) % p for a, k, b in zip(xs, ks, r)]
        for start in (0, p - 2, rnd.randrange(p), p + 5):
            got = mimc.first_mask(ctx, None, d["k"], d["r"], start=start)
            assert ctx.download_ints(got) == [(start + i + k - b) % p for i, (k, b) in enumerate(zip(ks, r))], start


def test_inputs_untouched_out_given_arguments_checked_and_asynchronous():
    from honeybadgermpc_amd import share_arithmetic as sa
    from honeybadgermpc_amd._capi import HB_ERR_BAD_ARG, HB_MIMC_SUB
    from honeybadgermpc_amd.progs import mimc

    p, count, ctr = BLS, 600, 5
    ctx = _ctx(p)
    torch = ctx.torch
    rnd = random.Random(4)
    y, r, r2, r3, rn, ks, xs = (_draw(rnd, p, count) for _ in range(7))
    ops = [ctx.upload_ints(v) for v in (y, r, r2, r3, rn, ks, xs)]
    y_d, r_d, r2_d, r3_d, rn_d, k_d, x_d = ops
    copies = [t.clone() for t in ops]
    key = ks[0]
    want = [_round_ref(p, *t, key, ctr, n) for *t, n in zip(y, r, r2, r3, rn)]
    want_last = [_round_ref(p, *t, key, ctr, None) for t in zip(y, r, r2, r3)]
    want_first = [(a + key - b) % p for a, b in zip(xs, r)]
    want_f = [mimc.mimc_plain(x, key, p, 9) for x in xs]
    # results consumed on the current stream without a synchronise, through another kernel of the library
    out = mimc.cube_round(ctx, y_d, r_d, r2_d, r3_d, key, ctr, r_next=rn_d)
    f = mimc.mimc_plain_device(ctx, x_d, key, rounds=9)
    assert ctx.download_ints(sa.add(ctx, out, out)) == [2 * v % p for v in want]
    assert ctx.download_ints(sa.neg(ctx, f)) == [-v % p for v in want_f]
    # on a side stream as well
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        o2 = mimc.cube_round(ctx, y_d, r_d, r2_d, r3_d, key, ctr)
        twice = sa.add(ctx, o2, o2)
        f2 = sa.add(ctx, mimc.first_mask(ctx, x_d, key, r_d), 1)
    side.synchronize()
    assert ctx.download_ints(twice) == [2 * v % p for v in want_last] and ctx.download_ints(f2) == [(v + 1) % p for v in want_first]
    # out given: written where asked, and handed back
    buf = ctx.empty(count)
    assert mimc.cube_round(ctx, y_d, r_d, r2_d, r3_d, key, ctr, r_next=rn_d, out=buf) is buf and ctx.download_ints(buf) == want
    assert mimc.cube_round(ctx, y_d, r_d, r2_d, r3_d, key, ctr, out=buf) is buf and ctx.download_ints(buf) == want_last
    assert mimc.first_mask(ctx, x_d, key, r_d, out=buf) is buf and ctx.download_ints(buf) == want_first
    assert mimc.mimc_plain_device(ctx, x_d, key, rounds=9, out=buf) is buf and ctx.download_ints(buf) == want_f
    assert all(torch.equal(t, c) for t, c in zip(ops, copies))
    assert out.data_ptr() not in {t.data_ptr() for t in ops}
    # in place over a same-index input
    yy = y_d.clone()
    assert mimc.cube_round(ctx, yy, r_d, r2_d, r3_d, key, ctr, r_next=rn_d, out=yy) is yy and ctx.download_ints(yy) == want
    xx = x_d.clone()
    assert mimc.mimc_plain_device(ctx, xx, key, rounds=9, out=xx, pair=True) is xx and ctx.download_ints(xx) == want_f
    # a strided view of an input is taken as its values
    wide = torch.zeros((count, 2, ctx.n_limbs), dtype=torch.int64, device=ctx.tdev)
    wide[:, 0] = y_d
    assert ctx.download_ints(mimc.cube_round(ctx, wide[:, 0], r_d, r2_d, r3_d, key, ctr, r_next=rn_d)) == want
    # argument checks raise before C and nothing is launched: the output buffer keeps its contents
    buf.fill_(7)
    seven = buf.clone()
    one_key = ctx.upload_ints([key])
    bad_calls = [
        lambda: mimc.cube_round(ctx, y_d, r_d[:-1], r2_d, r3_d, key, ctr, out=buf),                     # a short operand
        lambda: mimc.cube_round(ctx, y_d, r_d, r2_d, r3_d, key, ctr, r_next=rn_d[:3], out=buf),
        lambda: mimc.cube_round(ctx, y_d, r_d, r2_d, torch.cat([r3_d, r3_d]), key, ctr, out=buf),        # a long one
        lambda: mimc.cube_round(ctx, y_d, r_d, r2_d, r3_d, key, ctr, out=buf[:-1]),                      # a short out
        lambda: mimc.cube_round(ctx, y_d, r_d, r2_d, r3_d, key, ctr, out=torch.zeros((2 * count, ctx.n_limbs), dtype=torch.int64, device=ctx.tdev)[::2]),
        lambda: mimc.cube_round(ctx, y_d, r_d, r2_d, r3_d, k_d[:5], ctr, out=buf),                       # a key of neither 1 nor count elements
        lambda: mimc.cube_round(ctx, y_d, r_d, r2_d, r3_d, key, -1, out=buf),
        lambda: mimc.cube_round(ctx, y_d, r_d, r2_d, r3_d, key, 1.0, out=buf),
        lambda: mimc.cube_round(ctx, y_d.cpu(), r_d, r2_d, r3_d, key, ctr, out=buf),                     # another device
        lambda: mimc.cube_round(ctx, y_d, r_d, r2_d, r3_d, k_d.cpu(), ctr, out=buf),
        lambda: mimc.cube_round(ctx, y_d[:, :2], r_d, r2_d, r3_d, key, ctr, out=buf),                    # not `limbs` wide
        lambda: mimc.first_mask(ctx, x_d[:-1], key, r_d, out=buf),
        lambda: mimc.first_mask(ctx, x_d, k_d[:2], r_d, out=buf),
        lambda: mimc.first_mask(ctx, x_d, key, r_d, out=buf[:10]),
        lambda: mimc.mimc_plain_device(ctx, x_d, key, rounds=0, out=buf),
        lambda: mimc.mimc_plain_device(ctx, x_d, key, rounds=-3, out=buf),
        lambda: mimc.mimc_plain_device(ctx, x_d, k_d[:7], out=buf),
        lambda: mimc.mimc_plain_device(ctx, x_d, key, out=buf[:5]),
        lambda: mimc.mimc_encrypt(ctx, key, x_d, rounds=2.0, out=buf),
        lambda: mimc.mimc_keystream(ctx, key, -1),
        lambda: mimc.cube_round(ctx, y_d[:1], r_d[:1], r2_d[:1], r3_d[:1], k_d[:2], ctr, out=buf[:1]),
    ]
    for call in bad_calls:
        with pytest.raises(ValueError):
            call()
    for call in (
        lambda: mimc.cube_round(ctx, y_d.to(torch.int32), r_d, r2_d, r3_d, key, ctr, out=buf),
        lambda: mimc.cube_round(ctx, y, r_d, r2_d, r3_d, key, ctr, out=buf),
        lambda: mimc.cube_round(ctx, y_d, r_d, r2_d, r3_d, 1.5, ctr, out=buf),
        lambda: mimc.first_mask(ctx, None, key, r_d, start=1.5, out=buf),
        lambda: mimc.mimc_keystream(ctx, key, 4, start="0"),
    ):
        with pytest.raises(TypeError):
            call()
    assert torch.equal(buf, seven)
    # ... and the C ABI refuses what gets past Python
    lib, st = ctx.lib, ctx.stream()
    P = ctx.ptr
    good = [P(y_d), P(r_d), P(r2_d), P(r3_d), P(one_key)]
    assert lib.hb_mimc_round(ctx.h, *good, 1, ctr, P(rn_d), P(buf), -1, st) == HB_ERR_BAD_ARG
    assert lib.hb_mimc_round(ctx.h, *good, 1, -1, P(rn_d), P(buf), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_mimc_round(ctx.h, *good, 1, ctr, P(rn_d), None, count, st) == HB_ERR_BAD_ARG
    assert lib.hb_mimc_round(ctx.h, *good, 1, ctr, P(rn_d), P(one_key), count, st) == HB_ERR_BAD_ARG     # out is the key for all
    for i in range(5):
        args = list(good)
        args[i] = None
        assert lib.hb_mimc_round(ctx.h, *args, 1, ctr, P(rn_d), P(buf), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_mimc_first(ctx.h, P(x_d), None, None, 1, P(r_d), P(buf), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_mimc_first(ctx.h, P(x_d), None, P(one_key), 1, None, P(buf), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_mimc_first(ctx.h, P(x_d), None, P(one_key), 1, P(r_d), None, count, st) == HB_ERR_BAD_ARG
    assert lib.hb_mimc_first(ctx.h, P(x_d), None, P(one_key), 1, P(r_d), P(buf), -2, st) == HB_ERR_BAD_ARG
    too_big = ctx.host_elems([0])
    too_big[:] = np.frombuffer(int(p).to_bytes(32, "little"), dtype=np.uint64)                           # start == p
    assert lib.hb_mimc_first(ctx.h, None, too_big.ctypes.data, P(one_key), 1, P(r_d), P(buf), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_mimc_plain(ctx.h, None, too_big.ctypes.data, P(one_key), 1, None, 0, 9, P(buf), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_mimc_plain(ctx.h, P(x_d), None, P(one_key), 1, None, 0, 0, P(buf), count, st) == HB_ERR_BAD_ARG        # rounds < 1
    assert lib.hb_mimc_plain(ctx.h, P(x_d), None, P(one_key), 1, None, 0, 9, P(buf), -1, st) == HB_ERR_BAD_ARG
    assert lib.hb_mimc_plain(ctx.h, P(x_d), None, None, 1, None, 0, 9, P(buf), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_mimc_plain(ctx.h, P(x_d), None, P(one_key), 1, None, 0, 9, None, count, st) == HB_ERR_BAD_ARG
    assert lib.hb_mimc_plain(ctx.h, P(x_d), None, P(one_key), 1, None, HB_MIMC_SUB, 9, P(buf), count, st) == HB_ERR_BAD_ARG
    assert lib.hb_mimc_plain(ctx.h, P(x_d), None, P(one_key), 1, None, 8, 9, P(buf), count, st) == HB_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert torch.equal(buf, seven) and all(torch.equal(t, c) for t, c in zip(ops, copies))
    assert lib.hb_mimc_round(ctx.h, *good, 1, ctr, P(rn_d), P(buf), 0, st) == 0 and torch.equal(buf, seven)               # count == 0: nothing launched
    assert lib.hb_mimc_plain(ctx.h, P(x_d), None, P(one_key), 1, None, 0, 9, P(buf), 0, st) == 0 and torch.equal(buf, seven)
    assert lib.hb_mimc_round(ctx.h, *good, 1, ctr, P(rn_d), P(buf), count, st) == 0
    assert ctx.download_ints(buf) == want


# ---- the protocol, end to end over the in-process tagged network of tests/test_gpu_butterfly_network.py ----------------------
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
    out = [[0] * len(values) for _ in range(n)]
    for k, v in enumerate(values):
        coeffs = [rnd.randrange(p) for _ in range(degree)]
        for i in range(n):
            acc = 0
            for co in reversed(coeffs):
                acc = (acc + co) * (i + 1) % p
            out[i][k] = (acc + v) % p
    return out


def _deal_cubes(ctx, rnd, p, n, t, rounds, count):
    """-> [party] of (r, r2, r3) tensors (rounds, count, limbs): cubes dealt from Python ints"""
    rs = [rnd.randrange(p) for _ in range(rounds * count)]
    dealt = [_deal(rnd, p, n, t, vals) for vals in (rs, [v * v % p for v in rs], [v * v * v % p for v in rs])]
    return [tuple(ctx.upload_ints(d[i]).reshape(rounds, count, ctx.n_limbs) for d in dealt) for i in range(n)]


def _run_parties(p, n, t, bad, rnd, body):
    """every party runs `body(co, i)` over its own OpenCoalescer -> ([result per party], {batches per party})"""
    from honeybadgermpc_amd import wire
    from honeybadgermpc_amd.open_coalescer import OpenCoalescer

    def garble(msg):
        tag, blob = msg
        count = wire.unpack_limbs(blob).shape[0]
        return (tag, wire.pack_ints([rnd.randrange(p) for _ in range(count)], p))

    batches = set()

    async def party(i, net):
        co = OpenCoalescer(p, n, t, i, net.get_send_recv(i, garble if i in bad else None))
        res = await body(co, i)
        batches.add(co.batches)
        return res

    async def main():
        net = _TaggedNet(n)
        return await asyncio.gather(*[party(i, net) for i in range(n)])

    results = asyncio.run(main())
    _ctx(p).torch.cuda.synchronize()
    return results, batches


@pytest.mark.parametrize("n, t, liars", [(4, 1, 0), (7, 2, 0), (4, 1, 1), (7, 2, 2)])
@pytest.mark.parametrize("count", [1, 20, 256])
def test_protocol_end_to_end(n, t, liars, count):
    from honeybadgermpc_amd.progs import mimc

    p = BLS
    ctx = _ctx(p)
    rounds = mimc.ROUND
    rnd = random.Random(1000 * n + 10 * count + liars)
    bad = set(rnd.sample(range(n), liars))
    honest = [i for i in range(n) if i not in bad]
    cases = _golden()[-count:] if count < 41 else _golden()
    # (a) shared x under a public key (a key per element: the golden pairs come first), mimc_mpc_batch
    xs = [c[0] for c in cases] + [rnd.randrange(p) for _ in range(count - len(cases))]
    ks = [c[1] for c in cases] + [rnd.randrange(p) for _ in range(count - len(cases))]
    x_shares = _deal(rnd, p, n, t, xs)
    cubes = _deal_cubes(ctx, rnd, p, n, t, rounds, count)
    key_dev = ctx.upload_ints(ks)

    async def encrypt_shared(co, i):
        inputs = ctx.upload_ints(x_shares[i])
        before = inputs.clone()
        shares = await mimc.mimc_mpc_batch(co, inputs, key_dev, cubes[i])
        assert ctx.torch.equal(inputs, before) and shares.data_ptr() != inputs.data_ptr() and tuple(shares.shape) == (count, ctx.n_limbs)
        return ctx.download_ints(await co.open_share_array(shares))

    results, batches = _run_parties(p, n, t, bad, rnd, encrypt_shared)
    want = [mimc.mimc_plain(x, k) for x, k in zip(xs, ks)]
    assert want[:len(cases)] == [c[2] for c in cases]
    for i in honest:
        assert results[i] == want, i
    assert batches == {rounds + 1}                                       # one open a round, and one for the result
    # (b) public counters under a shared key: mimc_decrypt of mimc_encrypt's output opens to the messages
    key, start = rnd.randrange(p), rnd.choice([0, p - 3, rnd.randrange(p)])
    ms = [rnd.randrange(p) for _ in range(count)]
    ms[0] = p - 1
    cs = mimc.mimc_encrypt(ctx, key, ctx.upload_ints(ms), start=start)
    cs_before = cs.clone()
    key_shares = _deal(rnd, p, n, t, [key])
    cubes = _deal_cubes(ctx, rnd, p, n, t, rounds, count)

    async def decrypt(co, i):
        shares = await mimc.mimc_decrypt(co, ctx.upload_ints(key_shares[i]), cs, cubes[i], start=start)
        return ctx.download_ints(await co.open_share_array(shares))

    results, batches = _run_parties(p, n, t, bad, rnd, decrypt)
    assert ctx.torch.equal(cs, cs_before)
    assert ctx.download_ints(cs) == [(m + mimc.mimc_plain((start + i) % p, key)) % p for i, m in enumerate(ms)]
    for i in honest:
        assert results[i] == ms, i
    assert batches == {rounds + 1}


def test_protocol_fewer_rounds_narrow_field_and_bad_cubes():
    """the 8-byte width with its own round count (41 over 2^64 - 59), an explicit `rounds`, a key for all as an int, and the
    shape checks of the coroutines"""
    from honeybadgermpc_amd.progs import mimc

    p, n, t, count = P64, 4, 1, 33
    ctx = _ctx(p)
    rnd = random.Random(64)
    xs = _draw(rnd, p, count)
    key = rnd.randrange(p)
    x_shares = _deal(rnd, p, n, t, xs)
    for rounds in (None, 3):
        nr = mimc.rounds_for(p) if rounds is None else rounds
        assert nr == (41 if rounds is None else 3)
        cubes = _deal_cubes(ctx, rnd, p, n, t, nr + 1, count)            # a row more than needed is fine

        async def body(co, i):
            shares = await mimc.mimc_mpc_batch(co, ctx.upload_ints(x_shares[i]), key, cubes[i], rounds=rounds)
            return ctx.download_ints(await co.open_share_array(shares))

        results, batches = _run_parties(p, n, t, set(), rnd, body)
        assert all(res == [mimc.mimc_plain(x, key, p, nr) for x in xs] for res in results) and batches == {nr + 1}
    r, r2, r3 = cubes[0]
    x0 = ctx.upload_ints(x_shares[0])

    async def refused(co, i):
        if i:
            return None
        for bad in ((r[:2], r2, r3), (r, r2[:, :5], r3), (r, r2), (r, r2, r3.reshape(-1, ctx.n_limbs)), (r, r2, r3.cpu()), None):
            with pytest.raises(ValueError):
                await mimc.mimc_mpc_batch(co, x0, key, bad, rounds=3)
        with pytest.raises(ValueError):
            await mimc.mimc_mpc_batch(co, x0[:5], key, (r, r2, r3), rounds=3)
        with pytest.raises(ValueError):
            await mimc.mimc_decrypt(co, x0[:1], x0[:7], (r, r2, r3), rounds=3)
        with pytest.raises(ValueError):
            await mimc.mimc_mpc_batch(co, x0, key, (r, r2, r3), rounds=0)
        return co.batches

    results, _ = _run_parties(p, n, t, set(), rnd, refused)
    assert results[0] == 0                                               # nothing was opened


def _with_corners(rnd, p, count, shift):
    """random residues with 0, 1 and p - 1 among them, at positions that differ from operand to operand"""
    xs = [rnd.randrange(p) for _ in range(count)]
    for k, v in enumerate((0, 1, p - 1)):
        xs[(shift + k) % count] = v
    return xs


@pytest.mark.parametrize("count", (1, 255, 256, 257, 513))
@pytest.mark.parametrize("p", (BLS, P64), ids=("bls", "2^64-59"))
def test_first_and_round_equal_the_host_self_test(p, count):
    """One row body: the device's first mask (x an array, and the counters from start = p - 3, which wrap) and its cubing round (last
    and not, ctr = 0 and 2^62), each under a key for all and a key an element, equal, bit for bit, what hb_selftest_mimc computes on the
    host from the same inputs: the self test runs the rows the kernels run, addressing included.  Both instantiations; one lane, a
    full workgroup, one lane into a second, a ragged third."""
    import selftest_cases as stc
    from honeybadgermpc_amd.progs import mimc

    ROUND, FIRST = 1, 2
    ctx = _ctx(p)
    torch, nl = ctx.torch, ctx.n_limbs
    rnd = random.Random(7 * count + nl)
    x, r0, y, r, r2, r3, rn, keys = (_with_corners(rnd, p, count, k) for k in range(8))

    def same(dev, host):
        rc, want = host
        return rc == 0 and tuple(dev.shape) == (count, nl) and torch.equal(dev, ctx.upload_ints(want))

    up = ctx.upload_ints
    for key, bcast in [(k, 1) for k in (0, 1, p - 1, rnd.randrange(p))] + [(keys, 0)]:
        kdev, khost = (key, [key]) if bcast else (up(key), key)
        assert same(mimc.first_mask(ctx, up(x), kdev, up(r0)), stc.run_mimc(p, nl, FIRST, [x, khost, r0], count, bcast=bcast)), (bcast, key)
        assert same(mimc.first_mask(ctx, None, kdev, up(r0), start=p - 3), stc.run_mimc(p, nl, FIRST, [None, khost, r0], count, start=p - 3, bcast=bcast)), (bcast, key)
        for ctr in (0, 1 << 62):
            for nxt in (rn, None):
                got = mimc.cube_round(ctx, up(y), up(r), up(r2), up(r3), kdev, ctr, None if nxt is None else up(nxt))
                assert same(got, stc.run_mimc(p, nl, ROUND, [y, r, r2, r3, khost, nxt], count, arg=ctr, bcast=bcast)), (bcast, key, ctr, nxt is None)
    torch.cuda.synchronize()

"""GPU: the G1 kernels (csrc/hb_g1.hip) through honeybadgermpc_amd.g1 and poly_commit_lin.PolyCommitLin against the host model
honeybadgermpc_amd.bls12_381, bit-equal to hb_selftest_g1 (the same bodies on the host) on the same inputs.  Counts sit at the edge of a
256-thread workgroup; edge scalars and exceptional operands sit at the first and last index (g1_support's cases).  Exact equality."""
import random

import numpy as np
import pytest

import g1_support as s
from g1_support import ADD, CHECK, COMMIT, EVAL, SCALAR_MUL, SUBTRACT, VERIFY

from honeybadgermpc_amd.bls12_381 import G1, Q, R

pytestmark = pytest.mark.gpu

COUNTS = [1, 255, 256, 257]


@pytest.fixture(scope="module")
def ctx():
    from honeybadgermpc_amd._capi import Context

    return Context.get(R)


_fixed = {}


def fixed(ctx, c, which="h"):
    """device tables (tg, th) of g1_support.crs() (or of h = 2^c g), built once a module"""
    from honeybadgermpc_amd import g1

    if (c, which) not in _fixed:
        g, h = s.crs()
        if which == "shift":
            h = g ** (1 << c)
        _fixed[c, which] = (g1.FixedBase(ctx, g, c), g1.FixedBase(ctx, h, c))
    return _fixed[c, which]


def dev_points(ctx, arr):
    return ctx.torch.from_numpy(np.ascontiguousarray(arr).view(np.int64).reshape(-1, 2, 6)).to(ctx.tdev)


def dev_scalars(ctx, values):
    return ctx.torch.from_numpy(s.words(values, 4).view(np.int64)).to(ctx.tdev)


def host(t):
    return t.cpu().numpy().view(np.uint64).reshape(-1)


@pytest.mark.parametrize("count", COUNTS)
def test_scalar_mul(ctx, count):
    from honeybadgermpc_amd import g1

    ks, ps = s.scalar_mul_case(count, seed=count)
    got = host(g1.scalar_mul(ctx, dev_scalars(ctx, ks), dev_points(ctx, s.points(ps))))
    rc, ref = s.selftest(SCALAR_MUL, [s.words(ks, 4), s.points(ps)], 0, 0, count, 12 * count)
    assert rc == 0 and np.array_equal(got, ref[:12 * count])
    assert s.unpoints(got) == [s.mul_model(k, p) for k, p in zip(ks, ps)]


def test_scalar_mul_vectors_and_broadcasts(ctx):
    from honeybadgermpc_amd import g1

    vs = s.vectors()[:257]
    g = G1.generator()
    got = host(g1.scalar_mul(ctx, dev_scalars(ctx, range(257)), g))
    assert np.array_equal(got.reshape(257, 12), s.points(vs))
    out = ctx.torch.empty((257, 2, 6), dtype=ctx.torch.int64, device=ctx.tdev)
    assert g1.scalar_mul(ctx, -3, dev_points(ctx, s.points(vs)), out=out) is out
    assert s.unpoints(host(out)) == [p ** -3 for p in vs]
    assert s.unpoints(host(g1.scalar_mul(ctx, R + 2, g))) == [g ** 2]
    assert g1.scalar_mul(ctx, dev_scalars(ctx, []), dev_points(ctx, np.zeros((0, 12), dtype=np.uint64))).shape == (0, 2, 6)


@pytest.mark.parametrize("count", COUNTS)
def test_add_sub_neg_check(ctx, count):
    from honeybadgermpc_amd import g1

    pairs = s.add_case(count, seed=count)
    P, Qs = s.points([p for p, _ in pairs]), s.points([q for _, q in pairs])
    dp, dq = dev_points(ctx, P), dev_points(ctx, Qs)
    for fn, flags, model in ((g1.add, 0, lambda p, q: p * q), (g1.sub, SUBTRACT, lambda p, q: p / q)):
        got = host(fn(ctx, dp, dq))
        rc, ref = s.selftest(ADD, [P, Qs], flags, 0, count, 12 * count)
        assert rc == 0 and np.array_equal(got, ref[:12 * count])
        assert s.unpoints(got) == [model(p, q) for p, q in pairs]
    assert s.unpoints(host(g1.neg(ctx, dp))) == [p.invert() for p, _ in pairs]
    # the check: every point of the case is on the curve; a point off it and a coordinate not below Q at both ends are told apart
    raw = [row.tolist() for row in P]
    want = [1] * count
    g = G1.generator()
    for at, words in ((0, s.off_curve_raw()), (count - 1, s.raw_point(g.x + Q, g.y))):
        raw[at], want[at] = words, 0
    flags = g1.on_curve(ctx, dev_points(ctx, s.points(raw)))
    rc, ref = s.selftest(CHECK, [s.points(raw)], 0, 0, count, count)
    assert flags.dtype == ctx.torch.bool and flags.cpu().tolist() == [bool(v) for v in want] == [bool(v) for v in ref.view(np.int32)[:count]]


def test_in_subgroup(ctx):
    from honeybadgermpc_amd import g1

    p = s.off_subgroup_point()
    ps = [p] + s.vectors()[:255] + [p, s.vectors()[999]]
    got = g1.in_subgroup(ctx, g1.upload(ps, ctx))
    assert got.cpu().tolist() == [False] + [True] * 255 + [False, True]
    assert g1.download(g1.upload(ps)) == ps


@pytest.mark.parametrize("c", [4, 8])
def test_table_is_bit_equal_to_the_host_build(ctx, c):
    tg, th = fixed(ctx, c)
    hg, hh = s.tables(c)
    n = (256 // c) * ((1 << c) - 1) * 32 // 2                 # the entries; what lies behind them is scratch
    assert np.array_equal(host(tg.table)[:n], hg[:n]) and np.array_equal(host(th.table)[:n], hh[:n])


@pytest.mark.parametrize("c", [4, 8])
@pytest.mark.parametrize("count", COUNTS)
def test_commit(ctx, c, count):
    from honeybadgermpc_amd import g1

    g, h = s.crs()
    a, b = s.commit_case(count, c, seed=count + c)
    got = host(g1.commit(ctx, *fixed(ctx, c), dev_scalars(ctx, a), dev_scalars(ctx, b)))
    rc, ref = s.selftest(COMMIT, [s.words(a, 4), s.words(b, 4), *s.tables(c)], 0, c, count, 12 * count)
    assert rc == 0 and np.array_equal(got, ref[:12 * count])
    some = sorted(set(list(range(min(count, 16))) + list(range(max(count - 16, 0), count))))
    pts = s.unpoints(got)
    assert [pts[k] for k in some] == [s.mul_model(a[k], g) * s.mul_model(b[k], h) for k in some]


@pytest.mark.parametrize("c", [4, 8])
def test_commit_meets_equal_operands_inside_the_comb(ctx, c):
    from honeybadgermpc_amd import g1

    g, _ = s.crs()
    hs = g ** (1 << c)
    d = (1 << c) - 1
    a = [5 << c, d << c, (3 << c) | (7 << (2 * c)), 1 << c, 0] * 52
    b = [5, d, 3 | (7 << c), 1, 1] * 52
    got = s.unpoints(host(g1.commit(ctx, *fixed(ctx, c, "shift"), dev_scalars(ctx, a), dev_scalars(ctx, b))))
    want = [g ** x * hs ** y for x, y in zip(a[:5], b[:5])]
    assert got == want * 52


def check_eval_and_verify(ctx, B, t, i, c, bad, seed):
    from honeybadgermpc_amd import g1

    cs, shares, wits, want = s.verify_case(B, t, i, bad=bad, seed=seed)
    flat = s.flat_points(cs)
    dcs = dev_points(ctx, flat).reshape(B, t + 1, 2, 6)
    verdict, counter = g1.verify(ctx, *fixed(ctx, c), dcs, i, dev_scalars(ctx, shares), dev_scalars(ctx, wits))
    rc, ref = s.selftest(VERIFY, [flat, s.words(shares, 4), s.words(wits, 4), *s.tables(c)], (t + 1) | (c << 16), i, B, (B + 2) // 2 + 1)
    assert rc == 0
    assert verdict.cpu().tolist() == want == ref.view(np.int32)[:B].tolist()
    assert int(counter.item()) == len(bad) == int(ref.view(np.int32)[B])
    # the Horner side alone, on the items whose commitments are all curve points
    got = host(g1.eval_commitments(ctx, dcs, i))
    rc, ref = s.selftest(EVAL, [flat], t + 1, i, B, 12 * B)
    assert rc == 0 and np.array_equal(got, ref[:12 * B])
    on = [b for b in range(B) if all(isinstance(p, G1) for p in cs[b])]
    some = [b for b in on if b < 4 or b >= B - 4]
    pts = got.reshape(B, 12)
    assert [G1.from_limbs(pts[b].tolist()) for b in some] == [s.eval_model(cs[b], i) for b in some]


KINDS = ["share", "witness", "swap", "off"]


@pytest.mark.parametrize("i", [1, 3, 64])
def test_eval_and_verify_257_items(ctx, i):
    check_eval_and_verify(ctx, 257, 2, i, 8, [], seed=i)
    bad = [(0, KINDS[i % 4]), (255, KINDS[(i + 1) % 4]), (256, KINDS[(i + 2) % 4])]
    check_eval_and_verify(ctx, 257, 2, i, 4, bad, seed=i + 100)


@pytest.mark.parametrize("kind", KINDS)
def test_verify_one_bad_item_of_each_kind_at_each_position(ctx, kind):
    for pos in (0, 255, 256):
        check_eval_and_verify(ctx, 257, 2, 3, 8, [(pos, kind)], seed=pos)


def test_eval_and_verify_degree_21(ctx):
    check_eval_and_verify(ctx, 3, 21, 64, 8, [], seed=5)
    check_eval_and_verify(ctx, 3, 21, 64, 8, [(1, "swap")], seed=6)


@pytest.mark.parametrize("count", COUNTS)
def test_eval_exceptional_entries_and_indices(ctx, count):
    from honeybadgermpc_amd import g1

    cs = s.eval_case(count, 3, seed=count)
    flat = s.flat_points(cs)
    dcs = dev_points(ctx, flat).reshape(count, 3, 2, 6)
    for i in (0, 1, 2, 255, 65535, (1 << 32) - 1):
        got = host(g1.eval_commitments(ctx, dcs, i))
        rc, ref = s.selftest(EVAL, [flat], 3, i, count, 12 * count)
        assert rc == 0 and np.array_equal(got, ref[:12 * count]), i
        pts = got.reshape(count, 12)
        some = sorted(set(list(range(min(count, 6))) + list(range(max(count - 6, 0), count))))
        assert [G1.from_limbs(pts[b].tolist()) for b in some] == [s.eval_model(cs[b], i) for b in some], i


@pytest.mark.parametrize("n,t", [(4, 1), (7, 2)])
def test_poly_commit_lin_end_to_end(ctx, n, t):
    from honeybadgermpc_amd import g1, ntl
    from honeybadgermpc_amd.field import GF
    from honeybadgermpc_amd.poly_commit_lin import PolyCommitLin
    from honeybadgermpc_amd.polynomial import polynomials_over

    rnd = random.Random(n)
    g, h = s.crs()
    pc = PolyCommitLin([g, h], ctx=ctx)
    pc.preprocess(8)
    B = 5
    coeffs = [[rnd.randrange(R) for _ in range(t + 1)] for _ in range(B)]
    dco = dev_scalars(ctx, [c for row in coeffs for c in row]).reshape(B, t + 1, 4)
    cs, hat = pc.commit_batch(dco)
    assert cs.shape == (B, t + 1, 2, 6) and hat.shape == (B, t + 1, 4)
    hat_rows = [ctx.download_ints(hat[b]) for b in range(B)]
    assert all(0 <= v < R for row in hat_rows for v in row) and len({v for row in hat_rows for v in row}) == B * (t + 1)
    assert g1.download(cs) == [g ** coeffs[b][j] * h ** hat_rows[b][j] for b in range(B) for j in range(t + 1)]
    cs2, hat2 = pc.commit_batch(dco, hat=hat)
    assert ctx.torch.equal(cs2, cs) and ctx.torch.equal(hat2, hat)
    xs = list(range(1, n + 1))
    shares = ntl.vandermonde_batch_evaluate(xs, coeffs, R)            # [b][i - 1]
    wits = ntl.vandermonde_batch_evaluate(xs, hat_rows, R)
    host_cs = g1.download(cs)
    host_cs = [host_cs[b * (t + 1):(b + 1) * (t + 1)] for b in range(B)]
    field = GF(R)
    for i in xs:
        sh, wi = [row[i - 1] for row in shares], [row[i - 1] for row in wits]
        ok = pc.verify_batch(cs, i, dev_scalars(ctx, sh), dev_scalars(ctx, wi))
        assert ok.dtype == ctx.torch.bool and ok.cpu().tolist() == [True] * B
        assert pc.batch_verify_eval(cs, i, dev_scalars(ctx, sh), dev_scalars(ctx, wi)) is True
        assert pc.batch_verify_eval(host_cs, i, [field(v) for v in sh], wi) is True
        bad_s, bad_w = list(sh), list(wi)
        bad_s[1] = (bad_s[1] + 1) % R
        bad_w[B - 1] = (bad_w[B - 1] + 5) % R
        ok = pc.verify_batch(cs, i, dev_scalars(ctx, bad_s), dev_scalars(ctx, bad_w))
        assert ok.cpu().tolist() == [b not in (1, B - 1) for b in range(B)]
        assert pc.batch_verify_eval(cs, i, dev_scalars(ctx, bad_s), dev_scalars(ctx, wi)) is False
        assert pc.verify_eval(host_cs[0], i, sh[0], wi[0]) is True and pc.verify_eval(host_cs[0], i, sh[1], wi[0]) is False
    # the reference's own sequence on host objects: commit, create_witness, verify_eval
    poly = polynomials_over(field)
    phi = poly([rnd.randrange(R) for _ in range(t + 1)])
    c1, phi_hat = pc.commit(phi)
    assert len(c1) == t + 1 and c1 == [g ** int(a) * h ** int(b) for a, b in zip(phi.coeffs, phi_hat.coeffs)]
    for i in xs:
        w = pc.create_witness(phi_hat, i)
        assert w == phi_hat(i) and pc.verify_eval(c1, i, phi(i), w) and not pc.verify_eval(c1, i, phi(i) + 1, w)
    assert pc.batch_verify_eval([c1] * 3, 2, [phi(2)] * 3, [phi_hat(2)] * 3)
    assert not pc.batch_verify_eval([c1] * 3, 2, [phi(2), phi(2), phi(3)], [phi_hat(2)] * 3)
    assert pc.batch_verify_eval([], 1, [], [])


def test_argument_errors(ctx):
    from honeybadgermpc_amd import g1
    from honeybadgermpc_amd._capi import Context
    from honeybadgermpc_amd.poly_commit_lin import PolyCommitLin

    g, h = s.crs()
    tg, th = fixed(ctx, 8)
    pts = g1.upload([g, h, g], ctx)
    ks = dev_scalars(ctx, [1, 2])
    other = Context.get((1 << 255) - 19)
    with pytest.raises(ValueError, match="ctx"):
        g1.scalar_mul(other, 3, g)
    with pytest.raises(ValueError, match="ctx"):
        g1.FixedBase(other, g)
    with pytest.raises(ValueError, match="base"):
        g1.FixedBase(ctx, G1.one())
    with pytest.raises(TypeError, match="base"):
        g1.FixedBase(ctx, pts)
    with pytest.raises(ValueError, match="window"):
        g1.FixedBase(ctx, g, window=5)
    with pytest.raises(ValueError, match="ks and points"):
        g1.scalar_mul(ctx, ks, pts)
    with pytest.raises(ValueError, match="P and Q"):
        g1.add(ctx, pts, pts[:2])
    with pytest.raises(ValueError, match="b"):
        g1.commit(ctx, tg, th, ks, dev_scalars(ctx, [1, 2, 3]))
    with pytest.raises(ValueError, match="tg and th"):
        g1.commit(ctx, tg, fixed(ctx, 4)[1], ks, ks)
    with pytest.raises(TypeError, match="tg"):
        g1.commit(ctx, pts, th, ks, ks)
    cs = pts.reshape(1, 3, 2, 6)
    with pytest.raises(ValueError, match="i"):
        g1.eval_commitments(ctx, cs, 1 << 32)
    with pytest.raises(ValueError, match="i"):
        g1.verify(ctx, tg, th, cs, -1, ks[:1], ks[:1])
    with pytest.raises(TypeError, match="i"):
        g1.eval_commitments(ctx, cs, 1.0)
    with pytest.raises(ValueError, match="shares"):
        g1.verify(ctx, tg, th, cs, 1, ks, ks[:1])
    with pytest.raises(ValueError, match="cs"):
        g1.eval_commitments(ctx, pts, 1)
    with pytest.raises(TypeError, match="points"):
        g1.on_curve(ctx, [g])
    with pytest.raises(ValueError, match="points"):
        g1.on_curve(ctx, pts.cpu())
    with pytest.raises(TypeError, match="points"):
        g1.on_curve(ctx, pts.to(ctx.torch.int32))
    with pytest.raises(TypeError, match="crs"):
        PolyCommitLin([g, 5])
    # the C ABI refuses what the wrappers check first
    assert ctx.lib.hb_g1_eval(ctx.h, ctx.ptr(cs), 3, 1 << 32, ctx.ptr(pts), 1, ctx.stream()) == 2
    assert ctx.lib.hb_g1_table(ctx.h, np.zeros(12, dtype=np.uint64).ctypes.data, 8, ctx.ptr(tg.table), ctx.stream()) == 2
    assert ctx.lib.hb_g1_scalar_mul(other.h, ctx.ptr(ks), 1, ctx.ptr(pts), 0, ctx.ptr(pts), 3, ctx.stream()) == 2

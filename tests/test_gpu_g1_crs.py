"""GPU: the KZG prover in G1 (csrc/hb_crs.hip) through honeybadgermpc_amd.g1.FixedBases, msm_fixed and kzg_quotients and through
poly_commit_const.PolyCommitConst, against the Python-int model of g1_crs_support (a CRS with a known trapdoor) and bit-equal to
hb_selftest_g1_crs (the kernels' bodies on the host) on the same inputs.  Exact equality of words everywhere: affine canonical output is
unique, so every split and both window widths must agree.

Reference parity: the reference's poly_commit_const.py needs its pairing extension, which cannot be imported where this suite is built;
the trapdoor identities (a commitment is (phi(alpha) + lam hat(alpha)) g; c - share g - aux h == (alpha - x) w) stand in for it."""
import random

import numpy as np
import pytest

import g1_crs_support as cs
import g1_support as s

from honeybadgermpc_amd.bls12_381 import G1, R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from honeybadgermpc_amd._capi import Context

    return Context.get(R)


_FAMILIES = {}


def families(ctx, n, c, alpha=cs.ALPHA, lam=cs.LAM):
    """device tables (tg, th) of the CRS, built once a (n, c, alpha, lam)"""
    from honeybadgermpc_amd import g1

    key = (n, c, alpha, lam)
    if key not in _FAMILIES:
        gs, hs = cs.crs_points(n, alpha, lam)
        _FAMILIES[key] = (g1.FixedBases(ctx, gs, c), g1.FixedBases(ctx, hs, c))
    return _FAMILIES[key]


def dev_scalars(ctx, rows):
    M, K = len(rows), len(rows[0]) if rows else 0
    flat = s.words([v for row in rows for v in row], 4) if M * K else np.zeros((0, 4), dtype=np.uint64)
    return ctx.torch.from_numpy(flat.view(np.int64).reshape(M, K, 4)).to(ctx.tdev)


def host(t):
    return t.cpu().numpy().view(np.uint64).reshape(-1, 12)


def device_msm(ctx, case, split):
    from honeybadgermpc_amd import g1

    tg, th = families(ctx, case["n"], case["c"], case["alpha"], case["lam"])
    a = dev_scalars(ctx, case["a"])
    if case["b"] is None:
        out = g1.msm_fixed(ctx, tg, a, split=split)
    else:
        out = g1.msm_fixed(ctx, tg, a, th, dev_scalars(ctx, case["b"]), split=split)
    assert tuple(out.shape) == (len(case["a"]), 2, 6)
    return host(out)


# ---------------------------------------------------------------- the fixed-base sum
@pytest.mark.parametrize("name", sorted(cs.msm_cases()))
def test_msm_fixed_cases_at_every_split(ctx, name):
    case = cs.msm_cases()[name]
    want = cs.model_msm(case)
    assert np.array_equal(cs.host_msm(case, 64), want)
    for split in cs.SPLITS + [128, None]:
        assert np.array_equal(device_msm(ctx, case, split), want), (name, split)


def rows_case(rows, seed):
    rnd = random.Random(seed)
    edge = [0, 1, R - 1, cs.FULL, 0xFF << 248]
    a = [[rnd.randrange(1 << 256), edge[m % 5]] for m in range(rows)]
    b = [[edge[(m + 2) % 5], rnd.randrange(1 << 256)] for m in range(rows)]
    return dict(name=f"{rows} rows", n=2, terms=2, c=8, a=a, b=b, alpha=cs.ALPHA, lam=cs.LAM)


@pytest.mark.parametrize("rows", [1, 255, 256, 257])
def test_rows_around_a_workgroup_at_split_1(ctx, rows):
    case = rows_case(rows, rows)
    got = device_msm(ctx, case, 1)
    assert np.array_equal(got, cs.host_msm(case, 1))
    assert np.array_equal(got, cs.model_msm(case))


@pytest.mark.parametrize("split", [2, 64, 256])
@pytest.mark.parametrize("rows", [1, 3, 5])
def test_last_workgroup_with_idle_groups(ctx, rows, split):
    """256 / split rows a workgroup: 1, 3 and 5 rows leave groups of the last workgroup without a row (at split 256 there is none to leave)"""
    case = rows_case(rows, 10 * rows + split)
    got = device_msm(ctx, case, split)
    assert np.array_equal(got, cs.host_msm(case, split))
    assert np.array_equal(got, cs.model_msm(case))


def test_msm_fixed_equals_msm_and_out_reuse(ctx):
    from honeybadgermpc_amd import g1

    case = cs.msm_cases()["two families, edge scalars"]
    tg, th = families(ctx, 4, 8)
    a, b = dev_scalars(ctx, case["a"]), dev_scalars(ctx, case["b"])
    pts = g1.upload(tg.bases[:3] + th.bases[:3], ctx)
    want = g1.msm(ctx, ctx.torch.cat([a, b], dim=1), pts)
    out = ctx.torch.full((3, 2, 6), -1, dtype=ctx.torch.int64, device=ctx.tdev)
    assert g1.msm_fixed(ctx, tg, a, th, b, out=out) is out and ctx.torch.equal(out, want)
    assert ctx.torch.equal(g1.msm_fixed(ctx, tg, a), g1.msm(ctx, a, pts[:3]))
    # (K, 4) scalars are one row
    assert ctx.torch.equal(g1.msm_fixed(ctx, tg, a[1], th, b[1]), want[1:2])
    # no terms: identities; no rows: nothing
    empty = ctx.torch.empty((3, 0, 4), dtype=ctx.torch.int64, device=ctx.tdev)
    out.fill_(7)
    assert g1.msm_fixed(ctx, tg, empty, th, empty, out=out) is out and not out.cpu().numpy().any()
    assert g1.msm_fixed(ctx, tg, a[:0], th, b[:0]).shape == (0, 2, 6)


# ---------------------------------------------------------------- the tables
@pytest.mark.parametrize("c", [4, 8])
def test_tables_equal_the_host_tables_and_serve_commit(ctx, c):
    from honeybadgermpc_amd import g1

    tg, th = families(ctx, 3, c)
    tw = cs.table_words(c)
    ent = (256 // c) * ((1 << c) - 1) * 16                     # 64-bit words of entries a table; scratch and the base follow
    dev = tg.tables.cpu().numpy().view(np.uint64).reshape(3, tw)
    ref = cs.host_tables(3, c)[0].reshape(3, tw)
    assert np.array_equal(dev[:, :ent], ref[:, :ent])
    a, b = s.commit_case(40, c, seed=c)
    da, db = ctx.upload_ints([v % R for v in a]), ctx.upload_ints([v % R for v in b])
    for k in (0, 2):
        single = (g1.FixedBase(ctx, tg.bases[k], c), g1.FixedBase(ctx, th.bases[k], c))
        assert ctx.torch.equal(g1.commit(ctx, tg.base(k), th.base(k), da, db), g1.commit(ctx, single[0], single[1], da, db)), (c, k)
    assert ctx.torch.equal(g1.commit(ctx, tg.base(1), th.base(2), da, db), g1.commit(ctx, tg.base(1), g1.FixedBase(ctx, th.bases[2], c), da, db))


# ---------------------------------------------------------------- the quotient
def device_quotient(ctx, phis, xs, as_tensor=False):
    from honeybadgermpc_amd import g1

    B, n, t = len(phis), len(xs), len(phis[0]) - 1
    phi = ctx.upload_ints([v for p in phis for v in p]).reshape(B, t + 1, 4)
    q, rem = g1.kzg_quotients(ctx, phi, ctx.upload_ints(xs) if as_tensor else xs)
    assert tuple(q.shape) == (B, n, t, 4) and tuple(rem.shape) == (B, n, 4)
    qs, rs = ctx.download_ints(q.reshape(-1, 4)), ctx.download_ints(rem.reshape(-1, 4))
    return [[qs[(b * n + i) * t:(b * n + i + 1) * t] for i in range(n)] for b in range(B)], [rs[b * n:(b + 1) * n] for b in range(B)]


@pytest.mark.parametrize("t", [0, 1, 2, 21])
def test_quotient_cases(ctx, t):
    phis, xs = cs.quotient_case(t)
    got = device_quotient(ctx, phis, xs, as_tensor=t == 2)
    assert got == cs.host_quotient(phis, xs)
    for b, phi in enumerate(phis):
        for i, x in enumerate(xs):
            assert (got[0][b][i], got[1][b][i]) == cs.quotient_model(phi, x), (t, b, i)


@pytest.mark.parametrize("B,n", [(1, 1), (85, 3), (64, 4), (257, 1)])
def test_quotient_lanes_around_a_workgroup(ctx, B, n):
    rnd = random.Random(B * n)
    phis = [[rnd.randrange(R) for _ in range(3)] for _ in range(B)]
    xs = [R - 1 - i for i in range(n)]                           # ints reduced mod R: also negative and large ones
    got = device_quotient(ctx, phis, [x - R for x in xs])
    assert got == cs.host_quotient(phis, xs)
    assert got[1] == [[cs.poly_at(p, x) for x in xs] for p in phis]


# ---------------------------------------------------------------- PolyCommitConst
def test_poly_commit_const_end_to_end(ctx):
    from honeybadgermpc_amd import g1
    from honeybadgermpc_amd.field import GF
    from honeybadgermpc_amd.poly_commit_const import PolyCommitConst, gen_pc_const_crs
    from honeybadgermpc_amd.polynomial import polynomials_over

    n, t, B = 4, 1, 3
    g = G1.generator()
    crs = gen_pc_const_crs(t, alpha=cs.ALPHA, g=g, h=g ** cs.LAM, ctx=ctx)
    gs, hs = cs.crs_points(t + 1)
    assert crs[0] == gs and crs[1] is None and crs[2] == hs
    pc = PolyCommitConst(crs, ctx=ctx)
    assert pc.t == t and pc.ghats is None
    rnd = random.Random(3)
    phis = [[rnd.randrange(R) for _ in range(t + 1)] for _ in range(B)]
    phis[1] = [R - 1, 0]                                         # a zero top coefficient
    coeffs = ctx.upload_ints([v for p in phis for v in p]).reshape(B, t + 1, 4)
    c, hat = pc.commit_batch(coeffs)
    assert tuple(c.shape) == (B, 2, 6) and tuple(hat.shape) == (B, t + 1, 4)
    hats = [ctx.download_ints(hat[b]) for b in range(B)]
    assert len({tuple(h) for h in hats}) == B and all(0 <= v < R for h in hats for v in h)
    commits = g1.download(c)
    assert commits == [cs.commitment_model(p, h) for p, h in zip(phis, hats)]
    c2, hat2 = pc.commit_batch(coeffs, hat)
    assert hat2 is hat and ctx.torch.equal(c2, c)
    xs = list(range(1, n + 1))
    w, shares, aux = pc.witness_batch(coeffs, hat, xs)
    assert tuple(w.shape) == (B, n, 2, 6) and tuple(shares.shape) == (B, n, 4) and tuple(aux.shape) == (B, n, 4)
    wit, sh, ax = g1.download(w), ctx.download_ints(shares.reshape(-1, 4)), ctx.download_ints(aux.reshape(-1, 4))
    for b in range(B):
        for i, x in enumerate(xs):
            assert sh[b * n + i] == cs.poly_at(phis[b], x) and ax[b * n + i] == cs.poly_at(hats[b], x)
            assert cs.witness_holds(commits[b], sh[b * n + i], ax[b * n + i], wit[b * n + i], x), (b, i)
            assert not cs.witness_holds(commits[b], (sh[b * n + i] + 1) % R, ax[b * n + i], wit[b * n + i], x)
    # the reference's surface on host polynomials agrees with the batch calls
    poly = polynomials_over(GF(R))
    phi = poly(phis[0])
    ch, phi_hat = pc.commit(phi)
    assert isinstance(ch, G1) and ch == cs.commitment_model(phis[0], [int(v) for v in phi_hat.coeffs] + [0] * (t + 1 - len(phi_hat.coeffs)))
    assert pc.create_witness(phi, poly(hats[0]), 3) == wit[2]
    wh = pc.create_witness(phi, phi_hat, 2)
    assert cs.witness_holds(ch, int(phi(2)), int(phi_hat(2)), wh, 2)
    # window 4 gives the same words
    pc4 = PolyCommitConst(crs, ctx=ctx)
    pc4.preprocess_prover(4)
    assert pc4.window == 4 and ctx.torch.equal(pc4.commit_batch(coeffs, hat)[0], c) and ctx.torch.equal(pc4.witness_batch(coeffs, hat, xs)[0], w)
    # the verifier needs a pairing: no verdict
    for call in (lambda: pc.verify_eval(ch, 2, phi(2), phi_hat(2), wh), lambda: pc.batch_verify_eval([ch], 2, [phi(2)], [phi_hat(2)], [wh]),
                 lambda: pc.preprocess_verifier()):
        with pytest.raises(NotImplementedError, match="pairing"):
            call()
    with pytest.raises(ValueError, match="alpha"):
        gen_pc_const_crs(t, alpha=R, ctx=ctx)
    with pytest.raises(ValueError, match="coeffs"):
        pc.commit_batch(coeffs[:, :1])


def test_poly_commit_const_degree_zero(ctx):
    """t = 0: the commitment is phi_0 g + hat_0 h and every witness the identity, as the reference's empty product"""
    from honeybadgermpc_amd import g1
    from honeybadgermpc_amd.poly_commit_const import PolyCommitConst

    gs, hs = cs.crs_points(1)
    pc = PolyCommitConst([gs, None, hs], ctx=ctx)
    coeffs, hat = ctx.upload_ints([5, R - 1]).reshape(2, 1, 4), ctx.upload_ints([7, 0]).reshape(2, 1, 4)
    c, _ = pc.commit_batch(coeffs, hat)
    assert g1.download(c) == [cs.commitment_model([5], [7]), cs.commitment_model([R - 1], [0])]
    w, shares, aux = pc.witness_batch(coeffs, hat, [1, 2, 3])
    assert tuple(w.shape) == (2, 3, 2, 6) and not w.cpu().numpy().any()
    assert ctx.download_ints(shares.reshape(-1, 4)) == [5] * 3 + [R - 1] * 3 and ctx.download_ints(aux.reshape(-1, 4)) == [7] * 3 + [0] * 3


# ---------------------------------------------------------------- refusals
def test_argument_refusals(ctx):
    from honeybadgermpc_amd import g1
    from honeybadgermpc_amd._capi import Context, HbmpcBackendError

    torch = ctx.torch
    tg, th = families(ctx, 3, 8)
    tg4, _ = families(ctx, 3, 4)
    tg2, _ = families(ctx, 2, 8)
    case = cs.msm_cases()["one family"]
    a = dev_scalars(ctx, case["a"])
    want = host(g1.msm_fixed(ctx, tg, a))
    g = G1.generator()
    with pytest.raises(ValueError, match="identity"):
        g1.FixedBases(ctx, [g, G1.one()])
    with pytest.raises(ValueError, match="window"):
        g1.FixedBases(ctx, [g], window=5)
    with pytest.raises(ValueError, match="bases"):
        g1.FixedBases(ctx, [])
    with pytest.raises(TypeError, match="bases"):
        g1.FixedBases(ctx, [g, 3])
    with pytest.raises(IndexError):
        tg.base(3)
    with pytest.raises(ValueError, match="terms"):
        g1.msm_fixed(ctx, tg2, a)                                 # 3 terms against 2 bases
    for split in (0, 3, 512, 2.0, True):
        with pytest.raises(ValueError, match="split"):
            g1.msm_fixed(ctx, tg, a, split=split)
    with pytest.raises(ValueError, match="th and b"):
        g1.msm_fixed(ctx, tg, a, th)
    with pytest.raises(ValueError, match="tg and th"):
        g1.msm_fixed(ctx, tg, a, tg4, a)
    with pytest.raises(ValueError, match="tg and th"):
        g1.msm_fixed(ctx, tg, a[:, :2], tg2, a[:, :2])
    with pytest.raises(ValueError, match="a and b"):
        g1.msm_fixed(ctx, tg, a, th, a[:2])
    with pytest.raises(TypeError, match="tg"):
        g1.msm_fixed(ctx, tg.base(0), a)
    with pytest.raises(ValueError, match="out"):
        g1.msm_fixed(ctx, tg, a, out=torch.empty((2, 2, 6), dtype=torch.int64, device=ctx.tdev))
    with pytest.raises(ValueError, match="ctx"):
        g1.msm_fixed(Context.get((1 << 255) - 19), tg, a)
    with pytest.raises(ValueError, match="phi"):
        g1.kzg_quotients(ctx, a.reshape(9, 4), [1])
    # the C ABI
    lib, stream = ctx.lib, ctx.stream()
    out = torch.empty((3, 2, 6), dtype=torch.int64, device=ctx.tdev)

    def call(out_t=out, n_bases=3, window=8, terms=3, split=0, rows=3, tabs=tg.tables, a_t=a, th_t=None, b_t=None):
        p = lambda t: ctx.ptr(t) if t is not None else None
        return lib.hb_g1_crs_msm(ctx.h, p(tabs), p(th_t), n_bases, window, p(a_t), p(b_t), terms, split, p(out_t), rows, stream)

    ctx.check(call(), "hb_g1_crs_msm")
    assert np.array_equal(host(out), want)
    for rc in (call(terms=4), call(n_bases=2), call(split=3), call(split=512), call(split=-1), call(window=5), call(window=0), call(out_t=a), call(out_t=a[1:]),
               call(out_t=tg.tables), call(out_t=None), call(tabs=None), call(a_t=None), call(rows=-1), call(terms=-1), call(th_t=th.tables), call(b_t=a),
               call(out_t=a, th_t=th.tables, b_t=a)):
        assert rc == 2
        with pytest.raises(HbmpcBackendError, match="hb_g1_crs_msm"):
            ctx.check(rc, "hb_g1_crs_msm")
    assert call(rows=0) == 0
    assert np.array_equal(host(out), want)                       # a refused call writes nothing
    # the tables: an identity or a point off the curve among the bases, the window, the count
    buf = torch.empty((2 * cs.table_words(4),), dtype=torch.int64, device=ctx.tdev)
    good = s.points([g, g ** 2])
    tab = lambda bases, n=2, window=4, dst=buf: lib.hb_g1_crs_table(ctx.h, bases.ctypes.data if bases is not None else None, n, window,
                                                                    ctx.ptr(dst) if dst is not None else None, stream)
    assert tab(good) == 0 and tab(good, n=0) == 0
    for rc in (tab(s.points([g, G1.one()])), tab(s.points([g, s.off_curve_raw()])), tab(good, window=5), tab(good, n=-1), tab(good, n=4097), tab(None), tab(good, dst=None)):
        assert rc == 2
    # the quotient
    phi, xs = ctx.upload_ints([1, 2, 3, 4]).reshape(2, 2, 4), ctx.upload_ints([5, 6, 7])
    q, rem = torch.empty((2, 3, 1, 4), dtype=torch.int64, device=ctx.tdev), torch.empty((2, 3, 4), dtype=torch.int64, device=ctx.tdev)
    quo = lambda phi_t=phi, n_coef=2, xs_t=xs, n=3, q_t=q, rem_t=rem, B=2: lib.hb_kzg_quotient(ctx.h, ctx.ptr(phi_t) if phi_t is not None else None, n_coef,
                                                                                              ctx.ptr(xs_t) if xs_t is not None else None, n,
                                                                                              ctx.ptr(q_t) if q_t is not None else None,
                                                                                              ctx.ptr(rem_t) if rem_t is not None else None, B, stream)
    assert quo() == 0 and quo(B=0) == 0 and quo(n=0) == 0
    for rc in (quo(n_coef=0), quo(n=-1), quo(B=-1), quo(phi_t=None), quo(xs_t=None), quo(q_t=None), quo(rem_t=None), quo(q_t=phi), quo(rem_t=xs), quo(rem_t=q),
               quo(q_t=xs)):
        assert rc == 2

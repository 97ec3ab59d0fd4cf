"""Every route of hb_fft_batch_evaluate (csrc/hb_ntt.hip) and the omega-point interpolation, exactly against a radix-2 transform on
Python ints (tests/ntt_cases.py), on one modulus of every class the reduction code distinguishes: 4 limbs at and above 2^254 (the
one-digit Barrett quotient), 4 limbs below it (the generic REDC), 1 limb.  The cases come from ntt_cases with the route they expect; every
call first asks the library which kernel it is about to run (hb_debug_fft_route) and the test fails if that is not the expected one, so a
comparison never stands on another path than the one it names.

  (a) pruning: every d at the small orders, the d around n / 8, n / 2 and n at the larger ones, k = n and one partial k; ragged batches
  (b) the lazy-value bound: pool-valued coefficients and pool-valued outputs at moduli next to 2^256, 2^254, 2^64 and at 12289 on 4 limbs
  (c) the four-step transform at its smallest orders: d around n2, k around n1, small d behind full d on one stream; the stage loop
  (d) twiddle tables keyed by the root   (e) corners   (f) interpolation at omega^zs on the same classes of modulus"""
import functools
import random

import numpy as np
import pytest

import edge_values as ev
import ntt_cases as nc
from conftest import clear_hook, set_hook

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A5A5A5A5A


def _ctx(f):
    from honeybadgermpc_amd._capi import Context

    return Context.get(f.p, n_limbs=f.n_limbs)


def _route(f, n, d, k):
    from honeybadgermpc_amd._capi import np_ptr

    ctx = _ctx(f)
    out = np.full(4, -1, dtype=np.int32)
    ctx.check(ctx.lib.hb_debug_fft_route(ctx.h, n, d, k, np_ptr(out)), "hb_debug_fft_route")
    return tuple(int(v) for v in out)


def _eval_c(f, rows, omega, n, k, out=None):
    """the C entry itself, on the context of the field's limb count"""
    from honeybadgermpc_amd._capi import np_ptr

    ctx = _ctx(f)
    count, d = len(rows), len(rows[0]) if rows else 0
    din = ctx.upload_ints([v for r in rows for v in r]) if count * d else ctx.empty(1)
    dout = ctx.empty(max(count * k, 1)) if out is None else out
    rc = ctx.lib.hb_fft_batch_evaluate(ctx.h, np_ptr(ctx.host_elems([omega])), n, ctx.ptr(din), count, d, k, ctx.ptr(dout), ctx.stream())
    ctx.check(rc, "hb_fft_batch_evaluate")
    flat = ctx.download_ints(dout)
    return [flat[i * k : (i + 1) * k] for i in range(count)]


def _eval(f, rows, omega, n, k):
    """through ntl wherever its default context is the one wanted (12289 on 4 limbs is not)"""
    from honeybadgermpc_amd import ntl

    if nc.default_limbs(f.p) == f.n_limbs:
        return ntl.fft_batch_evaluate(rows, omega, f.p, n, k)
    return _eval_c(f, rows, omega, n, k)


def _run(case, rows, omega, want_full):
    """one case: the route first, then the values"""
    f = nc.FIELD[case.field]
    assert _route(f, case.n, case.d, case.k) == case.route, case
    assert all(len(r) == case.d for r in rows)
    got = _eval(f, rows, omega, case.n, case.k)
    assert got == [w[: case.k] for w in want_full], case


# ---- (a) pruning sweep -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid, n", nc.SWEEP, ids=["%s-%d" % c for c in nc.SWEEP])
def test_pruning_sweep(fid, n):
    f = nc.FIELD[fid]
    w = nc.root_of_unity(f.p, n)
    routes = set()
    for d in nc.sweep_ds(n):
        rows = nc.rows(f.p, d, 6, seed=n + d, n_limbs=f.n_limbs)
        want = [nc.dft(f.p, w, n, r) for r in rows]
        cases = [c for c in nc.sweep_cases(fid, n) if c.d == d]
        assert cases and cases[0].k == n
        for case in cases:
            _run(case, rows, w, want)
            routes.add(case.route[0])
    assert nc.LDS in routes


@pytest.mark.parametrize("fid, n, d", nc.BATCH, ids=["%s-%d-%d" % c for c in nc.BATCH])
def test_ragged_batches_on_the_lds_kernel(fid, n, d):
    """PB - 1, PB, PB + 1 and 2 PB + 3 polynomials, PB asked of the library: the ragged last workgroup and the uidx % npoly lane map"""
    f = nc.FIELD[fid]
    w = nc.root_of_unity(f.p, n)
    route = _route(f, n, d, n)
    assert route[0] == nc.LDS
    pb = route[3]
    sizes = [c for c in (pb - 1, pb, pb + 1, 2 * pb + 3) if c > 0]
    assert sizes == nc.batch_sizes(n)
    big = nc.rows(f.p, d, sizes[-1], seed=n, n_limbs=f.n_limbs)
    want = [nc.dft(f.p, w, n, r) for r in big]
    for count in sizes:
        # the p - 1, zero and uniform rows sit at the end of `big`: take the tail, so the ragged workgroup holds them
        _run(nc.Case(fid, n, d, n, (nc.LDS, 0, 0, pb)), big[-count:], w, want[-count:])


# ---- (b) lazy bound --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid, n", nc.LAZY, ids=["%s-%d" % c for c in nc.LAZY])
def test_lazy_bound_at_edge_values(fid, n):
    """d = k = n on the LDS kernel: coefficients that are pool values (the all-(p - 1) row among them), and coefficients chosen by the
    inverse transform so that the OUTPUTS are pool values; and the rows that hold p - 1 on one half of an index bit and 0 on the other
    (ntt_cases.half_rows), which put the first pass's u - v + m[u] at its lowest"""
    f = nc.FIELD[fid]
    w = nc.root_of_unity(f.p, n)
    case = nc.Case(fid, n, n, n, (nc.LDS, 0, 0, nc.lds_pb(n)))
    rows = nc.rows(f.p, n, nc.lazy_count(f, n), seed=n, n_limbs=f.n_limbs)
    assert [f.p - 1] * n in rows
    _run(case, rows, w, [nc.dft(f.p, w, n, r) for r in rows])
    _run(case, nc.inverse_rows(f.p, w, n, rows), w, rows)
    halves = nc.half_rows(f.p, n)
    _run(case, halves, w, [nc.dft(f.p, w, n, r) for r in halves])


# ---- (c) four-step ---------------------------------------------------------------------------------------------------------------
_PAIRS = [(0, 2), (3, 5), (1, 4)]          # of rows(.., 6): (walk, p - 1), (draw, uniform), (walk, zero)


@functools.lru_cache(maxsize=None)
def _four_io(fid, n, d, pair):
    """two different polynomials of d coefficients and their whole transforms, computed once and left unchanged"""
    f = nc.FIELD[fid]
    base = nc.rows(f.p, n + 7, 6, seed=n, n_limbs=f.n_limbs)
    rows = tuple(tuple(base[j][:d]) for j in _PAIRS[pair])
    w = nc.root_of_unity(f.p, n)
    return rows, tuple(tuple(nc.dft(f.p, w, n, list(r))) for r in rows)


def _pair_of(i, case):
    return 0 if case.d == case.n else i % 3


@pytest.mark.parametrize("fid, n", nc.FOUR, ids=["%s-%d" % c for c in nc.FOUR])
def test_four_step(fid, n):
    """the calls follow each other on one stream in the list's order: the smallest d right behind d = n (the scratch between the steps is
    kept per order and stream), then d around n2 (d1 = ceil(d / n2) coefficients a column), then k around n1 (rows3 = min(k, n1))"""
    f = nc.FIELD[fid]
    w = nc.root_of_unity(f.p, n)
    for i, case in enumerate(nc.four_step_cases(fid, n)):
        assert case.route[0] == nc.FOUR_STEP
        rows, want = _four_io(fid, n, case.d, _pair_of(i, case))
        _run(case, [list(r) for r in rows], w, [list(v) for v in want])
    if f.n_limbs == 4:
        # the lazy bound inside both factors (R = 2^261 leaves 4-limb values five bits; a 1-limb context's 2^87 leaves 23)
        halves = nc.half_rows(f.p, n)
        _run(nc.Case(fid, n, n, n, nc.route_model(4, n, n, n)), halves, w, [nc.dft(f.p, w, n, r) for r in halves])


@pytest.mark.parametrize("fid", list(nc.FOUR_STEP_ORDERS))
def test_stage_loop_equals_the_four_step(fid, monkeypatch):
    f = nc.FIELD[fid]
    for i, case in enumerate(nc.stage_loop_cases(fid)):
        n = case.n
        w = nc.root_of_unity(f.p, n)
        rows, want = _four_io(fid, n, case.d, _pair_of(i + 1, case))
        rows, want = [list(r) for r in rows], [list(v) for v in want]
        clear_hook(monkeypatch, "HB_NTT_STAGE_LOOP")
        assert _route(f, n, case.d, case.k)[0] == nc.FOUR_STEP
        four = _eval(f, rows, w, n, case.k)
        set_hook(monkeypatch, "HB_NTT_STAGE_LOOP", "1")
        try:
            assert case.route == (nc.STAGE_LOOP, 0, 0, 0)
            assert _route(f, n, case.d, case.k) == case.route, case
            loop = _eval(f, rows, w, n, case.k)
        finally:
            clear_hook(monkeypatch, "HB_NTT_STAGE_LOOP")
        assert loop == four, case
        assert four == [v[: case.k] for v in want], case
        assert _route(f, n, case.d, case.k)[0] == nc.FOUR_STEP


# ---- (d) twiddle tables are keyed by the root --------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid, n, d", nc.ROOTS, ids=["%s-%d-%d" % c for c in nc.ROOTS])
def test_twiddles_are_keyed_by_the_root(fid, n, d):
    """omega, 1 / omega and omega^3 interleaved in one context at one order: each call must find its own table (and, on the four-step,
    its own omega^n1 and omega^n2 tables)"""
    f = nc.FIELD[fid]
    w = nc.root_of_unity(f.p, n)
    roots = [w, pow(w, -1, f.p), pow(w, 3, f.p)]
    assert len(set(roots)) == 3 and all(pow(r, n // 2, f.p) == f.p - 1 for r in roots)
    rows = nc.rows(f.p, d, 3, seed=d, n_limbs=f.n_limbs)
    want = [[nc.dft(f.p, r, n, row) for row in rows] for r in roots]
    case = nc.Case(fid, n, d, n, nc.route_model(f.n_limbs, n, d, n))
    assert case.route[0] in (nc.LDS, nc.FOUR_STEP)
    for j in (0, 1, 2, 0, 2, 1, 1, 0):
        _run(case, rows, roots[j], want[j])


# ---- (e) corners -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", ["bls", "gen-hi", "tiny-wide", "goldilocks"])
def test_corners(fid):
    from honeybadgermpc_amd import ntl
    from honeybadgermpc_amd._capi import np_ptr

    f = nc.FIELD[fid]
    ctx = _ctx(f)
    p = f.p
    # order 1: the coefficient itself, whatever follows it
    rows = nc.rows(p, 3, 6, seed=1, n_limbs=f.n_limbs)
    for d in (1, 3):
        assert _route(f, 1, d, 1) == (nc.MATVEC, 0, 0, 0)
        assert _eval(f, [r[:d] for r in rows], 1, 1, 1) == [[r[0]] for r in rows]
    # d = 0: zeros, on an order of every route; the output buffer held something else before
    for n in (1, 8, 4096, nc.FOUR_STEP_ORDERS[fid][0]):
        w = nc.root_of_unity(p, n)
        k = min(n, 5)
        assert _route(f, n, 0, k) == (nc.MATVEC, 0, 0, 0)
        out = ctx.empty(3 * k)
        out.fill_(SENTINEL)
        assert _eval_c(f, [[], [], []], w, n, k, out=out) == [[0] * k] * 3
    if nc.default_limbs(p) == f.n_limbs:
        assert ntl.fft_batch_evaluate([[], []], nc.root_of_unity(p, 8), p, 8, 8) == [[0] * 8] * 2
    # d > n: the coefficients from n on are ignored, not wrapped around
    n = 8
    w = nc.root_of_unity(p, n)
    rows = nc.rows(p, 20, 6, seed=2, n_limbs=f.n_limbs)
    assert _route(f, n, 20, n)[0] == nc.LDS
    assert _eval(f, rows, w, n, n) == [nc.dft_horner(p, w, n, r[:n]) for r in rows]
    # k = 0 and C = 0: nothing is written
    for count, k in ((3, 0), (0, n)):
        out = ctx.empty(3 * n)
        out.fill_(SENTINEL)
        din = ctx.upload_ints([v for r in rows[:3] for v in r])
        rc = ctx.lib.hb_fft_batch_evaluate(ctx.h, np_ptr(ctx.host_elems([w])), n, ctx.ptr(din), count, 20, k, ctx.ptr(out), ctx.stream())
        assert rc == 0
        ctx.torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()), (count, k)
    # the route query refuses what the call refuses
    from honeybadgermpc_amd._capi import HB_ERR_BAD_ARG

    bad = np.zeros(4, dtype=np.int32)
    for order, d, k in ((3, 1, 1), (0, 1, 0), (8, 1, 9), (8, -1, 1)):
        assert ctx.lib.hb_debug_fft_route(ctx.h, order, d, k, np_ptr(bad)) == HB_ERR_BAD_ARG


def test_route_query_follows_the_hook_and_the_order(monkeypatch):
    """the stage loop is reported under HB_NTT_STAGE_LOOP=1 and beyond 2^22, the four-step's factors otherwise; nothing is launched"""
    for fid in ("bls", "gen-hi", "goldilocks"):
        f = nc.FIELD[fid]
        for logn in (12, 13, 14, 15, 20, 22, 23):
            n = 1 << logn
            assert _route(f, n, n, n) == nc.route_model(f.n_limbs, n, n, n), (fid, logn)
        assert _route(f, 1 << 23, 1 << 23, 1 << 23)[0] == nc.STAGE_LOOP
        set_hook(monkeypatch, "HB_NTT_STAGE_LOOP", "1")
        try:
            assert _route(f, 1 << 15, 1 << 15, 1 << 15) == (nc.STAGE_LOOP, 0, 0, 0)
            assert _route(f, 2048, 2048, 2048) == (nc.LDS, 0, 0, 1)            # the hook does not reach the orders that fit LDS
        finally:
            clear_hook(monkeypatch, "HB_NTT_STAGE_LOOP")
        assert _route(f, 1 << 15, 1 << 15, 1 << 15)[0] == nc.FOUR_STEP


# ---- (f) interpolation at omega^zs -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", nc.INTERP_BATCHES)
@pytest.mark.parametrize("k", nc.INTERP_KS)
@pytest.mark.parametrize("fid", nc.INTERP_FIELDS)
def test_interpolate_at_omega_points(fid, k, count):
    """the inverse Vandermonde mat-vec at the points omega^zs against Newton interpolation in Python ints; the same set in two more arrival
    orders (sorted: no permutation; shuffled: another one) gives the same polynomials"""
    from honeybadgermpc_amd import ntl

    f = nc.FIELD[fid]
    p, n = f.p, nc.INTERP_ORDER
    assert nc.default_limbs(p) == f.n_limbs
    w = nc.root_of_unity(p, n)
    rnd = random.Random(1000 * k + count)
    zs = rnd.sample(range(n), k)
    if k > 1 and zs == sorted(zs):
        zs.reverse()
    ys = nc.interp_values(p, k, count, seed=k + count)
    want = [ev.interpolate(p, [pow(w, z, p) for z in zs], y) for y in ys]
    assert ntl.fft_batch_interpolate(zs, ys, w, p, n) == want
    by_z = sorted(range(k), key=lambda i: zs[i])
    mixed = list(range(k))
    rnd.shuffle(mixed)
    for perm in (by_z, mixed):
        got = ntl.fft_batch_interpolate([zs[i] for i in perm], [[y[i] for i in perm] for y in ys], w, p, n)
        assert got == want, perm

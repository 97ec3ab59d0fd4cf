"""CPU-only: the reference and the case lists of tests/ntt_cases.py are what test_gpu_ntt.py takes them for -- the moduli are prime with
the 2-adicity the table claims, the radix-2 reference equals the definition and the repository's CPU port, and the lists reach every
remainder pass, every field and every route they promise.  This checks the lists, not the library."""
import random

import pytest

import edge_values as ev
import ntt_cases as nc


def _adicity(p):
    return ((p - 1) & -(p - 1)).bit_length() - 1


def test_moduli_are_prime_with_the_claimed_two_adicity():
    from honeybadgermpc_amd.field import is_probable_prime

    assert len({f.id for f in nc.FIELDS}) == len(nc.FIELDS) == 10
    for f in nc.FIELDS:
        assert is_probable_prime(f.p), f.id
        assert _adicity(f.p) == f.adicity, f.id
        assert f.n_limbs in (1, 4) and (f.n_limbs == 4 or f.p < 1 << 64), f.id
        assert f.psc == (f.n_limbs == 4 and f.p >= 1 << 254), f.id
    by = nc.FIELD
    assert by["top"].p > (1 << 256) - (1 << 29) and by["psc-lo"].p - (1 << 254) < 1 << 28 and (1 << 254) - by["gen-hi"].p < 1 << 24
    assert by["w65"].p.bit_length() == 65 and by["stark"].p.bit_length() == 252 and by["tiny-wide"].p == by["tiny"].p == 12289


def test_root_of_unity_has_exact_order():
    for f in nc.FIELDS:
        for order in {1, 2, 8, 1 << min(f.adicity, 15)}:
            w = nc.root_of_unity(f.p, order)
            assert pow(w, order, f.p) == 1
            assert order == 1 or pow(w, order // 2, f.p) == f.p - 1, (f.id, order)
    with pytest.raises(AssertionError):
        nc.root_of_unity(12289, 1 << 13)


@pytest.mark.parametrize("f", nc.FIELDS, ids=[f.id for f in nc.FIELDS])
def test_dft_equals_the_definition(f):
    rnd = random.Random(f.p % 1000)
    pool = ev.edge_pool(f.p, f.n_limbs)
    for n in (1, 2, 4, 8, 16, 64):
        w = nc.root_of_unity(f.p, n)
        for d in range(1, n + 4):
            row = [rnd.choice(pool) if rnd.random() < 0.3 else rnd.randrange(f.p) for _ in range(d)]
            full = nc.dft_horner(f.p, w, n, row)
            assert nc.dft(f.p, w, n, row) == full, (n, d)
            assert nc.dft(f.p, w, n, row, 1) == full[:1] == nc.dft_horner(f.p, w, n, row, 1)
            assert nc.dft(f.p, w, n, row, n) == full
        assert nc.dft(f.p, w, n, []) == [0] * n
        targets = [pool[(3 * i) % len(pool)] for i in range(n)]
        assert nc.dft(f.p, w, n, nc.inverse_rows(f.p, w, n, [targets])[0]) == targets


@pytest.mark.parametrize("fid", ["bls", "goldilocks"])
def test_dft_equals_the_cpu_port_at_4096(fid):
    import oracle

    f = nc.FIELD[fid]
    n = 4096
    w = nc.root_of_unity(f.p, n)
    for d, row in ((n, nc.rows(f.p, n, 1, seed=3)[0]), (1000, nc.rows(f.p, 1000, 4, seed=4)[3]), (n + 9, nc.rows(f.p, n + 9, 4, seed=5)[0])):
        assert len(row) == d
        assert nc.dft(f.p, w, n, row) == oracle.fft(row[:n], w, f.p, n), d


def test_rows_hold_what_they_promise():
    for f in nc.FIELDS:
        pool = ev.edge_pool(f.p, f.n_limbs)
        count = len(pool) + 5
        rs = nc.rows(f.p, 5, count, seed=2, n_limbs=f.n_limbs)
        assert len(rs) == count and [f.p - 1] * 5 in rs and [0] * 5 in rs
        for pos in range(5):
            assert {r[pos] for r in rs[: len(pool)]} == set(pool), (f.id, pos)
        for small in (1, 2, 3, 4, 6):
            rs = nc.rows(f.p, 3, small, seed=1, n_limbs=f.n_limbs)
            assert len(rs) == small and [f.p - 1] * 3 in rs and (small < 2 or [0] * 3 in rs)
    wide = ev.edge_pool(12289, 4)
    assert set(wide) != set(ev.edge_pool(12289, 1)) and any(v in wide for r in nc.rows(12289, 4, 6, n_limbs=4) for v in r)


def test_route_model_at_known_points():
    """a few decisions worked out by hand from the launcher's MAD counts (81 / 117 a product / a reduction on 9 digits, 9 / 21 on 3)"""
    assert nc.route_model(4, 64, 5, 64) == (nc.MATVEC, 0, 0, 0)          # 64 (5 81 + 117) = 33408 <= 32 6 198 = 38016
    assert nc.route_model(4, 64, 6, 64) == (nc.LDS, 0, 0, 32)            # 64 (6 81 + 117) = 38592
    assert nc.route_model(1, 64, 7, 64) == (nc.MATVEC, 0, 0, 0)          # 64 (7 9 + 21) = 5376 <= 32 6 30 = 5760
    assert nc.route_model(1, 64, 8, 64) == (nc.LDS, 0, 0, 32)
    assert nc.route_model(4, 2048, 2048, 2048) == (nc.LDS, 0, 0, 1) and nc.route_model(4, 4096, 4096, 4096) == (nc.FOUR_STEP, 64, 64, 0)
    assert nc.route_model(4, 8192, 8192, 8192) == (nc.FOUR_STEP, 128, 64, 0)
    assert nc.route_model(1, 8192, 8192, 8192) == (nc.LDS, 0, 0, 1) and nc.route_model(1, 1 << 15, 1 << 15, 1 << 15) == (nc.FOUR_STEP, 256, 128, 0)
    assert nc.route_model(4, 4096, 4096, 4096, stage_loop=True) == (nc.STAGE_LOOP, 0, 0, 0)
    assert nc.route_model(4, 1 << 23, 1 << 23, 1 << 23)[0] == nc.STAGE_LOOP
    assert nc.route_model(4, 1, 3, 1)[0] == nc.MATVEC and nc.route_model(4, 64, 0, 64)[0] == nc.MATVEC
    assert nc.route_model(4, 2, 1, 2)[0] == nc.LDS and nc.lds_pb(2) == nc.lds_pb(8) == 256


def test_case_lists_cover_what_they_promise():
    cases = nc.all_transform_cases()
    lds = [c for c in cases if c.route[0] == nc.LDS]
    four = [c for c in cases if c.route[0] == nc.FOUR_STEP]
    loop = [c for c in cases if c.route[0] == nc.STAGE_LOOP]
    assert {(c.n.bit_length() - 1) % 3 for c in lds} == {0, 1, 2}
    for f in nc.FIELDS:
        mine = [c for c in lds if c.field == f.id]
        assert mine, f.id
        # a partial k on the transform, and pruned inputs (d < n), in every field
        assert any(c.k < c.n for c in mine) and any(c.d < c.n for c in mine) and any(c.d > c.n for c in mine), f.id
    # the four-step starts where n + n / 2 elements leave the 160 KB of LDS: 4096 on 4 limbs, 2^14 on 1 limb
    reach = {f.id for f in nc.FIELDS if f.adicity >= (12 if f.n_limbs == 4 else 14)}
    assert {c.field for c in four} == reach
    # 12289 = 3 2^12 + 1 has no root of order 2^14: on 1 limb it cannot reach the four-step, tiny-wide runs it over the same modulus
    assert {f.id for f in nc.FIELDS if f.adicity >= 12} - reach == {"tiny"}
    for fid, n in nc.FOUR:
        cs = nc.four_step_cases(fid, n)
        assert all(c.route[0] == nc.FOUR_STEP for c in cs), (fid, n)
        n1, n2 = cs[0].route[1:3]
        assert n1 * n2 == n and cs[0].d == n and cs[1].d < n2 and {n2 - 1, n2, n2 + 1, 2 * n2 + 1, n - 1, n + 7} <= {c.d for c in cs}
        assert {n1 - 1, n1, n1 + 1, n - 1} <= {c.k for c in cs}
        f = nc.FIELD[fid]
        assert nc.route_model(f.n_limbs, n, cs[1].d - 1, n)[0] == nc.MATVEC
        kmin = min(c.k for c in cs)
        assert nc.route_model(f.n_limbs, n, n, kmin - 1)[0] == nc.MATVEC
    assert any(n1 != n2 for _, n1, n2, _ in (c.route for c in four))
    # routes 1, 2 and 3 on each kind of context
    kinds = {"narrow": lambda f: f.n_limbs == 1, "psc": lambda f: f.psc, "generic": lambda f: f.n_limbs == 4 and not f.psc}
    for name, pred in kinds.items():
        for group in (lds, four, loop):
            assert any(pred(nc.FIELD[c.field]) for c in group), name
    # every order a field is given has a root
    assert all((nc.FIELD[c.field].p - 1) % c.n == 0 for c in cases)
    # the batch cases stand on the LDS kernel and straddle a workgroup's polynomials
    for fid, n, d in nc.BATCH:
        assert nc.route_model(nc.FIELD[fid].n_limbs, n, d, n) == (nc.LDS, 0, 0, nc.lds_pb(n))
    assert nc.batch_sizes(64) == [31, 32, 33, 67] and nc.batch_sizes(2048) == [1, 2, 5] and nc.batch_sizes(2) == [255, 256, 257, 515]
    # the sweep meets both routes at every order from 4 on, on wide and narrow contexts
    for fid in ("bls", "goldilocks"):
        for n in nc.SWEEP_SMALL[1:] + nc.SWEEP_LARGE:
            assert {c.route[0] for c in nc.sweep_cases(fid, n)} == {nc.MATVEC, nc.LDS}, (fid, n)

"""The full-size matrix-core mat-vec k_mm8w and its balanced launch k_mm8w_flat (csrc/hb_mfma_wide.hip) on matrices of the tests' own
through hb_matrix_from_host + hb_matvec / hb_matvec_check, at the five wide moduli -- 2^256 - 189 and secp256k1's group order among
them, where no BatchOpen plan gets this kernel (test_gpu_edge_values.py) and where alone its remainder can reach 2^256 before the last
correction.  tests/wide_cases.py builds matrices whose entries all fit the int8 image and inputs SOLVED so that outputs are pool values
of edge_values.py; tests/test_wide_cases_host.py holds that these reach the short quotient and the remainder >= 2^256 hundreds of times
a launch.  Which kernel a launch runs is asked of the library (hb_debug_matvec_route), not assumed: an answer of the integer kernel
would pass every comparison here and prove nothing.  Exact equality against Python ints everywhere.

Unit launch: C = 290 chunks (18 full chunk tiles and one of 2), blocks of len(pool) = 55 chunks, edge-valued inputs and solved inputs in
turn.  The shapes' instantiations k_mm8w<CHECK, PEEL, K> are in UNIT_SHAPES and asserted through the route query.
Balanced launch: C = 4099 over (96, 64) and (80, 57): on 256 CUs ranges of 6 and 7 passes (a two-piece short round and a three-pass
round) and of 5 and 6 (four pieces and two).  Every chunk repeats one of 220 edge-valued chunks, so EVERY output is held against
Python ints, and against the integer kernel over a second handle of the same matrix.

Time a case on an MI355X, host-side Python and the case's share of the reference included (measured, the slowest modulus of each):
  unit     (8, 4) 0.01 s   (12, 9) 0.01 s   (16, 32) 0.03 s   (22, 22) 0.03 s   (33, 40) 0.07 s   (40, 24) 0.05 s   (64, 64) 0.26 s   (112, 57) 0.31 s
  check    0.01 s each (the reference is the unit case's), 0.07 s for the first of a process
  balanced (96, 64) 0.46 s   (80, 57) 0.27 s
  the table test 2.2 s when it is the first to load the library and make a context; the module 8.5 s."""
import ctypes
import os
import random

import numpy as np
import pytest

import flat_schedule_model as fsm
import wide_cases as wc
from conftest import clear_hook, set_hook
from test_gpu_edge_values import BLS, P256, SECP_N, WIDE, WIDE_IDS

pytestmark = pytest.mark.gpu

UNIT_CHUNKS = 290
# (n_out, d): K = outputs a lane keeps (row tiles of 4 K rows), K-blocks peeled, row tiles, K-blocks -- what the launch rule gives, asserted
# through the route query; the last entry: whether the row tiles are cut into row groups (rq < n_rt) on 256 CUs
UNIT_SHAPES = {
    (8, 4): (2, 1, 1, 1, False),
    (12, 9): (3, 2, 1, 2, False),
    (16, 32): (4, 4, 1, 4, False),
    (22, 22): (3, 3, 2, 3, False),       # a short second row tile
    (33, 40): (3, 3, 3, 5, False),       # three K-blocks peeled and one loop body
    (40, 24): (4, 3, 3, 3, False),       # the last row tile has 8 rows
    (64, 64): (4, 4, 4, 8, False),       # four peeled, two loop bodies
    (112, 57): (4, 4, 7, 8, True),       # seven row tiles in groups of four
}
LAYOUT_SHAPES = [(22, 22), (40, 24)]
FLAT_CHUNKS, FLAT_PERIOD = 4099, 220
FLAT_SHAPES = {(96, 64): {(2, 2), (1, 3)}, (80, 57): {(4, 1), (2, 2)}}     # (pieces, passes) of the short rounds that occur on 256 CUs
FLAT_MODULI, FLAT_IDS = [BLS, P256, SECP_N], ["bls", "2^256-189", "secp256k1-n"]


def unit_case(p, shape):
    return wc.case(p, shape[0], shape[1], UNIT_CHUNKS)


def flat_case(p, shape):
    return wc.case(p, shape[0], shape[1], FLAT_CHUNKS, FLAT_PERIOD)


def _skip_without_the_kernel():
    if os.environ.get("HB_NO_MFMA") or os.environ.get("HB_NO_MFMA_WIDE"):
        pytest.skip("full-size matrix-core path disabled by HB_NO_MFMA / HB_NO_MFMA_WIDE")


class _Matrix:
    """an hb_matrix handle of a case's matrix"""

    def __init__(self, ctx, m):
        from honeybadgermpc_amd._capi import np_ptr

        self.ctx, self.n_out, self.d = ctx, len(m), len(m[0])
        self.h = ctypes.c_void_p()
        host = ctx.host_elems([v for r in m for v in r])
        ctx.check(ctx.lib.hb_matrix_from_host(ctx.h, np_ptr(host), self.n_out, self.d, ctypes.byref(self.h), ctx.stream()), "hb_matrix_from_host")

    def route(self, count):
        from honeybadgermpc_amd._capi import np_ptr

        out = np.zeros(8, dtype=np.int32)
        self.ctx.check(self.ctx.lib.hb_debug_matvec_route(self.ctx.h, self.h, count, np_ptr(out)), "hb_debug_matvec_route")
        return [int(v) for v in out]

    def close(self):
        self.ctx.lib.hb_matrix_destroy(self.h)


def _view(party_major, rows, count):
    from honeybadgermpc_amd._capi import HbView

    return HbView(1, count) if party_major else HbView(rows, 1)


def _laid_out(vals, party_major):
    """[chunk][row] -> flat, party-major [row][chunk] or chunk-major [chunk][row]"""
    if party_major:
        return [vals[c][r] for r in range(len(vals[0])) for c in range(len(vals))]
    return [v for row in vals for v in row]


def _upload_inputs(ctx, cs, in_pm=True, perm=None):
    """perm: term l reads buffer row perm[l], so buffer row perm[l] holds x_l"""
    xs = [cs.x(c) for c in range(cs.count)]
    if perm is not None:
        where = {r: l for l, r in enumerate(perm)}
        xs = [[x[where[r]] for r in range(cs.d)] for x in xs]
    return ctx.upload_ints(_laid_out(xs, in_pm))


def _matvec(mat, cs, xin, in_pm=True, out_pm=True, perm=None):
    from honeybadgermpc_amd._capi import np_ptr

    ctx = mat.ctx
    out = ctx.empty(cs.count * cs.n_out)
    rows = np.array(perm, dtype=np.int32) if perm is not None else None
    ctx.check(ctx.lib.hb_matvec(ctx.h, mat.h, ctx.ptr(xin), _view(in_pm, cs.d, cs.count), np_ptr(rows) if perm is not None else None,
                                ctx.ptr(out), _view(out_pm, cs.n_out, cs.count), cs.count, ctx.stream()), "hb_matvec")
    return out


def _expected(cs, out_pm=True):
    return _laid_out([cs.outputs(c) for c in range(cs.count)], out_pm)


def _first_difference(cs, got, out_pm=True):
    """(row, chunk, got, want) of the first wrong output: what a failure names"""
    for c in range(cs.count):
        want = cs.outputs(c)
        for r in range(cs.n_out):
            g = got[r * cs.count + c] if out_pm else got[c * cs.n_out + r]
            if g != want[r]:
                return {"row": r, "chunk": c, "got": hex(g), "want": hex(want[r])}
    return None


def _assert_route(mat, shape, count=UNIT_CHUNKS):
    k, peel, n_rt, nkb, _ = UNIT_SHAPES[shape]
    kind, tile_rows, g_rt, g_kb, g_peel, tpw, rq, slots = mat.route(count)
    assert (kind, tile_rows, g_rt, g_kb, g_peel, slots) == (1, 4 * k, n_rt, nkb, peel, 0), (shape, mat.route(count))
    assert tpw >= 1 and 1 <= rq <= n_rt
    return rq < n_rt


def test_the_unit_shapes_cover_every_instantiation():
    """K in {2, 3, 4} and PEEL in {1, 2, 3, 4} all occur, and a shape whose row tiles are cut into row groups; a K-block loop too"""
    import torch
    from honeybadgermpc_amd._capi import Context

    _skip_without_the_kernel()
    assert {v[0] for v in UNIT_SHAPES.values()} == {2, 3, 4} and {v[1] for v in UNIT_SHAPES.values()} == {1, 2, 3, 4}
    assert any(v[3] > v[1] for v in UNIT_SHAPES.values())
    ctx = Context.get(BLS)
    grouped = set()
    for shape in UNIT_SHAPES:
        mat = _Matrix(ctx, unit_case(BLS, shape).m)
        if _assert_route(mat, shape):
            grouped.add(shape)
        # below the chunk count at which a wave pass of 16 chunks pays: the integer kernel
        assert mat.route(255) == [0] * 8
        mat.close()
    if torch.cuda.get_device_properties(ctx.device).multi_processor_count == 256:
        assert grouped == {s for s, v in UNIT_SHAPES.items() if v[4]} and grouped, grouped       # (the rule simulates the CU count)


@pytest.mark.parametrize("shape", list(UNIT_SHAPES), ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("p", WIDE, ids=WIDE_IDS)
def test_unit_launch_at_targeted_outputs(p, shape):
    from honeybadgermpc_amd._capi import Context

    _skip_without_the_kernel()
    ctx = Context.get(p)
    cs = unit_case(p, shape)
    mat = _Matrix(ctx, cs.m)
    _assert_route(mat, shape)
    got = ctx.download_ints(_matvec(mat, cs, _upload_inputs(ctx, cs)))
    # the solved chunks put the pool values where they were aimed
    for c in range(cs.count):
        for r, v in cs.targets_of(c):
            assert got[r * cs.count + c] == v, (hex(p), shape, "row", r, "chunk", c, hex(got[r * cs.count + c]), hex(v))
    assert got == _expected(cs), (hex(p), shape, _first_difference(cs, got))
    if shape in LAYOUT_SHAPES:
        perm = list(range(cs.d))
        random.Random(cs.d).shuffle(perm)
        for in_pm in (True, False):
            xin = _upload_inputs(ctx, cs, in_pm, perm)
            for out_pm in (True, False):
                got = ctx.download_ints(_matvec(mat, cs, xin, in_pm, out_pm, perm))
                assert got == _expected(cs, out_pm), (hex(p), shape, in_pm, out_pm, _first_difference(cs, got, out_pm))
    _assert_route(mat, shape)
    mat.close()


def _flag(ctx, mat, cs, xin, expect, check_rows):
    """hb_matvec_check over party-major buffers -> the mismatch flag"""
    import torch
    from honeybadgermpc_amd._capi import np_ptr

    flag = torch.zeros(1, dtype=torch.int32, device=ctx.tdev)
    rows = np.array(check_rows, dtype=np.int32)
    ctx.check(ctx.lib.hb_matvec_check(ctx.h, mat.h, ctx.ptr(xin), _view(True, cs.d, cs.count), None, ctx.ptr(expect), _view(True, cs.n_out, cs.count),
                                      np_ptr(rows), len(check_rows), ctx.ptr(flag), cs.count, ctx.stream()), "hb_matvec_check")
    return int(flag.item())


def _flips_are_caught(ctx, mat, cs, xin, expect, places, rnd):
    """one flipped bit at each (row, chunk) is caught, and is not when its row is left out of check_rows"""
    every = list(range(cs.n_out))
    for r, c in places:
        bad = expect.clone()
        bad[r * cs.count + c, rnd.randrange(4)] ^= 1 << rnd.randrange(63)
        assert _flag(ctx, mat, cs, xin, bad, every) == 1, (hex(cs.p), (cs.n_out, cs.d), "row", r, "chunk", c, "flip not caught")
        assert _flag(ctx, mat, cs, xin, bad, [i for i in every if i != r]) == 0, (hex(cs.p), (cs.n_out, cs.d), "row", r, "chunk", c, "flag without the row")


def _special_places(cs, limit):
    """a targeted (row, chunk) whose output is 0, one whose output is p - 1, one whose output is 2^256 - p"""
    p = cs.p
    places = []
    for special in (0, p - 1, ((1 << 256) - p) % p):
        places.append(next((r, c) for c in range(limit) for r, v in cs.targets_of(c) if v == special))
    return places


@pytest.mark.parametrize("shape", list(UNIT_SHAPES), ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("p", WIDE, ids=WIDE_IDS)
def test_unit_launch_check_variant(p, shape):
    """k_mm8w<true, ..>: the right outputs leave the flag 0; one flipped bit raises it in the first chunk tile, in the ragged one, in
    the last row of the last (short) row tile and at an output of 0, of p - 1 and of 2^256 - p"""
    from honeybadgermpc_amd._capi import Context

    _skip_without_the_kernel()
    ctx = Context.get(p)
    cs = unit_case(p, shape)
    mat = _Matrix(ctx, cs.m)
    _assert_route(mat, shape)
    xin = _upload_inputs(ctx, cs)
    expect = ctx.upload_ints(_expected(cs))
    assert _flag(ctx, mat, cs, xin, expect, list(range(cs.n_out))) == 0, (hex(p), shape, "right outputs refused")
    rnd = random.Random(cs.n_out * cs.d)
    last = cs.n_out - 1
    places = [(rnd.randrange(cs.n_out), rnd.randrange(16)), (rnd.randrange(cs.n_out), cs.count - 1 - rnd.randrange(2)),
              (last, rnd.randrange(cs.count)), (last, cs.count - 1)] + _special_places(cs, cs.count)
    _flips_are_caught(ctx, mat, cs, xin, expect, places, rnd)
    mat.close()


def _short_rounds(n_rt, nkb, slots, n_tiles, grid=256):
    """by the schedule model: (pieces, passes) of a workgroup's short round -> [(pass, ..)] of the first workgroup that has one"""
    found = {}
    for b in range(grid):
        _, q, _, _, rounds = fsm.workgroup(b, grid, n_tiles * n_rt, n_rt, nkb, slots)
        if q & 3:
            work, _, pieces = rounds[-1]
            found.setdefault((pieces, q & 3), sorted({w[1] for w in work}))
    return found


@pytest.mark.parametrize("shape", list(FLAT_SHAPES), ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("p", FLAT_MODULI, ids=FLAT_IDS)
def test_balanced_launch_at_targeted_outputs(p, shape, monkeypatch):
    import torch
    from honeybadgermpc_amd._capi import Context

    _skip_without_the_kernel()
    if os.environ.get("HB_MM8W_FLAT") is not None:
        pytest.skip("HB_MM8W_FLAT is set: the launch rule is overridden, and read once a process")
    ctx = Context.get(p)
    cus = torch.cuda.get_device_properties(ctx.device).multi_processor_count
    if cus != 256:
        pytest.skip("the shapes are chosen for the launch rule on 256 CUs; this device has %d" % cus)
    cs = flat_case(p, shape)
    n_tiles = (cs.count + 15) // 16
    clear_hook(monkeypatch, "HB_NO_MFMA_WIDE")
    mat = _Matrix(ctx, cs.m)
    kind, tile_rows, n_rt, nkb, _, _, _, slots = mat.route(cs.count)
    assert (kind, tile_rows, n_rt, nkb) == (2, 16, (cs.n_out + 15) // 16, (cs.d + 7) // 8) and slots >= 3, (shape, mat.route(cs.count))
    assert slots == fsm.ring_slots(n_rt, nkb)
    shorts = _short_rounds(n_rt, nkb, slots, n_tiles)
    assert set(shorts) == FLAT_SHAPES[shape], (shape, sorted(shorts))
    # a second handle of the same matrix, first used with the full-size path switched off: it stays on the integer kernel
    set_hook(monkeypatch, "HB_NO_MFMA_WIDE", "1")
    plain = _Matrix(ctx, cs.m)
    assert plain.route(cs.count) == [0] * 8
    clear_hook(monkeypatch, "HB_NO_MFMA_WIDE")
    assert plain.route(cs.count) == [0] * 8 and mat.route(cs.count)[0] == 2

    xin = _upload_inputs(ctx, cs)
    out = _matvec(mat, cs, xin)
    ref = _matvec(plain, cs, xin)
    got = ctx.download_ints(out)
    for c in range(cs.count):
        for r, v in cs.targets_of(c):
            assert got[r * cs.count + c] == v, (hex(p), shape, "row", r, "chunk", c, hex(got[r * cs.count + c]), hex(v))
    assert got == _expected(cs), (hex(p), shape, _first_difference(cs, got))
    assert bool((out == ref).all()), (hex(p), shape, "balanced launch and integer kernel differ")

    # the check variant: right outputs pass; a flip inside a short round of each kind, in the first and in the last tile is caught
    expect = ctx.upload_ints(_expected(cs))
    assert _flag(ctx, mat, cs, xin, expect, list(range(cs.n_out))) == 0, (hex(p), shape, "right outputs refused")
    rnd = random.Random(cs.n_out + cs.d)
    places = [(rnd.randrange(cs.n_out), rnd.randrange(16)), (cs.n_out - 1, cs.count - 1)]
    for kind_of_round, passes in sorted(shorts.items()):
        ps = rnd.choice(passes)
        tile, rt = divmod(ps, n_rt)
        chunk = min(16 * tile + rnd.randrange(16), cs.count - 1)
        places.append((min(16 * rt + rnd.randrange(16), cs.n_out - 1), chunk))
    places.append(_special_places(cs, cs.period)[rnd.randrange(3)])
    _flips_are_caught(ctx, mat, cs, xin, expect, places, rnd)
    assert mat.route(cs.count)[0] == 2
    mat.close()
    plain.close()

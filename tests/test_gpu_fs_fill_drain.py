"""The start and the end of a workgroup's life in the small-entry decode + validate kernel (k_mm8f, hb_mfma_fused.hip): the first unit is
scaled in the prologue, ahead of the tables' barrier, into element buffers of which only the padding terms' slots are zeroed; the last
unit has nothing left to scale.  Through BatchOpen at the production points x = i + 1 over BLS12-381's r: bit for bit against the same
plan on the integer-VALU family, and against the oracle's interpolation on a sample of chunks.

Shapes: d = 22 (two padding terms), d = 6, d = 4 (the kernel's smallest), d = 16 (d == 8 NKB: nothing to zero); chunk counts from one
partial tile to workgroups with one, two and three units (the grid is derived as fs_launch derives it).

BatchOpen reports a verdict only.  The first disagreeing chunk and the bitmap of disagreeing chunks of the same kernel are read through
hb_quick_interp_check_map; the integer-VALU family has no bitmap, so both are compared with the corrupted places themselves."""
import ctypes
import random

import numpy as np
import pytest

import oracle
from conftest import BLS as P

pytestmark = pytest.mark.gpu

INT_MAX = (1 << 31) - 1
SHAPES = [(64, 21), (16, 5), (13, 3), (48, 15)]
_plans = {}


def _grid(n_units, cus):
    """workgroups of a launch over n_units units (fs_launch: one per CU at most, trimmed to the rounds it takes)"""
    blocks = min(cus, n_units)
    rounds = (n_units + blocks - 1) // blocks
    return (n_units + rounds - 1) // rounds


def _chunk_counts():
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    # 64 G + 1: G + 1 units, some workgroups run one unit and some two
    u12 = cus + 1
    g = _grid(u12, cus)
    assert u12 % g != 0 and (u12 + g - 1) // g == 2
    # from 64 G 2 + 37 upwards (a ragged last tile): the first unit count whose trimmed grid leaves some workgroups two units and some three
    u23 = 2 * cus + 1
    while u23 % _grid(u23, cus) == 0 or (u23 + _grid(u23, cus) - 1) // _grid(u23, cus) != 3:
        u23 += 1
    return [1, 16, 17, 33, 64, 65, 64 * (u12 - 1) + 1, 64 * (u23 - 1) + 37]


def _plan(n, t, max_c):
    """the two plans of a shape (matrix cores, integer VALU) and its arrival sets: built once"""
    from honeybadgermpc_amd._capi import Context, np_ptr
    from honeybadgermpc_amd.device import BatchOpen

    if (n, t) not in _plans:
        ctx = Context.get(P)
        d = t + 1
        order = list(range(n))
        random.Random(n * 100 + t).shuffle(order)
        z, zc = order[:d], order[d : d + t]
        x = list(range(1, n + 1))
        op = BatchOpen(P, n, t, z=z, zc=zc, max_shares=max_c * d)
        op.set_fused_validate(True)
        assert op.uses_matrix_cores() and op.fused_validate_kernel() == "small"
        ref = BatchOpen(P, n, t, z=z, zc=zc, max_shares=max_c * d)
        ref.set_matrix_cores(False)
        assert not ref.uses_matrix_cores()
        V = ctypes.c_void_p()
        ctx.check(ctx.lib.hb_vand_matrix_create(ctx.h, np_ptr(ctx.host_elems(x)), n, d, ctypes.byref(V), ctx.stream()), "V")
        _plans[(n, t)] = (op, ref, z, zc, x, V)
    return _plans[(n, t)]


def _columns(ctx, V, n, d, c, seed):
    """c random polynomials of d coefficients (coefficient-major, canonical: 253 random bits) and their values at the n points, party-major"""
    import torch

    from honeybadgermpc_amd._capi import HbView

    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    coef = torch.randint(-(1 << 63), (1 << 63) - 1, (d * c, 4), dtype=torch.int64, device="cuda", generator=gen)
    coef[:, 3] &= (1 << 61) - 1
    cols = ctx.empty(n * c)
    ctx.check(ctx.lib.hb_matvec(ctx.h, V, ctx.ptr(coef), HbView(1, c), None, ctx.ptr(cols), HbView(1, c), c, ctx.stream()), "columns")
    return coef, cols


@pytest.mark.parametrize("ci", range(8))
@pytest.mark.parametrize("n,t", SHAPES)
def test_fill_and_drain_vs_valu_and_oracle(n, t, ci):
    import torch

    from honeybadgermpc_amd._capi import Context, np_ptr

    counts = _chunk_counts()
    c = counts[ci]
    d = t + 1
    ctx = Context.get(P)
    op, ref, z, zc, x, V = _plan(n, t, max(counts))
    coef, cols = _columns(ctx, V, n, d, c, seed=n * 1000 + c)
    b = c * d
    res, msg = op.r2_decode(cols, b), op.r1_decode(cols, b)
    assert op.ok()
    want_res, want_msg = ref.r2_decode(cols, b), ref.r1_decode(cols, b)
    assert ref.ok()
    assert torch.equal(res, want_res) and torch.equal(msg, want_msg)
    # what was decoded is what was encoded: chunk-major coefficients, the constant terms
    assert torch.equal(res.view(c, d, 4), coef.view(d, c, 4).transpose(0, 1)) and torch.equal(msg, coef[:c])
    # the oracle's interpolation of a sample of chunks from the received columns
    rnd = random.Random(c)
    sample = sorted({0, c - 1, min(c - 1, 37), c // 2} | {rnd.randrange(c) for _ in range(4)})
    got_cols = ctx.download_ints(cols.view(n, c, 4)[z][:, sample].reshape(-1, 4).contiguous())
    ys = [[got_cols[i * len(sample) + k] for i in range(d)] for k in range(len(sample))]
    want = oracle.vandermonde_batch_interpolate([x[i] for i in z], ys, P)
    got = ctx.download_ints(res.view(c, d, 4)[sample].reshape(-1, 4).contiguous())
    assert [got[k * d : (k + 1) * d] for k in range(len(sample))] == want
    assert ctx.download_ints(msg[sample].contiguous()) == [row[0] for row in want]
    if (n, t) != (64, 21):
        return
    # one compared column corrupted in a chunk of the first tile, of the first unit's third tile and in the last chunk
    places = sorted({min(5, c - 1), min(37, c - 1), c - 1})
    bad = cols.clone()
    for m in places:
        bad.view(n, c, 4)[zc[1], m, 0] ^= 1
    for plan in (op, ref):
        plan.r2_decode(bad, b)
        assert not plan.ok()
        plan.r1_decode(bad, b)
        assert not plan.ok()
        plan.r2_decode(cols, b)
        assert plan.ok()
    for n_coef in (d, 1):
        status = torch.tensor([0, INT_MAX], dtype=torch.int32, device="cuda")
        bad_map = torch.zeros((c + 31) // 32 + 1, dtype=torch.int32, device="cuda")
        out = ctx.empty(c * d)
        za, zca = np.array(z, dtype=np.int32), np.array(zc, dtype=np.int32)
        rc = ctx.lib.hb_quick_interp_check_map(ctx.h, np_ptr(ctx.host_elems(x)), n, np_ptr(za), d, np_ptr(zca), len(zc), ctx.ptr(bad), c, 0, c,
                                               ctx.ptr(out) if n_coef == d else None, ctx.ptr(status), ctx.ptr(bad_map), ctx.stream())
        ctx.check(rc, "hb_quick_interp_check_map")
        assert status.tolist() == [1, places[0]]
        bits = np.unpackbits(bad_map.cpu().numpy().view(np.uint8), bitorder="little")
        assert np.nonzero(bits)[0].tolist() == places
        if n_coef == d:
            assert torch.equal(out, want_res)

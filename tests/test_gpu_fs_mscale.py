"""k_mm8f's division of the received columns by den on the matrix cores (hb_mfma_fused.hip, scale_unit's MS branch) on the device, against
the same library with HB_NO_FUSED_MSCALE=1 (the T_q multiplication) and against the polynomials the inputs were encoded from (checked
once per case against the oracle's interpolation).

Shapes: n = 64, t = 21 at the benchmark's arrival order and at the 22 largest points (packed last tiles, k_mm8f<3, 2> and <3, 1>); the same
with ten compared senders (32 and 11 rows: nothing packs, k_mm8f<3, 0>); n = 13, t = 3 (d = 4, the smallest the kernel takes).  Chunk counts:
a lone partial unit, exactly one unit, one unit and a chunk, three units, a ragged last unit.  A launch has as many workgroups as units up to
the number of compute units, so at these counts every unit is a workgroup's first, whose tasks read the tables from global memory; the
task of the steady state (tables in LDS) runs from a workgroup's second unit on, which C = 64 * 260 + 17 reaches on every device: the
second test.  Inputs: tests/structured.py's rows with every third row one whose VALUES at the arrival points are
members of tests/edge_values.py's pool -- the inputs of the division themselves."""
import random

import numpy as np
import pytest

import edge_values
import oracle
from conftest import BLS, clear_hook, set_hook

pytestmark = pytest.mark.gpu

INT_MAX = (1 << 31) - 1
P189 = (1 << 256) - 189
CHUNKS = [1, 63, 64, 65, 129, 64 * 3 + 17]
C_MANY = 64 * 260 + 17           # more units than any device has compute units: every workgroup's second unit is scaled in the steady state
C_MAX = max(CHUNKS)
_cache = {}


def _shape(name):
    """(n, t, z, zc)"""
    if name == "bench-order":
        order = np.random.Generator(np.random.PCG64(2024)).permutation(64).tolist()
        return 64, 21, order[:22], order[22:43]
    rnd = random.Random(len(name))
    if name == "largest":
        z = list(range(64 - 22, 64))
        rnd.shuffle(z)
        return 64, 21, z, rnd.sample(range(64 - 22), 21)
    if name == "unpacked":
        order = list(range(64))
        rnd.shuffle(order)
        return 64, 21, order[:22], order[22:32]
    order = list(range(13))
    rnd.shuffle(order)
    return 13, 3, order[:4], order[4:7]


def _data(p, name):
    """polynomials (C_MAX rows), their codewords [chunk][party], the shape: built once, never changed"""
    from structured import structured_rows

    key = (p, name)
    if key not in _cache:
        n, t, z, zc = _shape(name)
        d = t + 1
        x = list(range(1, n + 1))
        rnd = random.Random(p % 1009 + len(name))
        polys = structured_rows(rnd, p, C_MAX, d)
        edge = edge_values.targeted_rows(p, x, z, d, (C_MAX + 1) // 3, seed=len(name))
        for i, row in enumerate(edge):
            polys[1 + 3 * i if 1 + 3 * i < C_MAX else 0] = row
        polys[0] = edge[0]                                        # (the lone chunk of C = 1 is edge-valued too)
        enc = oracle.vandermonde_batch_evaluate(x, polys, p)      # [C_MAX][n]
        want = oracle.vandermonde_batch_interpolate([x[i] for i in z], [[enc[k][i] for i in z] for k in range(C_MAX)], p)
        assert want == polys
        _cache[key] = (n, t, z, zc, x, polys, enc)
    return _cache[key]


def _last():
    from honeybadgermpc_amd._capi import load_library

    lib = load_library()
    return lib.hb_debug_fs_last_pack(), lib.hb_debug_fs_last_mscale()


def _check_map(ctx, x, z, zc, cols, c, n_coef):
    """the kernel through hb_quick_interp_check_map: (status words, chunks set in the bitmap, the bitmap, coefficients or None)"""
    import torch

    from honeybadgermpc_amd._capi import np_ptr

    n, d = len(x), len(z)
    status = torch.tensor([0, INT_MAX], dtype=torch.int32, device="cuda")
    bad_map = torch.zeros((c + 31) // 32 + 1, dtype=torch.int32, device="cuda")
    out = ctx.empty(c * d)
    za, zca = np.array(z, dtype=np.int32), np.array(zc, dtype=np.int32)
    rc = ctx.lib.hb_quick_interp_check_map(ctx.h, np_ptr(ctx.host_elems(x)), n, np_ptr(za), d, np_ptr(zca), len(zc), ctx.ptr(cols), c, 0, c,
                                           ctx.ptr(out) if n_coef == d else None, ctx.ptr(status), ctx.ptr(bad_map), ctx.stream())
    ctx.check(rc, "hb_quick_interp_check_map")
    bits = np.unpackbits(bad_map.cpu().numpy().view(np.uint8), bitorder="little")
    return status.tolist(), np.nonzero(bits)[0].tolist(), bad_map, out if n_coef == d else None


def _modes(monkeypatch):
    for on in (True, False):
        if on:
            clear_hook(monkeypatch, "HB_NO_FUSED_MSCALE")
        else:
            set_hook(monkeypatch, "HB_NO_FUSED_MSCALE", "1")
        yield on


@pytest.mark.parametrize("name", ["bench-order", "largest", "unpacked", "d4"])
@pytest.mark.parametrize("p", [BLS, P189], ids=["bls-r", "2^256-189"])
def test_matrix_core_division_agrees_with_the_multiplication_and_the_oracle(monkeypatch, p, name):
    import torch

    from honeybadgermpc_amd._capi import Context
    from honeybadgermpc_amd.device import BatchOpen

    ctx = Context.get(p)
    n, t, z, zc, x, polys, enc = _data(p, name)
    d = t + 1
    pack_r2, pack_r1 = {"bench-order": (2, 1), "largest": (2, 1), "unpacked": (0, 0), "d4": (1, 1)}[name]
    for c in CHUNKS:
        cols = ctx.upload_ints([enc[k][j] for j in range(n) for k in range(c)])
        want_res = [v for row in polys[:c] for v in row]
        want_msg = [row[0] for row in polys[:c]]
        # one lie at a time in a compared column: a middle chunk, the last chunk
        lies = []
        for sender, chunk in ((zc[-1], c // 2), (zc[0], c - 1)):
            bad = cols.clone()
            bad.view(n, c, 4)[sender, chunk, 2] ^= 1 << 33
            lies.append((chunk, bad))
        seen = {}
        for on in _modes(monkeypatch):
            b = c * d
            op = BatchOpen(p, n, t, z=z, zc=zc, max_shares=b)           # (the hook is read when the plan builds its images)
            assert op.fused_validate_kernel() == "small"
            res = op.r2_decode(cols, b)
            assert _last() == (pack_r2, 1 if on else 0)
            msg = op.r1_decode(cols, b)
            assert _last() == (pack_r1, 1 if on else 0)
            assert op.ok()
            assert ctx.download_ints(res) == want_res and ctx.download_ints(msg) == want_msg
            got = [res, msg]
            for chunk, bad in lies:
                res2 = op.r2_decode(bad, b)
                assert not op.ok() and torch.equal(res2, res)
                msg2 = op.r1_decode(bad, b)
                assert not op.ok() and torch.equal(msg2, msg)
            for n_coef in (d, 1):
                status, chunks, bad_map, out = _check_map(ctx, x, z, zc, cols, c, n_coef)
                assert _last() == (pack_r2 if n_coef == d else pack_r1, 1 if on else 0)
                assert status == [0, INT_MAX] and chunks == []
                if out is not None:
                    assert torch.equal(out, res)
                got.append(bad_map)
                for chunk, bad in lies:
                    status, chunks, bad_map, out = _check_map(ctx, x, z, zc, bad, c, n_coef)
                    assert status == [1, chunk] and chunks == [chunk], (c, chunk, n_coef, on)
                    if out is not None:
                        assert torch.equal(out, res)
                    got.append(bad_map)
            seen[on] = got
        assert len(seen[True]) == len(seen[False]) and all(torch.equal(a, b_) for a, b_ in zip(seen[True], seen[False]))


@pytest.mark.parametrize("name", ["bench-order", "largest", "unpacked", "d4"])
@pytest.mark.parametrize("p", [BLS, P189], ids=["bls-r", "2^256-189"])
def test_steady_state_units_of_every_workgroup(monkeypatch, p, name):
    """more units than workgroups: the second and later units of a workgroup are the ones the matrix-core task scales.  The inputs are the
    C_MAX edge-valued and structured codewords over and over; R2 and R1 through the one-shot check, both modes, bit for bit"""
    import torch

    from honeybadgermpc_amd._capi import Context

    ctx = Context.get(p)
    n, t, z, zc, x, polys, enc = _data(p, name)
    d = t + 1
    c = C_MANY
    base = ctx.upload_ints([enc[k][j] for j in range(n) for k in range(C_MAX)]).view(n, C_MAX, 4)
    reps = (c + C_MAX - 1) // C_MAX
    cols = base.repeat(1, reps, 1)[:, :c, :].contiguous().view(n * c, 4)
    want = ctx.upload_ints([v for row in polys for v in row]).view(C_MAX, d * 4).repeat(reps, 1)[:c].contiguous().view(c * d, 4)
    chunk = c - 3                                   # a chunk of the last unit: no workgroup's first
    bad = cols.clone()
    bad.view(n, c, 4)[zc[-1], chunk, 0] ^= 1
    seen = {}
    for on in _modes(monkeypatch):
        got = []
        for n_coef in (d, 1):
            status, chunks, bad_map, out = _check_map(ctx, x, z, zc, cols, c, n_coef)
            assert _last()[1] == (1 if on else 0)
            assert status == [0, INT_MAX] and chunks == []
            if out is not None:
                assert torch.equal(out.view(-1, 4), want)
            status, chunks, bad_map, out = _check_map(ctx, x, z, zc, bad, c, n_coef)
            assert status == [1, chunk] and chunks == [chunk]
            got.append(bad_map)
            if out is not None:
                assert torch.equal(out.view(-1, 4), want)
        seen[on] = got
    assert all(torch.equal(a, b_) for a, b_ in zip(seen[True], seen[False]))

"""k_mm8f's first unit with the division by den on the matrix cores (hb_mfma_fused.hip): a wave's terms wave, wave + 8, wave + 16 are scaled
as ONE block -- the division's tables copied to LDS by the wave that owns a term, the operands read from there, a term the wave does not
have loaded from a clamped address, masked and written as the zeros of its padding slot -- so what can go wrong depends on how many terms
each wave has.  tests/test_gpu_fs_mscale.py drives d = 22 (three terms / two) and d = 4; here:

    d = 8   one term each          (n, t) = (22, 7)       one K-block
    d = 9   two / one              (25, 8)                two K-blocks, the second with one term
    d = 16  two each               (46, 15)
    d = 17  three / two            (49, 16)               three K-blocks
    d = 5   one / none             (16, 4)                waves 5 .. 7 have no term at all

Points 1 .. n, seeded arrival orders, t compared senders.  Chunk counts: a lone partial unit, padding lanes, every unit a workgroup's first
(a launch has as many workgroups as units up to the number of compute units); C = 64 * 260 + 17 at d = 9 and d = 17 reaches the second and
later units of every workgroup on every device, with odd and even numbers of terms a wave in the steady state's deal.  Both moduli:
BLS12-381 r (p < 2^255: any representative is stored) and 2^256 - 189 (the conditional subtraction).  Inputs as in the existing file:
tests/structured.py's rows, every third row edge-valued at the arrival points.  Checked against the polynomials the inputs were encoded
from (the oracle, once per shape) and bit for bit -- outputs, flag, first disagreeing chunk, bitmap -- against the same library with
HB_NO_FUSED_MSCALE=1, the T_q multiplication, which this block is no part of."""
import random

import numpy as np
import pytest

import edge_values
import oracle
from conftest import BLS, clear_hook, set_hook

pytestmark = pytest.mark.gpu

INT_MAX = (1 << 31) - 1
P189 = (1 << 256) - 189
SHAPES = {"d8": (22, 7), "d9": (25, 8), "d16": (46, 15), "d17": (49, 16), "d5": (16, 4)}
CHUNKS = [1, 63, 64, 65, 129]
C_MANY = 64 * 260 + 17
C_MAX = max(CHUNKS)
_cache = {}


def _shape(name):
    """(n, t, z, zc): a seeded arrival order, the first d arrivals decode, the next t are compared"""
    n, t = SHAPES[name]
    order = list(range(n))
    random.Random(1000 * n + t).shuffle(order)
    return n, t, order[: t + 1], order[t + 1 : 2 * t + 1]


def _data(p, name):
    """polynomials (C_MAX rows), their codewords [chunk][party], the shape: built once, never changed"""
    from structured import structured_rows

    key = (p, name)
    if key not in _cache:
        n, t, z, zc = _shape(name)
        d = t + 1
        x = list(range(1, n + 1))
        rnd = random.Random(p % 1009 + n)
        polys = structured_rows(rnd, p, C_MAX, d)
        edge = edge_values.targeted_rows(p, x, z, d, (C_MAX + 1) // 3, seed=n)
        for i, row in enumerate(edge):
            polys[1 + 3 * i if 1 + 3 * i < C_MAX else 0] = row
        polys[0] = edge[0]                                        # (the lone chunk of C = 1 is edge-valued too)
        enc = oracle.vandermonde_batch_evaluate(x, polys, p)      # [C_MAX][n]
        want = oracle.vandermonde_batch_interpolate([x[i] for i in z], [[enc[k][i] for i in z] for k in range(C_MAX)], p)
        assert want == polys
        _cache[key] = (n, t, z, zc, x, polys, enc)
    return _cache[key]


def _mscale():
    from honeybadgermpc_amd._capi import load_library

    return load_library().hb_debug_fs_last_mscale()


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


def _lie_chunks(c):
    """the first unit's last chunk, the last chunk of the launch (one and the same up to C = 64)"""
    return sorted({min(c, 64) - 1, c - 1})


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("p", [BLS, P189], ids=["bls-r", "2^256-189"])
def test_first_unit_block_at_every_term_count(monkeypatch, p, name):
    import torch

    from honeybadgermpc_amd._capi import Context
    from honeybadgermpc_amd.device import BatchOpen

    ctx = Context.get(p)
    n, t, z, zc, x, polys, enc = _data(p, name)
    d = t + 1
    for c in CHUNKS:
        cols = ctx.upload_ints([enc[k][j] for j in range(n) for k in range(c)])
        want_res = [v for row in polys[:c] for v in row]
        want_msg = [row[0] for row in polys[:c]]
        lies = []
        for i, chunk in enumerate(_lie_chunks(c)):
            bad = cols.clone()
            bad.view(n, c, 4)[zc[-1 if i == 0 else 0], chunk, 2] ^= 1 << 33
            lies.append((chunk, bad))
        seen = {}
        for on in _modes(monkeypatch):
            b = c * d
            op = BatchOpen(p, n, t, z=z, zc=zc, max_shares=b)           # (the hook is read when the plan builds its images)
            assert op.fused_validate_kernel() == "small"
            res = op.r2_decode(cols, b)
            assert _mscale() == (1 if on else 0)
            msg = op.r1_decode(cols, b)
            assert _mscale() == (1 if on else 0)
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
                assert _mscale() == (1 if on else 0)
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


@pytest.mark.parametrize("name", ["d9", "d17"])
@pytest.mark.parametrize("p", [BLS, P189], ids=["bls-r", "2^256-189"])
def test_first_unit_block_ahead_of_steady_state_units(monkeypatch, p, name):
    """more units than workgroups: every workgroup scales its first unit with the block and its later ones with the steady state's task.
    The inputs are the C_MAX edge-valued and structured codewords over and over; R2 and R1 through the one-shot check, both modes"""
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
    lies = []
    for i, chunk in enumerate(_lie_chunks(c)):
        bad = cols.clone()
        bad.view(n, c, 4)[zc[-1 if i == 0 else 0], chunk, 0] ^= 1
        lies.append((chunk, bad))
    seen = {}
    for on in _modes(monkeypatch):
        got = []
        for n_coef in (d, 1):
            status, chunks, bad_map, out = _check_map(ctx, x, z, zc, cols, c, n_coef)
            assert _mscale() == (1 if on else 0)
            assert status == [0, INT_MAX] and chunks == []
            got.append(bad_map)
            if out is not None:
                assert torch.equal(out.view(-1, 4), want)
                got.append(out)
            for chunk, bad in lies:
                status, chunks, bad_map, out = _check_map(ctx, x, z, zc, bad, c, n_coef)
                assert status == [1, chunk] and chunks == [chunk], (chunk, n_coef, on)
                got.append(bad_map)
                if out is not None:
                    assert torch.equal(out.view(-1, 4), want)
        seen[on] = got
    assert len(seen[True]) == len(seen[False]) and all(torch.equal(a, b_) for a, b_ in zip(seen[True], seen[False]))

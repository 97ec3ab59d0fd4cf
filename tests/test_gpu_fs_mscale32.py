"""k_mm8f's division by den as two dense 32x32x32 products a task (hb_mfma_fused.hip: fetch_halves, ms_products, ms_words) on the device.
A lane no longer loads its own chunk: lane (r, h) loads half h of chunks r and 32 + r of a unit, and a half swap behind the products puts
chunk = lane back together.  So what can go wrong is a half in the wrong lane, and that shows only where every chunk differs from every
other and a single bad chunk must be named exactly -- which is what this file drives:

    shapes   (n, t) = (64, 21), (25, 8), (16, 4): d = 22, 9, 5 -- a wave with a masked third term, waves with two and one, waves with none
    moduli   BLS12-381 r (any representative below 2p is stored) and 2^256 - 189 (the canonical branch)
    chunks   1, 31, 32, 33, 63, 64, 65 (the new seam lies between chunks 31 and 32 of a unit) and 64 * 260 + 33: steady-state units in
             every workgroup on every device, and a last unit that ends one chunk past the seam
    inputs   every chunk's polynomial distinct: 65 random ones (decoded once by the oracle), and chunk k >= 65 is chunk k mod 65 plus the
             constant (k div 65) * DELTA, whose codeword is that of chunk k mod 65 plus the same constant at every party
    lies     one at a time in a compared column, at chunks 31, 32, 33, the launch's last and 64 * 259 + 32: the reported first chunk and
             the bitmap must name exactly that chunk

Outputs, flag, first disagreeing chunk and bitmap are compared bit for bit with the same library under HB_NO_FUSED_MSCALE=1 (the T_q
multiplication, no matrix-core division at all) and with the polynomials the inputs were encoded from."""
import random

import numpy as np
import pytest

import oracle
from conftest import BLS, clear_hook, set_hook

pytestmark = pytest.mark.gpu

INT_MAX = (1 << 31) - 1
P189 = (1 << 256) - 189
SHAPES = {"d22": (64, 21), "d9": (25, 8), "d5": (16, 4)}
CHUNKS = [1, 31, 32, 33, 63, 64, 65]
C_BIG = 64 * 260 + 33
BASE = 65
LIE_CHUNKS = [31, 32, 33, 64 * 259 + 32]        # (and the launch's last chunk)
_cache = {}


def _shape(name):
    """(n, t, z, zc): a seeded arrival order, the first d arrivals decode, the next t are compared"""
    n, t = SHAPES[name]
    order = list(range(n))
    random.Random(2000 * n + t).shuffle(order)
    return n, t, order[: t + 1], order[t + 1 : 2 * t + 1]


def _data(ctx, p, name):
    """the shape, the columns [n][C_BIG] and the coefficients [C_BIG][d] on the device: built once, never changed"""
    key = (p, name)
    if key not in _cache:
        n, t, z, zc = _shape(name)
        d = t + 1
        x = list(range(1, n + 1))
        rnd = random.Random(p % 1013 + n)
        polys = [[rnd.randrange(p) for _ in range(d)] for _ in range(BASE)]
        enc = oracle.vandermonde_batch_evaluate(x, polys, p)      # [BASE][n]
        assert oracle.vandermonde_batch_interpolate([x[i] for i in z], [[enc[k][i] for i in z] for k in range(BASE)], p) == polys
        delta = rnd.randrange(1, p)
        shift = [(g * delta) % p for g in range(C_BIG // BASE + 1)]
        c0 = [(polys[k % BASE][0] + shift[k // BASE]) % p for k in range(C_BIG)]
        assert len({(c0[k], polys[k % BASE][1]) for k in range(C_BIG)}) == C_BIG        # every chunk's polynomial is another
        cols = ctx.upload_ints([(enc[k % BASE][j] + shift[k // BASE]) % p for j in range(n) for k in range(C_BIG)]).view(n, C_BIG, 4)
        want = ctx.upload_ints([v for row in polys for v in row]).view(BASE, d, 4).repeat(C_BIG // BASE + 1, 1, 1)[:C_BIG].contiguous()
        want[:, 0, :] = ctx.upload_ints(c0)
        _cache[key] = (n, t, z, zc, x, cols, want)
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


def _lies(c):
    return sorted({k for k in LIE_CHUNKS if k < c} | {c - 1})


def _one_shot(monkeypatch, ctx, x, z, zc, cols, want, c):
    """R2 (all coefficients) and R1 (the constant term) through the one-shot check, clean and with each lie, in both modes"""
    import torch

    n, d = len(x), len(z)
    seen = {}
    for on in _modes(monkeypatch):
        got = []
        for n_coef in (d, 1):
            status, chunks, bad_map, out = _check_map(ctx, x, z, zc, cols, c, n_coef)
            assert _mscale() == (1 if on else 0)
            assert status == [0, INT_MAX] and chunks == []
            got.append(bad_map)
            if out is not None:
                assert torch.equal(out.view(c, d, 4), want)
                got.append(out)
            for i, chunk in enumerate(_lies(c)):
                sender = zc[i % len(zc)]
                word = cols.view(n, c, 4)[sender, chunk, 2].clone()
                cols.view(n, c, 4)[sender, chunk, 2] ^= 1 << 33
                status, chunks, bad_map, out = _check_map(ctx, x, z, zc, cols, c, n_coef)
                cols.view(n, c, 4)[sender, chunk, 2] = word
                assert status == [1, chunk] and chunks == [chunk], (c, chunk, n_coef, on)
                got.append(bad_map)
                if out is not None:
                    assert torch.equal(out.view(c, d, 4), want)
        seen[on] = got
    assert len(seen[True]) == len(seen[False]) and all(torch.equal(a, b_) for a, b_ in zip(seen[True], seen[False]))


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("p", [BLS, P189], ids=["bls-r", "2^256-189"])
def test_every_chunk_count_around_the_seam(monkeypatch, p, name):
    import torch

    from honeybadgermpc_amd._capi import Context
    from honeybadgermpc_amd.device import BatchOpen

    ctx = Context.get(p)
    n, t, z, zc, x, cols_big, want_big = _data(ctx, p, name)
    d = t + 1
    for c in CHUNKS:
        cols = cols_big[:, :c, :].contiguous().view(n * c, 4)
        want = want_big[:c].contiguous()
        b = c * d
        seen = {}
        for on in _modes(monkeypatch):
            op = BatchOpen(p, n, t, z=z, zc=zc, max_shares=b)           # (the hook is read when the plan builds its images)
            assert op.fused_validate_kernel() == "small"
            res = op.r2_decode(cols, b)
            assert _mscale() == (1 if on else 0)
            msg = op.r1_decode(cols, b)
            assert _mscale() == (1 if on else 0)
            assert op.ok()
            assert torch.equal(res.view(c, d, 4), want) and torch.equal(msg.view(c, 4), want[:, 0, :])
            seen[on] = (res, msg)
        assert all(torch.equal(a, b_) for a, b_ in zip(seen[True], seen[False]))
        _one_shot(monkeypatch, ctx, x, z, zc, cols, want, c)


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("p", [BLS, P189], ids=["bls-r", "2^256-189"])
def test_steady_state_units_and_a_last_unit_past_the_seam(monkeypatch, p, name):
    from honeybadgermpc_amd._capi import Context

    ctx = Context.get(p)
    n, t, z, zc, x, cols_big, want_big = _data(ctx, p, name)
    _one_shot(monkeypatch, ctx, x, z, zc, cols_big.view(n * C_BIG, 4), want_big, C_BIG)

"""The packed last row tile of the fused decode + validate kernel (k_mm8f, hb_mfma_fused.hip) on the device: plans at config 3's shape
(n = 64, t = 21: R1 has 16 + 6 rows, R2 has 32 + 3 merged + 8 single-group) run packed and with HB_NO_FUSED_PACK=1, against the
full-size kernel (set_fused_validate("wide"); at the modulus above 2^255, where that kernel has no image, the unfused pipeline) and the
oracle's interpolation -- bit for bit.

C = 64 * 3 + 5 chunks: three units, a ragged last unit, padding chunks.  Two arrival sets: a seeded random one, and the 22 largest
points (the largest entries of [N ; P]).  The inputs are tests/structured.py's rows (zero, constant, short, padded chunks among uniform
ones).  BatchOpen reports a verdict only; the first disagreeing chunk and the bitmap of the same kernel, packed the same way, are read
through hb_quick_interp_check_map."""
import random

import numpy as np
import pytest

import oracle
from conftest import BLS as P
from conftest import clear_hook, set_hook

pytestmark = pytest.mark.gpu

INT_MAX = (1 << 31) - 1
SECP_N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141      # a prime above 2^255: the scaled element is made canonical
N, T = 64, 21
D = T + 1
C = 64 * 3 + 5
X = list(range(1, N + 1))
_cache = {}


def _arrivals(which):
    rnd = random.Random(2024)
    if which == "random":
        order = list(range(N))
        rnd.shuffle(order)
        return order[:D], order[D : D + T]
    z = list(range(N - D, N))                      # the 22 largest points
    rnd.shuffle(z)
    return z, rnd.sample(range(N - D), T)


def _data(p, which):
    """polynomials, their codewords on the device, the arrival sets, and the oracle's interpolation of every chunk: built once"""
    from honeybadgermpc_amd._capi import Context
    from structured import structured_rows
    import wide_cases as wc

    key = (p, which)
    if key not in _cache:
        ctx = Context.get(p)
        rnd = random.Random(D * 1000 + len(which))
        polys = structured_rows(rnd, p, C, D)
        if p != P:
            # edge-valued words among the coefficients: the largest residue and the residue of the largest digit sum that 32 digits hold
            polys[7] = [wc.largest_fitting(p)] * D
            polys[8] = [wc.heaviest_fitting(p)] * D
            polys[9] = [p - 1] * D
        enc = oracle.vandermonde_batch_evaluate(X, polys, p)                    # [C][N]
        flat = [enc[k][j] for j in range(N) for k in range(C)]
        z, zc = _arrivals(which)
        want = oracle.vandermonde_batch_interpolate([X[i] for i in z], [[enc[k][i] for i in z] for k in range(C)], p)
        assert want == polys
        _cache[key] = (polys, flat, ctx.upload_ints(flat), z, zc)
    return _cache[key]


def _last_pack():
    from honeybadgermpc_amd._capi import load_library

    return load_library().hb_debug_fs_last_pack()


def _check_map(ctx, z, zc, cols, n_coef):
    """the kernel through hb_quick_interp_check_map: (status words, chunks set in the bitmap, coefficients or None)"""
    import torch

    from honeybadgermpc_amd._capi import np_ptr

    status = torch.tensor([0, INT_MAX], dtype=torch.int32, device="cuda")
    bad_map = torch.zeros((C + 31) // 32 + 1, dtype=torch.int32, device="cuda")
    out = ctx.empty(C * D)
    za, zca = np.array(z, dtype=np.int32), np.array(zc, dtype=np.int32)
    rc = ctx.lib.hb_quick_interp_check_map(ctx.h, np_ptr(ctx.host_elems(X)), N, np_ptr(za), D, np_ptr(zca), len(zc), ctx.ptr(cols), C, 0, C,
                                           ctx.ptr(out) if n_coef == D else None, ctx.ptr(status), ctx.ptr(bad_map), ctx.stream())
    ctx.check(rc, "hb_quick_interp_check_map")
    bits = np.unpackbits(bad_map.cpu().numpy().view(np.uint8), bitorder="little")
    return status.tolist(), np.nonzero(bits)[0].tolist(), out if n_coef == D else None


@pytest.mark.parametrize("p,which", [(P, "random"), (P, "largest"), (SECP_N, "largest")], ids=["bls-random", "bls-largest", "secp-n-largest"])
def test_packed_unpacked_wide_and_oracle_agree(monkeypatch, p, which):
    import torch

    from honeybadgermpc_amd._capi import Context
    from honeybadgermpc_amd.device import BatchOpen

    ctx = Context.get(p)
    polys, flat, cols, z, zc = _data(p, which)
    b = C * D
    want_res = [v for row in polys for v in row]
    want_msg = [row[0] for row in polys]
    outs = {}
    for packed in (True, False):
        if packed:
            clear_hook(monkeypatch, "HB_NO_FUSED_PACK")
        else:
            set_hook(monkeypatch, "HB_NO_FUSED_PACK", "1")
        op = BatchOpen(p, N, T, z=z, zc=zc, max_shares=b)           # (the hook is read when the plan builds its images)
        assert op.fused_validate_kernel() == "small"
        res = op.r2_decode(cols, b)
        assert _last_pack() == (2 if packed else 0)
        msg = op.r1_decode(cols, b)
        assert _last_pack() == (1 if packed else 0)
        assert op.ok()
        assert ctx.download_ints(res) == want_res and ctx.download_ints(msg) == want_msg
        outs[packed] = (res, msg)
        if packed:
            op.set_fused_validate("wide")
            # (no image of the full-size kernel at the modulus above 2^255: there the request leaves decode, re-encode, compare)
            assert op.fused_validate_kernel() == ("wide" if p == P else None)
            wres, wmsg = op.r2_decode(cols, b), op.r1_decode(cols, b)
            assert op.ok()
            assert torch.equal(wres, res) and torch.equal(wmsg, msg)
            op.set_fused_validate(True)
        # a lie, one place at a time: a compared row of the packed tile (R1: compared rows 15 .. 20, R2: 18 .. 20), one of an unpacked
        # tile, the first chunk, the last chunk
        for sender, chunk in ((zc[20], 70), (zc[0], 130), (zc[19], 0), (zc[19], C - 1)):
            bad = cols.clone()
            bad.view(N, C, 4)[sender, chunk, 1] ^= 4
            res2 = op.r2_decode(bad, b)
            assert not op.ok()
            assert torch.equal(res2, res)                       # (the decode reads the rows z alone)
            op.r1_decode(bad, b)
            assert not op.ok()
            for n_coef in (D, 1):
                status, chunks, out = _check_map(ctx, z, zc, bad, n_coef)
                assert _last_pack() == (0 if not packed else 2 if n_coef == D else 1)
                assert status == [1, chunk] and chunks == [chunk], (sender, chunk, n_coef)
                if out is not None:
                    assert torch.equal(out, res)
            op.r2_decode(cols, b)
            assert op.ok()
        status, chunks, out = _check_map(ctx, z, zc, cols, D)
        assert status == [0, INT_MAX] and chunks == [] and torch.equal(out, res)
    assert torch.equal(outs[True][0], outs[False][0]) and torch.equal(outs[True][1], outs[False][1])

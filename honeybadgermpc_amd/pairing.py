"""
Products of BLS12-381 pairings on the device (csrc/hb_pair.hip) against PREPARED G2 points: what the verifier of PolyCommitConst needs.
The G2 side is host work, done once a point (bls12_381_pairing.prepare_g2: 68 line coefficients); the device runs the Miller loop over
those lines and the final exponentiation for a batch of G1 points.  The host model is honeybadgermpc_amd.bls12_381_pairing.

A batch of G1 points is g1.py's tensor (count, 2, 6).  A batch of GT elements is ONE int64 tensor (count, 12, 6): twelve canonical
residues below Q in the tower's order c0.c0.c0, c0.c0.c1, ..., c1.c2.c1, six little-endian 64-bit words each; the values are the
reference crate's (the Miller value to the power 3 (Q^12 - 1) / R).

    PreparedG2(ctx, Q)                          owns the table of one host G2 (not the identity)
    pair(ctx, points, prepared)                 e(points[m], Q) -> (count, 12, 6)
    product(ctx, [(points, prepared), ...])     prod_k e(points_k[m], Q_k), 1 to 4 pairs, one launch -> (count, 12, 6)
    product_is_one(ctx, [...])                  -> (bool tensor (count,), counter (1,) int32: the items that are not 1).  An item with a
                                                point off the curve is rejected.
    download_gt(tensor)                         -> list of host Fq12 (copies to the host)

An identity point contributes 1, as the reference's miller_loop skips it.  Membership of the G1 points in the subgroup of order R is NOT
checked (g1.in_subgroup tells).  Everything is asynchronous on torch's current stream except PreparedG2() (the upload) and download_gt().
"""
import ctypes

import numpy as np

from . import g1
from ._capi import HB_PAIR_GT, HB_PAIR_VERDICT
from .bls12_381 import LIMBS
from .bls12_381_pairing import Fq12, G2, N_LINES, prepare_g2

GT_COORDS = 12
MAX_PAIRS = 4


def _words(v):
    return [(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(LIMBS)]


class PreparedG2:
    """The line coefficients of one G2 point, computed by the host model and uploaded in the library's layout."""

    def __init__(self, ctx, q):
        g1._ctx(ctx)
        if not isinstance(q, G2):
            raise TypeError(f"q: expected a host G2, got {type(q).__name__}")
        if q.is_one():
            raise ValueError("q: the identity has no lines (a pair with it contributes 1: leave it out)")
        self.ctx, self.point = ctx, q
        flat = [w for triple in prepare_g2(q) for c in triple for v in (c.c0, c.c1) for w in _words(v)]
        host = np.array(flat, dtype=np.uint64)
        nbytes = int(ctx.lib.hb_pair_table_bytes())
        self.table = ctx.torch.empty((nbytes // 8,), dtype=ctx.torch.int64, device=ctx.tdev)
        ctx.check(ctx.lib.hb_pair_prepare(ctx.h, host.ctypes.data, 3 * N_LINES, ctx.ptr(self.table), ctx.stream()), "hb_pair_prepare")


def _pairs(ctx, pairs):
    """-> (points (count, K, 2, 6), the array of K table pointers, the tables (kept alive), count, K)"""
    g1._ctx(ctx)
    pairs = list(pairs)
    if not 1 <= len(pairs) <= MAX_PAIRS:
        raise ValueError(f"pairs: between 1 and {MAX_PAIRS} pairs, got {len(pairs)}")
    cols, tables, count = [], [], None
    for k, pr in enumerate(pairs):
        if not isinstance(pr, (tuple, list)) or len(pr) != 2:
            raise TypeError(f"pairs[{k}]: expected (points, PreparedG2)")
        pts, prep = pr
        if not isinstance(prep, PreparedG2):
            raise TypeError(f"pairs[{k}]: expected a PreparedG2, got {type(prep).__name__}")
        if prep.ctx is not ctx:
            raise ValueError(f"pairs[{k}]: the prepared point belongs to another context")
        if prep.table.numel() * 8 != int(ctx.lib.hb_pair_table_bytes()):
            raise ValueError(f"pairs[{k}]: the prepared table has {prep.table.numel() * 8} bytes, not {int(ctx.lib.hb_pair_table_bytes())}")
        t, n = g1._operand(ctx, pts, f"pairs[{k}]")
        if count is None:
            count = n
        elif n != count:
            raise ValueError(f"pairs: {count} points in pair 0 against {n} in pair {k}")
        cols.append(t.reshape(n, 1, 2, LIMBS))
        tables.append(prep.table)
    points = cols[0].reshape(count, 1, 2, LIMBS) if len(cols) == 1 else ctx.torch.cat(cols, dim=1)
    ptrs = (ctypes.c_void_p * len(tables))(*[t.data_ptr() for t in tables])
    return points.contiguous(), ptrs, tables, count, len(tables)


def product(ctx, pairs):
    """prod_k e(points_k[m], Q_k) -> (count, 12, 6)"""
    points, ptrs, _keep, count, K = _pairs(ctx, pairs)
    out = ctx.torch.empty((count, GT_COORDS, LIMBS), dtype=ctx.torch.int64, device=ctx.tdev)
    ctx.check(ctx.lib.hb_pair_product(ctx.h, ptrs, K, ctx.ptr(points), HB_PAIR_GT, ctx.ptr(out), None, None, count, ctx.stream()), "hb_pair_product")
    return out


def pair(ctx, points, prepared):
    """e(points[m], Q) -> (count, 12, 6)"""
    return product(ctx, [(points, prepared)])


def product_is_one(ctx, pairs):
    """-> (bool tensor (count,), counter (1,) int32): whether prod_k e(points_k[m], Q_k) == 1 and every point of item m is on the
    curve; the counter holds the number of rejected items.  Nothing synchronises."""
    points, ptrs, _keep, count, K = _pairs(ctx, pairs)
    torch = ctx.torch
    flags = torch.empty((count,), dtype=torch.int32, device=ctx.tdev)
    counter = torch.zeros((1,), dtype=torch.int32, device=ctx.tdev)
    ctx.check(ctx.lib.hb_pair_product(ctx.h, ptrs, K, ctx.ptr(points), HB_PAIR_VERDICT, None, ctx.ptr(flags), ctx.ptr(counter), count, ctx.stream()),
              "hb_pair_product")
    return flags != 0, counter


def download_gt(tensor):
    """(..., 12, 6) tensor -> flat list of host Fq12.  Copies to the host."""
    import torch

    if not isinstance(tensor, torch.Tensor):
        raise TypeError(f"tensor: expected a torch tensor, got {type(tensor).__name__}")
    if tensor.dtype != torch.int64 or tensor.dim() < 2 or tuple(tensor.shape[-2:]) != (GT_COORDS, LIMBS):
        raise ValueError(f"tensor: expected an int64 tensor of shape (..., {GT_COORDS}, {LIMBS}), got {tensor.dtype} {tuple(tensor.shape)}")
    arr = tensor.cpu().contiguous().numpy().view(np.uint64).reshape(-1, GT_COORDS, LIMBS)
    return [Fq12.from_coords([sum(int(w) << (64 * k) for k, w in enumerate(c)) for c in row]) for row in arr]

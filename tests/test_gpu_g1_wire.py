"""k_g1_decompress, k_g1_compress and k_g1_subgroup (csrc/hb_g1_wire.hip) on the device, g1.in_subgroup's two methods, and
PolyCommitConst.verify_wire.  The device's words, bytes, statuses and flags are bit-equal to hb_selftest_g1_wire on the same inputs (the
same bodies on the host) and equal to the labels of the host model bls12_381.G1 (g1_wire_cases).  The references are computed once and
shared; the batches are 0, 1, 257 (a partial workgroup) and the 1000 vectors with the malformed items mixed in (five workgroups)."""
import functools

import numpy as np
import pytest

import g1_support as s
import g1_wire_cases as wc
import pairing_support as ps

from honeybadgermpc_amd.bls12_381 import G1, R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from honeybadgermpc_amd._capi import Context

    return Context.get(R)


@functools.lru_cache(maxsize=None)
def host_mixed(check):
    return wc.host_decompress(wc.mixed()[0], check_subgroup=check)


def dev_bytes(ctx, data):
    return ctx.torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).to(ctx.tdev).reshape(-1, wc.ENC)


def words(t):
    return t.cpu().numpy().view(np.uint64).reshape(-1, 12)


@pytest.mark.parametrize("check", [False, True])
def test_mixed_batch_is_bit_equal_to_the_selftest_and_labelled_by_the_model(ctx, check):
    from honeybadgermpc_amd import g1

    data, where = wc.mixed()
    count = len(data) // wc.ENC
    pts, status, rejected = g1.decompress(ctx, dev_bytes(ctx, data), check_subgroup=check)
    assert tuple(pts.shape) == (count, 2, 6) and tuple(status.shape) == (count,) and status.dtype == ctx.torch.int32 and tuple(rejected.shape) == (1,)
    h_pts, h_status, h_rejected = host_mixed(check)
    got_status = status.cpu().numpy()
    assert np.array_equal(got_status, h_status) and np.array_equal(words(pts), h_pts)
    assert int(rejected.item()) == h_rejected == int((got_status != 0).sum())
    assert not words(pts)[got_status != 0].any()
    # the model: the vectors are accepted with their points, the malformed items take their labels
    want_status, want_pts = wc.malformed_labels(check)
    assert got_status[where].tolist() == want_status and np.array_equal(words(pts)[where], want_pts)
    valid = np.ones(count, dtype=bool)
    valid[where] = False
    assert not got_status[valid].any() and np.array_equal(words(pts)[valid], wc.vector_points())


def test_compress_gives_the_vectors_back(ctx):
    from honeybadgermpc_amd import g1

    v = wc.vector_bytes()
    pts, status, _ = g1.decompress(ctx, dev_bytes(ctx, v))
    enc = g1.compress(ctx, pts)
    assert tuple(enc.shape) == (1000, wc.ENC) and enc.dtype == ctx.torch.uint8
    assert enc.cpu().numpy().tobytes() == v
    up = ctx.torch.from_numpy(wc.vector_points().view(np.int64)).to(ctx.tdev).reshape(1000, 2, 6)
    assert g1.compress(ctx, up).cpu().numpy().tobytes() == v == wc.host_compress(wc.vector_points())


@pytest.mark.parametrize("count", [0, 1, 257])
def test_small_and_partial_batches(ctx, count):
    from honeybadgermpc_amd import g1

    data = wc.mixed()[0][20 * wc.ENC:(20 + count) * wc.ENC]                  # item 23 of the mix is malformed
    h_pts, h_status, h_rejected = host_mixed(True)
    pts, status, rejected = g1.decompress(ctx, dev_bytes(ctx, data), check_subgroup=True)
    assert tuple(pts.shape) == (count, 2, 6) and tuple(status.shape) == (count,)
    assert np.array_equal(words(pts), h_pts[20:20 + count]) and np.array_equal(status.cpu().numpy(), h_status[20:20 + count])
    assert int(rejected.item()) == int((h_status[20:20 + count] != 0).sum())
    enc = g1.compress(ctx, pts)
    assert tuple(enc.shape) == (count, wc.ENC)
    assert enc.cpu().numpy().tobytes() == wc.host_compress(h_pts[20:20 + count]) if count else enc.numel() == 0
    flags = g1.in_subgroup(ctx, pts, method="endomorphism")
    assert flags.dtype == ctx.torch.bool and flags.cpu().tolist() == [True] * count      # rejected rows are zeros: the identity


def test_inputs_host_bytes_misaligned_views_and_out(ctx):
    from honeybadgermpc_amd import g1

    torch = ctx.torch
    data = wc.mixed()[0][:64 * wc.ENC]
    h_pts, h_status, _ = host_mixed(False)
    for form in (data, bytearray(data), np.frombuffer(data, dtype=np.uint8), np.frombuffer(data, dtype=np.uint8).reshape(64, wc.ENC)):
        pts, status, _ = g1.decompress(ctx, form)
        assert np.array_equal(words(pts), h_pts[:64]) and np.array_equal(status.cpu().numpy(), h_status[:64])
    # a view starting one byte into a larger buffer: copied, never handed to the kernel as it stands
    big = torch.zeros(64 * wc.ENC + 32, dtype=torch.uint8, device=ctx.tdev)
    big[1:1 + 64 * wc.ENC] = dev_bytes(ctx, data).reshape(-1)
    view = big[1:1 + 64 * wc.ENC].reshape(64, wc.ENC)
    assert view.data_ptr() % 16 == 1 and view.is_contiguous()
    pts, status, _ = g1.decompress(ctx, view)
    assert np.array_equal(words(pts), h_pts[:64]) and np.array_equal(status.cpu().numpy(), h_status[:64])
    # a strided tensor
    wide = torch.zeros((64, 2 * wc.ENC), dtype=torch.uint8, device=ctx.tdev)
    wide[:, :wc.ENC] = dev_bytes(ctx, data)
    pts, _, _ = g1.decompress(ctx, wide[:, :wc.ENC])
    assert np.array_equal(words(pts), h_pts[:64])
    # out= is honoured
    out = torch.full((64, 2, 6), -1, dtype=torch.int64, device=ctx.tdev)
    pts, _, _ = g1.decompress(ctx, data, out=out)
    assert pts.data_ptr() == out.data_ptr() and np.array_equal(words(out), h_pts[:64])
    enc_out = torch.zeros((64, wc.ENC), dtype=torch.uint8, device=ctx.tdev)
    enc = g1.compress(ctx, out, out=enc_out)
    assert enc.data_ptr() == enc_out.data_ptr() and enc_out.cpu().numpy().tobytes() == wc.host_compress(h_pts[:64])
    # refusals
    with pytest.raises(TypeError):
        g1.decompress(ctx, dev_bytes(ctx, data).to(torch.int8))
    with pytest.raises(TypeError):
        g1.decompress(ctx, np.zeros(48, dtype=np.int32))
    with pytest.raises(TypeError):
        g1.decompress(ctx, [0] * 48)
    with pytest.raises(ValueError):
        g1.decompress(ctx, data[:-1])
    with pytest.raises(ValueError):
        g1.decompress(ctx, torch.zeros(47, dtype=torch.uint8, device=ctx.tdev))
    with pytest.raises(ValueError):
        g1.compress(ctx, out, out=torch.zeros((63, wc.ENC), dtype=torch.uint8, device=ctx.tdev))
    with pytest.raises(ValueError):
        g1.in_subgroup(ctx, out, method="pairing")


def test_both_membership_methods_equal_the_model(ctx):
    from honeybadgermpc_amd import g1

    rows, want = wc.subgroup_set()
    reps = -(-257 // len(rows))
    tiled = np.tile(rows, (reps, 1))[:257]                                   # a partial second workgroup
    pts = ctx.torch.from_numpy(tiled.view(np.int64)).to(ctx.tdev).reshape(257, 2, 6)
    endo = g1.in_subgroup(ctx, pts, method="endomorphism")
    order = g1.in_subgroup(ctx, pts, method="order")
    default = g1.in_subgroup(ctx, pts)
    expected = [bool(f) for f in (want * reps)[:257]]
    assert endo.cpu().tolist() == expected == order.cpu().tolist() == default.cpu().tolist()
    assert endo.cpu().tolist() == [bool(f) for f in (wc.host_subgroup(rows) * reps)[:257]]
    assert g1.in_subgroup(ctx, G1.generator(), method="endomorphism").cpu().tolist() == [True]


def test_verify_wire(ctx):
    """t = 2, n = 4, B = 3 under the trapdoor CRS of g1_crs_support and pairing_support"""
    from honeybadgermpc_amd import g1
    from honeybadgermpc_amd.poly_commit_const import PolyCommitConst

    t, n, B = 2, 4, 3
    torch = ctx.torch
    gs, hs = ps.cs.crs_points(t + 1)
    pc = PolyCommitConst([gs, ps.ghats(), hs], ctx=ctx)
    phis, _ = ps.cs.quotient_case(t, B=B)
    hats, _ = ps.cs.quotient_case(t, B=B, seed=1)
    coeffs = ctx.upload_ints([v for p in phis for v in p]).reshape(B, t + 1, 4)
    hat = ctx.upload_ints([v for p in hats for v in p]).reshape(B, t + 1, 4)
    c, _ = pc.commit_batch(coeffs, hat)
    w, shares, aux = pc.witness_batch(coeffs, hat, list(range(1, n + 1)))
    x, k = 2, 1                                                              # every item opens at xs[1] = 2
    sh, au, wi = shares[:, k].contiguous(), aux[:, k].contiguous(), w[:, k].contiguous()
    c48, w48 = g1.compress(ctx, c), g1.compress(ctx, wi)
    assert [G1.decompress(bytes(row)) for row in c48.cpu().numpy()] == g1.download(c)
    ok = pc.verify_wire(c48, x, sh, au, w48)
    assert ok.dtype == torch.bool and ok.cpu().tolist() == [True] * B
    assert pc.verify_wire(c48.cpu().numpy().tobytes(), x, sh, au, w48, check_subgroup=False).cpu().tolist() == [True] * B
    # a wrong share
    bad = sh.clone()
    bad[0] = ctx.upload_ints([(ctx.download_ints(sh[0:1])[0] + 1) % R])[0]
    assert pc.verify_wire(c48, x, bad, au, w48).cpu().tolist() == [False, True, True]
    # a witness with the compression flag cleared: a verdict, not an exception
    flagless = w48.clone()
    flagless[1, 0] &= 0x7F
    assert pc.verify_wire(c48, x, sh, au, flagless).cpu().tolist() == [True, False, True]
    # a witness moved out of the subgroup
    moved = g1.download(wi)
    moved[2] = moved[2] * wc.lifted()[0]
    assert not moved[2].in_subgroup()
    moved48 = dev_bytes(ctx, b"".join(p.compress() for p in moved))
    assert pc.verify_wire(c48, x, sh, au, moved48).cpu().tolist() == [True, True, False]
    _, status, rejected = g1.decompress(ctx, moved48, check_subgroup=True)
    assert status.cpu().tolist() == [0, 0, wc.NOT_IN_SUBGROUP] and int(rejected.item()) == 1
    # verify_batch with the check on the decompressed tensors: the same verdicts
    wm, status, _ = g1.decompress(ctx, moved48)
    assert status.cpu().tolist() == [0, 0, 0]
    assert pc.verify_batch(c, x, sh, au, wm, check_subgroup=True).cpu().tolist() == [True, True, False]
    assert pc.verify_batch(c, x, sh, au, wi, check_subgroup=True).cpu().tolist() == [True] * B
    assert pc.verify_batch(c, x, bad, au, wi, check_subgroup=True).cpu().tolist() == [False, True, True]
    # without ghats
    pc0 = PolyCommitConst([gs, None, hs], ctx=ctx)
    with pytest.raises(NotImplementedError, match="pairing"):
        pc0.verify_wire(c48, x, sh, au, w48)

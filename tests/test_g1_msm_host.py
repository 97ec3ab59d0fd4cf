"""CPU-only: hb_selftest_g1_msm drives the per-lane steps of the MSM kernels (csrc/hb_msm.hip: the digit of a term, the walk of a bucket's
list, b * B_b, a tree step, the fold, the row's Horner end -- the same HB_HD functions the kernels call) lane by lane over host arrays,
against the Python-int model of g1_msm_support; and g1.lagrange_scalars against the definition.  Exact equality of affine words.

Reference parity: the reference's interpolate_g1_at_x (betterpairing.py:800) needs its pairing extension, which cannot be imported
where this suite is built; the Python-int model (bases with known logarithms, and the host G1 product of powers for opaque bases)
stands in for it.  lagrange_definition is a transcription of its lagrange_at_x."""
import numpy as np
import pytest

import g1_msm_support as ms
from g1_msm_support import BUCKET, DIRECT, HEAVY

from honeybadgermpc_amd.bls12_381 import R


def run(scalars, pts, method, chunk=0, per_row=False):
    M, K = len(scalars), len(scalars[0]) if scalars else 0
    rc, out = ms.selftest(scalars, pts, M, K, method, chunk, per_row)
    assert rc == 0
    return out


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("K", [0, 1, 2, 255, 256, 257])
def test_direct_path(M, K):
    per_row = K in (2, 257)
    scalars, logs, pts = ms.random_case(M, K, seed=K + M, per_row=per_row)
    if K == 0:
        rc, out = ms.selftest([[]] * M, pts, M, 0, DIRECT)
        assert rc == 0 and not out.any()
        return
    assert np.array_equal(run(scalars, pts, DIRECT, per_row=per_row), ms.model_logs(scalars, logs, per_row))


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("K", [1, 63, 64, 65, 129])
def test_bucket_path_at_chunk_64(M, K):
    per_row = K in (63, 129)
    scalars, logs, pts = ms.random_case(M, K, seed=100 + K + M, per_row=per_row)
    want = ms.model_logs(scalars, logs, per_row)
    assert np.array_equal(run(scalars, pts, BUCKET, 64, per_row), want)
    if M == 1:
        assert np.array_equal(run(scalars, pts, HEAVY, 64, per_row), want)


def test_bucket_path_at_the_default_chunk_and_no_terms():
    scalars, logs, pts = ms.random_case(2, 70, seed=9)
    assert np.array_equal(run(scalars, pts, BUCKET), ms.model_logs(scalars, logs))
    rc, out = ms.selftest([[], []], pts, 2, 0, BUCKET)
    assert rc == 0 and not out.any()


@pytest.mark.parametrize("name", ["all-zero rows", "all-equal scalars", "every byte 255", "single top byte", "identity bases", "all bases the identity",
                                  "one base repeated", "P and -P"])
def test_special_inputs(name):
    scalars, logs, pts, want = ms.special_cases()[name]
    for method, chunk in ((BUCKET, 64), (HEAVY, 64), (BUCKET, 0), (DIRECT, 0)):
        if method == DIRECT and len(scalars[0]) > 70:        # a full scalar multiplication a term on the host: the long case's prefix
            scalars, pts = [row[:70] for row in scalars[:1]], pts[:70]
            want = ms.model_logs(scalars, logs[:70])
        assert np.array_equal(run(scalars, pts, method, chunk), want), (name, method, chunk)
    if name in ("all-zero rows", "all bases the identity", "P and -P"):
        assert not want.any()


def test_generic_bases_against_the_host_product():
    scalars, pts, want = ms.generic_case()
    for method, chunk in ((DIRECT, 0), (BUCKET, 0), (BUCKET, 64), (HEAVY, 64)):
        assert np.array_equal(run(scalars, pts, method, chunk), want), (method, chunk)


def test_all_paths_agree_on_one_random_input():
    scalars, logs, pts = ms.random_case(2, 150, seed=31, per_row=True)
    outs = [run(scalars, pts, method, chunk, True) for method, chunk in ((DIRECT, 0), (BUCKET, 0), (BUCKET, 64), (BUCKET, 128), (HEAVY, 64), (0, 0))]
    assert all(np.array_equal(o, outs[0]) for o in outs) and np.array_equal(outs[0], ms.model_logs(scalars, logs, True))


def test_bad_arguments_and_workspace_size():
    from honeybadgermpc_amd._capi import load_library

    lib = load_library()
    scalars, _, pts = ms.random_case(1, 4, seed=1)
    for method, chunk in ((4, 0), (-1, 0), (BUCKET, 32), (BUCKET, 100), (BUCKET, 8192)):
        rc, _ = ms.selftest(scalars, pts, 1, 4, method, chunk)
        assert rc != 0, (method, chunk)
    ws = lib.hb_g1_msm_workspace_bytes
    assert ws(1, 4, 3, 0) == 0 and ws(-1, 4, 1, 0) == 0 and ws(1, -4, 1, 0) == 0 and ws(1, 4, 2, 96) == 0 and ws(1, 4, 2, 4160) == 0
    part = 48 * 4                                            # a Jacobian partial: 3 x 16 words
    assert ws(3, 257, 1, 0) == part * 3 * (2 + 1)            # direct: ceil(257 / 256) partials and one sum a row
    assert ws(3, 129, 2, 64) == part * 3 * 32 * (3 + 1)      # bucket: 32 windows of ceil(129 / 64) partials and one sum
    assert ws(1, 4097, 2, 0) == part * 32 * (2 + 1) and ws(1, 4096, 2, 0) == part * 32 * (1 + 1)
    assert ws(0, 5, 0, 0) > 0 and ws(2, 0, 0, 0) > 0


def test_auto_takes_the_bucket_path_from_the_module_constant_on():
    """method 0 of the C ABI and g1.msm's "auto" switch at the same K: the workspace of the path taken tells which one it is"""
    from honeybadgermpc_amd import g1
    from honeybadgermpc_amd._capi import load_library

    ws, K = load_library().hb_g1_msm_workspace_bytes, g1.MSM_CROSSOVER
    assert ws(1, K - 1, 0, 0) == ws(1, K - 1, DIRECT, 0) != ws(1, K - 1, BUCKET, 0)
    assert ws(1, K, 0, 0) == ws(1, K, BUCKET, 0) != ws(1, K, DIRECT, 0)


# ---------------------------------------------------------------- lagrange_scalars
def test_lagrange_shortcut_general_and_definition_agree():
    from honeybadgermpc_amd.g1 import lagrange_scalars

    for xs, targets in (([0, 1, 2, 3, 4], [0, 4, 5, 77, R - 1, -3]), (list(range(22)), list(range(4)) + [22, 1000]), ([7], [7, 9]), ([5, 6], [0, 5, 6, 7]),
                        (list(range(-3, 4)), [-3, 0, 10])):
        fast, slow = lagrange_scalars(xs, targets), lagrange_scalars(xs, targets, shortcut=False)
        assert fast == slow == ms.lagrange_definition(xs, targets), xs
        assert all(0 <= v < R for row in fast for v in row)


def test_lagrange_general_nodes_and_unit_rows():
    from honeybadgermpc_amd.g1 import lagrange_scalars

    xs = [3, 1, 4, 15, 9, 2, 6, R - 5]
    targets = [0, 5, 15, R - 5, 3, 123456789]
    got = lagrange_scalars(xs, targets)
    assert got == ms.lagrange_definition(xs, targets)
    for t, k in ((15, 3), (R - 5, 7), (3, 0)):
        assert got[targets.index(t)] == [1 if j == k else 0 for j in range(len(xs))]
    # the weights interpolate: a random cubic through 4 nodes, evaluated elsewhere
    f = lambda x: (5 + 7 * x + 11 * x * x + 13 * x ** 3) % R
    nodes = [2, 9, 4, 30]
    row = lagrange_scalars(nodes, [100])[0]
    assert sum(w * f(x) for w, x in zip(row, nodes)) % R == f(100)
    assert lagrange_scalars([], [1, 2]) == [[], []] and lagrange_scalars([1, 2], []) == []


def test_lagrange_duplicate_nodes():
    from honeybadgermpc_amd.g1 import lagrange_scalars

    with pytest.raises(ValueError, match="distinct"):
        lagrange_scalars([1, 2, 1], [0])
    with pytest.raises(ValueError, match="distinct"):
        lagrange_scalars([1, 2, R + 1], [0])

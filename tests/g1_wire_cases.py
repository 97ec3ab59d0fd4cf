"""Shared by tests/test_g1_wire_host.py and tests/test_gpu_g1_wire.py: marshalling for hb_selftest_g1_wire (the bodies of
csrc/hb_g1_wire.hip run on the host) and the case tables, every one labelled by the host model honeybadgermpc_amd.bls12_381.G1: the
expected status of an encoding is the branch of G1.decompress that raises, the expected flag of a point is G1.in_subgroup()."""
import ctypes
import functools
import os
import random

import numpy as np

import g1_support as s
from conftest import GOLDEN

from honeybadgermpc_amd.bls12_381 import G1, GX, GY, Q, R

SUBGROUP, DECOMPRESS, COMPRESS, SQRT, PHI = range(5)
OK, NOT_COMPRESSED, BAD_IDENTITY, X_NOT_BELOW_Q, NOT_ON_CURVE, NOT_IN_SUBGROUP = range(6)
X = 0xD201000000010000
BETA = 0x5F19672FDF76CE51BA69C6076A0F77EADDB3A93BE6F89688DE17D813620A00022E01FFFFFFFEFFFE
ENC = 48
# the message of each branch of G1.decompress that raises, in the order it makes its checks
_BRANCHES = [("compression flag", NOT_COMPRESSED), ("identity carries", BAD_IDENTITY), ("not below Q", X_NOT_BELOW_Q), ("not the abscissa", NOT_ON_CURVE),
             ("not in the subgroup", NOT_IN_SUBGROUP)]


def aligned(nbytes):
    """a zeroed uint8 array of nbytes whose first byte is aligned to 16"""
    raw = np.zeros(nbytes + 16, dtype=np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off:off + nbytes]


def selftest(what, data, flags, count, out_bytes):
    """data: bytes or an array -> (rc, uint8 array of out_bytes bytes, 0x5A where nothing was written)"""
    from honeybadgermpc_amd._capi import load_library

    lib = load_library()
    raw = np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    src = aligned(max(raw.size, 16))
    src[:raw.size] = raw
    out = aligned(max(out_bytes, 16))
    out[:] = 0x5A
    ptrs = (ctypes.c_void_p * 1)(src.ctypes.data)
    rc = lib.hb_selftest_g1_wire(what, ptrs, flags, 0, ctypes.c_void_p(out.ctypes.data), count)
    return rc, out[:out_bytes]


def host_decompress(data, check_subgroup=False):
    """-> (points (count, 12) uint64, status (count,) int32, rejected) from the self test"""
    count = len(data) // ENC
    rc, out = selftest(DECOMPRESS, data, 1 if check_subgroup else 0, count, count * 96 + 4 * count + 4)
    assert rc == 0
    st = out[count * 96:].view(np.int32)
    return out[:count * 96].view(np.uint64).reshape(count, 12).copy(), st[:count].copy(), int(st[count])


def host_compress(points):
    count = len(points)
    rc, out = selftest(COMPRESS, points, 0, count, count * ENC)
    assert rc == 0
    return out.tobytes()


def host_subgroup(points):
    count = len(points)
    rc, out = selftest(SUBGROUP, points, 0, count, 4 * count)
    assert rc == 0
    return out.view(np.int32).tolist()


def host_sqrt(values):
    """-> (roots, flags)"""
    count = len(values)
    rc, out = selftest(SQRT, s.words(values, 6), 0, count, count * 48 + 4 * count)
    assert rc == 0
    return s.unwords(out[:count * 48].view(np.uint64), 6), out[count * 48:].view(np.int32).tolist()


def host_phi(points):
    count = len(points)
    rc, out = selftest(PHI, points, 0, count, count * 96)
    assert rc == 0
    return out.view(np.uint64).reshape(count, 12).copy()


# ---- encodings
@functools.lru_cache(maxsize=None)
def vector_bytes():
    """the crate's 1000 valid vectors, 48 000 bytes; vector 0 is the identity"""
    with open(os.path.join(GOLDEN, "g1_compressed_valid_test_vectors.dat"), "rb") as f:
        data = f.read()
    assert len(data) == 1000 * ENC and data[0] == 0xC0
    return data


@functools.lru_cache(maxsize=None)
def vector_points():
    """(1000, 12) uint64: G1.decompress(v).to_limbs() of every vector"""
    return s.points(s.vectors())


def encode_x(x, flags):
    """x below 2^381 and the three flag bits (4 compressed, 2 identity, 1 sign) -> 48 bytes"""
    assert 0 <= x < 1 << 381 and 0 <= flags < 8
    raw = bytearray(x.to_bytes(ENC, "big"))
    raw[0] |= flags << 5
    return bytes(raw)


def model_label(enc, check_subgroup=False):
    """-> (status, 12 words): the branch of G1.decompress that raises, and the point it returns (zeros for a rejected item)"""
    try:
        return OK, G1.decompress(enc, check_subgroup=check_subgroup).to_limbs()
    except ValueError as err:
        hits = [code for text, code in _BRANCHES if text in str(err)]
        assert len(hits) == 1, str(err)
        return hits[0], [0] * 12


@functools.lru_cache(maxsize=None)
def malformed():
    """-> list of (name, 48 bytes): one item each of what an encoding can get wrong, and the edges of what it may hold"""
    v = vector_bytes()[5 * ENC:6 * ENC]
    cases = [
        ("compression flag clear on a valid vector", bytes([v[0] & 0x7F]) + v[1:]),
        ("0x40 alone", encode_x(0, 2)),
        ("0xC0 with a non-zero last byte", encode_x(1, 6)),
        ("0xE0 followed by zeros", encode_x(0, 7)),
        ("x = Q", encode_x(Q, 4)),
        ("x = Q + 1", encode_x(Q + 1, 5)),
        ("the 381 low bits all set", encode_x((1 << 381) - 1, 4)),
        ("x = Q - 1", encode_x(Q - 1, 4)),
        ("x = Q - 1, sign", encode_x(Q - 1, 5)),
        ("x = 0", encode_x(0, 4)),
        ("x = 0, sign", encode_x(0, 5)),
    ]
    cases += [(f"x = {x}, sign {x & 1}", encode_x(x, 4 | (x & 1))) for x in range(1, 24)]
    rnd = random.Random(381)
    cases += [(f"random x {k}", encode_x(rnd.randrange(Q), 4 | (k & 1))) for k in range(8)]
    return cases


@functools.lru_cache(maxsize=None)
def malformed_labels(check_subgroup):
    """-> (statuses, (count, 12) uint64 points) by the model"""
    labels = [model_label(enc, check_subgroup) for _, enc in malformed()]
    return [st for st, _ in labels], np.array([w for _, w in labels], dtype=np.uint64).reshape(len(labels), 12)


MIX_STRIDE = 23


@functools.lru_cache(maxsize=None)
def mixed():
    """the 1000 vectors with the malformed items mixed in, one after every MIX_STRIDE vectors -> (bytes, positions of the malformed items)"""
    v, bad = vector_bytes(), [enc for _, enc in malformed()]
    out, where = [], []
    for k in range(1000):
        out.append(v[k * ENC:(k + 1) * ENC])
        if k % MIX_STRIDE == MIX_STRIDE - 1 and len(where) < len(bad):
            where.append(len(out))
            out.append(bad[len(where) - 1])
    assert len(where) == len(bad)
    return b"".join(out), where


# ---- points for the membership test
@functools.lru_cache(maxsize=None)
def lifted(n=40):
    """the first n curve points lift_x finds from x = 5 upward (none of them in the subgroup)"""
    out, x = [], 5
    while len(out) < n:
        p = G1.lift_x(x)
        if p is not None:
            out.append(p)
        x += 1
    return out


@functools.lru_cache(maxsize=None)
def subgroup_set():
    """-> ((count, 12) uint64 rows, expected flags): members, non-members, and rows that are no points"""
    g = G1.generator()
    rnd = random.Random(2021)
    pts = [G1.one()] + [g ** k for k in (1, 2, 3, 0xFFFF, R - 1, R - 2, rnd.randrange(R), rnd.randrange(R))]
    pts += lifted() + [p * g for p in lifted()] + [G1(0, 2), G1(0, Q - 2)]
    want = [1 if p.in_subgroup() else 0 for p in pts]
    raw = [s.off_curve_raw(), s.raw_point(GX + Q, GY), s.raw_point(GX, GY + Q), s.raw_point(0, 1)]
    rows = np.concatenate([s.points(pts), np.array(raw, dtype=np.uint64).reshape(len(raw), 12)])
    return rows, want + [0] * len(raw)

"""The packed last row tile of the fused decode + validate kernel (k_mm8f, hb_mfma_fused.hip), without a device: the generator's packed
phase, the placement of the digits (the library's own slot map under an integer model of the MFMA pass), and the host's decision.

A packed pass puts digit group 0 of an output on M row m < 8 and digit group 1 on M row m + 8 of ONE A operand, so a window s of input
bytes is one MFMA: accumulator c' = s + 7 of M row m is column c' of the output, of M row m + 8 column c' + 8.  The model below computes
those accumulators from the bytes the image holds and checks that lo + hi 2^64 is the product the unpacked pass computes."""
import ctypes
import importlib.util
import os
import random

import numpy as np
import pytest

from conftest import REPO

BIAS = 5800000
BIAS_PACK = BIAS // 2
NC, NCP = 47, 39


def _gen():
    spec = importlib.util.spec_from_file_location("gen_mm8", os.path.join(REPO, "honeybadgermpc_amd", "csrc", "gen_mm8.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _lib():
    from honeybadgermpc_amd._capi import load_library

    return load_library()


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _decide_points(xz, n_coef, nc):
    lib = _lib()
    out = np.zeros(10, dtype=np.int32)
    small = np.zeros(32, dtype=np.uint8)
    xa = np.array(xz, dtype=np.int32)
    ok = lib.hb_debug_fs_pack_points(_ptr(xa), len(xz), n_coef, nc, _ptr(out), _ptr(small))
    return ok, int(out[0]), int(out[1]), out[2 : 2 + int(out[1])].tolist(), small[:n_coef].tolist()


def _decide_rows(d, n_coef, nc, small):
    lib = _lib()
    out = np.zeros(10, dtype=np.int32)
    sm = np.array(small, dtype=np.uint8)
    ok = lib.hb_debug_fs_pack_rows(d, n_coef, nc, _ptr(sm), _ptr(out))
    return ok, int(out[0]), int(out[1]), out[2 : 2 + int(out[1])].tolist()


def _slot(nm, ns, single, i, n_out):
    lib = _lib()
    kind = ctypes.c_int32(0)
    sa = np.array(list(single) + [0] * (8 - len(single)), dtype=np.int32)
    sl = lib.hb_debug_fs_slot(nm, ns, _ptr(sa), i, n_out, ctypes.byref(kind))
    return sl, kind.value


def test_generator_packed_phase_issues_one_mfma_a_window():
    g = _gen()
    for nkb in (1, 2, 3, 4):
        packed = [g.asm_half(h, nkb, packed=True) for h in (0, 1)]
        plain = [g.asm_half(h, nkb) for h in (0, 1)]
        n_packed = sum(sum("v_mfma_i32_16x16x64_i8" in ln for ln in lines) for lines, _ in packed)
        n_plain = sum(sum("v_mfma_i32_16x16x64_i8" in ln for ln in lines) for lines, _ in plain)
        assert n_packed == 39 * nkb and n_plain == 78 * nkb
        assert [nc for _, nc in packed] == [19, 20] and [nc for _, nc in plain] == [23, 24]
        # one A piece a K-block (and the four element pieces), against two
        assert sum("ds_read_b128" in ln for ln in packed[0][0]) == 5 * nkb and sum("ds_read_b128" in ln for ln in plain[0][0]) == 6 * nkb
    assert g.packed_columns(0) + g.packed_columns(1) == [c for c in range(NCP) if c % 4 in (0, 3)] + [c for c in range(NCP) if c % 4 in (1, 2)]
    text = g.emit()
    for nkb in (1, 2, 3):
        for half in (0, 1):
            assert f"struct Mm8PhasePacked<{nkb}, {half}>" in text and f"struct Mm8Phase<{nkb}, {half}, false>" in text


# ---- the integer model ---------------------------------------------------------------------------------------------------------
def _matrix(x, z, zc, n_coef):
    """[N ; P] over the integers: N[m][j] = coeff_m(A_j), P[i][j] = A_j(x_zci), A_j = prod_{q != j} (X - x_zq)"""
    d = len(z)
    rows = [[0] * d for _ in range(n_coef + len(zc))]
    for j in range(d):
        a = [1]
        for q in range(d):
            if q != j:
                a = [(a[k - 1] if k > 0 else 0) - x[z[q]] * (a[k] if k < len(a) else 0) for k in range(len(a) + 1)]
        for m in range(n_coef):
            rows[m][j] = a[m]
        for i, s in enumerate(zc):
            v = 1
            for q in range(d):
                if q != j:
                    v *= x[s] - x[z[q]]
            rows[n_coef + i][j] = v
    return rows


def _digits(v):
    """16 balanced base-256 digits (fs_build_body's loop)"""
    out, carry = [], 0
    u = v & ((1 << 128) - 1)
    for b in range(16):
        t = ((u >> (8 * b)) & 0xFF) + carry
        if t > 127:
            t -= 256
            carry = 1
        else:
            carry = 0
        out.append(t)
    assert sum(dg << (8 * b) for b, dg in enumerate(out)) == v
    return out


def _window_sum(dig8, xb, cprime):
    """one accumulator of an M row that holds the eight digits dig8 per term: sum_l sum_b dig8[l][b] * sx_l[c' - b], sx the signed bytes
    (x ^ 0x80) of the 32 input bytes and zero outside them"""
    acc = 0
    for l, dg in enumerate(dig8):
        for b in range(8):
            k = cprime - b
            if 0 <= k < 32:
                acc += dg[b] * (xb[l][k] - 128)
    return acc


@pytest.mark.parametrize("n,t", [(64, 21), (16, 5)])
def test_packed_placement_gives_the_unpacked_sums(n, t):
    rnd = random.Random(1000 * n + t)
    d = t + 1
    x = list(range(1, n + 1))
    packed_any = 0
    for trial in range(3):
        order = list(range(n))
        rnd.shuffle(order)
        z, zc = order[:d], order[d : d + t]
        xin = [rnd.randrange(1 << 256) for _ in range(d)]
        if trial == 0:
            xin = [(1 << 256) - 1] * d
        xb = [[(v >> (8 * k)) & 0xFF for k in range(32)] for v in xin]
        for n_coef in (1, d):
            ok, nm, ns, single, small = _decide_points([x[i] for i in z], n_coef, len(zc))
            rows = _matrix(x, z, zc, n_coef)
            n_out = len(rows)
            assert small == [int(all(abs(v) < (1 << 62) for v in rows[m])) for m in range(n_coef)]
            if not ok:
                continue
            packed_any += 1
            base = 16 * ((n_out + 15) // 16 - 1)
            # the image: slot -> eight-digit pieces per term, as fs_build_body places them (digit group 1 of a merged row on M row + 8)
            image, seen = {}, set()
            for i, row in enumerate(rows):
                sl, kind = _slot(nm, ns, single, i, n_out)
                assert sl not in seen and 0 <= sl < base + 16
                seen.add(sl)
                dg = [_digits(v) for v in row]
                if kind == 0:
                    assert sl < base
                    image[sl] = ("plain", dg)
                elif kind == 1:
                    assert base <= sl < base + nm and sl + 8 not in seen
                    seen.add(sl + 8)
                    image[sl] = ("lo", [r[:8] for r in dg])
                    image[sl + 8] = ("hi", [r[8:] for r in dg])
                else:
                    assert i in single and sl - base in (4, 5, 6, 7, 12, 13, 14, 15)
                    assert all(b == 0 for r in dg for b in r[8:])
                    image[sl] = ("single", [r[:8] for r in dg])
            assert sum(1 for sl in image if sl >= base) <= 16
            for i, row in enumerate(rows):
                sl, kind = _slot(nm, ns, single, i, n_out)
                want = sum(v * (xv - int("80" * 32, 16)) for v, xv in zip(row, xin))       # what any pass computes before its constants
                if kind == 0:
                    dg = image[sl][1]
                    total = sum((BIAS + _window_sum([r[:8] for r in dg], xb, c) + _window_sum([r[8:] for r in dg], xb, c - 8)) << (8 * c) for c in range(NC))
                    assert total - sum(BIAS << (8 * c) for c in range(NC)) == want
                    continue
                lo = [BIAS_PACK + _window_sum(image[sl][1], xb, c) for c in range(NCP)]
                assert all(0 <= v < 2 * BIAS_PACK for v in lo)
                if kind == 1:
                    hi = [BIAS_PACK + _window_sum(image[sl + 8][1], xb, c) for c in range(NCP)]
                    assert all(0 <= v < 2 * BIAS_PACK for v in hi)
                    # the 47 columns the reduction sees: each below 2 BIAS, as a column of an unpacked pass
                    cols = [(lo[c] if c < NCP else 0) + (hi[c - 8] if c >= 8 else 0) for c in range(NC)]
                    assert all(0 <= v < 2 * BIAS and v * 257 < (1 << 32) for v in cols)
                    total = sum(v << (8 * c) for c, v in enumerate(cols))
                    assert total == sum(v << (8 * c) for c, v in enumerate(lo)) + (sum(v << (8 * c) for c, v in enumerate(hi)) << 64)
                    bias = sum(BIAS_PACK << (8 * c) for c in range(NCP)) * (1 + (1 << 64))
                else:
                    total = sum(v << (8 * c) for c, v in enumerate(lo))
                    bias = sum(BIAS_PACK << (8 * c) for c in range(NCP))
                assert total - bias == want
                # no larger than the integer an unpacked pass hands its reduction (tests/fold_model.py's bounds hold unchanged)
                assert 0 <= total < sum((2 * BIAS) << (8 * c) for c in range(NC))
    assert packed_any >= 3


def test_predicate_packs_cfg3_for_200_arrival_sets():
    n, t = 64, 21
    d = t + 1
    x = list(range(1, n + 1))
    for seed in range(200):
        rnd = random.Random(seed)
        z = rnd.sample(range(n), d)
        xz = [x[i] for i in z]
        ok1, nm1, ns1, single1, _ = _decide_points(xz, 1, t)
        assert (ok1, nm1, ns1, single1) == (1, 6, 0, [])                      # R1: 22 rows, the six of the second tile merge
        ok2, nm2, ns2, single2, small = _decide_points(xz, d, t)
        assert (ok2, nm2, ns2, single2) == (1, 3, 8, list(range(14, 22)))      # R2: 43 rows = 32 + 3 merged + 8 single-group
        assert all(small[14:])
    # the largest points: the largest entries
    ok2, nm2, ns2, single2, small = _decide_points(x[-d:], d, t)
    assert (ok2, nm2, ns2, single2) == (1, 3, 8, list(range(14, 22))) and not any(small[:13])


def test_predicate_declines_what_does_not_fit():
    # nine rows that all need both digit groups are eighteen M rows; eight fit exactly
    assert _decide_rows(9, 9, 0, [0] * 9) == (0, 0, 0, [])
    assert _decide_rows(9, 8, 0, [0] * 8) == (1, 8, 0, [])
    # cfg3's R2 shape with too few single-group rows to trade places with: 11 rows in the last tile, at most 4 of them merged
    d = 22
    for n_small in range(0, 9):
        small = [0] * (d - n_small) + [1] * n_small
        got = _decide_rows(d, d, 21, small)
        if n_small >= 7:
            assert got == (1, 11 - n_small, n_small, list(range(d - n_small, d)))
        else:
            assert got == (0, 0, 0, [])
    # nine coefficient rows of the last tile's eleven need both groups: 2 compared + 9 = 11 merged rows
    assert _decide_rows(d, d, 21, [0] * d) == (0, 0, 0, [])
    # a full last tile has nothing to gain; more terms than the halved bias covers do not pack
    assert _decide_rows(16, 16, 16, [1] * 16)[0] == 0
    assert _decide_rows(23, 1, 5, [0])[0] == 0 and _decide_rows(22, 1, 5, [0]) == (1, 6, 0, [])


def test_hook_is_declared():
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    core = open(os.path.join(REPO, "honeybadgermpc_amd", "csrc", "hb_core.hip")).read()
    assert "HB_NO_FUSED_PACK" in design and '"HB_NO_FUSED_PACK"' in core

"""CPU-only: the case builder of the full-size mat-vec tests (tests/wide_cases.py) does what it says, and the case table of
tests/test_gpu_wide_matvec.py -- read from that module -- drives the reduction of k_mm8w where it can go wrong: by the big-integer
model of that reduction (tests/fold_model.py), the one-word Barrett quotient comes out one short ("under") and, over the two moduli next
to 2^256, the remainder reaches 2^256 before the last correction ("top1") in at least FLOOR outputs of every shape.  Without that floor
the GPU test could pass with the branch the round-3 defect lived in never taken.

The floor comes from the builder's design, not from a run of the kernel: a solved block aims at every pool value once per chosen row
(55 values, at least 4 rows), and the small pool values (2^32, 2^64 +- 1, 2^(29 j), ..) take both branches; a case has two solved
blocks and a part of a third.  Measured here: 371 and 162 or more of the first 500 solved outputs."""
import pytest

import edge_values as ev
import fold_model as fm
import test_gpu_wide_matvec as gw
import wide_cases as wc
from test_gpu_edge_values import P256, SECP_N, WIDE, WIDE_IDS

FLOOR = 50
EXAMINED = 1200          # solved outputs of a case put through the model: the count is a lower bound of the case's

CASES = [(p, shape, False) for p in WIDE for shape in gw.UNIT_SHAPES] + [(p, shape, True) for p in gw.FLAT_MODULI for shape in gw.FLAT_SHAPES]
IDS = ["%s-%dx%d%s" % (dict(zip(WIDE, WIDE_IDS))[p], s[0], s[1], "-balanced" if flat else "") for p, s, flat in CASES]


def _case(p, shape, flat):
    return gw.flat_case(p, shape) if flat else gw.unit_case(p, shape)


def test_the_tables_are_the_issue_s():
    assert gw.WIDE is WIDE and gw.UNIT_CHUNKS == 290 and gw.UNIT_CHUNKS % 16 == 2
    assert list(gw.UNIT_SHAPES) == [(8, 4), (12, 9), (16, 32), (22, 22), (33, 40), (40, 24), (64, 64), (112, 57)]
    assert list(gw.FLAT_SHAPES) == [(96, 64), (80, 57)] and gw.FLAT_CHUNKS == 4099 and gw.FLAT_MODULI == [WIDE[0], P256, SECP_N]
    assert gw.LAYOUT_SHAPES == [(22, 22), (40, 24)]


@pytest.mark.parametrize("p", WIDE, ids=WIDE_IDS)
def test_fixed_rows_and_fitting_entries(p):
    for v in (wc.largest_fitting(p), wc.heaviest_fitting(p)):
        assert v < p and ev.fits_32_balanced_digits(v)
    if p > wc.ALL_7F:
        assert wc.largest_fitting(p) == wc.ALL_7F and not ev.fits_32_balanced_digits(wc.ALL_7F + 1)
        assert wc.heaviest_fitting(p) == int("7e" + "7f" * 30 + "80", 16) and wc.digit_sum(wc.heaviest_fitting(p)) == 4095
    else:
        assert wc.largest_fitting(p) == p - 1
    # no fitting residue below p is heavier: a heavier one needs a larger top digit, and the lightest value of that is p or more
    top = wc.heaviest_fitting(p) >> 248
    assert wc.digit_sum(wc.heaviest_fitting(p)) == top + 1 + 31 * 128
    m = wc.fitting_matrix(p, 22, 22, seed=5)
    assert m[0] == [0] * 22 and m[1] == [1] * 22 and m[2] == [wc.largest_fitting(p)] * 22 and m[3] == [wc.heaviest_fitting(p)] * 22
    assert all(0 <= v < p and ev.fits_32_balanced_digits(v) for row in m for v in row)
    assert wc.image_bias(m) == 128 * 22 * wc.digit_sum(wc.heaviest_fitting(p)) + 1
    kinds = set(ev.operands(p, 4))
    rest = [v for row in m[4:] for v in row]
    assert 0.3 < sum(v in kinds for v in rest) / len(rest) < 0.7
    assert wc.fitting_matrix(p, 22, 22, seed=5) == m


@pytest.mark.parametrize("p, shape, flat", CASES, ids=IDS)
def test_case_reaches_the_short_quotient_and_the_top_bit(p, shape, flat):
    cs = _case(p, shape, flat)
    n_out, d = shape
    pool = set(ev.edge_pool(p, 4))
    assert (len(cs.m), len(cs.m[0])) == shape and all(0 <= v < p and ev.fits_32_balanced_digits(v) for row in cs.m for v in row)
    assert cs.bias == wc.image_bias(cs.m) < 1 << 30
    k = min(d, n_out - 3)
    assert len(cs.rows) == k and cs.rows[-1] == n_out - 1 and 0 not in cs.rows
    # the chosen rows touch every row tile, whatever its height (16, 12 or 8)
    for tile_rows in (16, 12, 8):
        if k >= -(-n_out // tile_rows):
            assert {r // tile_rows for r in cs.rows} == set(range(-(-n_out // tile_rows))), tile_rows
    # every chunk is edge-valued: pool values, their Montgomery pre-images, or solved
    known = pool | set(ev.montgomery_preimages(p, 4))
    solved = sorted(cs.targeted)
    assert len(solved) >= 2 * len(pool) and all(0 <= v < p for c in range(cs.period) for v in cs.x(c))
    assert all(v in known for c in range(cs.period) if c not in cs.targeted for v in cs.x(c))
    assert cs.x(cs.count - 1) is cs.x((cs.count - 1) % cs.period)
    # the solved chunks hit their targets at every targeted position, and every pool value is aimed at every chosen row
    aimed = {}
    for c in solved:
        for r, v in cs.targets_of(c):
            assert sum(a * b for a, b in zip(cs.m[r], cs.x(c))) % p == v, (c, r)
            aimed.setdefault(r, set()).add(v)
    assert sorted(aimed) == cs.rows and all(vals == pool for vals in aimed.values())
    # the model of the reduction over the kernel's integer: the plain product, every bound of the model kept, and the branches counted
    tb = fm.tables(p)
    under = top1 = examined = 0
    for c in solved:
        for r, v in cs.targets_of(c):
            if examined == EXAMINED:
                break
            facts = set()
            s, cr = wc.biased_sum(p, cs.m, cs.x(c), r, cs.bias)
            assert fm.reduce_model(s, cr, p, tb, facts) == v, (c, r)
            examined += 1
            under += "under" in facts
            top1 += "top1" in facts
    assert under >= FLOOR, (under, examined)
    if p in (P256, SECP_N):
        assert top1 >= FLOOR, (top1, examined)
    else:
        assert top1 == 0 or p >> 255
    # ... and over plain chunks and the fixed rows, the first and the last chunk whole
    for c in (0, len(pool), cs.period - 1):
        for r in range(n_out):
            s, cr = wc.biased_sum(p, cs.m, cs.x(c), r, cs.bias)
            assert fm.reduce_model(s, cr, p, tb) == sum(a * b for a, b in zip(cs.m[r], cs.x(c))) % p
    assert wc.biased_sum(p, cs.m, cs.x(0), n_out - 1) == wc.biased_sum(p, cs.m, cs.x(0), n_out - 1, cs.bias)


def test_outputs_are_the_plain_products():
    cs = gw.unit_case(SECP_N, (12, 9))
    p = cs.p
    for c in (0, 54, 55, 289):
        assert cs.outputs(c) == [sum(a * b for a, b in zip(row, cs.x(c))) % p for row in cs.m]
        assert cs.outputs(c)[0] == 0 and cs.outputs(c)[1] == sum(cs.x(c)) % p
    fl = gw.flat_case(SECP_N, (80, 57))
    assert fl.period == gw.FLAT_PERIOD and fl.outputs(4098) is fl.outputs(4098 % 220) and len(fl.base_outputs) == 220

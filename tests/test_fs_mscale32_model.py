"""The lane maps of k_mm8f's matrix-core division as two 32x32x32 products a task (tests/fs_mscale32_model.py): for every lane of a wave,
the words it holds behind the half swap are the words of chunk = lane by the definition, and the element written from them is the one
tests/fs_mscale_model.py's scale_model gives -- with 64 distinct elements a unit and with edge elements, at three moduli.  CPU only."""
import random

import numpy as np
import pytest

import fs_mscale32_model as m32
import fs_mscale_model as mm

BLS_R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
PRIMES = [BLS_R, (1 << 256) - 189, (1 << 254) + 0x4f]      # (the last is not prime: the arithmetic does not care, and every den here is a unit)
IDS = ["bls-r", "2^256-189", "2^254+79"]
N, D = 64, 22
ARRIVALS = [i + 1 for i in np.random.Generator(np.random.PCG64(2024)).permutation(N).tolist()[:D]]      # the benchmark's seeded order


def _tabs(p):
    return [mm.term_tables(p, mm.inv_den(p, ARRIVALS, j)) for j in (0, 9, 21)]


def _edge_unit(p):
    """64 elements: 0, p - 1, 2^256 - 1, every byte 00 / 7f / 80 / ff, the same bytes in halves and alternating, filled up with random ones"""
    ys = [0, p - 1, (1 << 256) - 1, 1, p, p + 1]
    for a in (0x00, 0x7f, 0x80, 0xff):
        ys.append(int.from_bytes(bytes([a] * 32), "little"))
        for b in (0x00, 0x7f, 0x80, 0xff):
            if a != b:
                ys.append(int.from_bytes(bytes([a] * 16 + [b] * 16), "little"))
                ys.append(int.from_bytes(bytes([a, b] * 16), "little"))
    rng = random.Random(p % 997)
    ys = ys[:64]
    while len(ys) < 64:
        ys.append(rng.randrange(1 << 256))
    # (the edge elements on both sides of the seam between chunks 31 and 32, and in both halves of a register)
    return ys[::2] + ys[1::2]


def _check_unit(p, tab, ys):
    words = m32.task_words(ys, tab)
    for lane in range(64):
        assert words[lane] == m32.direct_words(ys[lane], tab), lane
        assert m32.tail(words[lane], p) == mm.scale_model(ys[lane], p, tab), lane


def test_tables_hold_every_digit_and_constant_once():
    p = BLS_R
    digits, cinit = _tabs(p)[0]
    dt, ct = m32.digit_table(digits), m32.const_table(cinit)
    assert len(dt) == 64 and all(len(piece) == 16 for piece in dt)            # 1 KB a term, no block of zeros
    seen = {}
    for piece in range(64):
        h, m = piece >> 5, piece & 31
        for j in range(16):
            seen[(16 * h + j, m)] = dt[piece][j]
    assert seen == {(b, c): digits[b][c] for b in range(32) for c in range(32)}
    assert sorted(m32.reg_row(i, h) for h in range(2) for i in range(16)) == list(range(32))
    assert [ct[h][i] for h in range(2) for i in range(16)] == [cinit[m32.reg_row(i, h)] for h in range(2) for i in range(16)]


@pytest.mark.parametrize("p", PRIMES, ids=IDS)
def test_every_lane_holds_the_words_of_its_chunk_distinct_elements(p):
    rng = random.Random(p % 10007)
    for tab in _tabs(p):
        ys = [rng.randrange(p) for _ in range(64)]
        assert len(set(ys)) == 64
        _check_unit(p, tab, ys)


@pytest.mark.parametrize("p", PRIMES, ids=IDS)
def test_every_lane_holds_the_words_of_its_chunk_edge_elements(p):
    ys = _edge_unit(p)
    assert {0, p - 1, (1 << 256) - 1} <= set(ys)
    for tab in _tabs(p):
        _check_unit(p, tab, ys)


def test_without_the_swap_half_the_words_are_another_chunks():
    """the model's own check: leave the swap out and lanes 0 .. 31 hold chunk 32 + r's words in the odd places, lanes 32 .. 63 chunk r's"""
    p = BLS_R
    tab = _tabs(p)[0]
    rng = random.Random(5)
    ys = [rng.randrange(p) for _ in range(64)]
    words = m32.task_words(ys, tab, swap=False)
    wrong = [lane for lane in range(64) if words[lane] != m32.direct_words(ys[lane], tab)]
    assert wrong == list(range(64))

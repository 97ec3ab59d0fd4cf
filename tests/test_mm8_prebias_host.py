"""The pre-biased MFMA phases of k_mm8 / k_mm8f (honeybadgermpc_amd/csrc/gen_mm8.py: Mm8PhaseB, Mm8PhasePackedB) beside the phases they
stand in for.  A phase is an inline-asm string: nothing in it is padded or checked by the compiler, so the generator's own symbolic run
(check_phase) and the counts below are what stands between a wrong schedule and a rare wrong answer.  CPU-only: plain Python."""
import importlib.util
import os
import re

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "honeybadgermpc_amd", "csrc")


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("gen_mm8", os.path.join(CSRC, "gen_mm8.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _variants():
    out = []
    for nkb, skip in [(k, False) for k in range(1, 5)] + [(k, True) for k in range(2, 5)]:
        out += [(nkb, half, skip, False) for half in range(2)]
    for nkb in range(1, 5):
        out += [(nkb, half, False, True) for half in range(2)]
    return out


def _mfma_columns(gen, lines, half, packed):
    """(number of MFMAs, the columns whose accumulator starts from the bias operand) as the text says it, without the symbolic run"""
    cols = gen.packed_columns(half) if packed else gen.half_columns(half)
    bias = f"%{len(cols) + 2}"
    mf = [ln.replace(",", " ").split() for ln in lines if ln.startswith("v_mfma")]
    started = [cols[int(t[1].lstrip("%"))] for t in mf if t[4] == bias]
    assert len(started) == len(set(started))
    return len(mf), set(started)


def test_the_generator_lists_every_variant(gen):
    assert gen.variants() == _variants()


@pytest.mark.parametrize("nkb,half,skip,packed", _variants())
def test_same_mfmas_and_columns_as_the_existing_phase(gen, nkb, half, skip, packed):
    new, ncol = gen.asm_half_b(half, nkb, skip, packed)
    old, ncol_old = gen.asm_half(half, nkb, skip, packed)
    assert ncol == ncol_old
    assert _mfma_columns(gen, new, half, packed) == _mfma_columns(gen, old, half, packed)
    # the symbolic run: every MFMA reads the window and the digit piece of its column, each (column, K-block, group) once, no operand
    # younger than two wait states, none read while its LDS read is in flight
    got = gen.check_phase(new, half, nkb, skip, packed, True)
    assert got == gen.check_phase(old, half, nkb, skip, packed, False)
    assert got[0] == _mfma_columns(gen, new, half, packed)[0]
    assert got[1] == set(gen.packed_columns(half) if packed else gen.half_columns(half))
    # the MFMAs themselves, in order, are the existing phase's (the schedule around them is what changed)
    assert [ln for ln in new if ln.startswith("v_mfma")] == [ln for ln in old if ln.startswith("v_mfma")]


@pytest.mark.parametrize("nkb,half,skip,packed", _variants())
def test_no_bias_and_no_copy_left(gen, nkb, half, skip, packed):
    new, _ = gen.asm_half_b(half, nkb, skip, packed)
    old, _ = gen.asm_half(half, nkb, skip, packed)
    assert not any("0x80808080" in ln or ln.startswith("v_xor") for ln in new)
    assert sum(ln.startswith("v_xor") for ln in old) == 16 * nkb
    # the positions outside an element are written once, at the head
    movs = [i for i, ln in enumerate(new) if ln.startswith("v_mov_b32")]
    assert movs == list(range(10))
    # what is left of the preparation: the shifted files (18 a shift; half 1's in-place shift by two as well)
    aligns = sum(ln.startswith("v_alignbyte") for ln in new)
    assert aligns == 18 * nkb * (2 if half else 1)
    assert aligns == sum(ln.startswith("v_alignbyte") for ln in old)
    # four element reads a K-block, straight into file set 0 from k = 0 on
    reads = [ln for ln in new if ln.startswith("ds_read_b128") and f", %{len(gen.packed_columns(half) if packed else gen.half_columns(half))} " in ln]
    assert len(reads) == 4 * nkb
    for i, ln in enumerate(reads):
        kb, j = divmod(i, 4)
        r = gen.F_SETS[0] + 4 + 4 * j
        assert ln.startswith(f"ds_read_b128 v[{r}:{r + 3}],") and ln.endswith(f"offset:{(4 * kb + j) * 1024}")


@pytest.mark.parametrize("nkb,half,skip,packed", _variants())
def test_next_k_block_is_fetched_behind_its_last_reader(gen, nkb, half, skip, packed):
    """K-block kb + 1 lands in file set 0 only after the last MFMA that reads set 0 (the first shift of K-block kb) has been issued, and is
    waited for before the first MFMA that reads it"""
    new, _ = gen.asm_half_b(half, nkb, skip, packed)
    lo, hi = gen.F_SETS[0], gen.F_SETS[0] + 21
    reads0 = [i for i, ln in enumerate(new) if ln.startswith("v_mfma") and lo <= int(re.findall(r"v\[(\d+):", ln)[1]) <= hi]
    for kb in range(1, nkb):
        first_fetch = next(i for i, ln in enumerate(new) if ln.startswith("ds_read_b128") and ln.endswith(f"offset:{4 * kb * 1024}") and f"v[{lo + 4}:" in ln)
        before = [i for i in reads0 if i < first_fetch]
        after = [i for i in reads0 if i > first_fetch]
        assert len(before) * (nkb - kb) == len(after) * kb or skip          # (skip: K-block 0 has half the MFMAs)
        assert before and after
        assert any(ln.startswith("s_waitcnt lgkmcnt(0)") for ln in new[first_fetch:after[0]])
        # under the second shift's MFMAs: at least a handful of them stand between the fetch and its wait
        wait = next(i for i in range(first_fetch, len(new)) if new[i].startswith("s_waitcnt"))
        assert sum(ln.startswith("v_mfma") for ln in new[first_fetch:wait]) >= 4


def test_reserved_registers_are_the_clobber_list(gen):
    text = gen.emit()
    blocks = re.findall(r"template <> struct (Mm8Phase\w*)<[^>]*> \{(.*?)\n\};", text, re.S)
    assert len(blocks) == 2 * len(_variants())
    for name, body in blocks:
        lo = gen.CLOBBER_LO_B if name.endswith("B") else gen.CLOBBER_LO
        clob = [int(r) for r in re.findall(r'"v(\d+)"', body.split('"v"(biasv)')[1])]
        assert clob == list(range(lo, gen.CLOBBER_HI + 1)), name
        used = {int(r) for r in re.findall(r"\bv(\d+)\b", body.split('"v"(biasv)')[0])}
        for a, b in re.findall(r"\bv\[(\d+):(\d+)\]", body):
            used |= set(range(int(a), int(b) + 1))
        assert used and min(used) >= lo and max(used) <= gen.CLOBBER_HI, name
    assert gen.CLOBBER_LO_B == gen.CLOBBER_LO + 16 == gen.ABUF[0][0]          # XB's sixteen registers are given back


def test_existing_phases_keep_their_text(gen):
    """the new templates are appended: what the untouched kernels include is what it was"""
    text = gen.emit()
    head = text.split("// pre-biased phases:")[0]
    assert "Mm8PhaseB" not in head and "Mm8PhasePackedB" not in head
    assert head.count("template <> struct Mm8Phase<") == 14 and head.count("template <> struct Mm8PhasePacked<") == 8

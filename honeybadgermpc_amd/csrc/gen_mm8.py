#!/usr/bin/env python3
"""Emits hb_mm8_body.inc: the MFMA phases of k_mm8 (hb_mfma.hip) as inline-asm blocks.

Column c of an output is an int8 dot product between matrix digits (A operand) and a window of input bytes
(B operand): col_c = sum_l sum_b M_b[l] X_{c-b}[l].  One v_mfma_i32_16x16x64_i8 contracts 64 products per
(row, chunk); a lane's 16 B-operand bytes are cut as

    8 TERMS x 8 DIGITS per K-block:  lane (n, g) feeds terms t0 = 8 kb + 2 g and t1 = t0 + 1 of chunk n, the 16 digits of
    an entry are two groups G (b in [8 G, 8 G + 8)), and with s = c - 7 - 8 G = 4 q + rho the operand is the 8-byte
    windows [s, s + 7] of both elements: dwords q, q + 1 of each element shifted right by rho bytes.

Why 8 x 8 and not 4 terms x 16 digits (the first version of this kernel): a 16-byte window per element slides over 47
positions per term block (47 MFMAs per 4 terms = 11.75 per term, 68 % of the K slots useful); 8-byte windows take
39 positions x 2 groups per 8 terms = 9.75 per term -- 17 % fewer MFMAs -- and, more important for a kernel bound by
VALU issue, the operand files shrink to one: with the register file laid out [dword k][element e] the operand of window q
is registers 2 q .. 2 q + 3, ALWAYS even-aligned, so the second copy of the file one register apart (9 v_mov per group)
is gone, and a lane prepares two elements per group for eight terms instead of one for four: 270 preparation ops per wave
pass instead of 520.

The columns are produced in two halves BY SHIFT: half 0 = rho in {0, 1} (c = 3, 0 mod 4; 23 columns), half 1 = rho in
{2, 3} (c = 1, 2 mod 4; 24).  Within a half each (K-block, rho) group covers every window of that shift, so its shifted
dwords SH_rho[k], k = -1 .. 7, are computed once per element:
    F[k][e] = X_e[k] ^ 0x80808080                       (rho = 0: also the copy out of the LDS prefetch registers)
    F[k][e] = alignbyte(F[k+1][e], F[k][e], 2)          (rho = 2: in place on that copy)
    F'[k][e] = alignbyte(F[k+1][e], F[k][e], 1)         (rho 0 -> 1, 2 -> 3: into the OTHER of two file sets, built while the
                                                          MFMAs of the current group still read this one)
Registers v180..v255 are reserved (clobbers): XB (LDS prefetch of the next K-block's two elements), two pairs of A-operand
buffers, two file sets.  The accumulators are ordinary "=&v" outputs.

Hazards handled here (nothing inside an asm string is padded by the compiler): VALU write -> MFMA operand needs 2 wait
states (every preparation op of a group precedes the last MFMA of the previous one, plus s_nop 0); a file set is only
rewritten after every MFMA that reads it has been issued; MFMA result -> VALU read after the block (s_nop 7 x2).

The PRE-BIASED phases (Mm8PhaseB / Mm8PhasePackedB, asm_half_b) read an element buffer whose bytes are biased already and whose
sixteen-byte granule j of a lane's K-block is {e0[2j], e1[2j], e0[2j+1], e1[2j+1]} -- registers 4 j .. 4 j + 3 of a file set from
k = 0 on.  So a K-block's four ds_read_b128 land in file set 0 as the shift-0 operand: no XB, no XOR, no copy, and the reserved
range starts at v196.  K-block kb + 1 is fetched into set 0 as soon as the last MFMA of (kb, first shift) has been issued, under
the MFMAs of the second shift, which read set 1; k = -2, -1 and 8 are written once at the head (half 1's in-place shift by two
takes k = -1 from the constant).  check_phase() runs every emitted phase, old and new, on symbolic registers: every MFMA reads
the window and the digit piece its column needs, no operand was written by the VALU less than two wait states before, none is
read while its LDS read is in flight, and every (column, K-block, digit group) is contracted exactly once.
"""
import os
import re

NC = 47
MAXKB = 4                   # K-blocks of 8 terms: d <= 32
XB = 180                    # 16 dwords: element e dword k at XB + 8 e + k
ABUF = [[196, 200], [204, 208]]   # [K-block parity][digit group], 4 dwords each
F_SETS = [212, 234]         # 22 registers each: dword k = -2 .. 8 of element e at base + 2 (k + 2) + e
F_KMIN = -2
CLOBBER_LO, CLOBBER_HI = 180, 255
HALF_RHOS = [(0, 1), (2, 3)]


def f(s, k, e):
    assert -2 <= k <= 8 and e in (0, 1)
    return F_SETS[s] + 2 * (k - F_KMIN) + e


def windows(rho):
    """dword offsets q of the windows s = 4 q + rho in [-7, 31]"""
    return [q for q in range(-2, 8) if -7 <= 4 * q + rho <= 31]


def cols_of(rho):
    return sorted({4 * q + rho + 7 + 8 * g for q in windows(rho) for g in (0, 1)})


def half_columns(half):
    return sorted(c for rho in HALF_RHOS[half] for c in cols_of(rho))


NCP = 39                    # virtual columns of a packed pass: one per window


def packed_columns(half):
    """a packed pass has one accumulator per window s, the virtual column c' = s + 7: in M rows 0-7 (digit group 0) it is column
    c' of the output, in M rows 8-15 (the digit group 1 of the same outputs) column c' + 8"""
    return sorted(4 * q + rho + 7 for rho in HALF_RHOS[half] for q in windows(rho))


def lds_loads(kb, xs_op, as_op, packed=False):
    """K-block kb: both elements of the lane (2 x 32 bytes) and both digit groups (packed: the one piece that holds both)"""
    a0, a1 = ABUF[kb & 1]
    out = []
    for e in (0, 1):
        for h in (0, 1):
            out.append(f"ds_read_b128 v[{XB + 8 * e + 4 * h}:{XB + 8 * e + 4 * h + 3}], {xs_op} offset:{((kb * 2 + e) * 2 + h) * 1024}")
    out.append(f"ds_read_b128 v[{a0}:{a0 + 3}], {as_op} offset:{(kb * 2) * 1024}")
    if not packed:
        out.append(f"ds_read_b128 v[{a1}:{a1 + 3}], {as_op} offset:{(kb * 2 + 1) * 1024}")
    return out


def interleave(mfmas, ops):
    """one MFMA, then a share of ops; every op ends up before the last MFMA"""
    out = []
    if not mfmas:
        return list(ops)
    n = len(mfmas)
    per = (len(ops) + max(n - 1, 1) - 1) // max(n - 1, 1)
    pi = 0
    for i, m in enumerate(mfmas):
        if i == n - 1:
            out += ops[pi:]
            pi = len(ops)
        out.append(m)
        if i < n - 1:
            out += ops[pi:pi + per]
            pi += per
    return out


def asm_half(half, nkb, skip=False, packed=False):
    """packed: the row tile holds the two digit groups of an output on M rows m and m + 8 of ONE sixteen-byte piece per K-block, so a
    window is one MFMA instead of two (39 n_kb in all) and the accumulators are the virtual columns of packed_columns().
    skip: the matrix has no digit above the eighth in its first eight terms (Vandermonde matrices at small points: x^l < 2^56
    for l < 8), so the MFMAs of digit group 1 in K-block 0 would add zeros -- they are left out (39 of 78 n_kb), and the columns only
    group 1 reaches start from the bias in K-block 1 instead"""
    assert not skip or nkb >= 2
    assert not (skip and packed)
    cols = packed_columns(half) if packed else half_columns(half)
    pos = {c: i for i, c in enumerate(cols)}
    ncol = len(cols)
    xs_op, as_op, bias = f"%{ncol}", f"%{ncol + 1}", f"%{ncol + 2}"
    L = []
    # positions that are read but never written stay zero: k = -2 and k = 8
    for s in range(2):
        for k in (-2, 8):
            for e in (0, 1):
                L.append(f"v_mov_b32 v{f(s, k, e)}, 0")
    L += lds_loads(0, xs_op, as_op, packed)[:(5 if skip else 6)]          # (skip: group 1's digits of K-block 0 are not needed)
    groups = [(kb, rho) for kb in range(nkb) for rho in HALF_RHOS[half]]

    def prep(gi):
        """fill file set gi & 1 for group gi"""
        kb, rho = groups[gi]
        s = gi & 1
        ops = []
        if rho == HALF_RHOS[half][0]:
            ops.append("s_waitcnt lgkmcnt(0)")
            for e in (0, 1):
                for k in range(8):
                    ops.append(f"v_xor_b32 v{f(s, k, e)}, 0x80808080, v{XB + 8 * e + k}")
                ops.append(f"v_mov_b32 v{f(s, -1, e)}, 0")
            if rho != 0:                                    # half 1 starts at shift 2: in place, nobody reads this set yet
                for e in (0, 1):
                    for k in range(-1, 8):
                        ops.append(f"v_alignbyte_b32 v{f(s, k, e)}, v{f(s, k + 1, e)}, v{f(s, k, e)}, {rho}")
        else:
            for e in (0, 1):
                for k in range(-1, 8):
                    ops.append(f"v_alignbyte_b32 v{f(s, k, e)}, v{f(1 - s, k + 1, e)}, v{f(1 - s, k, e)}, 1")
        return ops

    started = set()

    def mfmas(gi):
        kb, rho = groups[gi]
        s = gi & 1
        out = []
        for q in windows(rho):
            r = f(s, q, 0)
            assert r % 2 == 0
            for grp in ((0,) if packed else (0, 1)):
                if skip and kb == 0 and grp == 1:
                    continue
                c = 4 * q + rho + 7 + 8 * grp
                ab = ABUF[kb & 1][grp]
                cin = f"%{pos[c]}"
                if c not in started:
                    assert kb == 0 or (skip and kb == 1)
                    cin = bias
                    started.add(c)
                out.append(f"v_mfma_i32_16x16x64_i8 %{pos[c]}, v[{ab}:{ab + 3}], v[{r}:{r + 3}], {cin}")
        return out

    L += prep(0) + ["s_nop 1"]
    for gi in range(len(groups)):
        nxt = gi + 1 < len(groups)
        kb, rho = groups[gi]
        if rho == HALF_RHOS[half][0] and kb + 1 < nkb:
            # XB was consumed by this group's preparation and every MFMA of K-block kb - 1 (the last reader of the other A
            # buffers) has been issued: fetch K-block kb + 1
            L += lds_loads(kb + 1, xs_op, as_op, packed)
        L += interleave(mfmas(gi), prep(gi + 1) if nxt else [])
        if nxt:
            L.append("s_nop 0")
    assert started == set(cols)
    L += ["s_nop 7", "s_nop 7"]
    return L, ncol


CLOBBER_LO_B = 196          # the pre-biased phases: everything above XB


def lds_loads_b(kb, xs_op, as_op, packed=False):
    """K-block kb of a pre-biased buffer: granule j is dwords 2 j, 2 j + 1 of both elements, file set 0's registers from k = 2 j on"""
    a0, a1 = ABUF[kb & 1]
    out = []
    for j in range(4):
        r = f(0, 2 * j, 0)
        out.append(f"ds_read_b128 v[{r}:{r + 3}], {xs_op} offset:{(kb * 4 + j) * 1024}")
    out.append(f"ds_read_b128 v[{a0}:{a0 + 3}], {as_op} offset:{(kb * 2) * 1024}")
    if not packed:
        out.append(f"ds_read_b128 v[{a1}:{a1 + 3}], {as_op} offset:{(kb * 2 + 1) * 1024}")
    return out


def asm_half_b(half, nkb, skip=False, packed=False):
    """asm_half on a pre-biased, interleaved element buffer (the docstring's last paragraph): same groups, same MFMAs, same accumulators"""
    assert not skip or nkb >= 2
    assert not (skip and packed)
    cols = packed_columns(half) if packed else half_columns(half)
    pos = {c: i for i, c in enumerate(cols)}
    ncol = len(cols)
    xs_op, as_op, bias = f"%{ncol}", f"%{ncol + 1}", f"%{ncol + 2}"
    rho0 = HALF_RHOS[half][0]
    L = []
    # written once: k = -2 and k = 8 of both sets, k = -1 of the set the LDS reads land in
    for s in range(2):
        for k in (-2, 8):
            for e in (0, 1):
                L.append(f"v_mov_b32 v{f(s, k, e)}, 0")
    for e in (0, 1):
        L.append(f"v_mov_b32 v{f(0, -1, e)}, 0")
    groups = [(kb, rho) for kb in range(nkb) for rho in HALF_RHOS[half]]

    def fetch(kb):
        ops = lds_loads_b(kb, xs_op, as_op, packed)
        return ops[:5] if skip and kb == 0 else ops          # (skip: group 1's digits of K-block 0 are not needed)

    def prep(gi):
        """what group gi needs before its first MFMA, the fetch apart"""
        kb, rho = groups[gi]
        s = gi & 1
        ops = []
        if rho == rho0:
            assert s == 0
            ops.append("s_waitcnt lgkmcnt(0)")
            if rho != 0:                                    # half 1 starts at shift 2: in place, nobody reads this set now
                for e in (0, 1):
                    ops.append(f"v_alignbyte_b32 v{f(0, -1, e)}, v{f(0, 0, e)}, 0, {rho}")
                    for k in range(0, 8):
                        ops.append(f"v_alignbyte_b32 v{f(0, k, e)}, v{f(0, k + 1, e)}, v{f(0, k, e)}, {rho}")
        else:
            assert s == 1
            for e in (0, 1):
                for k in range(-1, 8):
                    ops.append(f"v_alignbyte_b32 v{f(1, k, e)}, v{f(0, k + 1, e)}, v{f(0, k, e)}, 1")
        return ops

    started = set()

    def mfmas(gi):
        kb, rho = groups[gi]
        s = gi & 1
        out = []
        for q in windows(rho):
            r = f(s, q, 0)
            assert r % 2 == 0
            for grp in ((0,) if packed else (0, 1)):
                if skip and kb == 0 and grp == 1:
                    continue
                c = 4 * q + rho + 7 + 8 * grp
                ab = ABUF[kb & 1][grp]
                cin = f"%{pos[c]}"
                if c not in started:
                    assert kb == 0 or (skip and kb == 1)
                    cin = bias
                    started.add(c)
                out.append(f"v_mfma_i32_16x16x64_i8 %{pos[c]}, v[{ab}:{ab + 3}], v[{r}:{r + 3}], {cin}")
        return out

    L += fetch(0) + prep(0) + ["s_nop 1"]
    for gi in range(len(groups)):
        nxt = gi + 1 < len(groups)
        kb, rho = groups[gi]
        mm = mfmas(gi)
        if not nxt:
            L += mm
        elif rho == rho0:
            # the second shift of this K-block, built into set 1 under this group's MFMAs
            L += interleave(mm, prep(gi + 1)) + ["s_nop 0"]
        else:
            # every MFMA that reads set 0 (and the A buffers of K-block kb - 1) has been issued: K-block kb + 1 lands there under this
            # group's MFMAs, and what it needs behind its wait (half 1: the shift by two) shares the group's second half
            hold = len(mm) - 2 if rho0 == 0 else len(mm) // 2
            L += fetch(kb + 1) + mm[:hold] + interleave(mm[hold:], prep(gi + 1)) + ["s_nop 0"]
    assert started == set(cols)
    L += ["s_nop 7", "s_nop 7"]
    return L, ncol


def check_phase(lines, half, nkb, skip, packed, prebiased):
    """Symbolic run of one phase.  A register holds None (unknown), 'z' (zero), ('a', kb, grp, i) (dword i of a digit piece) or
    ('x', kb, k, rho, e): bytes 4 k + rho .. 4 k + rho + 3 of element e of K-block kb's pair, zero outside the element."""
    cols = packed_columns(half) if packed else half_columns(half)
    ncol = len(cols)
    reg = {}
    pending = {}                # register -> value of an LDS read in flight
    valu_age = {}               # register -> wait states since the VALU wrote it
    done = set()
    n_mfma = 0

    def outside(k, rho):
        return 4 * k + rho + 3 < 0 or 4 * k + rho >= 32

    def tick(n):
        for r in list(valu_age):
            valu_age[r] += n
            if valu_age[r] > 8:
                del valu_age[r]

    def rd(r):
        assert r not in pending, f"v{r} read while its LDS read is in flight"
        return reg.get(r)

    def wr(r, v):
        assert r not in pending, f"v{r} written while its LDS read is in flight"
        assert CLOBBER_LO_B <= r <= CLOBBER_HI if prebiased else CLOBBER_LO <= r <= CLOBBER_HI, f"v{r} outside the reserved range"
        reg[r] = v
        valu_age[r] = 0

    def num(tok):
        return int(tok.strip().rstrip(",").lstrip("v"))

    for ln in lines:
        t = ln.replace(",", " ").split()
        op = t[0]
        if op == "s_nop":
            tick(int(t[1]) + 1)
            continue
        if op == "s_waitcnt":
            assert t[1] == "lgkmcnt(0)"
            for r, v in pending.items():
                reg[r] = v
            pending.clear()
            tick(1)
            continue
        tick(1)
        if op == "v_mov_b32":
            assert t[2] == "0"
            wr(num(t[1]), "z")
        elif op == "v_xor_b32":
            assert not prebiased and t[2] == "0x80808080"
            v = rd(num(t[3]))
            assert v is not None and v != "z"
            wr(num(t[1]), v)
        elif op == "v_alignbyte_b32":
            d, n = num(t[1]), int(t[4])
            hi = rd(num(t[2]))
            lo = "z" if t[3] == "0" else rd(num(t[3]))
            assert hi is not None and lo is not None, ln
            if hi == "z" and lo == "z":
                wr(d, "z")
                continue
            ref = lo if lo != "z" else hi
            _, kb, k, rho, e = ref
            if lo == "z":
                k -= 1
            assert lo == ("x", kb, k, rho, e) or (lo == "z" and outside(k, rho)), ln
            assert hi == ("x", kb, k + 1, rho, e) or (hi == "z" and outside(k + 1, rho)), ln
            assert rho + n <= 3
            wr(d, ("x", kb, k, rho + n, e))
        elif op == "ds_read_b128":
            m = re.match(r"v\[(\d+):(\d+)\]", t[1])
            lo_r, hi_r = int(m.group(1)), int(m.group(2))
            assert hi_r == lo_r + 3 and (CLOBBER_LO_B if prebiased else CLOBBER_LO) <= lo_r and hi_r <= CLOBBER_HI
            slot, rem = divmod(int(t[3].split(":")[1]), 1024)
            assert rem == 0
            for i in range(4):
                if t[2] == f"%{ncol}":
                    if prebiased:
                        kb, j = divmod(slot, 4)
                        v = ("x", kb, 2 * j + (i >> 1), 0, i & 1)
                    else:
                        kb, eh = divmod(slot, 4)
                        v = ("x", kb, 4 * (eh & 1) + i, 0, eh >> 1)
                else:
                    assert t[2] == f"%{ncol + 1}"
                    v = ("a", slot >> 1, slot & 1, i)
                assert lo_r + i not in pending
                pending[lo_r + i] = v
                reg.pop(lo_r + i, None)
                valu_age.pop(lo_r + i, None)
        elif op == "v_mfma_i32_16x16x64_i8":
            n_mfma += 1
            acc = int(t[1].lstrip("%"))
            ma, mb = re.match(r"v\[(\d+):(\d+)\]", t[2]), re.match(r"v\[(\d+):(\d+)\]", t[3])
            a0, b0 = int(ma.group(1)), int(mb.group(1))
            for r in list(range(a0, a0 + 4)) + list(range(b0, b0 + 4)):
                assert valu_age.get(r, 99) > 2, f"v{r}: VALU write {valu_age[r]} wait states before the MFMA that reads it"
            av = [rd(a0 + i) for i in range(4)]
            assert av[0] is not None and av[0][0] == "a"
            _, kb, grp, _ = av[0]
            assert av == [("a", kb, grp, i) for i in range(4)], ln
            bv = [rd(b0 + i) for i in range(4)]
            ref = next(v for v in bv if v not in (None, "z"))
            _, kbx, k, rho, e = ref
            q = k - bv.index(ref) // 2
            for i in range(4):
                kk, ee = q + (i >> 1), i & 1
                assert bv[i] == ("x", kb, kk, rho, ee) or (bv[i] == "z" and outside(kk, rho)), (ln, bv)
            assert kbx == kb and rho in HALF_RHOS[half]
            c = 4 * q + rho + 7 + 8 * grp
            assert not packed or grp == 0
            assert cols[acc] == c, ln
            cin = t[4]
            first = not any(dc == c for dc, _, _ in done)
            assert cin == (f"%{ncol + 2}" if first else f"%{acc}"), ln
            assert (c, kb, grp) not in done
            done.add((c, kb, grp))
        else:
            raise AssertionError(ln)
    assert not pending
    want = set()
    for rho in HALF_RHOS[half]:
        for q in windows(rho):
            for grp in ((0,) if packed else (0, 1)):
                for kb in range(nkb):
                    if not (skip and kb == 0 and grp == 1):
                        want.add((4 * q + rho + 7 + 8 * grp, kb, grp))
    assert done == want and n_mfma == len(want)
    assert lines[-2:] == ["s_nop 7", "s_nop 7"]      # MFMA result -> VALU
    return n_mfma, {c for c, _, _ in done}


def variants():
    """(nkb, half, skip, packed) of every generated phase"""
    out = []
    for nkb, skip in [(k, False) for k in range(1, MAXKB + 1)] + [(k, True) for k in range(2, MAXKB + 1)]:
        out += [(nkb, half, skip, False) for half in range(2)]
    for nkb in range(1, MAXKB + 1):
        out += [(nkb, half, False, True) for half in range(2)]
    return out


def emit():
    out = ["// GENERATED by gen_mm8.py -- do not edit", ""]
    out.append("// column held by accumulator i of each half (half 0: rho in {0,1}; half 1: rho in {2,3})")
    for half in range(2):
        cols = half_columns(half)
        out.append(f"// half {half}: {cols}")
    assert half_columns(0) == [c for c in range(NC) if c % 4 in (0, 3)] and half_columns(1) == [c for c in range(NC) if c % 4 in (1, 2)]
    out.append("template <int NKB, int HALF, bool SKIP = false> struct Mm8Phase;")
    clob = ", ".join(f'"v{r}"' for r in range(CLOBBER_LO, CLOBBER_HI + 1))
    for nkb, skip in [(k, False) for k in range(1, MAXKB + 1)] + [(k, True) for k in range(2, MAXKB + 1)]:
        for half in range(2):
            lines, ncol = asm_half(half, nkb, skip)
            check_phase(lines, half, nkb, skip, False, False)
            out.append(f"template <> struct Mm8Phase<{nkb}, {half}, {'true' if skip else 'false'}> {{")
            out.append("    static __device__ __forceinline__ void run(v4i (&acc)[24], uint32_t xs_addr, uint32_t as_addr, v4i biasv) {")
            out.append("        asm volatile(")
            for ln in lines:
                out.append(f'            "{ln}\\n\\t"')
            outs = ", ".join(f'"=&v"(acc[{i}])' for i in range(ncol))
            out.append(f"            : {outs}")
            out.append('            : "v"(xs_addr), "v"(as_addr), "v"(biasv)')
            out.append(f'            : {clob}, "memory");')
            out.append("    }")
            out.append("};")
    # the packed phases (k_mm8f's narrow last row tile): their own template, so that the text above stays what it was
    assert packed_columns(0) == [c for c in range(NCP) if c % 4 in (0, 3)] and packed_columns(1) == [c for c in range(NCP) if c % 4 in (1, 2)]
    out.append("// packed phases: accumulator i of a half is the virtual column (one per window) of the same two lists cut at 38")
    out.append("template <int NKB, int HALF> struct Mm8PhasePacked;")
    for nkb in range(1, MAXKB + 1):
        for half in range(2):
            lines, ncol = asm_half(half, nkb, packed=True)
            check_phase(lines, half, nkb, False, True, False)
            assert sum("v_mfma" in ln for ln in lines) == len(windows(HALF_RHOS[half][0]) + windows(HALF_RHOS[half][1])) * nkb
            out.append(f"template <> struct Mm8PhasePacked<{nkb}, {half}> {{")
            out.append("    static __device__ __forceinline__ void run(v4i (&acc)[20], uint32_t xs_addr, uint32_t as_addr, v4i biasv) {")
            out.append("        asm volatile(")
            for ln in lines:
                out.append(f'            "{ln}\\n\\t"')
            outs = ", ".join(f'"=&v"(acc[{i}])' for i in range(ncol))
            out.append(f"            : {outs}")
            out.append('            : "v"(xs_addr), "v"(as_addr), "v"(biasv)')
            out.append(f'            : {clob}, "memory");')
            out.append("    }")
            out.append("};")
    # the pre-biased phases, beside the ones above (whose text stays what it was)
    out.append("// pre-biased phases: the element buffer holds biased bytes in interleaved granules (gen_mm8.py); accumulators as above")
    out.append("template <int NKB, int HALF, bool SKIP = false> struct Mm8PhaseB;")
    out.append("template <int NKB, int HALF> struct Mm8PhasePackedB;")
    clob_b = ", ".join(f'"v{r}"' for r in range(CLOBBER_LO_B, CLOBBER_HI + 1))
    for nkb, half, skip, packed in variants():
        lines, ncol = asm_half_b(half, nkb, skip, packed)
        old_lines, _ = asm_half(half, nkb, skip, packed)
        assert check_phase(lines, half, nkb, skip, packed, True) == check_phase(old_lines, half, nkb, skip, packed, False)
        assert not any("0x80808080" in ln or "v_xor" in ln for ln in lines)
        if packed:
            out.append(f"template <> struct Mm8PhasePackedB<{nkb}, {half}> {{")
        else:
            out.append(f"template <> struct Mm8PhaseB<{nkb}, {half}, {'true' if skip else 'false'}> {{")
        out.append(f"    static __device__ __forceinline__ void run(v4i (&acc)[{20 if packed else 24}], uint32_t xs_addr, uint32_t as_addr, v4i biasv) {{")
        out.append("        asm volatile(")
        for ln in lines:
            out.append(f'            "{ln}\\n\\t"')
        outs = ", ".join(f'"=&v"(acc[{i}])' for i in range(ncol))
        out.append(f"            : {outs}")
        out.append('            : "v"(xs_addr), "v"(as_addr), "v"(biasv)')
        out.append(f'            : {clob_b}, "memory");')
        out.append("    }")
        out.append("};")
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    text = emit()
    path = os.path.join(here, "hb_mm8_body.inc")
    old = open(path).read() if os.path.exists(path) else None
    if old != text:
        open(path, "w").write(text)
    print(path)

"""Lane-level model of k_mm8f's division by den_l as two dense 32x32x32 int8 products a task (hb_mfma_fused.hip: ms_products, ms_words,
fetch_halves and the builder's tables): where every byte lies in the two tables, which bytes a lane holds in each operand, which column an
accumulator register is, and what the half swap leaves in which lane -- in exact integers.  CPU only; tests/test_fs_mscale32_model.py
runs it against tests/fs_mscale_model.py, whose digits, constants and bounds it takes as they are: a column here is the same sum of the
same 32 products as there (below 2^21 and positive by that file's assertions; nothing new to prove), only gathered through other lanes.

A wave is 64 lanes, lane = (r, h) = (lane & 31, lane >> 5).  A task is term l of a unit's 64 chunks:

    tables      digits: piece h * 32 + m, byte j = digit m of U_l[16 h + j]                  (1 KB a term: piece `lane` is the lane's A operand)
                constants: [h][i] = CINIT[(i & 3) + 8 (i >> 2) + 4 h], int32                 (128 B a term: a lane's C operand, register i)
    B           lane (r, h), product s: bytes 16 h .. 16 h + 15 of chunk 32 s + r, XOR 0x80 read as int8
    MFMA        D[row][col] = C[row][col] + sum_k A[row][k] B[k][col] with row on the registers and col on the lane:
                register i of lane (n, h') is row (i & 3) + 8 (i >> 2) + 4 h', column n
    K           the ONLY assumption about the order of the 32 values of k: element j of A's lane (m, h) and element j of B's lane (n, h)
                carry the same k.  The sum over k is symmetric, so which k that is does not matter -- the model sums over (h, j)
    addends     registers 4 q .. 4 q + 3 of lane (r, h) are the four columns of 32-bit word 2 q + h
    half swap   lanes 32 .. 63 of the destination (product 0's addend) trade places with lanes 0 .. 31 of the source (product 1's):
                the destination then holds word 2 q of chunk = lane, the source word 2 q + 1 of chunk = lane, in every lane
"""

BIAS = 1 << 20


def reg_row(i, h):
    """the accumulator map of the 32x32 MFMA: the row (here: the column c of the division) of register i in a lane of half h"""
    return (i & 3) + 8 * (i >> 2) + 4 * h


def digit_table(digits):
    """the 1 KB row of a term as 64 pieces of 16 int8: piece h * 32 + m, byte j = digit m of U[16 h + j]  (digits[b][c]: fs_mscale_model)"""
    return [[digits[16 * h + j][m] for j in range(16)] for h in range(2) for m in range(32)]


def const_table(cinit):
    """the 128 B of a term as [h][i] int32 in the accumulators' order"""
    return [[cinit[reg_row(i, h)] for i in range(16)] for h in range(2)]


def b_operand(ys, s):
    """the B fragment of product s: lane (r, h) holds bytes 16 h .. 16 h + 15 of chunk 32 s + r, XOR 0x80 as int8  (ys: the unit's 64 elements)"""
    frag = []
    for lane in range(64):
        r, h = lane & 31, lane >> 5
        y = ys[32 * s + r]
        raw = [((y >> (8 * (16 * h + j))) & 0xff) ^ 0x80 for j in range(16)]
        frag.append([v - 256 if v > 127 else v for v in raw])
    return frag


def mfma_32x32x32_i8(a, b, c):
    """d[lane][i] for fragments a[lane][16], b[lane][16] (int8) and c[lane][16] (int32): a plain integer product over the maps above"""
    out = []
    for lane in range(64):
        n, hh = lane & 31, lane >> 5
        regs = []
        for i in range(16):
            m = reg_row(i, hh)
            acc = c[lane][i]
            for h in range(2):
                acc += sum(a[32 * h + m][j] * b[32 * h + n][j] for j in range(16))
            assert -(1 << 31) <= acc < 1 << 31
            regs.append(acc)
        out.append(regs)
    return out


def addends(acc):
    """the four 64-bit addends of a lane: q -> lo + 2^16 hi of registers 4 q .. 4 q + 3 (two shifted 32-bit adds, one multiply-add)"""
    out = []
    for lane in range(64):
        row = []
        for q in range(4):
            lo = acc[lane][4 * q] + (acc[lane][4 * q + 1] << 8)
            hi = acc[lane][4 * q + 2] + (acc[lane][4 * q + 3] << 8)
            assert 0 <= lo < 1 << 32 and 0 <= hi < 1 << 32
            row.append(lo + (hi << 16))
        out.append(row)
    return out


def permlane32_swap(dst, src):
    """v_permlane32_swap on one register of 64 lanes: (new dst, new src)"""
    return dst[:32] + src[:32], dst[32:] + src[32:]


def task_words(ys, tab, swap=True):
    """the eight 32-bit-word addends each lane holds behind the swap, [lane][k]; ys: the unit's 64 elements, tab: fs_mscale_model.term_tables"""
    digits, cinit = tab
    dt, ct = digit_table(digits), const_table(cinit)
    a = [dt[lane] for lane in range(64)]                       # piece `lane`
    c = [ct[lane >> 5] for lane in range(64)]
    ad = [addends(mfma_32x32x32_i8(a, b_operand(ys, s), c)) for s in range(2)]
    words = [[None] * 8 for _ in range(64)]
    for q in range(4):
        d0, s0 = [ad[0][lane][q] for lane in range(64)], [ad[1][lane][q] for lane in range(64)]
        # (the kernel swaps the low and the high dword of an addend with one instruction each: the same lanes, so one swap here)
        d1, s1 = permlane32_swap(d0, s0) if swap else (d0, s0)
        for lane in range(64):
            words[lane][2 * q], words[lane][2 * q + 1] = d1[lane], s1[lane]
    return words


def direct_words(y, tab):
    """the same eight addends from the definition (fs_mscale_model.scale_model's columns and words), no lanes involved"""
    digits, cinit = tab
    hb = [((y >> (8 * b)) & 0xff) - 128 for b in range(32)]
    cols = [cinit[c] + sum(hb[b] * digits[b][c] for b in range(32)) for c in range(32)]
    return [cols[4 * k] + (cols[4 * k + 1] << 8) + ((cols[4 * k + 2] + (cols[4 * k + 3] << 8)) << 16) for k in range(8)]


def tail(words, p):
    """the kernel's one-word quotient, carries and conditional subtraction over a lane's eight addends: the words written to LDS"""
    mu = (1 << 286) // p
    pneg = (1 << 256) - p
    tq = words[7] + (words[6] >> 32)
    q = ((tq >> 16) * mu) >> 46
    rp = sum((words[k] + q * ((pneg >> (32 * k)) & 0xffffffff)) << (32 * k) for k in range(8))
    r = rp - (q << 256)
    assert 0 <= r < 2 * p
    if p >> 255 and r >= p:
        r -= p
    return r

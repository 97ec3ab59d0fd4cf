"""Driver of the host self test of csrc/hb_sort.hip over lists of Python ints, and the three steps as Python-int formulas, shared by
test_sorting_host.py and by test_gpu_sorting.py, which holds every device step bit-equal to the self test of the same row.  Every
operand and output is a buffer of exactly the documented size (one element where the size is zero), so a row that reads or writes
a row too far does not stay inside its array."""
import ctypes

import numpy as np

CMP_MASK, SWAP_MASK, SWAP_FINISH = 0, 1, 2


def run_sort(p, nl, what, operands, n, batch, width, layer, k, kappa, outs):
    """hb_selftest_sort over lists of ints (None: a NULL operand; arrays of several rows are flat, row-major).  outs: for each output
    its number of elements, or a list of ints: its contents before the call (the table of SWAP_FINISH) -> (rc, [out lists])"""
    from honeybadgermpc_amd._capi import ints_to_limbs, limbs_to_ints, load_library, np_ptr

    lib = load_library()
    nb = 8 * nl
    arrays = [None if o is None else ints_to_limbs(list(o) or [0], p, nb) for o in operands]
    ptrs = (ctypes.c_void_p * 8)(*([None if x is None else x.ctypes.data for x in arrays] + [None] * (8 - len(arrays))))
    sizes = [o if isinstance(o, int) else len(o) for o in outs]
    bufs = [np.zeros((max(o, 1), nl), dtype=np.uint64) if isinstance(o, int) else ints_to_limbs(list(o) or [0], p, nb).copy() for o in outs]
    optrs = (ctypes.c_void_p * 2)(*([b.ctypes.data for b in bufs] + [None] * (2 - len(bufs))))
    a, r, d, cnt = layer
    prm = (ctypes.c_int64 * 9)(n, batch, width, a, r, d, cnt, k, kappa)
    rc = lib.hb_selftest_sort(np_ptr(ints_to_limbs([p], p + 1, nb)), nl, what, ptrs, prm, optrs)
    return rc, [limbs_to_ints(b[:s], nb) for b, s in zip(bufs, sizes)]


def slot_rows(s, n, layer):
    """slot s -> its two rows within a column of batch n elements"""
    a, r, d, cnt = layer
    b, e = divmod(s, cnt)
    lo = b * n + (((e >> a) << (a + 1)) | (e & ((1 << a) - 1)) | r)
    return lo, lo + d


def cmp_mask_model(p, table, bits, n, batch, layer, k, kappa):
    """table: [column][row], bits: [plane][slot] -> (masked, r1)"""
    slots = batch * layer[3]
    masked, r1 = [], []
    for s in range(slots):
        lo, hi = slot_rows(s, n, layer)
        r1.append(sum(bits[i][s] << i for i in range(k - 1)) % p)
        masked.append((table[0][lo] - table[0][hi] + (1 << (k - 1)) + sum(bits[i][s] << i for i in range(k + kappa))) % p)
    return masked, r1


def swap_mask_model(p, table, c, r1, carry, tp, tq, n, batch, layer, k):
    """tp, tq: [column][slot] -> [2 width][slots]"""
    slots, m, inv = batch * layer[3], k - 1, pow(2, -(k - 1), p)
    out = [[0] * slots for _ in range(2 * len(table))]
    for s in range(slots):
        lo, hi = slot_rows(s, n, layer)
        d = table[0][lo] - table[0][hi]
        a2 = c[s] % (1 << m) - r1[s] + (1 << m) * (1 - carry[s])
        u = 1 - (a2 - d) * inv
        for w, col in enumerate(table):
            out[2 * w][s] = (u - tp[w][s]) % p
            out[2 * w + 1][s] = (col[lo] - col[hi] - tq[w][s]) % p
    return out


def swap_finish_model(p, table, opened, tp, tq, tpq, n, batch, layer):
    """opened: [2 width][slots] -> the new table"""
    out = [list(col) for col in table]
    for s in range(batch * layer[3]):
        lo, hi = slot_rows(s, n, layer)
        for w in range(len(table)):
            d, e = opened[2 * w][s], opened[2 * w + 1][s]
            m = (d * e + d * tq[w][s] + e * tp[w][s] + tpq[w][s]) % p
            out[w][lo], out[w][hi] = (out[w][lo] - m) % p, (out[w][hi] + m) % p
    return out


def flat(rows):
    return [v for row in rows for v in row]


def unflat(values, rows):
    count = len(values) // rows if rows else 0
    return [values[r * count:(r + 1) * count] for r in range(rows)]

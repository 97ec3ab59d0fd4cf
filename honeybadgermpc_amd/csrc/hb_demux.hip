// hb_demux.hip -- the one-hot demultiplexer of shared index bits (honeybadgermpc_amd/progs/demux.py): from shares
// of the m bits of an index s = sum_i 2^i b_i, least significant first as hb_bd.hip returns them, shares of e_j = [s == j], j < 2^m,
// for arrays of indices.  Neighbouring groups of bits are merged by a Beaver OUTER product: the one-hot vector A of a low group of
// wl bits and B of a high group of wh bits give out[hi * 2^wl + lo] = A[lo] * B[hi], and only the two factor vectors are opened --
// 2^wl + 2^wh elements for 2^(wl + wh) products -- against a triple (P, Q, PQ = outer product), offline.generate_matrix_triples with
// inner dimension 1.
//
// The wiring (dm_plan below; demux_plan in progs/demux.py states the same): level 0 starts from m groups of width 1; a level merges
// the groups (0, 1), (2, 3), .. counted from the least significant and carries an odd last group unchanged; ceil(log2 m) levels.  A
// width-1 group is never stored: its vector is (1 - b, b), read from the bit plane by the level that consumes it.  Every merged group
// lives in ONE array of planes, `groups`: level l writes its merges one after another from row G_l = products of the levels before it,
// so a carried group stays where it is, and the rows of the last level, 2^m of them, are the result.
//
// The steps are rows under the generic kernel k_rows (hb_rows.hpp):
//   DmLeavesRow   m = 1 only: rows (1 - b, b) of the one bit plane.
//   DmMaskRow     row y of the level's array to open, sum (2^wl + 2^wh) rows: for merge k in order 2^wl rows A[lo] - P[lo], then 2^wh
//                 rows B[hi] - Q[hi]; ta holds P then Q in exactly that row order, so row y of the result is (factor row) - ta[y].
//   DmFinishRow   row y of the level's products, sum 2^(wl + wh) rows: merge k, r = y - (products of the merges before) = hi 2^wl + lo,
//                 groups[G_l + y] = d_lo e_hi + d_lo Q_hi + e_hi P_lo + PQ[y] by the fused Beaver body of hb_ew_elem.hpp, d, e, P, Q rows
//                 of `opened` and `ta` at the mask's numbering.
// The level's descriptors -- at most DM_MAX_MERGES = MAX_BITS / 2 merges: offsets into the opened array and into the products, widths,
// and where each factor lives -- travel by value in the argument struct; the row-to-merge map is a scan over at most 6 offsets, on
// blockIdx.y, so it is uniform over the workgroup (scalar work), and a descriptor field is picked by a chain of selects, not by an
// indexed read of the struct.  Operands and results are packed canonical residues; host_rows runs the very same rows, addressing
// included, on host memory for hb_selftest_demux.
//
// Launch shape: k_rows (256-thread workgroups, one element a thread in x, no LDS, no grid stride), the row in blockIdx.y -- at most
// 2^12 rows, which is why m stops at DM_MAX_BITS -- one launch a call.  The finish is bound by memory: PQ and the output are touched
// once (PQ takes the read-once load), 64 bytes an output at the wide width that no schedule can save.  The rows of d, e, P, Q are read
// again by 2^wh or 2^wl rows of the grid and take the PLAIN loads: a level opens at most 260 rows, which stay in cache while the
// workgroups of one x block walk y.  In the mask the bit planes (two rows read each) and ta (the finish reads it again) take the plain
// loads too, the stored groups the read-once one.
// A finish row that keeps d_lo and P_lo in registers across two neighbouring hi (8 loads for two outputs, not 12) was compiled beside
// this one and is NOT kept: by the compiler's report it takes 90 VGPRs against 70 at <9, 8> -- five waves a SIMD, not seven -- and 43
// against 28 at <3, 2>, to save reads that hit the cache anyway.  It was judged by that report alone; neither was timed against the other.
// Compiler's report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; scratch = 0 bytes for every kernel):
//   k_rows<DmLeavesRow, 9, 8>   29 VGPRs: 8 waves a SIMD       k_rows<DmLeavesRow, 3, 2>   11 VGPRs: 8 waves
//   k_rows<DmMaskRow, 9, 8>     29 VGPRs: 8 waves              k_rows<DmMaskRow, 3, 2>     11 VGPRs: 8 waves
//   k_rows<DmFinishRow, 9, 8>   70 VGPRs: 7 waves              k_rows<DmFinishRow, 3, 2>   28 VGPRs: 8 waves
#include "hb_common.hpp"
#include "hb_ew_elem.hpp"
#include "hb_rows.hpp"

using namespace hb;

namespace hb {

constexpr int DM_MAX_BITS = 12;                    // a level's rows go in blockIdx.y, and preprocessing grows as 2^m an index
constexpr int DM_MAX_MERGES = DM_MAX_BITS / 2;
constexpr int DM_NONE = 0x7fffffff;                // the offset of a merge the level does not have: no row reaches it

// ---------------------------------------------------------------- the wiring (host)
// One level.  Merge k < n: its rows of the opened array start at open_off[k] (2^wl of the low factor, then 2^wh of the high one), its
// products at prod_off[k]; a factor of width 1 is bit plane lo_row / hi_row, a wider one starts at that row of `groups`.  out_row: the
// row of `groups` the level's products start at.
struct DmLevel {
    int n, opened, products, out_row;
    int open_off[DM_MAX_MERGES], prod_off[DM_MAX_MERGES], wl[DM_MAX_MERGES], wh[DM_MAX_MERGES], lo_row[DM_MAX_MERGES], hi_row[DM_MAX_MERGES];
};

static int dm_levels(int m) { int l = 0; while ((1 << l) < m) l++; return l; }

// rows of `groups`: the products of every level
static int dm_group_rows(int m) {
    int width[DM_MAX_BITS], n = m, rows = 0;
    for (int i = 0; i < m; i++) width[i] = 1;
    while (n > 1) {
        int k = 0;
        for (; 2 * k + 1 < n; k++) { width[k] = width[2 * k] + width[2 * k + 1]; rows += 1 << width[k]; }
        if (n & 1) width[k] = width[n - 1];
        n = (n + 1) / 2;
    }
    return rows;
}

// the descriptors of `level` < dm_levels(m), 1 <= m <= DM_MAX_BITS
static void dm_plan(int m, int level, DmLevel &D) {
    int width[DM_MAX_BITS], row[DM_MAX_BITS], n = m, base = 0;             // a group: its width and where it lives
    for (int i = 0; i < m; i++) { width[i] = 1; row[i] = i; }
    for (int l = 0;; l++) {
        D.n = n / 2; D.opened = D.products = 0; D.out_row = base;
        for (int k = 0; k < DM_MAX_MERGES; k++) {
            D.open_off[k] = D.prod_off[k] = DM_NONE;
            D.wl[k] = D.wh[k] = D.lo_row[k] = D.hi_row[k] = 0;
        }
        for (int k = 0; k < D.n; k++) {
            D.open_off[k] = D.opened; D.prod_off[k] = D.products;
            D.wl[k] = width[2 * k]; D.wh[k] = width[2 * k + 1]; D.lo_row[k] = row[2 * k]; D.hi_row[k] = row[2 * k + 1];
            D.opened += (1 << D.wl[k]) + (1 << D.wh[k]);
            D.products += 1 << (D.wl[k] + D.wh[k]);
        }
        if (l == level) return;
        for (int k = 0; k < D.n; k++) { width[k] = D.wl[k] + D.wh[k]; row[k] = base + D.prod_off[k]; }
        if (n & 1) { width[D.n] = width[n - 1]; row[D.n] = row[n - 1]; }
        n = (n + 1) / 2;
        base += D.products;
    }
}

// ---------------------------------------------------------------- the rows' index arithmetic (host and device)
// the merge row y belongs to: off[k] <= y < off[k + 1], off ascending, DM_NONE past the last merge
HB_HD int dm_merge_of(const int (&off)[DM_MAX_MERGES], int y) {
    int k = 0;
#pragma unroll
    for (int q = 1; q < DM_MAX_MERGES; q++) k += y >= off[q] ? 1 : 0;
    return k;
}
// field[k] by selects: the struct stays where kernel arguments live
HB_HD int dm_pick(const int (&field)[DM_MAX_MERGES], int k) {
    int v = field[0];
#pragma unroll
    for (int q = 1; q < DM_MAX_MERGES; q++) v = q == k ? field[q] : v;
    return v;
}

// ---------------------------------------------------------------- per-element bodies (host and device)
// row r of the vector of a width-1 group: (1 - b, b)
template <int NL, int NW> HB_HD void dm_leaf_elem(uint32_t (&o)[NW], int r, const uint32_t (&bw)[NW], const FpParams<NL> &P) {
    uint32_t b[NL], one[NL], nb[NL];
    unpack<NL, NW>(b, bw);
    small_digits<NL>(one, 1);
    fp_sub<NL>(nb, one, b, P);
#pragma unroll
    for (int q = 0; q < NL; q++) nb[q] = r ? b[q] : nb[q];
    pack<NL, NW>(o, nb);
}

// ---------------------------------------------------------------- the steps' rows (host and device, over a memory policy: hb_rows.hpp)
struct DmArgs { const uint32_t *bits, *groups_in, *opened, *ta, *tab; uint32_t *out; DmLevel L; };

// m = 1: out (2, count) = (1 - b, b)
struct DmLeavesRow {
    template <int NL, int NW, class Mem>
    HB_HD static void run(const DmArgs &A, int y, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
        uint32_t bw[NW], ow[NW];
        mem.load(bw, A.bits, i);
        dm_leaf_elem<NL, NW>(ow, y, bw, P);
        mem.store(A.out, (int64_t)y * count + i, ow);
    }
};

// row y of the level's array to open
struct DmMaskRow {
    template <int NL, int NW, class Mem>
    HB_HD static void run(const DmArgs &A, int y, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
        const int k = dm_merge_of(A.L.open_off, y), wl = dm_pick(A.L.wl, k);
        int r = y - dm_pick(A.L.open_off, k);
        const bool high = r >= (1 << wl);
        r -= high ? (1 << wl) : 0;
        const int w = high ? dm_pick(A.L.wh, k) : wl, row = high ? dm_pick(A.L.hi_row, k) : dm_pick(A.L.lo_row, k);
        uint32_t xw[NW], aw[NW], ow[NW];
        if (w == 1) {
            mem.load(xw, A.bits, (int64_t)row * count + i);
            dm_leaf_elem<NL, NW>(xw, r, xw, P);
        } else {
            mem.once(xw, A.groups_in, (int64_t)(row + r) * count + i);
        }
        mem.load(aw, A.ta, (int64_t)y * count + i);
        diff_elem<NL, NW>(ow, xw, aw, P);
        mem.store(A.out, (int64_t)y * count + i, ow);
    }
};

// row y of the level's products
struct DmFinishRow {
    template <int NL, int NW, class Mem>
    HB_HD static void run(const DmArgs &A, int y, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
        product<NL, NW>(A.opened, A.ta, A.tab, A.out, A.L, y, i, count, mem, P);
    }
    // what is only read is apart from the output: __restrict__ (pointers in an argument struct do not carry it)
    template <int NL, int NW, class Mem>
    HB_HD static void product(const uint32_t *__restrict__ opened, const uint32_t *__restrict__ ta, const uint32_t *__restrict__ tab, uint32_t *__restrict__ out,
                              const DmLevel &L, int y, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
        const int k = dm_merge_of(L.prod_off, y), wl = dm_pick(L.wl, k), base = dm_pick(L.open_off, k);
        const int r = y - dm_pick(L.prod_off, k), lo = r & ((1 << wl) - 1), hi = r >> wl;
        const int64_t d = base + lo, e = base + (1 << wl) + hi;
        uint32_t dw[NW], pw[NW], ew[NW], qw[NW], pqw[NW], ow[NW];
        mem.load(dw, opened, d * count + i);
        mem.load(pw, ta, d * count + i);
        mem.load(ew, opened, e * count + i);
        mem.load(qw, ta, e * count + i);
        mem.once(pqw, tab, (int64_t)y * count + i);
        ew_beaver_elem<NL, NW>(ow, dw, ew, pw, qw, pqw, P);
        mem.store(out, ((int64_t)L.out_row + y) * count + i, ow);
    }
};

// ---------------------------------------------------------------- host side: what the steps refuse, and the step functions (hb_rows.hpp)
// A step function is the checks, the Args fill and the row count, run with a DeviceRun by the entry point and with a HostRun by
// hb_selftest_demux.
static bool dm_m_ok(int m) { return m >= 1 && m <= DM_MAX_BITS; }
static bool dm_level_ok(int m, int level) { return level >= 0 && level < dm_levels(m); }

// bytes of `count` elements a row, or -1 where 2^12 rows of them overflow
static int64_t dm_row_bytes(int64_t count, int64_t elem_bytes) {
    int64_t row;
    if (__builtin_mul_overflow(count, elem_bytes, &row) || row > INT64_MAX >> (DM_MAX_BITS + 1)) return -1;
    return row;
}

static bool dm_leaves_ok(const void *bits, const void *out, int64_t count, int64_t elem_bytes) {
    if (count < 0) return false;
    if (count == 0) return true;
    const int64_t row = dm_row_bytes(count, elem_bytes);
    if (!bits || !out || row < 0) return false;
    const RowSpan outs[1] = {{out, 2}}, ins[1] = {{bits, 1}};
    return outputs_apart(outs, 1, ins, 1, row);
}

// groups is looked at where a factor of the level is a stored group; level 0 reads bit planes alone
static bool dm_mask_ok(const void *bits, const void *groups, const void *ta, const void *out, int m, const DmLevel &D, int64_t count, int64_t elem_bytes) {
    if (count < 0) return false;
    if (count == 0) return true;
    bool stored = false, planes = false;
    for (int k = 0; k < D.n; k++) {
        stored = stored || D.wl[k] > 1 || D.wh[k] > 1;
        planes = planes || D.wl[k] == 1 || D.wh[k] == 1;
    }
    const int64_t row = dm_row_bytes(count, elem_bytes);
    if (!ta || !out || (stored && !groups) || (planes && !bits) || row < 0) return false;
    const RowSpan outs[1] = {{out, D.opened}}, ins[3] = {{planes ? bits : nullptr, m}, {stored ? groups : nullptr, dm_group_rows(m)}, {ta, D.opened}};
    return outputs_apart(outs, 1, ins, 3, row);
}

static bool dm_finish_ok(const void *opened, const void *ta, const void *tab, const void *groups, int m, const DmLevel &D, int64_t count, int64_t elem_bytes) {
    if (count < 0) return false;
    if (count == 0) return true;
    const int64_t row = dm_row_bytes(count, elem_bytes);
    if (!opened || !ta || !tab || !groups || row < 0) return false;
    const RowSpan outs[1] = {{groups, dm_group_rows(m)}}, ins[3] = {{opened, D.opened}, {ta, D.opened}, {tab, D.products}};
    return outputs_apart(outs, 1, ins, 3, row);
}

template <class Run> static int demux_leaves_step(const Run &run, const uint64_t *bits, uint64_t *out, int64_t count) {
    if (!dm_leaves_ok(bits, out, count, run.elem_bytes())) return run.fail(HB_ERR_BAD_ARG, "hb_demux_leaves: null operand, count < 0, or out not an array of its own");
    if (count == 0) return HB_OK;
    DmArgs A{};
    A.bits = u32(bits); A.out = u32(out);
    return run.template rows<DmLeavesRow>(A, 2, count);
}

template <class Run> static int demux_mask_step(const Run &run, const uint64_t *bits, const uint64_t *groups, int m, int level, const uint64_t *ta, uint64_t *out,
                                                int64_t count) {
    if (!dm_m_ok(m)) return run.fail(HB_ERR_BAD_ARG, "hb_demux_mask: needs 1 <= m <= 12");
    if (!dm_level_ok(m, level)) return run.fail(HB_ERR_BAD_ARG, "hb_demux_mask: no such level");
    DmArgs A{};
    dm_plan(m, level, A.L);
    if (!dm_mask_ok(bits, groups, ta, out, m, A.L, count, run.elem_bytes()))
        return run.fail(HB_ERR_BAD_ARG, "hb_demux_mask: null operand, count < 0, or out not an array of its own");
    if (count == 0) return HB_OK;
    A.bits = u32(bits); A.groups_in = u32(groups); A.ta = u32(ta); A.out = u32(out);
    return run.template rows<DmMaskRow>(A, A.L.opened, count);
}

template <class Run> static int demux_finish_step(const Run &run, const uint64_t *opened, const uint64_t *ta, const uint64_t *tab, int m, int level, uint64_t *groups,
                                                  int64_t count) {
    if (!dm_m_ok(m)) return run.fail(HB_ERR_BAD_ARG, "hb_demux_finish: needs 1 <= m <= 12");
    if (!dm_level_ok(m, level)) return run.fail(HB_ERR_BAD_ARG, "hb_demux_finish: no such level");
    DmArgs A{};
    dm_plan(m, level, A.L);
    if (!dm_finish_ok(opened, ta, tab, groups, m, A.L, count, run.elem_bytes()))
        return run.fail(HB_ERR_BAD_ARG, "hb_demux_finish: null operand, count < 0, or groups not an array of its own");
    if (count == 0) return HB_OK;
    A.opened = u32(opened); A.ta = u32(ta); A.tab = u32(tab); A.out = u32(groups);
    return run.template rows<DmFinishRow>(A, A.L.products, count);
}

}  // namespace hb

extern "C" {

int hb_demux_leaves(hb_ctx *ctx, const uint64_t *bits_dev, uint64_t *out_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : demux_leaves_step(DeviceRun{ctx, (hipStream_t)stream, "hb_demux_leaves"}, bits_dev, out_dev, count);
}

int hb_demux_mask(hb_ctx *ctx, const uint64_t *bits_dev, const uint64_t *groups_dev, int m, int level, const uint64_t *ta_dev, uint64_t *out_dev, int64_t count,
                  void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : demux_mask_step(DeviceRun{ctx, (hipStream_t)stream, "hb_demux_mask"}, bits_dev, groups_dev, m, level, ta_dev, out_dev, count);
}

int hb_demux_finish(hb_ctx *ctx, const uint64_t *opened_dev, const uint64_t *ta_dev, const uint64_t *tab_dev, int m, int level, uint64_t *groups_dev, int64_t count,
                    void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : demux_finish_step(DeviceRun{ctx, (hipStream_t)stream, "hb_demux_finish"}, opened_dev, ta_dev, tab_dev, m, level, groups_dev, count);
}

// params: m, level
int hb_selftest_demux(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *operands, const int64_t *params, uint64_t *const *outs, int64_t count) {
    if (!p_limbs || !operands || !params || !outs || (n_limbs != 1 && n_limbs != 4)) return HB_ERR_BAD_ARG;
    for (int i = 0; i < 2; i++) if (params[i] < -(1 << 30) || params[i] > (1 << 30)) return HB_ERR_BAD_ARG;
    const HostRun run = {p_limbs, n_limbs};
    const int m = (int)params[0], level = (int)params[1];
    switch (what) {
    case HB_DEMUX_SELFTEST_LEAVES: return demux_leaves_step(run, operands[0], outs[0], count);
    case HB_DEMUX_SELFTEST_MASK: return demux_mask_step(run, operands[0], operands[1], m, level, operands[2], outs[0], count);
    case HB_DEMUX_SELFTEST_FINISH: return demux_finish_step(run, operands[0], operands[1], operands[2], m, level, outs[0], count);
    default: return HB_ERR_BAD_ARG;
    }
}

}  // extern "C"

// hb_fxexp.hip -- base-2 and natural exponential of shared fixed-point numbers (honeybadgermpc_amd/progs/fixedpoint_exp.py; DESIGN.md
// section 3ac), for arrays of values: the steps that hb_demux.hip and hb_div.hip do not already have.  2^x is multiplicative over the
// bits of x, so it is a product of a few PUBLIC table reads at one-hot vectors of groups of those bits.  (The reference has no
// exponential: nothing here is a translation.)  Everything between two opens of the product tree is ONE launch.
//
// FxExpLookupRow    blockIdx.y = a group of bits whose LAST demultiplexer level was just opened.  That level merges a low factor of wl
//                   bits and a high one of wh bits: the one-hot entry y = hi 2^wl + lo is the Beaver product d_lo e_hi + d_lo Q_hi + e_hi P_lo
//                   + PQ_y (d, e the opened rows, P, Q, PQ the outer-product triple, hb_demux.hip's numbering), and the group's factor is
//                   F = sum_y T_y (that product) for the group's public table T.  The 2^(wl + wh) one-hot rows are never written:
//                       F = sum_y T_y PQ_y + sum_hi ((e_hi + Q_hi) sum_lo T_y d_lo + e_hi sum_lo T_y P_lo)
//                   so an entry costs three products by the wave-uniform constant T_y (its digits live in SGPRs), accumulated in 64-bit
//                   columns, and a high index two full products.  A column takes NL * Lazy::GROUP = 63 digit products before carries
//                   must move; a constant of n digits spends n of them, so a table of 3-digit constants (at most s + 1 <= 87 bits: the
//                   protocol's) is reduced once every 21 entries, a table of arbitrary residues every 7.  An entry that is 0 (the whole
//                   sign half of the integer group's table) is skipped before its PQ is read.
//                   A group of width 1 (wl = 1, wh = 0) has no level: F = T_0 + (T_1 - T_0) b from its bit plane.
//                   Writes kept[slot] = F and, for slot < 2 pairs, the factor's row of the first tree level's masked pairs,
//                   masked[slot] = F - (slot even ? nxt_a : nxt_b)[slot / 2]: that row depends on no other group.
// FxExpProductsRow  blockIdx.y = a product of a tree level (1 .. 128; hb_div_product_step(HB_DIV_TRUNC) stops at two): the Beaver combine
//                   and the truncation mask of the product, masked = v + 2^(width-1) + r1 + 2^m r2 and s = v + r1 kept.
// FxExpTreeRow      after the open of the masked truncations, blockIdx.y = a pair of the next level: value j < rows is t_j = (s_j -
//                   (opened_j mod 2^m)) 2^(-m), value `rows` the carried factor if there is one; pair q is masked against the next
//                   level's triple, rows 2q, 2q + 1 = v_2q - ta[q], v_(2q+1) - tb[q], and an odd last value is kept.
// The last truncation is hb_div_trunc_step(HB_DIV_T_RESULT) as it stands.
//
// Operands and results are packed canonical residues.  A step's row is an HB_HD function over a memory policy (hb_rows.hpp): k_rows runs
// it on the device, host_rows the very same row in hb_selftest_fxexp, and each step is ONE step function behind both.
//
// Launch shape (all kernels): 256-thread workgroups, one element a thread in x, the group / product / pair in blockIdx.y.  No LDS, no
// grid stride, one launch a call.  PQ, the bit planes, the triples of the next level and what was opened for a truncation are read once
// and take the non-temporal loads; the rows of d, e, P, Q are read again by every high or low index and take the plain ones (at most
// 2^wl + 2^wh <= 272 rows a group: they stay in cache while the thread walks); a table entry is one address a wave (same).
// Compiler's report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; scratch = 0 bytes for every kernel):
//   FxExpLookupRow<9, 8>     163 VGPRs: 3 waves a SIMD                          FxExpLookupRow<3, 2>     56 VGPRs: 8 waves
//   FxExpProductsRow<9, 8>   90 VGPRs: 5 waves                                  FxExpProductsRow<3, 2>   42 VGPRs: 8 waves
//   FxExpTreeRow<9, 8>       49 VGPRs: 8 waves                                  FxExpTreeRow<3, 2>       16 VGPRs: 8 waves
// (FxExpLookupRow holds three sets of 18 64-bit columns, 108 registers, beside four running sums; the table's digits are in SGPRs.)
// (Measured, DESIGN.md section 3ac: FxExpLookupRow reaches 15 % of the HBM peak at 2^16 elements and is slower than its composed form at
// 2^12, a thread walking its element's entries alone; FxExpProductsRow with ONE product is slower than hb_ew_beaver + hb_fxp_mask.)
#include "hb_common.hpp"
#include "hb_div_elem.hpp"

using namespace hb;

namespace hb {

constexpr int FXEXP_MAX_GROUPS = 8;                // a launch's group descriptors travel by value
constexpr int FXEXP_MAX_ROWS = 128;                // products of a tree level, values into the next
constexpr int FXEXP_MAX_WIDTH = 12;                // hb_demux.hip's DM_MAX_BITS
constexpr int FXEXP_DESC = 6;                      // ints a group in the entry point's descriptor array

// ---------------------------------------------------------------- per-element bodies (host and device)
// digits of d up to the highest one that is not 0 (d wave-uniform: scalar work)
template <int NL> HB_HD int fxexp_digits_used(const uint32_t (&d)[NL]) {
    int n = 0;
#pragma unroll
    for (int q = 0; q < NL; q++) n = d[q] ? q + 1 : n;
    return n;
}

// F = sum_y T_y (d_lo e_hi + d_lo Q_hi + e_hi P_lo + PQ_y), y = hi 2^wl + lo.  opened(w, r) and ta(w, r) load row r of the group's opened
// array and of its triple's factors (2^wl low rows, then 2^wh high ones), tab(w, y) the triple's product y, table(w, y) the canonical T_y.
// accA = sum T PQ / R, accB = sum_hi ((e + Q) (sum T d / R) + e (sum T P / R)) / R; every partial sum is reduced below p before it is
// used.  The two-product combine is ew_beaver_elem's: e + Q digit by digit with no carry, columns below 4 NL 2^58 + 2^35, value < 3 p^2.
template <int NL, int NW, class Opened, class Ta, class Tab, class Table>
HB_HD void fxexp_lookup_elem(uint32_t (&fw)[NW], Opened &&opened, Ta &&ta, Tab &&tab, Table &&table, int wl, int wh, const FpParams<NL> &P) {
    constexpr int CAP = NL * Lazy<NL>::GROUP;
    uint32_t accA[NL], accB[NL], s2[NL], s3[NL], T[NL], x[NL], r[NL], t[NL], w[NW];
    uint64_t c1[2 * NL], c2[2 * NL], c3[2 * NL];
#pragma unroll
    for (int q = 0; q < NL; q++) { accA[q] = 0u; accB[q] = 0u; }
    const auto flush = [&]() {
        finish<NL>(r, c1, P, 1); fp_add<NL>(t, accA, r, P); fp_set<NL>(accA, t);
        finish<NL>(r, c2, P, 1); fp_add<NL>(t, s2, r, P); fp_set<NL>(s2, t);
        finish<NL>(r, c3, P, 1); fp_add<NL>(t, s3, r, P); fp_set<NL>(s3, t);
        col_zero(c1); col_zero(c2); col_zero(c3);
    };
    for (int hi = 0; hi < (1 << wh); hi++) {
#pragma unroll
        for (int q = 0; q < NL; q++) { s2[q] = 0u; s3[q] = 0u; }
        col_zero(c1); col_zero(c2); col_zero(c3);
        int load = 0;
        for (int lo = 0; lo < (1 << wl); lo++) {
            const int y = (hi << wl) | lo;
            table(w, y);
            unpack<NL, NW>(T, w);
            const int na = fxexp_digits_used<NL>(T);
            if (na == 0) continue;
            if (load + na > CAP) { flush(); load = 0; }
            load += na;
            tab(w, y);
            unpack<NL, NW>(x, w);
            mac_short<NL>(c1, T, na, x);
            ta(w, lo);
            unpack<NL, NW>(x, w);
            mac_short<NL>(c2, T, na, x);
            opened(w, lo);
            unpack<NL, NW>(x, w);
            mac_short<NL>(c3, T, na, x);
        }
        if (load == 0) continue;                                                // a high index whose entries are all 0
        flush();
        opened(w, (1 << wl) + hi);
        unpack<NL, NW>(x, w);
        ta(w, (1 << wl) + hi);
        unpack<NL, NW>(t, w);
#pragma unroll
        for (int q = 0; q < NL; q++) t[q] += x[q];
        mac<NL>(c1, t, s3);
        mac<NL>(c1, x, s2);
        redc<NL>(r, c1, P);
        cond_sub_p<NL>(r, P);
        fp_add<NL>(t, accB, r, P);
        fp_set<NL>(accB, t);
    }
    mont_mul<NL>(t, P.r2, accA, P);
    mont_mul<NL>(r, P.r2, accB, P);
    mont_mul<NL>(x, P.r2, r, P);
    fp_add<NL>(r, t, x, P);
    pack<NL, NW>(fw, r);
}

// a group of width 1: F = T_0 + (T_1 - T_0) b
template <int NL, int NW>
HB_HD void fxexp_linear_elem(uint32_t (&fw)[NW], const uint32_t (&bw)[NW], const uint32_t (&t0w)[NW], const uint32_t (&t1w)[NW], const FpParams<NL> &P) {
    uint32_t b[NL], t0[NL], t1[NL], d[NL], r[NL];
    unpack<NL, NW>(b, bw);
    unpack<NL, NW>(t0, t0w);
    unpack<NL, NW>(t1, t1w);
    fp_sub<NL>(d, t1, t0, P);
    mont_mul<NL>(r, d, b, P);
    mont_mul<NL>(d, P.r2, r, P);
    fp_add<NL>(r, d, t0, P);
    pack<NL, NW>(fw, r);
}

// ---------------------------------------------------------------- the steps' rows (host and device, over a memory policy)
// group g < n: its last merge (wl, wh) -- (1, 0): a width-1 group --, the first row of its opened array and triple factors (width 1: its
// bit plane), of its triple products and of its table, and the factor's slot
struct FxExpGroups { int n, wl[FXEXP_MAX_GROUPS], wh[FXEXP_MAX_GROUPS], open_off[FXEXP_MAX_GROUPS], prod_off[FXEXP_MAX_GROUPS], table_off[FXEXP_MAX_GROUPS], slot[FXEXP_MAX_GROUPS]; };
struct FxExpLookupArgs { const uint32_t *bits, *opened, *ta, *tab, *tables, *nxt_a, *nxt_b; uint32_t *masked, *kept; int pairs; FxExpGroups G; };

// field[g] by selects: the struct stays where kernel arguments live (g is blockIdx.y: scalar work)
HB_HD int fxexp_pick(const int (&field)[FXEXP_MAX_GROUPS], int g) {
    int v = field[0];
#pragma unroll
    for (int q = 1; q < FXEXP_MAX_GROUPS; q++) v = q == g ? field[q] : v;
    return v;
}

struct FxExpLookupRow {
template <int NL, int NW, class Mem>
HB_HD static void run(const FxExpLookupArgs &A, int g, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
    const int wl = fxexp_pick(A.G.wl, g), wh = fxexp_pick(A.G.wh, g), slot = fxexp_pick(A.G.slot, g);
    const int64_t oo = fxexp_pick(A.G.open_off, g), po = fxexp_pick(A.G.prod_off, g), to = fxexp_pick(A.G.table_off, g);
    uint32_t fw[NW], aw[NW], o[NW];
    if (wh == 0) {
        uint32_t bw[NW], t0[NW], t1[NW];
        mem.once(bw, A.bits, oo * count + i);
        mem.same(t0, A.tables + to * NW);
        mem.same(t1, A.tables + (to + 1) * NW);
        fxexp_linear_elem<NL, NW>(fw, bw, t0, t1, P);
    } else {
        lookup<NL, NW>(fw, A.opened + oo * count * NW, A.ta + oo * count * NW, A.tab + po * count * NW, A.tables + to * NW, wl, wh, i, count, mem, P);
    }
    mem.store(A.kept, (int64_t)slot * count + i, fw);
    if (slot < 2 * A.pairs) {
        mem.once(aw, (slot & 1) ? A.nxt_b : A.nxt_a, (int64_t)(slot >> 1) * count + i);
        diff_elem<NL, NW>(o, fw, aw, P);
        mem.store(A.masked, (int64_t)slot * count + i, o);
    }
}
// what is only read is apart from the outputs: __restrict__ (pointers in an argument struct do not carry it)
template <int NL, int NW, class Mem>
HB_HD static void lookup(uint32_t (&fw)[NW], const uint32_t *__restrict__ opened, const uint32_t *__restrict__ ta, const uint32_t *__restrict__ tab,
                         const uint32_t *__restrict__ table, int wl, int wh, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
    fxexp_lookup_elem<NL, NW>(fw, [&](uint32_t (&w)[NW], int r) { mem.load(w, opened, (int64_t)r * count + i); },
                              [&](uint32_t (&w)[NW], int r) { mem.load(w, ta, (int64_t)r * count + i); },
                              [&](uint32_t (&w)[NW], int y) { mem.once(w, tab, (int64_t)y * count + i); },
                              [&](uint32_t (&w)[NW], int y) { mem.same(w, table + (int64_t)y * NW); }, wl, wh, P);
}
};

template <int NL> struct FxExpProductsArgs {
    const uint32_t *opened, *ta, *tb, *tab, *bits;
    uint32_t *masked, *s;
    int nbits, m;
    FpConst<NL> half;
};

struct FxExpProductsRow {
template <int NL, int NW, class Mem>
HB_HD static void run(const FxExpProductsArgs<NL> &A, int r, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
    uint32_t dw[NW], ew[NW], aw[NW], bw[NW], abw[NW], pw[NW], o0[NW], o1[NW];
    mem.once(dw, A.opened, (int64_t)(2 * r) * count + i); mem.once(ew, A.opened, (int64_t)(2 * r + 1) * count + i);
    mem.once(aw, A.ta, (int64_t)r * count + i); mem.once(bw, A.tb, (int64_t)r * count + i); mem.once(abw, A.tab, (int64_t)r * count + i);
    ew_beaver_elem<NL, NW>(pw, dw, ew, aw, bw, abw, P);
    const uint32_t *planes = A.bits + (int64_t)r * A.nbits * count * NW;
    div_trunc_mask_elem<NL, NW>(o0, o1, pw, [&](uint32_t (&w)[NW], int row) { mem.once(w, planes, (int64_t)row * count + i); }, A.nbits, A.m, A.half.d, P);
    mem.store(A.masked, (int64_t)r * count + i, o0);
    mem.store(A.s, (int64_t)r * count + i, o1);
}
};

template <int NL> struct FxExpTreeArgs {
    const uint32_t *opened, *s, *carry, *ta, *tb;
    uint32_t *masked, *kept;
    int rows, values, m;
    FpConst<NL> invm;
};

struct FxExpTreeRow {
template <int NL, int NW, class Mem>
HB_HD static void value(uint32_t (&v)[NW], const FxExpTreeArgs<NL> &A, int j, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
    if (j < A.rows) {
        uint32_t sw[NW], cw[NW];
        mem.once(sw, A.s, (int64_t)j * count + i); mem.once(cw, A.opened, (int64_t)j * count + i);
        div_trunc_elem<NL, NW>(v, sw, cw, A.m, A.invm.d, P);
    } else {
        mem.once(v, A.carry, i);
    }
}
template <int NL, int NW, class Mem>
HB_HD static void run(const FxExpTreeArgs<NL> &A, int q, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
    uint32_t v[NW], aw[NW], o[NW];
    value<NL, NW>(v, A, 2 * q, i, count, mem, P);
    if (2 * q + 1 >= A.values) { mem.store(A.kept, i, v); return; }           // the odd one out
    mem.once(aw, A.ta, (int64_t)q * count + i);
    diff_elem<NL, NW>(o, v, aw, P);
    mem.store(A.masked, (int64_t)(2 * q) * count + i, o);
    value<NL, NW>(v, A, 2 * q + 1, i, count, mem, P);
    mem.once(aw, A.tb, (int64_t)q * count + i);
    diff_elem<NL, NW>(o, v, aw, P);
    mem.store(A.masked, (int64_t)(2 * q + 1) * count + i, o);
}
};

// ---------------------------------------------------------------- host side
// One step function a step (hb_rows.hpp): a DeviceRun in the entry point, a HostRun in hb_selftest_fxexp.
// desc: FXEXP_DESC ints a group -- wl, wh, open_off, prod_off, table_off, slot.  Fills G and the row extents the overlap check needs;
// false for a shape the step does not take (two groups in one slot among them: both would write one row).
static bool fxexp_groups(FxExpGroups &G, int n_groups, const int *desc, int kept_rows, int64_t &bit_rows, int64_t &open_rows, int64_t &prod_rows, int64_t &table_rows) {
    if (n_groups < 1 || n_groups > FXEXP_MAX_GROUPS || kept_rows < 1 || kept_rows > 2 * FXEXP_MAX_ROWS + 1) return false;
    G = FxExpGroups{};
    G.n = n_groups;
    bit_rows = open_rows = prod_rows = table_rows = 0;
    for (int g = 0; g < n_groups; g++) {
        const int *d = desc + FXEXP_DESC * g;
        const int wl = d[0], wh = d[1], oo = d[2], po = d[3], to = d[4], slot = d[5];
        const bool linear = wl == 1 && wh == 0;
        if (!linear && (wl < 1 || wh < 1 || wl + wh > FXEXP_MAX_WIDTH)) return false;
        if (oo < 0 || po < 0 || to < 0 || oo > (1 << 20) || po > (1 << 20) || to > (1 << 20) || slot < 0 || slot >= kept_rows) return false;
        for (int h = 0; h < g; h++) if (G.slot[h] == slot) return false;
        G.wl[g] = wl; G.wh[g] = wh; G.open_off[g] = oo; G.prod_off[g] = po; G.table_off[g] = to; G.slot[g] = slot;
        const int64_t entries = (int64_t)1 << (wl + wh);
        if (linear) { if (oo + 1 > bit_rows) bit_rows = oo + 1; }
        else {
            if (oo + (1 << wl) + (1 << wh) > open_rows) open_rows = oo + (1 << wl) + (1 << wh);
            if (po + entries > prod_rows) prod_rows = po + entries;
        }
        if (to + entries > table_rows) table_rows = to + entries;
    }
    return true;
}

template <class Run> static int fxexp_finish_lookup_mask_step(const Run &run, const uint64_t *bits, const uint64_t *opened, const uint64_t *ta, const uint64_t *tab,
                                                              const uint64_t *tables, int n_groups, const int *desc, const uint64_t *nxt_a, const uint64_t *nxt_b,
                                                              int pairs, uint64_t *masked, uint64_t *kept, int kept_rows, int64_t count) {
    if (count < 0 || !desc) return HB_ERR_BAD_ARG;
    FxExpLookupArgs A{};
    int64_t bit_rows, open_rows, prod_rows, table_rows;
    if (!fxexp_groups(A.G, n_groups, desc, kept_rows, bit_rows, open_rows, prod_rows, table_rows) || pairs < 0 || pairs > FXEXP_MAX_ROWS)
        return run.fail(HB_ERR_BAD_ARG, "hb_fxexp_finish_lookup_mask: needs 1 .. 8 groups in slots of their own below kept_rows, merges with 1 <= wl, wh and wl + wh <= 12 "
                                        "(or wl = 1, wh = 0: a group of one bit), and 0 <= pairs <= 128");
    if (count == 0) return HB_OK;
    bool masks = false;
    for (int g = 0; g < n_groups; g++) masks = masks || A.G.slot[g] < 2 * pairs;
    if (!tables || !kept || (bit_rows && !bits) || (open_rows && (!opened || !ta || !tab)) || (masks && (!nxt_a || !nxt_b || !masked))) return HB_ERR_BAD_ARG;
    if (count > INT64_MAX >> 24) return HB_ERR_BAD_ARG;
    const int64_t rb = run.elem_bytes() * count;
    const RowSpan outs[2] = {{masks ? masked : nullptr, 2 * pairs}, {kept, kept_rows}};
    const RowSpan ins[6] = {{bit_rows ? bits : nullptr, bit_rows}, {open_rows ? opened : nullptr, open_rows}, {open_rows ? ta : nullptr, open_rows},
                            {open_rows ? tab : nullptr, prod_rows}, {masks ? nxt_a : nullptr, pairs}, {masks ? nxt_b : nullptr, pairs}};
    if (!outputs_apart(outs, 2, ins, 6, rb) || overlap(tables, run.elem_bytes() * table_rows, kept, kept_rows * rb) ||
        (masks && overlap(tables, run.elem_bytes() * table_rows, masked, 2 * pairs * rb)))
        return run.fail(HB_ERR_BAD_ARG, "hb_fxexp_finish_lookup_mask: masked and kept are arrays of their own");
    A.bits = u32(bits); A.opened = u32(opened); A.ta = u32(ta); A.tab = u32(tab); A.tables = u32(tables); A.nxt_a = u32(nxt_a); A.nxt_b = u32(nxt_b);
    A.masked = u32(masked); A.kept = u32(kept); A.pairs = pairs;
    return run.template rows<FxExpLookupRow>(A, n_groups, count);
}

template <class Run> static int fxexp_products_trunc_step(const Run &run, int products, const uint64_t *opened, const uint64_t *ta, const uint64_t *tb, const uint64_t *tab,
                                                          const uint64_t *bits, int width, int m, int kappa, uint64_t *masked, uint64_t *s, int64_t count) {
    if (count < 0) return HB_ERR_BAD_ARG;
    if (products < 1 || products > FXEXP_MAX_ROWS || !fxp_params_ok(run.bits(), width, m, kappa))
        return run.fail(HB_ERR_BAD_ARG, "hb_fxexp_products_trunc: needs 1 <= products <= 128 and a truncation the modulus has room for");
    if (count > 0 && (!opened || !ta || !tb || !tab || !bits || !masked || !s)) return HB_ERR_BAD_ARG;
    if (count > INT64_MAX >> 24) return HB_ERR_BAD_ARG;
    const int64_t rb = run.elem_bytes() * count;
    const RowSpan outs[2] = {{masked, products}, {s, products}};
    const RowSpan ins[5] = {{opened, 2 * products}, {ta, products}, {tb, products}, {tab, products}, {bits, (int64_t)products * (width + kappa)}};
    if (count > 0 && !outputs_apart(outs, 2, ins, 5, rb)) return run.fail(HB_ERR_BAD_ARG, "hb_fxexp_products_trunc: masked and s are arrays of their own");
    return run.template rows<FxExpProductsRow, FxExpProductsArgs>([&](auto &A, const auto &P) {
        A.opened = u32(opened); A.ta = u32(ta); A.tb = u32(tb); A.tab = u32(tab); A.bits = u32(bits); A.masked = u32(masked); A.s = u32(s);
        A.nbits = width + kappa; A.m = m;
        constexpr int NL = sizeof(A.half.d) / sizeof(uint32_t);
        fxp_pow2<NL>(A.half.d, width - 1, false, P);
        return true;
    }, products, count);
}

template <class Run> static int fxexp_tree_step(const Run &run, int rows, const uint64_t *opened, const uint64_t *s, int m, const uint64_t *inv2m_host, const uint64_t *carry,
                                                const uint64_t *ta, const uint64_t *tb, uint64_t *masked, uint64_t *kept, int64_t count) {
    if (count < 0) return HB_ERR_BAD_ARG;
    if (rows < 1 || rows > FXEXP_MAX_ROWS || !fxp_m_ok(run.bits(), m))
        return run.fail(HB_ERR_BAD_ARG, "hb_fxexp_tree_step: needs 1 <= rows <= 128 and 0 < m <= bits(p) - 2");
    if (!inv2m_host) return HB_ERR_BAD_ARG;
    const int values = rows + (carry ? 1 : 0), pairs = values / 2, odd = values & 1;
    if (count > 0 && (!opened || !s || (pairs && (!ta || !tb || !masked)) || (odd && !kept))) return HB_ERR_BAD_ARG;
    if (count > INT64_MAX >> 24) return HB_ERR_BAD_ARG;
    const int64_t rb = run.elem_bytes() * count;
    const RowSpan outs[2] = {{pairs ? masked : nullptr, 2 * pairs}, {odd ? kept : nullptr, 1}};
    const RowSpan ins[5] = {{opened, rows}, {s, rows}, {carry, 1}, {pairs ? ta : nullptr, pairs}, {pairs ? tb : nullptr, pairs}};
    if (count > 0 && !outputs_apart(outs, 2, ins, 5, rb)) return run.fail(HB_ERR_BAD_ARG, "hb_fxexp_tree_step: masked and kept are arrays of their own");
    const int rc = run.template rows<FxExpTreeRow, FxExpTreeArgs>([&](auto &A, const auto &P) {
        A.opened = u32(opened); A.s = u32(s); A.carry = u32(carry); A.ta = u32(ta); A.tb = u32(tb); A.masked = u32(masked); A.kept = u32(kept);
        A.rows = rows; A.values = values; A.m = m;
        constexpr int NL = sizeof(A.invm.d) / sizeof(uint32_t);
        return host_mont<NL, words_of(NL)>(A.invm.d, P, inv2m_host);
    }, pairs + odd, count);
    return rc == HB_ERR_BAD_ARG ? run.fail(rc, "hb_fxexp_tree_step: 2^(-m) is not below the modulus") : rc;
}

}  // namespace hb

extern "C" {

int hb_fxexp_finish_lookup_mask(hb_ctx *ctx, const uint64_t *bits_dev, const uint64_t *opened_dev, const uint64_t *ta_dev, const uint64_t *tab_dev, const uint64_t *tables_dev,
                                int n_groups, const int *desc_host, const uint64_t *nxt_a_dev, const uint64_t *nxt_b_dev, int pairs, uint64_t *masked_dev, uint64_t *kept_dev,
                                int kept_rows, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : fxexp_finish_lookup_mask_step(DeviceRun{ctx, (hipStream_t)stream, "hb_fxexp_finish_lookup_mask"}, bits_dev, opened_dev, ta_dev, tab_dev,
                                                                 tables_dev, n_groups, desc_host, nxt_a_dev, nxt_b_dev, pairs, masked_dev, kept_dev, kept_rows, count);
}

int hb_fxexp_products_trunc(hb_ctx *ctx, int products, const uint64_t *opened_dev, const uint64_t *ta_dev, const uint64_t *tb_dev, const uint64_t *tab_dev,
                            const uint64_t *bits_dev, int width, int m, int kappa, uint64_t *masked_dev, uint64_t *s_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : fxexp_products_trunc_step(DeviceRun{ctx, (hipStream_t)stream, "hb_fxexp_products_trunc"}, products, opened_dev, ta_dev, tb_dev, tab_dev,
                                                             bits_dev, width, m, kappa, masked_dev, s_dev, count);
}

int hb_fxexp_tree_step(hb_ctx *ctx, int rows, const uint64_t *opened_dev, const uint64_t *s_dev, int m, const uint64_t *inv2m_host, const uint64_t *carry_dev,
                       const uint64_t *ta_dev, const uint64_t *tb_dev, uint64_t *masked_dev, uint64_t *kept_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : fxexp_tree_step(DeviceRun{ctx, (hipStream_t)stream, "hb_fxexp_tree_step"}, rows, opened_dev, s_dev, m, inv2m_host, carry_dev, ta_dev, tb_dev,
                                                   masked_dev, kept_dev, count);
}

// params: as the header lists them for each step
int hb_selftest_fxexp(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *ops, const int64_t *params, uint64_t *const *outs, int64_t count) {
    if (!p_limbs || !ops || !params || !outs || (n_limbs != 1 && n_limbs != 4)) return HB_ERR_BAD_ARG;
    const HostRun run = {p_limbs, n_limbs};
    switch (what) {
    case HB_FXEXP_SELFTEST_FINISH_LOOKUP_MASK: {                                // n_groups, pairs, kept_rows, then FXEXP_DESC ints a group
        int desc[FXEXP_DESC * FXEXP_MAX_GROUPS] = {0};
        if (params[0] < 1 || params[0] > FXEXP_MAX_GROUPS) return HB_ERR_BAD_ARG;
        for (int i = 0; i < 3 + FXEXP_DESC * (int)params[0]; i++) if (params[i] < -(1 << 30) || params[i] > (1 << 30)) return HB_ERR_BAD_ARG;
        for (int i = 0; i < FXEXP_DESC * (int)params[0]; i++) desc[i] = (int)params[3 + i];
        return fxexp_finish_lookup_mask_step(run, ops[0], ops[1], ops[2], ops[3], ops[4], (int)params[0], desc, ops[5], ops[6], (int)params[1], outs[0], outs[1],
                                             (int)params[2], count);
    }
    case HB_FXEXP_SELFTEST_PRODUCTS_TRUNC:                                      // products, width, m, kappa
        for (int i = 0; i < 4; i++) if (params[i] < -(1 << 30) || params[i] > (1 << 30)) return HB_ERR_BAD_ARG;
        return fxexp_products_trunc_step(run, (int)params[0], ops[0], ops[1], ops[2], ops[3], ops[4], (int)params[1], (int)params[2], (int)params[3], outs[0], outs[1], count);
    case HB_FXEXP_SELFTEST_TREE_STEP:                                           // rows, m
        for (int i = 0; i < 2; i++) if (params[i] < -(1 << 30) || params[i] > (1 << 30)) return HB_ERR_BAD_ARG;
        return fxexp_tree_step(run, (int)params[0], ops[0], ops[1], (int)params[1], ops[2], ops[3], ops[4], ops[5], outs[0], outs[1], count);
    default: return HB_ERR_BAD_ARG;
    }
}

}  // extern "C"

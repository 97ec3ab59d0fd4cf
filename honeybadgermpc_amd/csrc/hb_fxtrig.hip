// hb_fxtrig.hip -- sine and cosine of shared fixed-point numbers (honeybadgermpc_amd/progs/fixedpoint_trig.py), for
// arrays of values: the steps that hb_demux.hip and hb_fxexp.hip do not already have.  cis(t) = cos t + i sin t is multiplicative over the
// bits of t, so the sine and cosine of an angle given in turns are a product of a few PUBLIC table reads at one-hot vectors of groups of
// its fraction bits -- a product of COMPLEX factors.  (The reference has no circular functions: nothing here is a translation.)
// Everything between two opens of the product tree is ONE launch.  hb_fxexp.hip is left as it stands; what is shared lives in headers.
//
// FxTrigLookupRow    blockIdx.y = a group of bits whose LAST demultiplexer level was just opened (hb_fxexp.hip's FxExpLookupRow has the
//                    algebra and the descriptors): the group's cos table C and, right after it, its sin table S are read through the
//                    SAME one-hot vector,
//                        F = sum_y T_y PQ_y + sum_hi ((e_hi + Q_hi) sum_lo T_y d_lo + e_hi sum_lo T_y P_lo),   T = C and T = S
//                    with each of d, e, P, Q, PQ loaded ONCE for both tables.  A high index is three sweeps over lo -- PQ, then P, then d --
//                    each into ONE pair of lazy column sets (C's and S's): two sets live, not six, so the wide field stays at the
//                    registers of hb_fxexp.hip's row (three sets, one table).  The table digits are wave-uniform (SGPRs) and read again
//                    by every sweep; the share arrays are not.
//                    Entries are SIGNED: an entry is a canonical residue; where p - T has fewer digits than T the row multiplies the
//                    NEGATED operand by p - T (the negation is NL digit subtractions beside n NL multiply-adds; deciding is scalar
//                    work), so a negative table entry costs its magnitude's digits, never the modulus' NL.  Any residue is accepted and
//                    gives the same bits either way.
//                    SPLIT: the high indices of an element are dealt round robin to `split` neighbouring lanes (1, 2, 4, 8 or 16), each
//                    forming a canonical partial (re, im), summed across the lanes by butterfly shuffles; lane 0 of the element stores.
//                    The host row sums the same partials in turn: canonical sums mod p, the same bits for every split.  The lanes of
//                    a wave then walk different entries at one time, so the split row (FxTrigLookupRowT<true>, a kernel of its own)
//                    holds an entry's digits in VGPRs, picks the sign by a select a digit and multiplies as many digits as the
//                    longest entry among the wave's lanes has; split 1 (FxTrigLookupRowT<false>) keeps the SGPR walk.
//                    A group of width 1 (wl = 1, wh = 0) has no level: F = T_0 + (T_1 - T_0) b from its bit plane.
//                    Writes kept[2 slot] = re, kept[2 slot + 1] = im and, for slot < 2 pairs, the factor's rows of the first tree level's
//                    masked operands (fxtrig_mask_value): they depend on no other group.
// FxTrigProductsRow  blockIdx.y = a complex product of a tree level (1 .. 64): its Beaver combines, the components kept, and the
//                    truncation mask of each, masked = v + 2^(width-1) + r1 + 2^m r2 and s = v + r1.
//                      mode 0 (both):  Karatsuba over THREE triples, p0 = a.re b.re, p1 = a.im b.im, p2 = (a.re + a.im)(b.re + b.im);
//                                      re = p0 - p1, im = p2 - p0 - p1, formed before truncation: two truncations a complex product
//                      mode 1 (cos):   the first TWO of them, re = p0 - p1: one truncation
//                      mode 2 (sin):   all three, im = p2 - p0 - p1: one truncation
//                    so a component kept alone is, share for share, the component the level would have kept beside the other.
// FxTrigTreeRow      after the open of the masked truncations, t_j = (s_j - (opened_j mod 2^m)) 2^(-m).  final: blockIdx.y = j, kept[j] = t_j,
//                    the results.  Otherwise blockIdx.y = a complex value -- (t_2u, t_(2u+1)), and after them the carried factor if there is
//                    one --: value u is operand u & 1 of product u / 2 of the next level and its masked rows are written in that level's
//                    mode; an odd last value is kept (two rows).
// Masked operands of product q in a mode with tp triples a product (3 or 2): triple r = tp q + t takes rows 2 r (operand a's value minus
// ta[r]) and 2 r + 1 (operand b's minus tb[r]), hb_fxexp_products_trunc's convention.  The values: re, im and (modes 0 and 2) re + im.
//
// Launch shape: hb_rows.hpp's k_rows (256-thread workgroups, one element -- for the lookup one element's lane -- a thread in x, the
// group / product / value in blockIdx.y), no LDS, no grid stride, one launch a call.
// Compiler's report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; scratch = 0 bytes for every kernel): see
// DESIGN.md section 3ae.
#include "hb_common.hpp"
#include "hb_div_elem.hpp"

using namespace hb;

namespace hb {

constexpr int FXTRIG_MAX_GROUPS = 8;               // a launch's group descriptors travel by value
constexpr int FXTRIG_MAX_PRODUCTS = 64;            // complex products of a tree level
constexpr int FXTRIG_MAX_WIDTH = 12;               // hb_demux.hip's DM_MAX_BITS
constexpr int FXTRIG_DESC = 6;                     // ints a group in the entry point's descriptor array
constexpr int FXTRIG_MAX_SPLIT = 16;               // lanes an element's entries are spread over

HB_HD int fxtrig_triples(int mode) { return mode == 1 ? 2 : 3; }
HB_HD int fxtrig_comps(int mode) { return mode == 0 ? 2 : 1; }

// ---------------------------------------------------------------- per-element bodies (host and device)
// T (wave-uniform digits of a canonical residue) -> its shorter form: T itself or, with neg set, p - T; -> the digits in use (0: T is 0)
template <int NL> HB_HD int fxtrig_magnitude(uint32_t (&T)[NL], bool &neg, const FpParams<NL> &P) {
    uint32_t M[NL];
    int n = 0, nm = 0;
    int32_t borrow = 0;
#pragma unroll
    for (int q = 0; q < NL; q++) {
        const int32_t v = (int32_t)P.p[q] - (int32_t)T[q] + borrow;
        borrow = v >> 31;
        M[q] = (uint32_t)v & DMASK;
        n = T[q] ? q + 1 : n;
        nm = M[q] ? q + 1 : nm;
    }
    neg = n > 0 && nm < n;
    if (neg) {
#pragma unroll
        for (int q = 0; q < NL; q++) T[q] = M[q];
    }
    return neg ? nm : n;
}

// the largest v among the lanes of the wave that are here, 0 <= v <= NL (the host: its own): what keeps a count of digits wave-uniform
template <int NL> HB_HD int fxtrig_wave_max(int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    int r = 0;
#pragma unroll
    for (int q = 1; q <= NL; q++) r = __any(v >= q) ? q : r;
    return r;
#else
    return v;
#endif
}

// The partial (re, im) of the high indices part, part + split, ... of one group, canonical digits.  opened(w, r) and ta(w, r) load row r of
// the group's opened array and of its triple's factors (2^wl low rows, then 2^wh high ones), tab(w, y) the triple's product y,
// table(w, e) entry e of the group's tables (C: e < 2^(wl + wh), S after it).  Sums are kept divided by R as in fxexp_lookup_elem.
// SPLIT: the lanes of a wave walk DIFFERENT entries at one time, so an entry's digits are a vector operand, its sign a select a digit,
// and the digits multiplied are the most any lane of the wave needs (control flow stays wave-uniform; the extra digits are zeros).
template <int NL, int NW, bool SPLIT, class Opened, class Ta, class Tab, class Table>
HB_HD void fxtrig_lookup_part(uint32_t (&fre)[NL], uint32_t (&fim)[NL], Opened &&opened, Ta &&ta, Tab &&tab, Table &&table, int wl, int wh, int part, int split,
                              const FpParams<NL> &P) {
    constexpr int CAP = NL * Lazy<NL>::GROUP;
    const int entries = 1 << (wl + wh);
    uint32_t accAc[NL], accAs[NL], accBc[NL], accBs[NL], pc[NL], ps[NL], sumc[NL], sums[NL], Tc[NL], Ts[NL], x[NL], xn[NL], r[NL], t[NL], w[NW];
    uint64_t cc[2 * NL], cs[2 * NL];
#pragma unroll
    for (int q = 0; q < NL; q++) { accAc[q] = 0u; accAs[q] = 0u; accBc[q] = 0u; accBs[q] = 0u; pc[q] = 0u; ps[q] = 0u; }
    const auto flush = [&]() {
        finish<NL>(r, cc, P, 1); fp_add<NL>(t, sumc, r, P); fp_set<NL>(sumc, t);
        finish<NL>(r, cs, P, 1); fp_add<NL>(t, sums, r, P); fp_set<NL>(sums, t);
        col_zero(cc); col_zero(cs);
    };
    for (int hi = part; hi < (1 << wh); hi += split) {
        // three sweeps over lo, ONE body: sumc = sum_lo C_y x_lo / R, sums likewise with S; sweep 0: x = PQ_y (joins accA), 1: x = P_lo (kept
        // as pc, ps), 2: x = d_lo (stays in sumc, sums for the combine)
#pragma unroll 1
        for (int which = 0; which < 3; which++) {
#pragma unroll
            for (int q = 0; q < NL; q++) { sumc[q] = 0u; sums[q] = 0u; }
            col_zero(cc); col_zero(cs);
            int load = 0;
            for (int lo = 0; lo < (1 << wl); lo++) {
                const int y = (hi << wl) | lo;
                bool negc, negs;
                table(w, y);
                unpack<NL, NW>(Tc, w);
                const int nc = fxtrig_magnitude<NL>(Tc, negc, P);
                table(w, entries + y);
                unpack<NL, NW>(Ts, w);
                const int ns = fxtrig_magnitude<NL>(Ts, negs, P);
                int na = nc > ns ? nc : ns;
                if constexpr (SPLIT) na = fxtrig_wave_max<NL>(na);
                if (na == 0) continue;
                if (load + na > CAP) { flush(); load = 0; }
                load += na;
                if (which == 0) tab(w, y); else if (which == 1) ta(w, lo); else opened(w, lo);
                unpack<NL, NW>(x, w);
                if constexpr (SPLIT) {
                    uint32_t xv[NL];
                    fp_neg<NL>(xn, x, P);
#pragma unroll
                    for (int q = 0; q < NL; q++) xv[q] = negc ? xn[q] : x[q];
                    mac_short<NL>(cc, Tc, na, xv);
#pragma unroll
                    for (int q = 0; q < NL; q++) xv[q] = negs ? xn[q] : x[q];
                    mac_short<NL>(cs, Ts, na, xv);
                } else {
                    if (negc || negs) fp_neg<NL>(xn, x, P);
                    if (negc) mac_short<NL>(cc, Tc, nc, xn); else mac_short<NL>(cc, Tc, nc, x);
                    if (negs) mac_short<NL>(cs, Ts, ns, xn); else mac_short<NL>(cs, Ts, ns, x);
                }
            }
            flush();
            if (which == 0) {
                fp_add<NL>(t, accAc, sumc, P); fp_set<NL>(accAc, t);
                fp_add<NL>(t, accAs, sums, P); fp_set<NL>(accAs, t);
            } else if (which == 1) {
                fp_set<NL>(pc, sumc); fp_set<NL>(ps, sums);
            }
        }
        // (e + Q) (sum T d / R) + e (sum T P / R), the two-product combine of ew_beaver_elem (columns below 4 NL 2^58 + 2^35)
        opened(w, (1 << wl) + hi);
        unpack<NL, NW>(x, w);
        ta(w, (1 << wl) + hi);
        unpack<NL, NW>(xn, w);
#pragma unroll
        for (int q = 0; q < NL; q++) xn[q] += x[q];
        mac<NL>(cc, xn, sumc);
        mac<NL>(cc, x, pc);
        redc<NL>(r, cc, P);
        cond_sub_p<NL>(r, P);
        fp_add<NL>(t, accBc, r, P);
        fp_set<NL>(accBc, t);
        mac<NL>(cs, xn, sums);
        mac<NL>(cs, x, ps);
        redc<NL>(r, cs, P);
        cond_sub_p<NL>(r, P);
        fp_add<NL>(t, accBs, r, P);
        fp_set<NL>(accBs, t);
    }
    mont_mul<NL>(t, P.r2, accAc, P);
    mont_mul<NL>(r, P.r2, accBc, P);
    mont_mul<NL>(x, P.r2, r, P);
    fp_add<NL>(fre, t, x, P);
    mont_mul<NL>(t, P.r2, accAs, P);
    mont_mul<NL>(r, P.r2, accBs, P);
    mont_mul<NL>(x, P.r2, r, P);
    fp_add<NL>(fim, t, x, P);
}

// a group of width 1: F = T_0 + (T_1 - T_0) b, digits
template <int NL, int NW>
HB_HD void fxtrig_linear_elem(uint32_t (&f)[NL], const uint32_t (&b)[NL], const uint32_t (&t0w)[NW], const uint32_t (&t1w)[NW], const FpParams<NL> &P) {
    uint32_t t0[NL], t1[NL], d[NL], r[NL];
    unpack<NL, NW>(t0, t0w);
    unpack<NL, NW>(t1, t1w);
    fp_sub<NL>(d, t1, t0, P);
    mont_mul<NL>(r, d, b, P);
    mont_mul<NL>(d, P.r2, r, P);
    fp_add<NL>(f, d, t0, P);
}

// the masked rows of the complex value (re, im) as operand `side` (0: a, 1: b) of product q of a level in `mode`; nxt = the level's ta
// (side 0) or tb (side 1), masked its array of 2 tp rows a product
template <int NL, int NW, class Mem>
HB_HD void fxtrig_mask_value(const uint32_t (&re)[NL], const uint32_t (&im)[NL], int mode, int q, int side, const uint32_t *nxt, uint32_t *masked, int64_t i, int64_t count,
                             const Mem &mem, const FpParams<NL> &P) {
    const int tp = fxtrig_triples(mode);
    uint32_t v[NL], a[NL], o[NL], aw[NW], ow[NW];
    for (int t = 0; t < tp; t++) {
        if (t == 2) fp_add<NL>(v, re, im, P);
        else if (t == 1) fp_set<NL>(v, im);
        else fp_set<NL>(v, re);
        const int64_t r = (int64_t)tp * q + t;
        mem.once(aw, nxt, r * count + i);
        unpack<NL, NW>(a, aw);
        fp_sub<NL>(o, v, a, P);
        pack<NL, NW>(ow, o);
        mem.store(masked, (2 * r + side) * count + i, ow);
    }
}

// ---------------------------------------------------------------- the steps' rows (host and device, over a memory policy)
struct FxTrigGroups { int n, wl[FXTRIG_MAX_GROUPS], wh[FXTRIG_MAX_GROUPS], open_off[FXTRIG_MAX_GROUPS], prod_off[FXTRIG_MAX_GROUPS], table_off[FXTRIG_MAX_GROUPS], slot[FXTRIG_MAX_GROUPS]; };
struct FxTrigLookupArgs { const uint32_t *bits, *opened, *ta, *tab, *tables, *nxt_a, *nxt_b; uint32_t *masked, *kept; int pairs, mode, split; int64_t count; FxTrigGroups G; };

// field[g] by selects: the struct stays where kernel arguments live (g is blockIdx.y: scalar work)
HB_HD int fxtrig_pick(const int (&field)[FXTRIG_MAX_GROUPS], int g) {
    int v = field[0];
#pragma unroll
    for (int q = 1; q < FXTRIG_MAX_GROUPS; q++) v = q == g ? field[q] : v;
    return v;
}

// SPLIT = false: split is 1 and a table entry is one address a wave (SGPR digits); true: the lanes of a wave read different entries
template <bool SPLIT> struct FxTrigLookupRowT {
// i2 = element * split + lane part, count2 = count * split: the lanes of an element are neighbours and enter or leave together
template <int NL, int NW, class Mem>
HB_HD static void run(const FxTrigLookupArgs &A, int g, int64_t i2, int64_t, const Mem &mem, const FpParams<NL> &P) {
    const int wl = fxtrig_pick(A.G.wl, g), wh = fxtrig_pick(A.G.wh, g), slot = fxtrig_pick(A.G.slot, g), split = A.split;
    const int64_t oo = fxtrig_pick(A.G.open_off, g), po = fxtrig_pick(A.G.prod_off, g), to = fxtrig_pick(A.G.table_off, g);
    const int64_t count = A.count, i = i2 / split;
    const int part = (int)(i2 % split);
    uint32_t re[NL], im[NL];
    if (wh == 0) {
        if (part) return;
        uint32_t bw[NW], b[NL], t0[NW], t1[NW];
        mem.once(bw, A.bits, oo * count + i);
        unpack<NL, NW>(b, bw);
        mem.same(t0, A.tables + to * NW);
        mem.same(t1, A.tables + (to + 1) * NW);
        fxtrig_linear_elem<NL, NW>(re, b, t0, t1, P);
        mem.same(t0, A.tables + (to + 2) * NW);
        mem.same(t1, A.tables + (to + 3) * NW);
        fxtrig_linear_elem<NL, NW>(im, b, t0, t1, P);
    } else {
        const uint32_t *opened = A.opened + oo * count * NW, *ta = A.ta + oo * count * NW, *tab = A.tab + po * count * NW, *table = A.tables + to * NW;
#if defined(__HIP_DEVICE_COMPILE__)
        lookup<NL, NW>(re, im, opened, ta, tab, table, wl, wh, part, split, i, count, mem, P);
        for (int mask = 1; mask < split; mask <<= 1) {                          // every lane of the element is here: none left early
            uint32_t ore[NL], oim[NL], t[NL];
#pragma unroll
            for (int q = 0; q < NL; q++) { ore[q] = __shfl_xor(re[q], mask); oim[q] = __shfl_xor(im[q], mask); }
            fp_add<NL>(t, re, ore, P); fp_set<NL>(re, t);
            fp_add<NL>(t, im, oim, P); fp_set<NL>(im, t);
        }
        if (part) return;
#else
        if (part) return;
        lookup<NL, NW>(re, im, opened, ta, tab, table, wl, wh, 0, split, i, count, mem, P);
        for (int other = 1; other < split; other++) {
            uint32_t ore[NL], oim[NL], t[NL];
            lookup<NL, NW>(ore, oim, opened, ta, tab, table, wl, wh, other, split, i, count, mem, P);
            fp_add<NL>(t, re, ore, P); fp_set<NL>(re, t);
            fp_add<NL>(t, im, oim, P); fp_set<NL>(im, t);
        }
#endif
    }
    uint32_t ow[NW];
    pack<NL, NW>(ow, re);
    mem.store(A.kept, (int64_t)(2 * slot) * count + i, ow);
    pack<NL, NW>(ow, im);
    mem.store(A.kept, (int64_t)(2 * slot + 1) * count + i, ow);
    if (slot < 2 * A.pairs) fxtrig_mask_value<NL, NW>(re, im, A.mode, slot >> 1, slot & 1, (slot & 1) ? A.nxt_b : A.nxt_a, A.masked, i, count, mem, P);
}
// what is only read is apart from the outputs: __restrict__ (pointers in an argument struct do not carry it)
template <int NL, int NW, class Mem>
HB_HD static void lookup(uint32_t (&re)[NL], uint32_t (&im)[NL], const uint32_t *__restrict__ opened, const uint32_t *__restrict__ ta, const uint32_t *__restrict__ tab,
                         const uint32_t *__restrict__ table, int wl, int wh, int part, int split, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
    fxtrig_lookup_part<NL, NW, SPLIT>(re, im, [&](uint32_t (&w)[NW], int r) { mem.load(w, opened, (int64_t)r * count + i); },
                                      [&](uint32_t (&w)[NW], int r) { mem.load(w, ta, (int64_t)r * count + i); },
                                      [&](uint32_t (&w)[NW], int y) { mem.once(w, tab, (int64_t)y * count + i); },
                                      [&](uint32_t (&w)[NW], int e) { if constexpr (SPLIT) mem.load(w, table, e); else mem.same(w, table + (int64_t)e * NW); },
                                      wl, wh, part, split, P);
}
};

template <int NL> struct FxTrigProductsArgs {
    const uint32_t *opened, *ta, *tb, *tab, *bits;
    uint32_t *masked, *s;
    int nbits, m, mode;
    FpConst<NL> half;
};

struct FxTrigProductsRow {
template <int NL, int NW, class Mem>
HB_HD static void run(const FxTrigProductsArgs<NL> &A, int q, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
    const int tp = fxtrig_triples(A.mode), comps = fxtrig_comps(A.mode);
    uint32_t dw[NW], ew[NW], aw[NW], bw[NW], abw[NW], pw[NW], o0[NW], o1[NW], pr[3][NL], v[NL], t[NL];
    for (int k = 0; k < tp; k++) {
        const int64_t r = (int64_t)tp * q + k;
        mem.once(dw, A.opened, 2 * r * count + i); mem.once(ew, A.opened, (2 * r + 1) * count + i);
        mem.once(aw, A.ta, r * count + i); mem.once(bw, A.tb, r * count + i); mem.once(abw, A.tab, r * count + i);
        ew_beaver_elem<NL, NW>(pw, dw, ew, aw, bw, abw, P);
        if (k == 0) unpack<NL, NW>(pr[0], pw); else if (k == 1) unpack<NL, NW>(pr[1], pw); else unpack<NL, NW>(pr[2], pw);
    }
    for (int c = 0; c < comps; c++) {
        if (c == 0 && A.mode != 2) fp_sub<NL>(v, pr[0], pr[1], P);
        else { fp_sub<NL>(t, pr[2], pr[0], P); fp_sub<NL>(v, t, pr[1], P); }
        pack<NL, NW>(pw, v);
        const int64_t row = (int64_t)comps * q + c;
        const uint32_t *planes = A.bits + row * A.nbits * count * NW;
        div_trunc_mask_elem<NL, NW>(o0, o1, pw, [&](uint32_t (&w)[NW], int plane) { mem.once(w, planes, (int64_t)plane * count + i); }, A.nbits, A.m, A.half.d, P);
        mem.store(A.masked, row * count + i, o0);
        mem.store(A.s, row * count + i, o1);
    }
}
};

template <int NL> struct FxTrigTreeArgs {
    const uint32_t *opened, *s, *carry, *ta, *tb;
    uint32_t *masked, *kept;
    int rows, values, m, mode, final;
    FpConst<NL> invm;
};

struct FxTrigTreeRow {
template <int NL, int NW, class Mem>
HB_HD static void trunc(uint32_t (&vw)[NW], const FxTrigTreeArgs<NL> &A, int j, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
    uint32_t sw[NW], cw[NW];
    mem.once(sw, A.s, (int64_t)j * count + i); mem.once(cw, A.opened, (int64_t)j * count + i);
    div_trunc_elem<NL, NW>(vw, sw, cw, A.m, A.invm.d, P);
}
template <int NL, int NW, class Mem>
HB_HD static void run(const FxTrigTreeArgs<NL> &A, int u, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
    uint32_t rw[NW], iw[NW];
    if (A.final) {
        trunc<NL, NW>(rw, A, u, i, count, mem, P);
        mem.store(A.kept, (int64_t)u * count + i, rw);
        return;
    }
    if (2 * u < A.rows) { trunc<NL, NW>(rw, A, 2 * u, i, count, mem, P); trunc<NL, NW>(iw, A, 2 * u + 1, i, count, mem, P); }
    else { mem.once(rw, A.carry, i); mem.once(iw, A.carry, count + i); }
    if (u == A.values - 1 && (A.values & 1)) {                                  // the odd one out
        mem.store(A.kept, i, rw);
        mem.store(A.kept, count + i, iw);
        return;
    }
    uint32_t re[NL], im[NL];
    unpack<NL, NW>(re, rw);
    unpack<NL, NW>(im, iw);
    fxtrig_mask_value<NL, NW>(re, im, A.mode, u >> 1, u & 1, (u & 1) ? A.tb : A.ta, A.masked, i, count, mem, P);
}
};

// ---------------------------------------------------------------- host side
// One step function a step (hb_rows.hpp): a DeviceRun in the entry point, a HostRun in hb_selftest_fxtrig.
static bool fxtrig_mode_ok(int mode) { return mode >= 0 && mode <= 2; }

// desc: FXTRIG_DESC ints a group -- wl, wh, open_off, prod_off, table_off, slot.  Fills G and the row extents the overlap check needs;
// false for a shape the step does not take (two groups in one slot among them: both would write one row).
static bool fxtrig_groups(FxTrigGroups &G, int n_groups, const int *desc, int kept_slots, int64_t &bit_rows, int64_t &open_rows, int64_t &prod_rows, int64_t &table_rows) {
    if (n_groups < 1 || n_groups > FXTRIG_MAX_GROUPS || kept_slots < 1 || kept_slots > 2 * FXTRIG_MAX_PRODUCTS + 1) return false;
    G = FxTrigGroups{};
    G.n = n_groups;
    bit_rows = open_rows = prod_rows = table_rows = 0;
    for (int g = 0; g < n_groups; g++) {
        const int *d = desc + FXTRIG_DESC * g;
        const int wl = d[0], wh = d[1], oo = d[2], po = d[3], to = d[4], slot = d[5];
        const bool linear = wl == 1 && wh == 0;
        if (!linear && (wl < 1 || wh < 1 || wl + wh > FXTRIG_MAX_WIDTH)) return false;
        if (oo < 0 || po < 0 || to < 0 || oo > (1 << 20) || po > (1 << 20) || to > (1 << 20) || slot < 0 || slot >= kept_slots) return false;
        for (int h = 0; h < g; h++) if (G.slot[h] == slot) return false;
        G.wl[g] = wl; G.wh[g] = wh; G.open_off[g] = oo; G.prod_off[g] = po; G.table_off[g] = to; G.slot[g] = slot;
        const int64_t entries = (int64_t)1 << (wl + wh);
        if (linear) { if (oo + 1 > bit_rows) bit_rows = oo + 1; }
        else {
            if (oo + (1 << wl) + (1 << wh) > open_rows) open_rows = oo + (1 << wl) + (1 << wh);
            if (po + entries > prod_rows) prod_rows = po + entries;
        }
        if (to + 2 * entries > table_rows) table_rows = to + 2 * entries;
    }
    return true;
}

template <class Run> static int fxtrig_finish_lookup_mask_step(const Run &run, const uint64_t *bits, const uint64_t *opened, const uint64_t *ta, const uint64_t *tab,
                                                               const uint64_t *tables, int n_groups, const int *desc, const uint64_t *nxt_a, const uint64_t *nxt_b,
                                                               int pairs, int mode, int split, uint64_t *masked, uint64_t *kept, int kept_slots, int64_t count) {
    if (count < 0 || !desc) return HB_ERR_BAD_ARG;
    FxTrigLookupArgs A{};
    int64_t bit_rows, open_rows, prod_rows, table_rows;
    if (!fxtrig_groups(A.G, n_groups, desc, kept_slots, bit_rows, open_rows, prod_rows, table_rows) || pairs < 0 || pairs > FXTRIG_MAX_PRODUCTS || !fxtrig_mode_ok(mode) ||
        split < 1 || split > FXTRIG_MAX_SPLIT || (split & (split - 1)))
        return run.fail(HB_ERR_BAD_ARG, "hb_fxtrig_finish_lookup_mask: needs 1 .. 8 groups in slots of their own below kept_slots, merges with 1 <= wl, wh and wl + wh <= 12 "
                                        "(or wl = 1, wh = 0: a group of one bit), 0 <= pairs <= 64, a mode 0 .. 2 and a split 1, 2, 4, 8 or 16");
    if (count == 0) return HB_OK;
    bool masks = false;
    for (int g = 0; g < n_groups; g++) masks = masks || A.G.slot[g] < 2 * pairs;
    if (!tables || !kept || (bit_rows && !bits) || (open_rows && (!opened || !ta || !tab)) || (masks && (!nxt_a || !nxt_b || !masked))) return HB_ERR_BAD_ARG;
    if (count > INT64_MAX >> 24) return HB_ERR_BAD_ARG;
    const int tp = fxtrig_triples(mode);
    const int64_t rb = run.elem_bytes() * count;
    const RowSpan outs[2] = {{masks ? masked : nullptr, 2 * tp * pairs}, {kept, 2 * kept_slots}};
    const RowSpan ins[6] = {{bit_rows ? bits : nullptr, bit_rows}, {open_rows ? opened : nullptr, open_rows}, {open_rows ? ta : nullptr, open_rows},
                            {open_rows ? tab : nullptr, prod_rows}, {masks ? nxt_a : nullptr, tp * pairs}, {masks ? nxt_b : nullptr, tp * pairs}};
    if (!outputs_apart(outs, 2, ins, 6, rb) || overlap(tables, run.elem_bytes() * table_rows, kept, 2 * kept_slots * rb) ||
        (masks && overlap(tables, run.elem_bytes() * table_rows, masked, 2 * tp * pairs * rb)))
        return run.fail(HB_ERR_BAD_ARG, "hb_fxtrig_finish_lookup_mask: masked and kept are arrays of their own");
    A.bits = u32(bits); A.opened = u32(opened); A.ta = u32(ta); A.tab = u32(tab); A.tables = u32(tables); A.nxt_a = u32(nxt_a); A.nxt_b = u32(nxt_b);
    A.masked = u32(masked); A.kept = u32(kept); A.pairs = pairs; A.mode = mode; A.split = split; A.count = count;
    return split == 1 ? run.template rows<FxTrigLookupRowT<false>>(A, n_groups, count) : run.template rows<FxTrigLookupRowT<true>>(A, n_groups, count * split);
}

template <class Run> static int fxtrig_cproducts_trunc_step(const Run &run, int products, int mode, const uint64_t *opened, const uint64_t *ta, const uint64_t *tb,
                                                            const uint64_t *tab, const uint64_t *bits, int width, int m, int kappa, uint64_t *masked, uint64_t *s, int64_t count) {
    if (count < 0) return HB_ERR_BAD_ARG;
    if (products < 1 || products > FXTRIG_MAX_PRODUCTS || !fxtrig_mode_ok(mode) || !fxp_params_ok(run.bits(), width, m, kappa))
        return run.fail(HB_ERR_BAD_ARG, "hb_fxtrig_cproducts_trunc: needs 1 <= products <= 64, a mode 0 .. 2 and a truncation the modulus has room for");
    if (count > 0 && (!opened || !ta || !tb || !tab || !bits || !masked || !s)) return HB_ERR_BAD_ARG;
    if (count > INT64_MAX >> 24) return HB_ERR_BAD_ARG;
    const int64_t rb = run.elem_bytes() * count, trips = (int64_t)fxtrig_triples(mode) * products, comps = (int64_t)fxtrig_comps(mode) * products;
    const RowSpan outs[2] = {{masked, comps}, {s, comps}};
    const RowSpan ins[5] = {{opened, 2 * trips}, {ta, trips}, {tb, trips}, {tab, trips}, {bits, comps * (width + kappa)}};
    if (count > 0 && !outputs_apart(outs, 2, ins, 5, rb)) return run.fail(HB_ERR_BAD_ARG, "hb_fxtrig_cproducts_trunc: masked and s are arrays of their own");
    return run.template rows<FxTrigProductsRow, FxTrigProductsArgs>([&](auto &A, const auto &P) {
        A.opened = u32(opened); A.ta = u32(ta); A.tb = u32(tb); A.tab = u32(tab); A.bits = u32(bits); A.masked = u32(masked); A.s = u32(s);
        A.nbits = width + kappa; A.m = m; A.mode = mode;
        constexpr int NL = sizeof(A.half.d) / sizeof(uint32_t);
        fxp_pow2<NL>(A.half.d, width - 1, false, P);
        return true;
    }, products, count);
}

template <class Run> static int fxtrig_tree_step(const Run &run, int rows, int final, const uint64_t *opened, const uint64_t *s, int m, const uint64_t *inv2m_host,
                                                 const uint64_t *carry, int mode, const uint64_t *ta, const uint64_t *tb, uint64_t *masked, uint64_t *kept, int64_t count) {
    if (count < 0) return HB_ERR_BAD_ARG;
    if (rows < 1 || rows > 2 * FXTRIG_MAX_PRODUCTS || !fxp_m_ok(run.bits(), m) || !fxtrig_mode_ok(mode) || (final != 0 && final != 1) || (final ? carry != nullptr : (rows & 1) != 0))
        return run.fail(HB_ERR_BAD_ARG, "hb_fxtrig_tree_step: needs 1 <= rows <= 128 (two a complex value unless final; no carry when final), a mode 0 .. 2 and 0 < m <= bits(p) - 2");
    if (!inv2m_host) return HB_ERR_BAD_ARG;
    const int values = final ? 0 : rows / 2 + (carry ? 1 : 0), pairs = values / 2, odd = values & 1, tp = fxtrig_triples(mode);
    if (count > 0 && (!opened || !s || (pairs && (!ta || !tb || !masked)) || ((odd || final) && !kept))) return HB_ERR_BAD_ARG;
    if (count > INT64_MAX >> 24) return HB_ERR_BAD_ARG;
    const int64_t rb = run.elem_bytes() * count;
    const RowSpan outs[2] = {{pairs ? masked : nullptr, 2 * tp * pairs}, {odd || final ? kept : nullptr, final ? rows : 2}};
    const RowSpan ins[5] = {{opened, rows}, {s, rows}, {carry, 2}, {pairs ? ta : nullptr, tp * pairs}, {pairs ? tb : nullptr, tp * pairs}};
    if (count > 0 && !outputs_apart(outs, 2, ins, 5, rb)) return run.fail(HB_ERR_BAD_ARG, "hb_fxtrig_tree_step: masked and kept are arrays of their own");
    const int rc = run.template rows<FxTrigTreeRow, FxTrigTreeArgs>([&](auto &A, const auto &P) {
        A.opened = u32(opened); A.s = u32(s); A.carry = u32(carry); A.ta = u32(ta); A.tb = u32(tb); A.masked = u32(masked); A.kept = u32(kept);
        A.rows = rows; A.values = values; A.m = m; A.mode = mode; A.final = final;
        constexpr int NL = sizeof(A.invm.d) / sizeof(uint32_t);
        return host_mont<NL, words_of(NL)>(A.invm.d, P, inv2m_host);
    }, final ? rows : values, count);
    return rc == HB_ERR_BAD_ARG ? run.fail(rc, "hb_fxtrig_tree_step: 2^(-m) is not below the modulus") : rc;
}

}  // namespace hb

extern "C" {

int hb_fxtrig_finish_lookup_mask(hb_ctx *ctx, const uint64_t *bits_dev, const uint64_t *opened_dev, const uint64_t *ta_dev, const uint64_t *tab_dev, const uint64_t *tables_dev,
                                 int n_groups, const int *desc_host, const uint64_t *nxt_a_dev, const uint64_t *nxt_b_dev, int pairs, int mode, int split, uint64_t *masked_dev,
                                 uint64_t *kept_dev, int kept_slots, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : fxtrig_finish_lookup_mask_step(DeviceRun{ctx, (hipStream_t)stream, "hb_fxtrig_finish_lookup_mask"}, bits_dev, opened_dev, ta_dev, tab_dev,
                                                                  tables_dev, n_groups, desc_host, nxt_a_dev, nxt_b_dev, pairs, mode, split, masked_dev, kept_dev, kept_slots, count);
}

int hb_fxtrig_cproducts_trunc(hb_ctx *ctx, int products, int mode, const uint64_t *opened_dev, const uint64_t *ta_dev, const uint64_t *tb_dev, const uint64_t *tab_dev,
                              const uint64_t *bits_dev, int width, int m, int kappa, uint64_t *masked_dev, uint64_t *s_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : fxtrig_cproducts_trunc_step(DeviceRun{ctx, (hipStream_t)stream, "hb_fxtrig_cproducts_trunc"}, products, mode, opened_dev, ta_dev, tb_dev,
                                                               tab_dev, bits_dev, width, m, kappa, masked_dev, s_dev, count);
}

int hb_fxtrig_tree_step(hb_ctx *ctx, int rows, int final, const uint64_t *opened_dev, const uint64_t *s_dev, int m, const uint64_t *inv2m_host, const uint64_t *carry_dev,
                        int mode, const uint64_t *ta_dev, const uint64_t *tb_dev, uint64_t *masked_dev, uint64_t *kept_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : fxtrig_tree_step(DeviceRun{ctx, (hipStream_t)stream, "hb_fxtrig_tree_step"}, rows, final, opened_dev, s_dev, m, inv2m_host, carry_dev, mode,
                                                    ta_dev, tb_dev, masked_dev, kept_dev, count);
}

// params: as the header lists them for each step
int hb_selftest_fxtrig(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *ops, const int64_t *params, uint64_t *const *outs, int64_t count) {
    if (!p_limbs || !ops || !params || !outs || (n_limbs != 1 && n_limbs != 4)) return HB_ERR_BAD_ARG;
    const HostRun run = {p_limbs, n_limbs};
    switch (what) {
    case HB_FXTRIG_SELFTEST_FINISH_LOOKUP_MASK: {                               // n_groups, pairs, kept_slots, mode, split, then FXTRIG_DESC ints a group
        int desc[FXTRIG_DESC * FXTRIG_MAX_GROUPS] = {0};
        if (params[0] < 1 || params[0] > FXTRIG_MAX_GROUPS) return HB_ERR_BAD_ARG;
        for (int i = 0; i < 5 + FXTRIG_DESC * (int)params[0]; i++) if (params[i] < -(1 << 30) || params[i] > (1 << 30)) return HB_ERR_BAD_ARG;
        for (int i = 0; i < FXTRIG_DESC * (int)params[0]; i++) desc[i] = (int)params[5 + i];
        return fxtrig_finish_lookup_mask_step(run, ops[0], ops[1], ops[2], ops[3], ops[4], (int)params[0], desc, ops[5], ops[6], (int)params[1], (int)params[3], (int)params[4],
                                              outs[0], outs[1], (int)params[2], count);
    }
    case HB_FXTRIG_SELFTEST_CPRODUCTS_TRUNC:                                    // products, mode, width, m, kappa
        for (int i = 0; i < 5; i++) if (params[i] < -(1 << 30) || params[i] > (1 << 30)) return HB_ERR_BAD_ARG;
        return fxtrig_cproducts_trunc_step(run, (int)params[0], (int)params[1], ops[0], ops[1], ops[2], ops[3], ops[4], (int)params[2], (int)params[3], (int)params[4], outs[0],
                                           outs[1], count);
    case HB_FXTRIG_SELFTEST_TREE_STEP:                                          // rows, final, m, mode
        for (int i = 0; i < 4; i++) if (params[i] < -(1 << 30) || params[i] > (1 << 30)) return HB_ERR_BAD_ARG;
        return fxtrig_tree_step(run, (int)params[0], (int)params[1], ops[0], ops[1], (int)params[2], ops[2], ops[3], (int)params[3], ops[4], ops[5], outs[0], outs[1], count);
    default: return HB_ERR_BAD_ARG;
    }
}

}  // extern "C"

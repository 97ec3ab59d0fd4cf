// hb_div.hip -- division of shared fixed-point numbers by a shared divisor (Catrina and Saxena's FPDiv / AppRcr / Norm, "Secure
// Computation With Fixed-Point Numbers", for signed k-bit values with f fractional bits), for arrays of values.  Everything between two
// opens is ONE launch.  (The reference stops at division by a public number, fixedpoint.py:277-280: nothing here is a translation.)
//
// DivPairMaskRow      (x - a, y - b): the masked pair of one product [x y] as one array to open (the sign step's [u b]).
// DivOrMaskRow / DivOrCombineRow   one level of a Sklansky prefix OR over N planes, the wiring of hb_bd.hip (bd_node, bd_partner):
//                      node t is network plane j, its partner q, and y_j <- y_j + y_q - [y_j y_q], ONE triple a node, triple row t for
//                      node t.  from_top: network plane r is plane N - 1 - r of the array, so plane i ends as OR_{j >= i}; nothing is
//                      copied, only the index is reversed.  Bit l of q is clear, so q is no node of level l and the level runs in place.
// DivNormMaskRow      v = sum_i 2^(N-1-i) (y_i - y_{i+1}) = 2^(N-1) y_0 - sum_{i>=1} 2^(N-1-i) y_i by Horner, acc = 2 acc - y_i, one doubling
//                      and one subtraction a plane and no product (the planes are walked in the thread: each is read once); writes v and
//                      the masked pairs of [x v] and, signed, [u v] as one array to open.
// DivProductRow   after an open of masked products: the Beaver combine of one or two products, the step's affine map, and what the
//                      next open needs.  blockIdx.y = the row.
//                        HB_DIV_SIGN    x = b - 2 [u b]
//                        HB_DIV_NORM    row 0: c = [x v], d = alpha' - 2 c; row 1: v' = v - 2 [u v] (one product: v' = v).  With the next triple's
//                                       factors: (d - a, v' - b), the masked pair of W = [d v']; without: (c, v').
//                        HB_DIV_FIRST   row 0: x0 = alpha - [b w], kept; row 1: Y = [a w] and its truncation mask
//                        HB_DIV_TRUNC   row r: the product and its truncation mask (W, the iteration's Y and X, the last Y)
//                      A truncation mask is hb_fxp_mask's (fxp_mask_elem: Horner over width + kappa bit planes): masked = V + 2^(width-1) + r1
//                      + 2^m r2 to open, and s = V + r1 kept, so the step after the open reads ONE array a value, not V and r1.
// DivTruncRow     after the open of masked truncations: t = (s - (c mod 2^m)) 2^(-m) for one or two values, and what the next open
//                      needs.  blockIdx.y = the product the thread masks.
//                        HB_DIV_T_RESULT  t alone
//                        HB_DIV_T_RECIP   (b - a0, w - b0, a - a1, w - b1): the masked pairs of [b w] and [a w]
//                        HB_DIV_T_GOLD    (y - a0, alpha + x - b0) and, but for the last product, (x - a1, x - b1); x is the second truncated
//                                         value or, after the first truncation, the x0 kept by HB_DIV_FIRST
//
// Operands and results are packed canonical residues.  The per-element bodies are HB_HD functions (hb_div_elem.hpp, hb_fxp_elem.hpp and
// hb_ew_elem.hpp); a step's row -- which operands it loads, which body it calls, where it stores -- is an HB_HD function over a memory
// policy (hb_rows.hpp): k_rows runs a row on the device, host_rows the very same row in hb_selftest_div.
//
// Launch shape (all kernels): 256-thread workgroups, one element a thread in x, the node / triple / row in blockIdx.y (DivNormMaskRow
// walks the planes in the thread).  No LDS, no grid stride, one launch a call.  Triples, opened values, bit planes and kept values are
// read once and take the non-temporal loads (load_once); y_j and y_q of a level, which the mask and the combine both read, and the
// operands a and b of the division take the plain ones.
// Compiler's report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; scratch = 0 bytes for every kernel):
//   DivPairMaskRow<9, 8>      26 VGPRs: 8 waves a SIMD                            DivPairMaskRow<3, 2>      14 VGPRs: 8 waves
//   DivOrMaskRow<9, 8>        39 VGPRs: 8 waves                                   DivOrMaskRow<3, 2>        15 VGPRs: 8 waves
//   DivOrCombineRow<9, 8>     74 VGPRs: 6 waves                                   DivOrCombineRow<3, 2>     30 VGPRs: 8 waves
//   DivNormMaskRow<9, 8>      59 VGPRs: 8 waves                                   DivNormMaskRow<3, 2>      28 VGPRs: 8 waves
//   DivProductRow<9, 8>       81 VGPRs: 5 waves                                   DivProductRow<3, 2>       32 VGPRs: 8 waves
//   DivTruncRow<9, 8>         56 VGPRs: 8 waves                                   DivTruncRow<3, 2>         18 VGPRs: 8 waves
// (DESIGN.md section 3t has the schedule, the error and width derivations and the counts.)
#include "hb_common.hpp"
#include "hb_div_elem.hpp"

using namespace hb;

namespace hb {

// ---------------------------------------------------------------- the steps' rows (host and device, over a memory policy)
// (Mem, k_rows and host_rows: hb_rows.hpp)
struct DivOrArgs { const uint32_t *opened, *ta, *tb, *tab; uint32_t *y, *masked; int n, level, from_top; };

HB_HD int64_t div_plane(const DivOrArgs &A, int j) { return A.from_top ? A.n - 1 - j : j; }

struct DivOrMaskRow {
template <int NL, int NW, class Mem>
HB_HD static void run(const DivOrArgs &A, int y, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
    const int64_t t = y;
    const int j = bd_node(y, A.level), q = bd_partner(j, A.level);
    uint32_t yj[NW], yq[NW], aw[NW], bw[NW], o0[NW], o1[NW];
    mem.load(yj, A.y, div_plane(A, j) * count + i);
    mem.load(yq, A.y, div_plane(A, q) * count + i);
    mem.once(aw, A.ta, t * count + i);
    mem.once(bw, A.tb, t * count + i);
    diff_elem<NL, NW>(o0, yj, aw, P);
    diff_elem<NL, NW>(o1, yq, bw, P);
    mem.store(A.masked, (2 * t) * count + i, o0);
    mem.store(A.masked, (2 * t + 1) * count + i, o1);
}
};

struct DivOrCombineRow {
template <int NL, int NW, class Mem>
HB_HD static void run(const DivOrArgs &A, int y, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
    const int64_t t = y;
    const int j = bd_node(y, A.level), q = bd_partner(j, A.level);
    uint32_t yj[NW], yq[NW], dw[NW], ew[NW], aw[NW], bw[NW], abw[NW], ow[NW];
    mem.load(yj, A.y, div_plane(A, j) * count + i);
    mem.load(yq, A.y, div_plane(A, q) * count + i);
    mem.once(dw, A.opened, (2 * t) * count + i); mem.once(ew, A.opened, (2 * t + 1) * count + i);
    mem.once(aw, A.ta, t * count + i); mem.once(bw, A.tb, t * count + i); mem.once(abw, A.tab, t * count + i);
    div_or_elem<NL, NW>(ow, yj, yq, dw, ew, aw, bw, abw, P);
    mem.store(A.y, div_plane(A, j) * count + i, ow);
}
};

struct DivPairArgs { const uint32_t *x, *y, *ta, *tb; uint32_t *masked; };

struct DivPairMaskRow {
template <int NL, int NW, class Mem>
HB_HD static void run(const DivPairArgs &A, int, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
    uint32_t w[NW], aw[NW], o[NW];
    mem.load(w, A.x, i); mem.once(aw, A.ta, i);
    diff_elem<NL, NW>(o, w, aw, P);
    mem.store(A.masked, i, o);
    mem.load(w, A.y, i); mem.once(aw, A.tb, i);
    diff_elem<NL, NW>(o, w, aw, P);
    mem.store(A.masked, count + i, o);
}
};

struct DivNormArgs { const uint32_t *x, *y, *u, *ta, *tb; uint32_t *masked, *v; int n; };

struct DivNormMaskRow {
template <int NL, int NW, class Mem>
HB_HD static void run(const DivNormArgs &A, int, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
    uint32_t vw[NW], w[NW], aw[NW], o[NW];
    div_scale_elem<NL, NW>(vw, [&](uint32_t (&pw)[NW], int row) { mem.once(pw, A.y, (int64_t)row * count + i); }, A.n, P);
    mem.store(A.v, i, vw);
    mem.load(w, A.x, i); mem.once(aw, A.ta, i);
    diff_elem<NL, NW>(o, w, aw, P);
    mem.store(A.masked, i, o);
    mem.once(aw, A.tb, i);
    diff_elem<NL, NW>(o, vw, aw, P);
    mem.store(A.masked, count + i, o);
    if (!A.u) return;
    mem.load(w, A.u, i); mem.once(aw, A.ta, count + i);
    diff_elem<NL, NW>(o, w, aw, P);
    mem.store(A.masked, 2 * count + i, o);
    mem.once(aw, A.tb, count + i);
    diff_elem<NL, NW>(o, vw, aw, P);
    mem.store(A.masked, 3 * count + i, o);
}
};

template <int NL> struct DivProductArgs {
    const uint32_t *opened, *ta, *tb, *tab, *aux, *nxt_a, *nxt_b, *bits;
    uint32_t *out0, *out1;
    int mode, products, nbits, m;
    FpConst<NL> cst, half;
};

struct DivProductRow {
template <int NL, int NW, class Mem>
HB_HD static void run(const DivProductArgs<NL> &A, int r, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
    uint32_t pw[NW], vw[NW], xw[NW], o0[NW], o1[NW], zero[NL];
#pragma unroll
    for (int q = 0; q < NL; q++) zero[q] = 0u;
#pragma unroll
    for (int q = 0; q < NW; q++) { pw[q] = 0u; xw[q] = 0u; }
    if (r < A.products) {
        uint32_t dw[NW], ew[NW], aw[NW], bw[NW], abw[NW];
        mem.once(dw, A.opened, (int64_t)(2 * r) * count + i); mem.once(ew, A.opened, (int64_t)(2 * r + 1) * count + i);
        mem.once(aw, A.ta, (int64_t)r * count + i); mem.once(bw, A.tb, (int64_t)r * count + i); mem.once(abw, A.tab, (int64_t)r * count + i);
        ew_beaver_elem<NL, NW>(pw, dw, ew, aw, bw, abw, P);
    }
    if (A.mode == HB_DIV_SIGN) {
        mem.load(xw, A.aux, i);
        div_affine_elem<NL, NW>(vw, pw, -2, zero, xw, P);
        mem.store(A.out0, i, vw);
    } else if (A.mode == HB_DIV_NORM) {
        if (r == 0) {
            if (A.nxt_a) div_affine_elem<NL, NW>(vw, pw, -2, A.cst.d, xw, P);
            else div_affine_elem<NL, NW>(vw, pw, 1, zero, xw, P);
        } else {
            mem.once(xw, A.aux, i);
            div_affine_elem<NL, NW>(vw, pw, -2, zero, xw, P);
        }
        if (A.nxt_a) {
            mem.once(xw, r == 0 ? A.nxt_a : A.nxt_b, i);
            diff_elem<NL, NW>(o0, vw, xw, P);
            mem.store(A.out0, (int64_t)r * count + i, o0);
        } else {
            mem.store(A.out0, (int64_t)r * count + i, vw);
        }
    } else if (A.mode == HB_DIV_FIRST && r == 0) {
        div_affine_elem<NL, NW>(vw, pw, -1, A.cst.d, xw, P);
        mem.store(A.out1, count + i, vw);
    } else {
        const int set = A.mode == HB_DIV_FIRST ? 0 : r;                      // FIRST truncates row 1 alone: one set of planes, row 0 of both outputs
        const uint32_t *planes = A.bits + (int64_t)set * A.nbits * count * NW;
        div_trunc_mask_elem<NL, NW>(o0, o1, pw, [&](uint32_t (&bw)[NW], int row) { mem.once(bw, planes, (int64_t)row * count + i); }, A.nbits, A.m, A.half.d, P);
        mem.store(A.out0, (int64_t)set * count + i, o0);
        mem.store(A.out1, (int64_t)set * count + i, o1);
    }
}
};

template <int NL> struct DivTruncArgs {
    const uint32_t *opened, *s, *x_in, *ext0, *ext1, *ta, *tb;
    uint32_t *out;
    int mode, rows, products, m;
    FpConst<NL> invm, alpha;
};

struct DivTruncRow {
template <int NL, int NW, class Mem>
HB_HD static void run(const DivTruncArgs<NL> &A, int q, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
    uint32_t sw[NW], cw[NW], t0[NW], xw[NW], first[NW], second[NW], aw[NW], o[NW], zero[NW];
#pragma unroll
    for (int w = 0; w < NW; w++) zero[w] = 0u;
    mem.once(sw, A.s, i); mem.once(cw, A.opened, i);
    div_trunc_elem<NL, NW>(t0, sw, cw, A.m, A.invm.d, P);
    if (A.mode == HB_DIV_T_RESULT) { mem.store(A.out, i, t0); return; }
    if (A.mode == HB_DIV_T_RECIP) {
        mem.load(first, q ? A.ext1 : A.ext0, i);
#pragma unroll
        for (int w = 0; w < NW; w++) second[w] = t0[w];
    } else {
        if (A.rows == 2) {
            mem.once(sw, A.s, count + i); mem.once(cw, A.opened, count + i);
            div_trunc_elem<NL, NW>(xw, sw, cw, A.m, A.invm.d, P);
        } else {
            mem.load(xw, A.x_in, i);
        }
        if (q == 0) {
#pragma unroll
            for (int w = 0; w < NW; w++) first[w] = t0[w];
            div_affine_elem<NL, NW>(second, zero, 1, A.alpha.d, xw, P);
        } else {
#pragma unroll
            for (int w = 0; w < NW; w++) { first[w] = xw[w]; second[w] = xw[w]; }
        }
    }
    mem.once(aw, A.ta, (int64_t)q * count + i);
    diff_elem<NL, NW>(o, first, aw, P);
    mem.store(A.out, (int64_t)(2 * q) * count + i, o);
    mem.once(aw, A.tb, (int64_t)q * count + i);
    diff_elem<NL, NW>(o, second, aw, P);
    mem.store(A.out, (int64_t)(2 * q + 1) * count + i, o);
}
};

// ---------------------------------------------------------------- host side
// One step function a step (hb_rows.hpp): its checks, Args fill and row count run under a DeviceRun in the entry point, a HostRun in hb_selftest_div.
static bool div_or_ok(int n, int level) { return n >= 1 && n <= 256 && level >= 0 && level < bd_levels(n); }
static bool div_product_ok(int bits, int mode, int products, int width, int m, int kappa) {
    switch (mode) {
    case HB_DIV_SIGN: return products == 1;
    case HB_DIV_NORM: return products == 1 || products == 2;
    case HB_DIV_FIRST: return products == 2 && fxp_params_ok(bits, width, m, kappa);
    case HB_DIV_TRUNC: return (products == 1 || products == 2) && fxp_params_ok(bits, width, m, kappa);
    default: return false;
    }
}
static int div_product_rows(int mode, int products) { return mode == HB_DIV_SIGN ? 1 : (mode == HB_DIV_NORM ? 2 : products); }
static int div_product_sets(int mode, int products) { return mode == HB_DIV_FIRST ? 1 : (mode == HB_DIV_TRUNC ? products : 0); }
static int div_product_out0_rows(int mode, int products) { return mode == HB_DIV_SIGN ? 1 : (mode == HB_DIV_NORM ? 2 : div_product_sets(mode, products)); }
static int div_product_out1_rows(int mode, int products) { return mode == HB_DIV_FIRST ? 2 : (mode == HB_DIV_TRUNC ? products : 0); }
static bool div_trunc_ok(int bits, int mode, int rows, int products, int m) {
    if (!fxp_m_ok(bits, m)) return false;
    switch (mode) {
    case HB_DIV_T_RESULT: return rows == 1 && products == 0;
    case HB_DIV_T_RECIP: return rows == 1 && products == 2;
    case HB_DIV_T_GOLD: return (rows == 1 || rows == 2) && (products == 1 || products == 2);
    default: return false;
    }
}

template <int NL>
static bool div_product_consts(DivProductArgs<NL> &A, const FpParams<NL> &P, const uint64_t *cst_host, int width) {
    for (int q = 0; q < NL; q++) { A.cst.d[q] = 0; A.half.d[q] = 0; }
    if (A.mode == HB_DIV_FIRST || A.mode == HB_DIV_TRUNC) fxp_pow2<NL>(A.half.d, width - 1, false, P);
    if (A.mode == HB_DIV_FIRST || (A.mode == HB_DIV_NORM && A.nxt_a)) return host_digits<NL, words_of(NL)>(A.cst.d, P, cst_host);
    return true;
}
template <int NL>
static bool div_trunc_consts(DivTruncArgs<NL> &A, const FpParams<NL> &P, const uint64_t *inv2m_host, const uint64_t *alpha_host) {
    for (int q = 0; q < NL; q++) A.alpha.d[q] = 0;
    if (!host_mont<NL, words_of(NL)>(A.invm.d, P, inv2m_host)) return false;
    return A.mode == HB_DIV_T_GOLD ? host_digits<NL, words_of(NL)>(A.alpha.d, P, alpha_host) : true;
}

// which operands a step reads, as a bit mask over the operand tables of the header
static unsigned div_product_needs(int mode, bool nxt) {
    unsigned need = 0xFu;                                                       // opened, ta, tb, tab
    if (mode == HB_DIV_SIGN || mode == HB_DIV_NORM) need |= 1u << 4;             // aux
    if (mode == HB_DIV_FIRST || (mode == HB_DIV_NORM && nxt)) need |= 1u << 5;   // cst
    if (mode == HB_DIV_NORM && nxt) need |= 3u << 6;                             // nxt_a, nxt_b
    if (mode == HB_DIV_FIRST || mode == HB_DIV_TRUNC) need |= 1u << 8;           // bits
    return need;
}
static unsigned div_trunc_needs(int mode, int rows, int products) {
    unsigned need = 0x7u;                                                       // opened, s, inv2m
    if (mode == HB_DIV_T_GOLD) need |= 1u << 3;                                  // alpha
    if (mode == HB_DIV_T_GOLD && rows == 1) need |= 1u << 4;                     // x_in
    if (mode == HB_DIV_T_RECIP) need |= 3u << 5;                                 // ext0, ext1
    if (products) need |= 3u << 7;                                               // ta, tb
    return need;
}

template <class Run> static int div_or_mask_step(const Run &run, const uint64_t *y, int n_planes, int level, int from_top, const uint64_t *ta, const uint64_t *tb,
                                                 uint64_t *masked, int64_t count) {
    if (count < 0 || (count > 0 && (!y || !ta || !tb || !masked))) return HB_ERR_BAD_ARG;
    if (!div_or_ok(n_planes, level)) return run.fail(HB_ERR_BAD_ARG, "hb_div_or_mask: needs 1 <= n_planes <= 256 and a level the network has");
    if (count == 0) return HB_OK;
    const int nodes = bd_active(n_planes, level);
    const int64_t rb = run.elem_bytes() * count;
    const RowSpan outs[1] = {{masked, 2 * nodes}}, ins[3] = {{y, n_planes}, {ta, nodes}, {tb, nodes}};
    if (!outputs_apart(outs, 1, ins, 3, rb)) return run.fail(HB_ERR_BAD_ARG, "hb_div_or_mask: masked is an array of its own");
    const DivOrArgs A = {nullptr, u32(ta), u32(tb), nullptr, const_cast<uint32_t *>(u32(y)), u32(masked), n_planes, level, from_top ? 1 : 0};
    return run.template rows<DivOrMaskRow>(A, nodes, count);
}

template <class Run> static int div_or_combine_step(const Run &run, const uint64_t *opened, uint64_t *y, int n_planes, int level, int from_top, const uint64_t *ta,
                                                    const uint64_t *tb, const uint64_t *tab, int64_t count) {
    if (count < 0 || (count > 0 && (!opened || !y || !ta || !tb || !tab))) return HB_ERR_BAD_ARG;
    if (!div_or_ok(n_planes, level)) return run.fail(HB_ERR_BAD_ARG, "hb_div_or_combine: needs 1 <= n_planes <= 256 and a level the network has");
    if (count == 0) return HB_OK;
    const int nodes = bd_active(n_planes, level);
    const int64_t rb = run.elem_bytes() * count;
    const RowSpan outs[1] = {{y, n_planes}}, ins[4] = {{opened, 2 * nodes}, {ta, nodes}, {tb, nodes}, {tab, nodes}};
    if (!outputs_apart(outs, 1, ins, 4, rb)) return run.fail(HB_ERR_BAD_ARG, "hb_div_or_combine: y is an array of its own");
    const DivOrArgs A = {u32(opened), u32(ta), u32(tb), u32(tab), u32(y), nullptr, n_planes, level,
                         from_top ? 1 : 0};
    return run.template rows<DivOrCombineRow>(A, nodes, count);
}

template <class Run> static int div_pair_mask_step(const Run &run, const uint64_t *x, const uint64_t *y, const uint64_t *ta, const uint64_t *tb, uint64_t *masked,
                                                   int64_t count) {
    if (count < 0 || (count > 0 && (!x || !y || !ta || !tb || !masked))) return HB_ERR_BAD_ARG;
    if (count == 0) return HB_OK;
    const int64_t rb = run.elem_bytes() * count;
    const RowSpan outs[1] = {{masked, 2}}, ins[4] = {{x, 1}, {y, 1}, {ta, 1}, {tb, 1}};
    if (!outputs_apart(outs, 1, ins, 4, rb)) return run.fail(HB_ERR_BAD_ARG, "hb_div_pair_mask: masked is an array of its own");
    const DivPairArgs A = {u32(x), u32(y), u32(ta), u32(tb), u32(masked)};
    return run.template rows<DivPairMaskRow>(A, 1, count);
}

template <class Run> static int div_norm_mask_step(const Run &run, const uint64_t *x, const uint64_t *y, int n_planes, const uint64_t *u, const uint64_t *ta,
                                                   const uint64_t *tb, uint64_t *masked, uint64_t *v, int64_t count) {
    if (count < 0 || (count > 0 && (!x || !y || !ta || !tb || !masked || !v))) return HB_ERR_BAD_ARG;
    if (n_planes < 1 || n_planes > 256) return run.fail(HB_ERR_BAD_ARG, "hb_div_norm_mask: needs 1 <= n_planes <= 256");
    if (count == 0) return HB_OK;
    const int products = u ? 2 : 1;
    const int64_t rb = run.elem_bytes() * count;
    const RowSpan outs[2] = {{masked, 2 * products}, {v, 1}}, ins[5] = {{x, 1}, {y, n_planes}, {u, 1}, {ta, products}, {tb, products}};
    if (!outputs_apart(outs, 2, ins, 5, rb)) return run.fail(HB_ERR_BAD_ARG, "hb_div_norm_mask: masked and v are arrays of their own");
    const DivNormArgs A = {u32(x), u32(y), u32(u), u32(ta), u32(tb), u32(masked),
                           u32(v), n_planes};
    return run.template rows<DivNormMaskRow>(A, 1, count);
}

template <class Run> static int div_product_step(const Run &run, int mode, int products, const uint64_t *opened, const uint64_t *ta, const uint64_t *tb,
                                                 const uint64_t *tab, const uint64_t *aux, const uint64_t *cst_host, const uint64_t *nxt_a, const uint64_t *nxt_b,
                                                 const uint64_t *bits, int width, int m, int kappa, uint64_t *out0, uint64_t *out1, int64_t count) {
    if (count < 0) return HB_ERR_BAD_ARG;
    if (!div_product_ok(run.bits(), mode, products, width, m, kappa))
        return run.fail(HB_ERR_BAD_ARG, "hb_div_product_step: unknown mode, a product count the mode does not take, or a truncation the modulus has no room for");
    if (mode == HB_DIV_NORM && (!nxt_a) != (!nxt_b)) return run.fail(HB_ERR_BAD_ARG, "hb_div_product_step: nxt_a and nxt_b go together");
    const bool nxt = mode == HB_DIV_NORM && nxt_a;
    const unsigned need = div_product_needs(mode, nxt);
    const int o0 = div_product_out0_rows(mode, products), o1 = div_product_out1_rows(mode, products), sets = div_product_sets(mode, products);
    if ((need & (1u << 5)) && !cst_host) return HB_ERR_BAD_ARG;
    if (count > 0 && (!opened || !ta || !tb || !tab || !out0 || (o1 && !out1) || ((need & (1u << 4)) && !aux) || ((need & (1u << 8)) && !bits)))
        return HB_ERR_BAD_ARG;
    const int64_t rb = run.elem_bytes() * count;
    const RowSpan outs[2] = {{out0, o0}, {o1 ? out1 : nullptr, o1}};
    const RowSpan ins[8] = {{opened, 2 * products}, {ta, products}, {tb, products}, {tab, products}, {(need & (1u << 4)) ? aux : nullptr, 1},
                            {nxt ? nxt_a : nullptr, 1}, {nxt ? nxt_b : nullptr, 1}, {sets ? bits : nullptr, (int64_t)sets * (width + kappa)}};
    if (count > 0 && !outputs_apart(outs, 2, ins, 8, rb)) return run.fail(HB_ERR_BAD_ARG, "hb_div_product_step: the outputs are arrays of their own");
    const int rc = run.template rows<DivProductRow, DivProductArgs>([&](auto &A, const auto &P) {
        A = {u32(opened), u32(ta), u32(tb), u32(tab), u32(aux), nxt ? u32(nxt_a) : nullptr, nxt ? u32(nxt_b) : nullptr, u32(bits),
             u32(out0), u32(out1), mode, products, width + kappa, m};
        return div_product_consts(A, P, cst_host, width);
    }, div_product_rows(mode, products), count);
    return rc == HB_ERR_BAD_ARG ? run.fail(rc, "hb_div_product_step: the constant is not below the modulus") : rc;
}

template <class Run> static int div_trunc_step(const Run &run, int mode, int rows, int products, const uint64_t *opened, const uint64_t *s, int m,
                                               const uint64_t *inv2m_host, const uint64_t *alpha_host, const uint64_t *x, const uint64_t *ext0, const uint64_t *ext1,
                                               const uint64_t *ta, const uint64_t *tb, uint64_t *out, int64_t count) {
    if (count < 0) return HB_ERR_BAD_ARG;
    if (!div_trunc_ok(run.bits(), mode, rows, products, m))
        return run.fail(HB_ERR_BAD_ARG, "hb_div_trunc_step: unknown mode, row or product counts the mode does not take, or m outside 0 < m <= bits(p) - 2");
    const unsigned need = div_trunc_needs(mode, rows, products);
    if (!inv2m_host || ((need & (1u << 3)) && !alpha_host)) return HB_ERR_BAD_ARG;
    if (count > 0 && (!opened || !s || !out || ((need & (1u << 4)) && !x) || ((need & (1u << 5)) && (!ext0 || !ext1)) ||
                      ((need & (1u << 7)) && (!ta || !tb))))
        return HB_ERR_BAD_ARG;
    const int64_t rb = run.elem_bytes() * count;
    const RowSpan outs[1] = {{out, products ? 2 * products : 1}};
    const RowSpan ins[7] = {{opened, rows}, {s, rows}, {(need & (1u << 4)) ? x : nullptr, 1}, {(need & (1u << 5)) ? ext0 : nullptr, 1},
                            {(need & (1u << 5)) ? ext1 : nullptr, 1}, {products ? ta : nullptr, products}, {products ? tb : nullptr, products}};
    if (count > 0 && !outputs_apart(outs, 1, ins, 7, rb)) return run.fail(HB_ERR_BAD_ARG, "hb_div_trunc_step: out is an array of its own");
    const int rc = run.template rows<DivTruncRow, DivTruncArgs>([&](auto &A, const auto &P) {
        A = {u32(opened), u32(s), u32(x), u32(ext0), u32(ext1), u32(ta), u32(tb), u32(out), mode, rows, products, m};
        return div_trunc_consts(A, P, inv2m_host, alpha_host);
    }, products ? products : 1, count);
    return rc == HB_ERR_BAD_ARG ? run.fail(rc, "hb_div_trunc_step: a constant is not below the modulus") : rc;
}

}  // namespace hb

extern "C" {

int hb_div_or_mask(hb_ctx *ctx, const uint64_t *y_dev, int n_planes, int level, int from_top, const uint64_t *ta_dev, const uint64_t *tb_dev, uint64_t *masked_dev,
                   int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : div_or_mask_step(DeviceRun{ctx, (hipStream_t)stream, "hb_div_or_mask"}, y_dev, n_planes, level, from_top, ta_dev, tb_dev, masked_dev,
                                                    count);
}

int hb_div_or_combine(hb_ctx *ctx, const uint64_t *opened_dev, uint64_t *y_dev, int n_planes, int level, int from_top, const uint64_t *ta_dev, const uint64_t *tb_dev,
                      const uint64_t *tab_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : div_or_combine_step(DeviceRun{ctx, (hipStream_t)stream, "hb_div_or_combine"}, opened_dev, y_dev, n_planes, level, from_top, ta_dev,
                                                       tb_dev, tab_dev, count);
}

int hb_div_pair_mask(hb_ctx *ctx, const uint64_t *x_dev, const uint64_t *y_dev, const uint64_t *ta_dev, const uint64_t *tb_dev, uint64_t *masked_dev, int64_t count,
                     void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : div_pair_mask_step(DeviceRun{ctx, (hipStream_t)stream, "hb_div_pair_mask"}, x_dev, y_dev, ta_dev, tb_dev, masked_dev, count);
}

int hb_div_norm_mask(hb_ctx *ctx, const uint64_t *x_dev, const uint64_t *y_dev, int n_planes, const uint64_t *u_dev, const uint64_t *ta_dev, const uint64_t *tb_dev,
                     uint64_t *masked_dev, uint64_t *v_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : div_norm_mask_step(DeviceRun{ctx, (hipStream_t)stream, "hb_div_norm_mask"}, x_dev, y_dev, n_planes, u_dev, ta_dev, tb_dev, masked_dev,
                                                      v_dev, count);
}

int hb_div_product_step(hb_ctx *ctx, int mode, int products, const uint64_t *opened_dev, const uint64_t *ta_dev, const uint64_t *tb_dev, const uint64_t *tab_dev,
                        const uint64_t *aux_dev, const uint64_t *cst_host, const uint64_t *nxt_a_dev, const uint64_t *nxt_b_dev, const uint64_t *bits_dev, int width, int m,
                        int kappa, uint64_t *out0_dev, uint64_t *out1_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : div_product_step(DeviceRun{ctx, (hipStream_t)stream, "hb_div_product_step"}, mode, products, opened_dev, ta_dev, tb_dev, tab_dev,
                                                    aux_dev, cst_host, nxt_a_dev, nxt_b_dev, bits_dev, width, m, kappa, out0_dev, out1_dev, count);
}

int hb_div_trunc_step(hb_ctx *ctx, int mode, int rows, int products, const uint64_t *opened_dev, const uint64_t *s_dev, int m, const uint64_t *inv2m_host,
                      const uint64_t *alpha_host, const uint64_t *x_dev, const uint64_t *ext0_dev, const uint64_t *ext1_dev, const uint64_t *ta_dev, const uint64_t *tb_dev,
                      uint64_t *out_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : div_trunc_step(DeviceRun{ctx, (hipStream_t)stream, "hb_div_trunc_step"}, mode, rows, products, opened_dev, s_dev, m, inv2m_host,
                                                  alpha_host, x_dev, ext0_dev, ext1_dev, ta_dev, tb_dev, out_dev, count);
}

// params: as the header lists them for each step
int hb_selftest_div(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *ops, const int64_t *params, uint64_t *const *outs, int64_t count) {
    if (!p_limbs || !ops || !params || !outs || (n_limbs != 1 && n_limbs != 4)) return HB_ERR_BAD_ARG;
    for (int i = 0; i < 5; i++) if (params[i] < -(1 << 30) || params[i] > (1 << 30)) return HB_ERR_BAD_ARG;
    const HostRun run = {p_limbs, n_limbs};
    const int a = (int)params[0], b = (int)params[1], c = (int)params[2], d = (int)params[3], e = (int)params[4];
    switch (what) {
    case HB_DIV_SELFTEST_OR_MASK: return div_or_mask_step(run, ops[0], a, b, c, ops[1], ops[2], outs[0], count);
    case HB_DIV_SELFTEST_OR_COMBINE: return div_or_combine_step(run, ops[0], outs[0], a, b, c, ops[1], ops[2], ops[3], count);
    case HB_DIV_SELFTEST_PAIR_MASK: return div_pair_mask_step(run, ops[0], ops[1], ops[2], ops[3], outs[0], count);
    case HB_DIV_SELFTEST_NORM_MASK: return div_norm_mask_step(run, ops[0], ops[1], a, ops[2], ops[3], ops[4], outs[0], outs[1], count);
    case HB_DIV_SELFTEST_PRODUCT_STEP:                                          // mode, products, width, m, kappa
        return div_product_step(run, a, b, ops[0], ops[1], ops[2], ops[3], ops[4], ops[5], ops[6], ops[7], ops[8], c, d, e, outs[0], outs[1], count);
    case HB_DIV_SELFTEST_TRUNC_STEP:                                            // mode, rows, products, m
        return div_trunc_step(run, a, b, c, ops[0], ops[1], d, ops[2], ops[3], ops[4], ops[5], ops[6], ops[7], ops[8], outs[0], count);
    default: return HB_ERR_BAD_ARG;
    }
}

}  // extern "C"

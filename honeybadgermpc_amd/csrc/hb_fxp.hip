// hb_fxp.hip -- fixed-point arithmetic on share arrays, the reference's progs/fixedpoint.py ("Secure Computation With Fixed-Point
// Numbers", Catrina and Saxena): random2m (:91-98), trunc_pr (:108-120), get_carry_bit / bit_ltl (:131-172), div2m (:184-193), trunc
// (:208-211) and FixedPoint.ltz (:266-268) for arrays of values -- restated on fp29.hpp, not translated.
//
// A value x has k bits (signed: |x| < 2^(k-1)), m of them are cut off, kappa is the statistical security parameter.  The protocol
// opens c = x + 2^(k-1) + r1 + 2^m r2 with r1 < 2^m, r2 < 2^(k+kappa-m) made of k + kappa preprocessed random bit shares, takes
// c2 = c mod 2^m in the clear and corrects it by the borrow of c2 - r1, the carry bit of c2 + (2^m - 1 - r1) + 1 out of a prefix tree.
// The bit shares arrive as planes: row i of `bits` holds [b_i] of every element, so a wave's loads of a plane cover consecutive elements.
//
// The steps are rows under the generic kernel k_rows (hb_rows.hpp); the leaves' row runs under k_leaves (hb_fxp_elem.hpp):
// FxpMaskRow       r1 = sum_{i<m} 2^i b_i and r1 + 2^m r2 = sum_{i<k+kappa} 2^i b_i by Horner from the top plane down: one modular
//                  doubling and one addition a plane, no product (the planes below m feed two accumulators).  Writes x + 2^(k-1) + r1 +
//                  2^m r2 and r1; without x (random2m alone) r2 and r1.  k + kappa + 1 reads and two writes an element.
// FxpTruncPrRow    after the open: (x - (c mod 2^m) + r1) 2^(-m); c mod 2^m is a mask on the packed words, 2^(-m) a kernel argument in
//                  Montgomery form (wave-uniform, SGPRs: the `a` operand of mac), so the scaling is ONE product.
// FxpLeavesRow     the tree's leaves with no product: a_i, bit i of c2, is public, so carry_i = a_i (1 - b_i) and all_one_i = a_i +
//                  (1 - b_i) - 2 carry_i are selects: a_i = 1 -> (g, p) = (1 - b_i, b_i), a_i = 0 -> (0, 1 - b_i).  m + 1 leaf planes, most
//                  significant bit first, the low carry (1, 0) last.  (The reference spends a triple and an open on each of these.)
// FxpCarryMaskRow / FxpCarryCombineRow   one level of the tree, (g1, p1) o (g2, p2) = (g1 + p1 g2, p1 p2) on adjacent planes: the mask
//                  writes the two masked differences of every Beaver product of the level into one array (one thread a triple), the
//                  combine takes that array opened and writes the next level's planes (one thread a node, ew_beaver_elem twice; an odd
//                  last plane is copied).  At the root only g is computed.
// FxpFinishRow     u = 1 - carry, a2 = c2 - r1 + 2^m u = [x mod 2^m]; or (x - a2) 2^(-m) = [floor(x / 2^m)]; or its negation (ltz).
//
// Operands and results are packed canonical residues.  The per-element bodies are HB_HD functions (hb_fxp_elem.hpp and below); a
// step's row -- which operands it loads, which body it calls, where it stores -- is an HB_HD function over a memory policy, so
// hb_selftest_fxp runs on the host the very rows, arithmetic and addressing, that k_rows runs on the device.
//
// Launch shape (all kernels): 256-thread workgroups, one element a thread in x; the tree's rows take the triple / node in
// blockIdx.y.  No LDS, no grid stride, one launch a call.  Planes, triples and opened values are read once: the 32-byte width takes
// the non-temporal loads, as EwBeaverRow.
// Compiler's report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; scratch = 0 bytes for every kernel):
//   FxpMaskRow<9, 8>           83 VGPRs with x (5 waves a SIMD), 68 without (7)     FxpMaskRow<3, 2>           34 / 27 VGPRs: 8 waves
//   FxpTruncPrRow<9, 8>        43 VGPRs: 8 waves                                   FxpTruncPrRow<3, 2>        15 VGPRs: 8 waves
//   FxpLeavesRow<9, 8>         69 VGPRs: 7 waves                                   FxpLeavesRow<3, 2>         49 VGPRs: 8 waves
//   FxpCarryMaskRow<9, 8>      41 VGPRs: 8 waves                                   FxpCarryMaskRow<3, 2>      15 VGPRs: 8 waves
//   FxpCarryCombineRow<9, 8>   67 VGPRs: 7 waves                                   FxpCarryCombineRow<3, 2>   27 VGPRs: 8 waves
//   FxpFinishRow<9, 8>         64 VGPRs: 8 waves                                   FxpFinishRow<3, 2>         27 VGPRs: 8 waves
// (DESIGN.md section 3m has the schedule and the counts.)
#include "hb_common.hpp"
#include "hb_fxp_elem.hpp"

using namespace hb;

namespace hb {

// ---------------------------------------------------------------- per-element bodies (host and device)
// (fxp_horner, fxp_mask_elem, fxp_low_bits, fxp_trunc_pr_elem, fxp_leaf_elem, fxp_node_g_elem, fxp_finish_elem with FxpFinishConsts
// and the host helpers fxp_params_ok, fxp_pow2, fxp_finish_fill: hb_fxp_elem.hpp, shared with hb_bd.hip, hb_div.hip and hb_sort.hip;
// FpConst, host_mont, word_bit, diff_elem: hb_rows.hpp)

// ---------------------------------------------------------------- the steps' rows (host and device, over a memory policy: hb_rows.hpp)
// Where the header allows an output to be an input, a thread reads its element before it writes it.
template <int NL> struct FxpMaskArgs { const uint32_t *x, *bits; uint32_t *masked, *r1; int nbits, m; FpConst<NL> half; };

template <bool HAS_X> struct FxpMaskRow {
    template <int NL, int NW, class Mem>
    HB_HD static void run(const FxpMaskArgs<NL> &A, int, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
        uint32_t xw[NW], o0[NW], o1[NW];
        if constexpr (HAS_X) mem.load(xw, A.x, i);
        fxp_mask_elem<NL, NW, HAS_X>(o0, o1, xw, [&](uint32_t (&w)[NW], int row) { mem.once(w, A.bits, (int64_t)row * count + i); }, A.nbits, A.m, A.half.d, P);
        mem.store(A.masked, i, o0);
        mem.store(A.r1, i, o1);
    }
};

template <int NL> struct FxpTruncPrArgs { const uint32_t *x, *c, *r1; uint32_t *out; int m; FpConst<NL> invm; };

struct FxpTruncPrRow {
    template <int NL, int NW, class Mem>
    HB_HD static void run(const FxpTruncPrArgs<NL> &A, int, int64_t i, int64_t, const Mem &mem, const FpParams<NL> &P) {
        uint32_t xw[NW], cw[NW], rw[NW], ow[NW];
        mem.load(xw, A.x, i); mem.once(cw, A.c, i); mem.once(rw, A.r1, i);
        fxp_trunc_pr_elem<NL, NW>(ow, xw, cw, rw, A.m, A.invm.d, P);
        mem.store(A.out, i, ow);
    }
};

// g, p: m + 1 planes each, distinct from c and bits (the body under k_leaves, hb_fxp_elem.hpp, which has the __restrict__)
struct FxpLeavesRow {
    template <int NL, int NW, class Mem>
    HB_HD static void planes(const uint32_t *c, const uint32_t *bits, uint32_t *g, uint32_t *p, int m, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
        uint32_t cw[NW], bw[NW], gw[NW], pw[NW];
        mem.load(cw, c, i);
#pragma unroll 4
        for (int j = 0; j < m; j++) {
            const int bit = m - 1 - j;
            mem.once(bw, bits, (int64_t)bit * count + i);
            fxp_leaf_elem<NL, NW>(gw, pw, word_bit<NW>(cw, bit), bw, P);
            mem.store(g, (int64_t)j * count + i, gw);
            mem.store(p, (int64_t)j * count + i, pw);
        }
#pragma unroll
        for (int q = 0; q < NW; q++) { gw[q] = q == 0 ? 1u : 0u; pw[q] = 0u; }
        mem.store(g, (int64_t)m * count + i, gw);
        mem.store(p, (int64_t)m * count + i, pw);
    }
    template <int NL, int NW, class Mem>
    HB_HD static void run(const LeavesArgs &A, int, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
        planes<NL, NW>(A.c, A.bits, A.g, A.p, A.m, i, count, mem, P);
    }
};

// triple t of the level: node t / 2; its first factor is p1, its second g2 (t even) or p2 (t odd)
struct FxpCarryMaskArgs { const uint32_t *g, *p, *ta, *tb; uint32_t *masked; };

struct FxpCarryMaskRow {
    template <int NL, int NW, class Mem>
    HB_HD static void run(const FxpCarryMaskArgs &A, int y, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
        const int64_t t = y, node = t >> 1;
        uint32_t p1[NW], yw[NW], aw[NW], bw[NW], o0[NW], o1[NW];
        mem.load(p1, A.p, (2 * node) * count + i);
        mem.load(yw, (t & 1) ? A.p : A.g, (2 * node + 1) * count + i);
        mem.once(aw, A.ta, t * count + i);
        mem.once(bw, A.tb, t * count + i);
        diff_elem<NL, NW>(o0, p1, aw, P);
        diff_elem<NL, NW>(o1, yw, bw, P);
        mem.store(A.masked, (2 * t) * count + i, o0);
        mem.store(A.masked, (2 * t + 1) * count + i, o1);
    }
};

// node j of the next level: from planes 2j, 2j + 1, or plane 2j alone moved up (an odd count of planes)
struct FxpCarryCombineArgs { const uint32_t *opened, *g, *p, *ta, *tb, *tab; uint32_t *g_out, *p_out; int pairs, root; };

struct FxpCarryCombineRow {
    template <int NL, int NW, class Mem>
    HB_HD static void run(const FxpCarryCombineArgs &A, int y, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
        const int64_t j = y;
        uint32_t g1[NW], dw[NW], ew[NW], aw[NW], bw[NW], abw[NW], ow[NW];
        mem.load(g1, A.g, (2 * j) * count + i);
        if (j >= A.pairs) {                                                     // both loads ahead of the stores
            mem.load(ow, A.p, (2 * j) * count + i);
            mem.store(A.g_out, j * count + i, g1);
            mem.store(A.p_out, j * count + i, ow);
            return;
        }
        int64_t t = 2 * j;
        mem.once(dw, A.opened, (2 * t) * count + i); mem.once(ew, A.opened, (2 * t + 1) * count + i);
        mem.once(aw, A.ta, t * count + i); mem.once(bw, A.tb, t * count + i); mem.once(abw, A.tab, t * count + i);
        fxp_node_g_elem<NL, NW>(ow, g1, dw, ew, aw, bw, abw, P);
        mem.store(A.g_out, j * count + i, ow);
        if (A.root) return;
        t = 2 * j + 1;
        mem.once(dw, A.opened, (2 * t) * count + i); mem.once(ew, A.opened, (2 * t + 1) * count + i);
        mem.once(aw, A.ta, t * count + i); mem.once(bw, A.tb, t * count + i); mem.once(abw, A.tab, t * count + i);
        ew_beaver_elem<NL, NW>(ow, dw, ew, aw, bw, abw, P);
        mem.store(A.p_out, j * count + i, ow);
    }
};

template <int NL> struct FxpFinishArgs { const uint32_t *x, *c, *r1, *carry; uint32_t *out; int m, mode; FxpFinishConsts<NL> K; };

struct FxpFinishRow {
    template <int NL, int NW, class Mem>
    HB_HD static void run(const FxpFinishArgs<NL> &A, int, int64_t i, int64_t, const Mem &mem, const FpParams<NL> &P) {
        uint32_t xw[NW], cw[NW], rw[NW], kw[NW], ow[NW];
        if (A.mode != HB_FXP_MOD) mem.load(xw, A.x, i);
        else {
#pragma unroll
            for (int q = 0; q < NW; q++) xw[q] = 0;
        }
        mem.once(cw, A.c, i); mem.once(rw, A.r1, i); mem.once(kw, A.carry, i);
        fxp_finish_elem<NL, NW>(ow, xw, cw, rw, kw, A.m, A.mode, A.K, P);
        mem.store(A.out, i, ow);
    }
};

// ---------------------------------------------------------------- host side
// the constants of a step from its parameters; false if inv2m is not below the modulus
template <int NL> static bool fxp_mask_consts(FxpMaskArgs<NL> &A, const FpParams<NL> &P, int k, int m, int kappa) {
    A.nbits = k + kappa; A.m = m;
    fxp_pow2<NL>(A.half.d, k - 1, false, P);
    return true;
}
template <int NL> static bool fxp_trunc_pr_consts(FxpTruncPrArgs<NL> &A, const FpParams<NL> &P, int m, const uint64_t *inv2m_host) {
    A.m = m;
    return host_mont<NL, words_of(NL)>(A.invm.d, P, inv2m_host);
}
template <int NL> static bool fxp_finish_consts(FxpFinishArgs<NL> &A, const FpParams<NL> &P, int m, int mode, const uint64_t *inv2m_host) {
    A.m = m; A.mode = mode;
    return fxp_finish_fill<NL>(A.K, P, m, mode, inv2m_host);
}

// nodes planes of a level; root: the level of two planes whose p is not wanted
static bool fxp_level_ok(int nodes, int root) { return nodes >= 2 && nodes <= 257 && (!root || nodes == 2); }
static int fxp_level_triples(int nodes, int root) { return root ? 1 : 2 * (nodes / 2); }

// host: the same rows over `count` elements
template <int NL, int NW>
static int selftest_fxp(const uint64_t *p_limbs, int what, const uint64_t *const *ops, const int64_t *params, uint64_t *const *outs, int64_t count) {
    FpParams<NL> P;
    fp_params_from_limbs(P, p_limbs);
    const int k = (int)params[0], m = (int)params[1], kappa = (int)params[2], aux = (int)params[3], root = (int)params[4];
    if (what == HB_FXP_SELFTEST_MASK) {
        FxpMaskArgs<NL> A = {u32(ops[0]), u32(ops[1]), u32(outs[0]), u32(outs[1])};
        fxp_mask_consts<NL>(A, P, k, m, kappa);
        if (A.x) host_rows<FxpMaskRow<true>, NL, NW>(A, 1, count, P);
        else host_rows<FxpMaskRow<false>, NL, NW>(A, 1, count, P);
    } else if (what == HB_FXP_SELFTEST_TRUNC_PR) {
        FxpTruncPrArgs<NL> A = {u32(ops[0]), u32(ops[1]), u32(ops[2]), u32(outs[0])};
        if (!fxp_trunc_pr_consts<NL>(A, P, m, ops[3])) return HB_ERR_BAD_ARG;
        host_rows<FxpTruncPrRow, NL, NW>(A, 1, count, P);
    } else if (what == HB_FXP_SELFTEST_LEAVES) {
        const LeavesArgs A = {u32(ops[0]), u32(ops[1]), u32(outs[0]), u32(outs[1]), m};
        host_rows<FxpLeavesRow, NL, NW>(A, 1, count, P);
    } else if (what == HB_FXP_SELFTEST_CARRY_MASK) {
        const FxpCarryMaskArgs A = {u32(ops[0]), u32(ops[1]), u32(ops[2]), u32(ops[3]), u32(outs[0])};
        host_rows<FxpCarryMaskRow, NL, NW>(A, fxp_level_triples(aux, root), count, P);
    } else if (what == HB_FXP_SELFTEST_CARRY_COMBINE) {
        const FxpCarryCombineArgs A = {u32(ops[0]), u32(ops[1]), u32(ops[2]), u32(ops[3]), u32(ops[4]), u32(ops[5]), u32(outs[0]), u32(outs[1]), aux / 2, root};
        host_rows<FxpCarryCombineRow, NL, NW>(A, (aux + 1) / 2, count, P);
    } else {
        FxpFinishArgs<NL> A = {u32(ops[0]), u32(ops[1]), u32(ops[2]), u32(ops[3]), u32(outs[0])};
        if (!fxp_finish_consts<NL>(A, P, m, aux, ops[4])) return HB_ERR_BAD_ARG;
        host_rows<FxpFinishRow, NL, NW>(A, 1, count, P);
    }
    return HB_OK;
}

}  // namespace hb

extern "C" {

int hb_fxp_mask(hb_ctx *ctx, const uint64_t *x_dev, const uint64_t *bits_dev, int k, int m, int kappa, uint64_t *masked_dev, uint64_t *r1_dev, int64_t count,
                void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0 || (count > 0 && (!bits_dev || !masked_dev || !r1_dev))) return HB_ERR_BAD_ARG;
    if (!fxp_params_ok(modulus_bits(ctx->p_limbs, ctx->n_limbs), k, m, kappa))
        return fail(ctx, HB_ERR_BAD_ARG, "hb_fxp_mask: needs 0 < m < k, kappa >= 0 and k + kappa + 1 <= bits(p) - 1");
    if (count > 0 && masked_dev == r1_dev) return fail(ctx, HB_ERR_BAD_ARG, "hb_fxp_mask: masked and r1 are one array");
    if (count == 0) return HB_OK;
    HB_ROW_BLOCKS(ctx, "hb_fxp_mask");
    const auto fill = [&](auto &A, const auto &P) {
        A.x = u32(x_dev); A.bits = u32(bits_dev); A.masked = u32(masked_dev); A.r1 = u32(r1_dev);
        return fxp_mask_consts(A, P, k, m, kappa);
    };
    if (x_dev) return launch_rows<FxpMaskRow<true>, FxpMaskArgs>(ctx, fill, (unsigned)blocks, s, count);
    return launch_rows<FxpMaskRow<false>, FxpMaskArgs>(ctx, fill, (unsigned)blocks, s, count);
}

int hb_fxp_trunc_pr(hb_ctx *ctx, const uint64_t *x_dev, const uint64_t *c_dev, const uint64_t *r1_dev, int m, const uint64_t *inv2m_host, uint64_t *out_dev,
                    int64_t count, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0 || !inv2m_host || (count > 0 && (!x_dev || !c_dev || !r1_dev || !out_dev))) return HB_ERR_BAD_ARG;
    if (!fxp_m_ok(modulus_bits(ctx->p_limbs, ctx->n_limbs), m)) return fail(ctx, HB_ERR_BAD_ARG, "hb_fxp_trunc_pr: needs 0 < m <= bits(p) - 2");
    HB_ROW_BLOCKS(ctx, "hb_fxp_trunc_pr");
    const int rc = launch_rows<FxpTruncPrRow, FxpTruncPrArgs>(ctx, [&](auto &A, const auto &P) {
        A.x = u32(x_dev); A.c = u32(c_dev); A.r1 = u32(r1_dev); A.out = u32(out_dev);
        return fxp_trunc_pr_consts(A, P, m, inv2m_host);
    }, (unsigned)blocks, s, count);
    return rc == HB_ERR_BAD_ARG ? fail(ctx, rc, "hb_fxp_trunc_pr: inv2m is not below the modulus") : rc;
}

int hb_fxp_ltl_leaves(hb_ctx *ctx, const uint64_t *c_dev, const uint64_t *bits_dev, int m, uint64_t *g_dev, uint64_t *p_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0 || (count > 0 && (!c_dev || !bits_dev || !g_dev || !p_dev))) return HB_ERR_BAD_ARG;
    if (!fxp_m_ok(modulus_bits(ctx->p_limbs, ctx->n_limbs), m)) return fail(ctx, HB_ERR_BAD_ARG, "hb_fxp_ltl_leaves: needs 0 < m <= bits(p) - 2");
    if (count == 0) return HB_OK;
    const RowSpan outs[2] = {{g_dev, m + 1}, {p_dev, m + 1}}, ins[2] = {{c_dev, 1}, {bits_dev, m}};
    if (!outputs_apart(outs, 2, ins, 2, 8 * (int64_t)ctx->n_limbs * count)) return fail(ctx, HB_ERR_BAD_ARG, "hb_fxp_ltl_leaves: g and p are arrays of their own");
    HB_ROW_BLOCKS(ctx, "hb_fxp_ltl_leaves");
    return launch_leaves<FxpLeavesRow>(ctx, {u32(c_dev), u32(bits_dev), u32(g_dev), u32(p_dev), m}, (unsigned)blocks, s, count);
}

int hb_fxp_carry_mask(hb_ctx *ctx, const uint64_t *g_dev, const uint64_t *p_dev, int nodes, int root, const uint64_t *ta_dev, const uint64_t *tb_dev,
                      uint64_t *masked_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0 || (count > 0 && (!g_dev || !p_dev || !ta_dev || !tb_dev || !masked_dev))) return HB_ERR_BAD_ARG;
    if (!fxp_level_ok(nodes, root)) return fail(ctx, HB_ERR_BAD_ARG, "hb_fxp_carry_mask: needs 2 <= nodes <= 257, and nodes == 2 at the root");
    if (count == 0) return HB_OK;
    const int triples = fxp_level_triples(nodes, root);
    const RowSpan outs[1] = {{masked_dev, 2 * triples}}, ins[4] = {{g_dev, nodes}, {p_dev, nodes}, {ta_dev, triples}, {tb_dev, triples}};
    if (!outputs_apart(outs, 1, ins, 4, 8 * (int64_t)ctx->n_limbs * count)) return fail(ctx, HB_ERR_BAD_ARG, "hb_fxp_carry_mask: masked is an array of its own");
    HB_ROW_BLOCKS(ctx, "hb_fxp_carry_mask");
    const FxpCarryMaskArgs A = {u32(g_dev), u32(p_dev), u32(ta_dev), u32(tb_dev), u32(masked_dev)};
    return launch_rows<FxpCarryMaskRow>(ctx, A, dim3((unsigned)blocks, (unsigned)triples), s, count);
}

int hb_fxp_carry_combine(hb_ctx *ctx, const uint64_t *opened_dev, const uint64_t *g_dev, const uint64_t *p_dev, int nodes, int root, const uint64_t *ta_dev,
                         const uint64_t *tb_dev, const uint64_t *tab_dev, uint64_t *g_out_dev, uint64_t *p_out_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0 || (count > 0 && (!opened_dev || !g_dev || !p_dev || !ta_dev || !tb_dev || !tab_dev || !g_out_dev || (!root && !p_out_dev)))) return HB_ERR_BAD_ARG;
    if (!fxp_level_ok(nodes, root)) return fail(ctx, HB_ERR_BAD_ARG, "hb_fxp_carry_combine: needs 2 <= nodes <= 257, and nodes == 2 at the root");
    if (count == 0) return HB_OK;
    const int pairs = nodes / 2, out_nodes = (nodes + 1) / 2, triples = fxp_level_triples(nodes, root);
    const RowSpan outs[2] = {{g_out_dev, out_nodes}, {root ? nullptr : p_out_dev, out_nodes}};
    const RowSpan ins[6] = {{g_dev, nodes}, {p_dev, nodes}, {opened_dev, 2 * triples}, {ta_dev, triples}, {tb_dev, triples}, {tab_dev, triples}};
    if (!outputs_apart(outs, 2, ins, 6, 8 * (int64_t)ctx->n_limbs * count)) return fail(ctx, HB_ERR_BAD_ARG, "hb_fxp_carry_combine: the outputs are arrays of their own");
    HB_ROW_BLOCKS(ctx, "hb_fxp_carry_combine");
    const FxpCarryCombineArgs A = {u32(opened_dev), u32(g_dev), u32(p_dev), u32(ta_dev), u32(tb_dev), u32(tab_dev), u32(g_out_dev), u32(p_out_dev), pairs, root};
    return launch_rows<FxpCarryCombineRow>(ctx, A, dim3((unsigned)blocks, (unsigned)out_nodes), s, count);
}

int hb_fxp_div2m_finish(hb_ctx *ctx, const uint64_t *x_dev, const uint64_t *c_dev, const uint64_t *r1_dev, const uint64_t *carry_dev, int m, const uint64_t *inv2m_host,
                        int mode, uint64_t *out_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0) return HB_ERR_BAD_ARG;
    if (mode != HB_FXP_MOD && mode != HB_FXP_TRUNC && mode != HB_FXP_NEG_TRUNC) return fail(ctx, HB_ERR_BAD_ARG, "hb_fxp_div2m_finish: unknown mode");
    if ((mode != HB_FXP_MOD && !inv2m_host) || (count > 0 && (!c_dev || !r1_dev || !carry_dev || !out_dev || (mode != HB_FXP_MOD && !x_dev)))) return HB_ERR_BAD_ARG;
    if (!fxp_m_ok(modulus_bits(ctx->p_limbs, ctx->n_limbs), m)) return fail(ctx, HB_ERR_BAD_ARG, "hb_fxp_div2m_finish: needs 0 < m <= bits(p) - 2");
    HB_ROW_BLOCKS(ctx, "hb_fxp_div2m_finish");
    const int rc = launch_rows<FxpFinishRow, FxpFinishArgs>(ctx, [&](auto &A, const auto &P) {
        A.x = u32(x_dev); A.c = u32(c_dev); A.r1 = u32(r1_dev); A.carry = u32(carry_dev); A.out = u32(out_dev);
        return fxp_finish_consts(A, P, m, mode, inv2m_host);
    }, (unsigned)blocks, s, count);
    return rc == HB_ERR_BAD_ARG ? fail(ctx, rc, "hb_fxp_div2m_finish: inv2m is not below the modulus") : rc;
}

int hb_selftest_fxp(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *operands, const int64_t *params, uint64_t *const *outs, int64_t count) {
    if (!p_limbs || !operands || !params || !outs || count < 0 || (n_limbs != 1 && n_limbs != 4)) return HB_ERR_BAD_ARG;
    for (int i = 0; i < 5; i++) if (params[i] < -(1 << 30) || params[i] > (1 << 30)) return HB_ERR_BAD_ARG;
    const int bits = modulus_bits(p_limbs, n_limbs);
    const int k = (int)params[0], m = (int)params[1], kappa = (int)params[2], aux = (int)params[3], root = (int)params[4];
    int n_ops = 0, n_outs = 1, first_op = 0;
    switch (what) {
    case HB_FXP_SELFTEST_MASK: if (!fxp_params_ok(bits, k, m, kappa)) return HB_ERR_BAD_ARG; n_ops = 2; n_outs = 2; first_op = 1; break;
    case HB_FXP_SELFTEST_TRUNC_PR: if (!fxp_m_ok(bits, m) || !operands[3]) return HB_ERR_BAD_ARG; n_ops = 4; break;
    case HB_FXP_SELFTEST_LEAVES: if (!fxp_m_ok(bits, m)) return HB_ERR_BAD_ARG; n_ops = 2; n_outs = 2; break;
    case HB_FXP_SELFTEST_CARRY_MASK: if (!fxp_level_ok(aux, root)) return HB_ERR_BAD_ARG; n_ops = 4; break;
    case HB_FXP_SELFTEST_CARRY_COMBINE: if (!fxp_level_ok(aux, root)) return HB_ERR_BAD_ARG; n_ops = 6; n_outs = root ? 1 : 2; break;
    case HB_FXP_SELFTEST_FINISH:
        if (!fxp_m_ok(bits, m) || (aux != HB_FXP_MOD && aux != HB_FXP_TRUNC && aux != HB_FXP_NEG_TRUNC) || (aux != HB_FXP_MOD && !operands[4])) return HB_ERR_BAD_ARG;
        n_ops = 4; first_op = aux == HB_FXP_MOD ? 1 : 0; break;
    default: return HB_ERR_BAD_ARG;
    }
    for (int i = first_op; i < n_ops; i++) if (count > 0 && !operands[i]) return HB_ERR_BAD_ARG;
    for (int i = 0; i < n_outs; i++) if (count > 0 && !outs[i]) return HB_ERR_BAD_ARG;
    if (n_limbs == 4) return selftest_fxp<9, 8>(p_limbs, what, operands, params, outs, count);
    return selftest_fxp<3, 2>(p_limbs, what, operands, params, outs, count);
}

}  // extern "C"

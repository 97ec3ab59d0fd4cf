// hb_bd.hip -- bit decomposition of shared values (Catrina and de Hoogh's BitDec on the masks of hb_fxp.hip): shares of the low m bits
// of a signed k-bit value, for arrays of values.
//
// After the open of c = x + 2^(k-1) + r1 + 2^m r2 (hb_fxp_mask) the bits wanted are those of (c2 - r1) mod 2^m = c2 + (2^m - 1 - r1) + 1
// mod 2^m with c2 = c mod 2^m public and b_i the bit shares of r1.  hb_fxp.hip runs the carry tree of that sum and keeps its root; here
// a Sklansky parallel prefix network over the same (generate, propagate) leaves keeps EVERY carry, at the tree's depth, and one product
// a bit turns carries into sum bits.  N = m - 1 planes (bits 0 .. m - 2: the carry out of bit m - 1 is never used), least significant
// first, updated in place.
//
// The steps are rows under the generic kernel k_rows (hb_rows.hpp); the leaves' row runs under k_leaves (hb_fxp_elem.hpp):
// BdLeavesRow          plane i < m - 1 from bit i of c2 (public) and b_i with no product, fxp_leaf_elem: a_i = 1 -> (1 - b_i, b_i),
//                      a_i = 0 -> (0, 1 - b_i); the carry-in 1 is folded into plane 0: (g_0 + p_0, 0).
// BdPrefixMaskRow / BdPrefixCombineRow   level l: node y is plane j = ((y >> l) << (l + 1)) | (1 << l) | (y & ((1 << l) - 1)) while
//                      j <= N - 1, its partner q = ((j >> l) << l) - 1, and (g_j, p_j) <- (g_j + p_j g_q, p_j p_q).  Bit l of q is clear,
//                      so q is no node of level l and the level runs in place.  The nodes y < 2^l lie in the block that starts at plane
//                      0, whose p is 0 after the fold: they are g-only, ONE product, p never written (and never read again: such a j has
//                      no bit above l set).  With G = min(2^l, active) the g-only node y takes triple row y, the full node y rows
//                      G + 2 (y - G) [p_j g_q] and G + 2 (y - G) + 1 [p_j p_q].  The mask writes the two masked differences of every
//                      product of the level into one array (one thread a triple), the combine takes that array opened and updates the
//                      planes (one thread a node).  After the last level plane i holds the carry into bit i + 1.
// BdSumMaskRow / BdSumCombineRow   s_0 = a_0 xor b_0 is a select; s_i = p_i + C_i - 2 p_i C_i with p_i the leaf's propagate, recomputed
//                      from bit i of c and plane i of `bits` (not kept), and C_i = g of plane i - 1: m - 1 products in one batch.
//
// Operands and results are packed canonical residues.  The per-element bodies are HB_HD functions (hb_fxp_elem.hpp, hb_ew_elem.hpp and
// below); a step's row -- which operands it loads, which body it calls, where it stores -- is an HB_HD function over a memory policy,
// so hb_selftest_bd runs on the host the very rows, arithmetic and addressing, that k_rows runs on the device.
//
// Launch shape (all kernels): 256-thread workgroups, one element a thread in x, so a wave's accesses to a plane cover consecutive
// elements (64 x 32 bytes = 2 KiB, whole dwordx4 accesses); the triple / node / plane in blockIdx.y (BdLeavesRow walks the planes in
// the thread: c is read once).  No LDS, no grid stride, one launch a call.  Triples, opened values and bit planes are read once and
// take the non-temporal loads (load_once); p_j, which the two triples of a full node both read, and c, which every plane of the
// sum step reads, take the plain ones and are served from cache the second time.
// Compiler's report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; scratch = 0 bytes for every kernel):
//   BdLeavesRow<9, 8>          56 VGPRs: 8 waves a SIMD                            BdLeavesRow<3, 2>          56 VGPRs: 8 waves
//   BdPrefixMaskRow<9, 8>      41 VGPRs: 8 waves                                   BdPrefixMaskRow<3, 2>      15 VGPRs: 8 waves
//   BdPrefixCombineRow<9, 8>   74 VGPRs: 6 waves                                   BdPrefixCombineRow<3, 2>   32 VGPRs: 8 waves
//   BdSumMaskRow<9, 8>         40 VGPRs: 8 waves                                   BdSumMaskRow<3, 2>         20 VGPRs: 8 waves
//   BdSumCombineRow<9, 8>      76 VGPRs: 6 waves                                   BdSumCombineRow<3, 2>      38 VGPRs: 8 waves
// (DESIGN.md section 3s has the schedule and the counts.)
#include "hb_common.hpp"
#include "hb_fxp_elem.hpp"

using namespace hb;

namespace hb {

// ---------------------------------------------------------------- the wiring (host and device)
// (bd_node, bd_partner, bd_levels and bd_active: hb_fxp_elem.hpp, shared with hb_div.hip)
// triple row t of a level with G g-only nodes -> its node; second: 0 the product p_j g_q, 1 the product p_j p_q
HB_HD int bd_triple_node(int t, int G, int &second) {
    second = t >= G ? ((t - G) & 1) : 0;
    return t < G ? t : G + ((t - G) >> 1);
}
HB_HD int bd_node_triple(int y, int G) { return y < G ? y : G + 2 * (y - G); }

static int bd_g_only(int n, int l) { const int a = bd_active(n, l); return a < (1 << l) ? a : (1 << l); }
static int bd_level_triples(int n, int l) { return 2 * bd_active(n, l) - bd_g_only(n, l); }

// ---------------------------------------------------------------- per-element bodies (host and device)
// the carry-in 1 folded into plane 0: (g, p) <- (g + p, 0)
template <int NL, int NW> HB_HD void bd_fold_elem(uint32_t (&gw)[NW], uint32_t (&pw)[NW], const FpParams<NL> &P) {
    uint32_t g[NL], p[NL], r[NL];
    unpack<NL, NW>(g, gw);
    unpack<NL, NW>(p, pw);
    fp_add<NL>(r, g, p, P);
    pack<NL, NW>(gw, r);
#pragma unroll
    for (int q = 0; q < NW; q++) pw[q] = 0u;
}

// s_0 = a xor b for a public bit a: a = 1 -> 1 - b, a = 0 -> b
template <int NL, int NW> HB_HD void bd_sum0_elem(uint32_t (&o)[NW], uint32_t a, const uint32_t (&bw)[NW], const FpParams<NL> &P) {
    uint32_t b[NL], one[NL], nb[NL];
    unpack<NL, NW>(b, bw);
    small_digits<NL>(one, 1);
    fp_sub<NL>(nb, one, b, P);
#pragma unroll
    for (int q = 0; q < NL; q++) nb[q] = a ? nb[q] : b[q];
    pack<NL, NW>(o, nb);
}

// the leaf's propagate of bit a against the share bw: a = 1 -> b, a = 0 -> 1 - b
template <int NL, int NW> HB_HD void bd_leaf_p_elem(uint32_t (&pw)[NW], uint32_t a, const uint32_t (&bw)[NW], const FpParams<NL> &P) {
    uint32_t gw[NW];
    fxp_leaf_elem<NL, NW>(gw, pw, a, bw, P);
}

// s = p + C - 2 [p C], the product by the fused Beaver step of hb_ew_elem.hpp
template <int NL, int NW>
HB_HD void bd_sum_elem(uint32_t (&o)[NW], const uint32_t (&pw)[NW], const uint32_t (&cw)[NW], const uint32_t (&dw)[NW], const uint32_t (&ew)[NW],
                       const uint32_t (&aw)[NW], const uint32_t (&bw)[NW], const uint32_t (&abw)[NW], const FpParams<NL> &P) {
    uint32_t mw[NW], mm[NL], x[NL], y[NL], t[NL];
    ew_beaver_elem<NL, NW>(mw, dw, ew, aw, bw, abw, P);
    unpack<NL, NW>(mm, mw);
    unpack<NL, NW>(x, pw);
    unpack<NL, NW>(y, cw);
    fp_add<NL>(t, x, y, P);
    fp_sub<NL>(x, t, mm, P);
    fp_sub<NL>(t, x, mm, P);
    pack<NL, NW>(o, t);
}

// ---------------------------------------------------------------- the steps' rows (host and device, over a memory policy: hb_rows.hpp)
// g, p: m - 1 planes each, distinct from c and bits (the body under k_leaves, hb_fxp_elem.hpp, which has the __restrict__)
struct BdLeavesRow {
    template <int NL, int NW, class Mem>
    HB_HD static void planes(const uint32_t *c, const uint32_t *bits, uint32_t *g, uint32_t *p, int m, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
        uint32_t cw[NW], bw[NW], gw[NW], pw[NW];
        mem.load(cw, c, i);
#pragma unroll 4
        for (int j = 0; j < m - 1; j++) {
            mem.once(bw, bits, (int64_t)j * count + i);
            fxp_leaf_elem<NL, NW>(gw, pw, word_bit<NW>(cw, j), bw, P);
            if (j == 0) bd_fold_elem<NL, NW>(gw, pw, P);
            mem.store(g, (int64_t)j * count + i, gw);
            mem.store(p, (int64_t)j * count + i, pw);
        }
    }
    template <int NL, int NW, class Mem>
    HB_HD static void run(const LeavesArgs &A, int, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
        planes<NL, NW>(A.c, A.bits, A.g, A.p, A.m, i, count, mem, P);
    }
};

// One level.  The mask reads g and p; the combine works in place: g and p are read and written at plane j alone.
struct BdPrefixArgs { const uint32_t *opened, *ta, *tb, *tab; uint32_t *g, *p, *masked; int l, G; };

// triple t of level l: its first factor is p_j, its second g_q or p_q
struct BdPrefixMaskRow {
    template <int NL, int NW, class Mem>
    HB_HD static void run(const BdPrefixArgs &A, int y, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
        const int64_t t = y;
        int second;
        const int64_t j = bd_node(bd_triple_node(y, A.G, second), A.l), q = bd_partner((int)j, A.l);
        uint32_t p1[NW], yw[NW], aw[NW], bw[NW], o0[NW], o1[NW];
        mem.load(p1, A.p, j * count + i);
        mem.load(yw, second ? A.p : A.g, q * count + i);
        mem.once(aw, A.ta, t * count + i);
        mem.once(bw, A.tb, t * count + i);
        diff_elem<NL, NW>(o0, p1, aw, P);
        diff_elem<NL, NW>(o1, yw, bw, P);
        mem.store(A.masked, (2 * t) * count + i, o0);
        mem.store(A.masked, (2 * t + 1) * count + i, o1);
    }
};

// node y of level l
struct BdPrefixCombineRow {
    template <int NL, int NW, class Mem>
    HB_HD static void run(const BdPrefixArgs &A, int y, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
        update<NL, NW>(A.opened, A.ta, A.tb, A.tab, A, y, i, count, mem, P);
    }
    // what is only read is apart from the planes: __restrict__ (pointers in an argument struct do not carry it)
    template <int NL, int NW, class Mem>
    HB_HD static void update(const uint32_t *__restrict__ opened, const uint32_t *__restrict__ ta, const uint32_t *__restrict__ tb, const uint32_t *__restrict__ tab,
                             const BdPrefixArgs &A, int y, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
        const int64_t j = bd_node(y, A.l);
        int64_t t = bd_node_triple(y, A.G);
        uint32_t g1[NW], dw[NW], ew[NW], aw[NW], bw[NW], abw[NW], ow[NW];
        mem.load(g1, A.g, j * count + i);
        mem.once(dw, opened, (2 * t) * count + i); mem.once(ew, opened, (2 * t + 1) * count + i);
        mem.once(aw, ta, t * count + i); mem.once(bw, tb, t * count + i); mem.once(abw, tab, t * count + i);
        fxp_node_g_elem<NL, NW>(ow, g1, dw, ew, aw, bw, abw, P);
        mem.store(A.g, j * count + i, ow);
        if (y < A.G) return;
        t++;
        mem.once(dw, opened, (2 * t) * count + i); mem.once(ew, opened, (2 * t + 1) * count + i);
        mem.once(aw, ta, t * count + i); mem.once(bw, tb, t * count + i); mem.once(abw, tab, t * count + i);
        ew_beaver_elem<NL, NW>(ow, dw, ew, aw, bw, abw, P);
        mem.store(A.p, j * count + i, ow);
    }
};

// The sum step.  The mask writes `masked`, the combine `out`.
struct BdSumArgs { const uint32_t *opened, *c, *bits, *g, *ta, *tb, *tab; uint32_t *masked, *out; };

// triple t, the product of bit t + 1: the leaf's p_{t+1} times the carry g[t]
struct BdSumMaskRow {
    template <int NL, int NW, class Mem>
    HB_HD static void run(const BdSumArgs &A, int y, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
        const int64_t t = y;
        uint32_t cw[NW], xw[NW], pw[NW], aw[NW], bw[NW], o0[NW], o1[NW];
        mem.load(cw, A.c, i);
        mem.once(xw, A.bits, (t + 1) * count + i);
        bd_leaf_p_elem<NL, NW>(pw, word_bit<NW>(cw, y + 1), xw, P);
        mem.load(xw, A.g, t * count + i);
        mem.once(aw, A.ta, t * count + i);
        mem.once(bw, A.tb, t * count + i);
        diff_elem<NL, NW>(o0, pw, aw, P);
        diff_elem<NL, NW>(o1, xw, bw, P);
        mem.store(A.masked, (2 * t) * count + i, o0);
        mem.store(A.masked, (2 * t + 1) * count + i, o1);
    }
};

// plane b of the result
struct BdSumCombineRow {
    template <int NL, int NW, class Mem>
    HB_HD static void run(const BdSumArgs &A, int y, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
        const int64_t b = y, t = b - 1;
        uint32_t cw[NW], xw[NW], pw[NW], gw[NW], dw[NW], ew[NW], aw[NW], bw[NW], abw[NW], ow[NW];
        mem.load(cw, A.c, i);
        mem.once(xw, A.bits, b * count + i);
        if (b == 0) {
            bd_sum0_elem<NL, NW>(ow, word_bit<NW>(cw, 0), xw, P);
            mem.store(A.out, i, ow);
            return;
        }
        bd_leaf_p_elem<NL, NW>(pw, word_bit<NW>(cw, y), xw, P);
        mem.once(gw, A.g, t * count + i);
        mem.once(dw, A.opened, (2 * t) * count + i); mem.once(ew, A.opened, (2 * t + 1) * count + i);
        mem.once(aw, A.ta, t * count + i); mem.once(bw, A.tb, t * count + i); mem.once(abw, A.tab, t * count + i);
        bd_sum_elem<NL, NW>(ow, pw, gw, dw, ew, aw, bw, abw, P);
        mem.store(A.out, b * count + i, ow);
    }
};

// ---------------------------------------------------------------- host: the same rows over `count` elements
template <int NL, int NW>
static int selftest_bd(const uint64_t *p_limbs, int what, const uint64_t *const *ops, const int64_t *params, uint64_t *const *outs, int64_t count) {
    FpParams<NL> P;
    fp_params_from_limbs(P, p_limbs);
    const int m = (int)params[0], l = (int)params[1], n = m - 1;
    if (what == HB_BD_SELFTEST_LEAVES) {
        const LeavesArgs A = {u32(ops[0]), u32(ops[1]), u32(outs[0]), u32(outs[1]), m};
        host_rows<BdLeavesRow, NL, NW>(A, n ? 1 : 0, count, P);                  // m == 1: no plane, and c is not looked at
    } else if (what == HB_BD_SELFTEST_PREFIX_MASK) {
        const BdPrefixArgs A = {nullptr, u32(ops[2]), u32(ops[3]), nullptr, const_cast<uint32_t *>(u32(ops[0])), const_cast<uint32_t *>(u32(ops[1])), u32(outs[0]), l, bd_g_only(n, l)};
        host_rows<BdPrefixMaskRow, NL, NW>(A, bd_level_triples(n, l), count, P);
    } else if (what == HB_BD_SELFTEST_PREFIX_COMBINE) {
        const BdPrefixArgs A = {u32(ops[0]), u32(ops[1]), u32(ops[2]), u32(ops[3]), u32(outs[0]), u32(outs[1]), nullptr, l, bd_g_only(n, l)};
        host_rows<BdPrefixCombineRow, NL, NW>(A, bd_active(n, l), count, P);
    } else if (what == HB_BD_SELFTEST_SUM_MASK) {
        const BdSumArgs A = {nullptr, u32(ops[0]), u32(ops[1]), u32(ops[2]), u32(ops[3]), u32(ops[4]), nullptr, u32(outs[0]), nullptr};
        host_rows<BdSumMaskRow, NL, NW>(A, n, count, P);
    } else {
        const BdSumArgs A = {u32(ops[0]), u32(ops[1]), u32(ops[2]), u32(ops[3]), u32(ops[4]), u32(ops[5]), u32(ops[6]), nullptr, u32(outs[0])};
        host_rows<BdSumCombineRow, NL, NW>(A, m, count, P);
    }
    return HB_OK;
}

// m within the modulus and at most 256 planes
static bool bd_m_ok(int bits, int m) { return fxp_m_ok(bits, m) && m - 1 <= 256; }
static bool bd_level_ok(int m, int level) { return level >= 0 && level < bd_levels(m - 1); }

}  // namespace hb

extern "C" {

int hb_bd_leaves(hb_ctx *ctx, const uint64_t *c_dev, const uint64_t *bits_dev, int m, uint64_t *g_dev, uint64_t *p_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0) return HB_ERR_BAD_ARG;
    if (!bd_m_ok(modulus_bits(ctx->p_limbs, ctx->n_limbs), m)) return fail(ctx, HB_ERR_BAD_ARG, "hb_bd_leaves: needs 0 < m <= bits(p) - 2 and m - 1 <= 256");
    if (count > 0 && m > 1 && (!c_dev || !bits_dev || !g_dev || !p_dev)) return HB_ERR_BAD_ARG;
    if (count == 0 || m == 1) return HB_OK;
    const RowSpan outs[2] = {{g_dev, m - 1}, {p_dev, m - 1}}, ins[2] = {{c_dev, 1}, {bits_dev, m - 1}};
    if (!outputs_apart(outs, 2, ins, 2, 8 * (int64_t)ctx->n_limbs * count)) return fail(ctx, HB_ERR_BAD_ARG, "hb_bd_leaves: g and p are arrays of their own");
    HB_ROW_BLOCKS(ctx, "hb_bd_leaves");
    return launch_leaves<BdLeavesRow>(ctx, {u32(c_dev), u32(bits_dev), u32(g_dev), u32(p_dev), m}, (unsigned)blocks, s, count);
}

int hb_bd_prefix_mask(hb_ctx *ctx, const uint64_t *g_dev, const uint64_t *p_dev, int m, int level, const uint64_t *ta_dev, const uint64_t *tb_dev,
                      uint64_t *masked_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0 || (count > 0 && (!g_dev || !p_dev || !ta_dev || !tb_dev || !masked_dev))) return HB_ERR_BAD_ARG;
    if (!bd_m_ok(modulus_bits(ctx->p_limbs, ctx->n_limbs), m)) return fail(ctx, HB_ERR_BAD_ARG, "hb_bd_prefix_mask: needs 0 < m <= bits(p) - 2 and m - 1 <= 256");
    if (!bd_level_ok(m, level)) return fail(ctx, HB_ERR_BAD_ARG, "hb_bd_prefix_mask: no such level");
    if (count == 0) return HB_OK;
    const int n = m - 1, triples = bd_level_triples(n, level);
    const RowSpan outs[1] = {{masked_dev, 2 * triples}}, ins[4] = {{g_dev, n}, {p_dev, n}, {ta_dev, triples}, {tb_dev, triples}};
    if (!outputs_apart(outs, 1, ins, 4, 8 * (int64_t)ctx->n_limbs * count)) return fail(ctx, HB_ERR_BAD_ARG, "hb_bd_prefix_mask: masked is an array of its own");
    HB_ROW_BLOCKS(ctx, "hb_bd_prefix_mask");
    const BdPrefixArgs A = {nullptr, u32(ta_dev), u32(tb_dev), nullptr, const_cast<uint32_t *>(u32(g_dev)), const_cast<uint32_t *>(u32(p_dev)), u32(masked_dev), level,
                            bd_g_only(n, level)};
    return launch_rows<BdPrefixMaskRow>(ctx, A, dim3((unsigned)blocks, (unsigned)triples), s, count);
}

int hb_bd_prefix_combine(hb_ctx *ctx, const uint64_t *opened_dev, uint64_t *g_dev, uint64_t *p_dev, int m, int level, const uint64_t *ta_dev,
                         const uint64_t *tb_dev, const uint64_t *tab_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0 || (count > 0 && (!opened_dev || !g_dev || !p_dev || !ta_dev || !tb_dev || !tab_dev))) return HB_ERR_BAD_ARG;
    if (!bd_m_ok(modulus_bits(ctx->p_limbs, ctx->n_limbs), m)) return fail(ctx, HB_ERR_BAD_ARG, "hb_bd_prefix_combine: needs 0 < m <= bits(p) - 2 and m - 1 <= 256");
    if (!bd_level_ok(m, level)) return fail(ctx, HB_ERR_BAD_ARG, "hb_bd_prefix_combine: no such level");
    if (count == 0) return HB_OK;
    const int n = m - 1, triples = bd_level_triples(n, level);
    const RowSpan outs[2] = {{g_dev, n}, {p_dev, n}}, ins[4] = {{opened_dev, 2 * triples}, {ta_dev, triples}, {tb_dev, triples}, {tab_dev, triples}};
    if (!outputs_apart(outs, 2, ins, 4, 8 * (int64_t)ctx->n_limbs * count)) return fail(ctx, HB_ERR_BAD_ARG, "hb_bd_prefix_combine: g and p are arrays of their own");
    HB_ROW_BLOCKS(ctx, "hb_bd_prefix_combine");
    const BdPrefixArgs A = {u32(opened_dev), u32(ta_dev), u32(tb_dev), u32(tab_dev), u32(g_dev), u32(p_dev), nullptr, level, bd_g_only(n, level)};
    return launch_rows<BdPrefixCombineRow>(ctx, A, dim3((unsigned)blocks, (unsigned)bd_active(n, level)), s, count);
}

int hb_bd_sum_mask(hb_ctx *ctx, const uint64_t *c_dev, const uint64_t *bits_dev, const uint64_t *g_dev, int m, const uint64_t *ta_dev, const uint64_t *tb_dev,
                   uint64_t *masked_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0) return HB_ERR_BAD_ARG;
    if (!bd_m_ok(modulus_bits(ctx->p_limbs, ctx->n_limbs), m)) return fail(ctx, HB_ERR_BAD_ARG, "hb_bd_sum_mask: needs 0 < m <= bits(p) - 2 and m - 1 <= 256");
    if (count > 0 && m > 1 && (!c_dev || !bits_dev || !g_dev || !ta_dev || !tb_dev || !masked_dev)) return HB_ERR_BAD_ARG;
    if (count == 0 || m == 1) return HB_OK;
    const RowSpan outs[1] = {{masked_dev, 2 * (m - 1)}}, ins[5] = {{c_dev, 1}, {bits_dev, m}, {g_dev, m - 1}, {ta_dev, m - 1}, {tb_dev, m - 1}};
    if (!outputs_apart(outs, 1, ins, 5, 8 * (int64_t)ctx->n_limbs * count)) return fail(ctx, HB_ERR_BAD_ARG, "hb_bd_sum_mask: masked is an array of its own");
    HB_ROW_BLOCKS(ctx, "hb_bd_sum_mask");
    const BdSumArgs A = {nullptr, u32(c_dev), u32(bits_dev), u32(g_dev), u32(ta_dev), u32(tb_dev), nullptr, u32(masked_dev), nullptr};
    return launch_rows<BdSumMaskRow>(ctx, A, dim3((unsigned)blocks, (unsigned)(m - 1)), s, count);
}

int hb_bd_sum_combine(hb_ctx *ctx, const uint64_t *opened_dev, const uint64_t *c_dev, const uint64_t *bits_dev, const uint64_t *g_dev, int m, const uint64_t *ta_dev,
                      const uint64_t *tb_dev, const uint64_t *tab_dev, uint64_t *out_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0) return HB_ERR_BAD_ARG;
    if (!bd_m_ok(modulus_bits(ctx->p_limbs, ctx->n_limbs), m)) return fail(ctx, HB_ERR_BAD_ARG, "hb_bd_sum_combine: needs 0 < m <= bits(p) - 2 and m - 1 <= 256");
    if (count > 0 && (!c_dev || !bits_dev || !out_dev || (m > 1 && (!opened_dev || !g_dev || !ta_dev || !tb_dev || !tab_dev)))) return HB_ERR_BAD_ARG;
    if (count == 0) return HB_OK;
    const bool prod = m > 1;                                                    // with m == 1 there is no product: its operands are not looked at
    const RowSpan outs[1] = {{out_dev, m}};
    const RowSpan ins[7] = {{c_dev, 1}, {bits_dev, m}, {prod ? opened_dev : nullptr, 2 * (m - 1)}, {prod ? g_dev : nullptr, m - 1}, {prod ? ta_dev : nullptr, m - 1},
                            {prod ? tb_dev : nullptr, m - 1}, {prod ? tab_dev : nullptr, m - 1}};
    if (!outputs_apart(outs, 1, ins, 7, 8 * (int64_t)ctx->n_limbs * count)) return fail(ctx, HB_ERR_BAD_ARG, "hb_bd_sum_combine: out is an array of its own");
    HB_ROW_BLOCKS(ctx, "hb_bd_sum_combine");
    const BdSumArgs A = {u32(opened_dev), u32(c_dev), u32(bits_dev), u32(g_dev), u32(ta_dev), u32(tb_dev), u32(tab_dev), nullptr, u32(out_dev)};
    return launch_rows<BdSumCombineRow>(ctx, A, dim3((unsigned)blocks, (unsigned)m), s, count);
}

int hb_selftest_bd(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *operands, const int64_t *params, uint64_t *const *outs, int64_t count) {
    if (!p_limbs || !operands || !params || !outs || count < 0 || (n_limbs != 1 && n_limbs != 4)) return HB_ERR_BAD_ARG;
    for (int i = 0; i < 2; i++) if (params[i] < -(1 << 30) || params[i] > (1 << 30)) return HB_ERR_BAD_ARG;
    const int m = (int)params[0], level = (int)params[1];
    if (!bd_m_ok(modulus_bits(p_limbs, n_limbs), m)) return HB_ERR_BAD_ARG;
    int n_ops = 0, n_outs = 1;
    switch (what) {
    case HB_BD_SELFTEST_LEAVES: n_ops = 2; n_outs = 2; break;
    case HB_BD_SELFTEST_PREFIX_MASK: if (!bd_level_ok(m, level)) return HB_ERR_BAD_ARG; n_ops = 4; break;
    case HB_BD_SELFTEST_PREFIX_COMBINE: if (!bd_level_ok(m, level)) return HB_ERR_BAD_ARG; n_ops = 4; n_outs = 2; break;
    case HB_BD_SELFTEST_SUM_MASK: n_ops = 5; break;
    case HB_BD_SELFTEST_SUM_COMBINE: n_ops = 7; break;
    default: return HB_ERR_BAD_ARG;
    }
    // with m == 1 there is no plane and no product: only c, bits and the result of the sum step are looked at
    for (int i = 0; i < n_ops; i++)
        if (count > 0 && !operands[i] && (m > 1 || (what == HB_BD_SELFTEST_SUM_COMBINE && (i == 1 || i == 2)))) return HB_ERR_BAD_ARG;
    for (int i = 0; i < n_outs; i++)
        if (count > 0 && !outs[i] && (m > 1 || what == HB_BD_SELFTEST_SUM_COMBINE)) return HB_ERR_BAD_ARG;
    if (n_limbs == 4) return selftest_bd<9, 8>(p_limbs, what, operands, params, outs, count);
    return selftest_bd<3, 2>(p_limbs, what, operands, params, outs, count);
}

}  // extern "C"

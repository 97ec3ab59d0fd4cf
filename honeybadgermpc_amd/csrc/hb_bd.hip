// hb_bd.hip -- bit decomposition of shared values (Catrina and de Hoogh's BitDec on the masks of hb_fxp.hip): shares of the low m bits
// of a signed k-bit value, for arrays of values.
//
// After the open of c = x + 2^(k-1) + r1 + 2^m r2 (hb_fxp_mask) the bits wanted are those of (c2 - r1) mod 2^m = c2 + (2^m - 1 - r1) + 1
// mod 2^m with c2 = c mod 2^m public and b_i the bit shares of r1.  hb_fxp.hip runs the carry tree of that sum and keeps its root; here
// a Sklansky parallel prefix network over the same (generate, propagate) leaves keeps EVERY carry, at the tree's depth, and one product
// a bit turns carries into sum bits.  N = m - 1 planes (bits 0 .. m - 2: the carry out of bit m - 1 is never used), least significant
// first, updated in place.
//
// k_bd_leaves          plane i < m - 1 from bit i of c2 (public) and b_i with no product, fxp_leaf_elem: a_i = 1 -> (1 - b_i, b_i),
//                      a_i = 0 -> (0, 1 - b_i); the carry-in 1 is folded into plane 0: (g_0 + p_0, 0).
// k_bd_prefix_mask / k_bd_prefix_combine   level l: node y is plane j = ((y >> l) << (l + 1)) | (1 << l) | (y & ((1 << l) - 1)) while
//                      j <= N - 1, its partner q = ((j >> l) << l) - 1, and (g_j, p_j) <- (g_j + p_j g_q, p_j p_q).  Bit l of q is clear,
//                      so q is no node of level l and the level runs in place.  The nodes y < 2^l lie in the block that starts at plane
//                      0, whose p is 0 after the fold: they are g-only, ONE product, p never written (and never read again: such a j has
//                      no bit above l set).  With G = min(2^l, active) the g-only node y takes triple row y, the full node y rows
//                      G + 2 (y - G) [p_j g_q] and G + 2 (y - G) + 1 [p_j p_q].  The mask writes the two masked differences of every
//                      product of the level into one array (one thread a triple), the combine takes that array opened and updates the
//                      planes (one thread a node).  After the last level plane i holds the carry into bit i + 1.
// k_bd_sum_mask / k_bd_sum_combine   s_0 = a_0 xor b_0 is a select; s_i = p_i + C_i - 2 p_i C_i with p_i the leaf's propagate, recomputed
//                      from bit i of c and plane i of `bits` (not kept), and C_i = g of plane i - 1: m - 1 products in one batch.
//
// Operands and results are packed canonical residues.  The per-element bodies are HB_HD functions (hb_fxp_elem.hpp, hb_ew_elem.hpp and
// below): the __global__ wrappers only load, call them and store, and hb_selftest_bd runs the very same functions on the host.
//
// Launch shape (all kernels): 256-thread workgroups, one element a thread in x, so a wave's accesses to a plane cover consecutive
// elements (64 x 32 bytes = 2 KiB, whole dwordx4 accesses); the triple / node / plane in blockIdx.y (k_bd_leaves walks the planes in
// the thread: c is read once).  No LDS, no grid stride, one launch a call.  Triples, opened values and bit planes are read once and
// take the non-temporal loads (fxp_load_once); p_j, which the two triples of a full node both read, and c, which every plane of the
// sum step reads, take the plain ones and are served from cache the second time.
// Compiler's report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; scratch = 0 bytes for every kernel):
//   k_bd_leaves<9, 8>          56 VGPRs: 8 waves a SIMD                            k_bd_leaves<3, 2>          56 VGPRs: 8 waves
//   k_bd_prefix_mask<9, 8>     38 VGPRs: 8 waves                                   k_bd_prefix_mask<3, 2>     15 VGPRs: 8 waves
//   k_bd_prefix_combine<9, 8>  74 VGPRs: 6 waves                                   k_bd_prefix_combine<3, 2>  33 VGPRs: 8 waves
//   k_bd_sum_mask<9, 8>        40 VGPRs: 8 waves                                   k_bd_sum_mask<3, 2>        22 VGPRs: 8 waves
//   k_bd_sum_combine<9, 8>     77 VGPRs: 6 waves                                   k_bd_sum_combine<3, 2>     39 VGPRs: 8 waves
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
#pragma unroll
    for (int q = 0; q < NL; q++) one[q] = q == 0 ? 1u : 0u;
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

// ---------------------------------------------------------------- kernels
// g, p: m - 1 planes each, distinct from c and bits
template <int NL, int NW>
__global__ void __launch_bounds__(256) k_bd_leaves(const FpParams<NL> P, const uint32_t *__restrict__ c, const uint32_t *__restrict__ bits, int m,
                                                   uint32_t *__restrict__ g, uint32_t *__restrict__ p, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    uint32_t cw[NW], bw[NW], gw[NW], pw[NW];
    load_words<NW>(cw, c + i * NW);
#pragma unroll 4
    for (int j = 0; j < m - 1; j++) {
        fxp_load_once<NW>(bw, bits + ((int64_t)j * count + i) * NW);
        fxp_leaf_elem<NL, NW>(gw, pw, fxp_bit<NW>(cw, j), bw, P);
        if (j == 0) bd_fold_elem<NL, NW>(gw, pw, P);
        store_words<NW>(g + ((int64_t)j * count + i) * NW, gw);
        store_words<NW>(p + ((int64_t)j * count + i) * NW, pw);
    }
}

// triple t = blockIdx.y of level l: its first factor is p_j, its second g_q or p_q
template <int NL, int NW>
__global__ void __launch_bounds__(256) k_bd_prefix_mask(const FpParams<NL> P, const uint32_t *__restrict__ g, const uint32_t *__restrict__ p, int l, int G,
                                                        const uint32_t *__restrict__ ta, const uint32_t *__restrict__ tb, uint32_t *__restrict__ masked,
                                                        int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int64_t t = blockIdx.y;
    int second;
    const int64_t j = bd_node(bd_triple_node((int)t, G, second), l), q = bd_partner((int)j, l);
    uint32_t p1[NW], y[NW], aw[NW], bw[NW], o0[NW], o1[NW];
    load_words<NW>(p1, p + (j * count + i) * NW);
    load_words<NW>(y, (second ? p : g) + (q * count + i) * NW);
    fxp_load_once<NW>(aw, ta + (t * count + i) * NW);
    fxp_load_once<NW>(bw, tb + (t * count + i) * NW);
    fxp_diff_elem<NL, NW>(o0, p1, aw, P);
    fxp_diff_elem<NL, NW>(o1, y, bw, P);
    store_words<NW>(masked + ((2 * t) * count + i) * NW, o0);
    store_words<NW>(masked + ((2 * t + 1) * count + i) * NW, o1);
}

// node y = blockIdx.y of level l, in place: g and p are read and written at plane j alone (no __restrict__: they alias themselves)
template <int NL, int NW>
__global__ void __launch_bounds__(256) k_bd_prefix_combine(const FpParams<NL> P, const uint32_t *__restrict__ opened, uint32_t *g, uint32_t *p, int l, int G,
                                                           const uint32_t *__restrict__ ta, const uint32_t *__restrict__ tb, const uint32_t *__restrict__ tab,
                                                           int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int y = (int)blockIdx.y;
    const int64_t j = bd_node(y, l);
    int64_t t = bd_node_triple(y, G);
    uint32_t g1[NW], dw[NW], ew[NW], aw[NW], bw[NW], abw[NW], ow[NW];
    load_words<NW>(g1, g + (j * count + i) * NW);
    fxp_load_once<NW>(dw, opened + ((2 * t) * count + i) * NW); fxp_load_once<NW>(ew, opened + ((2 * t + 1) * count + i) * NW);
    fxp_load_once<NW>(aw, ta + (t * count + i) * NW); fxp_load_once<NW>(bw, tb + (t * count + i) * NW); fxp_load_once<NW>(abw, tab + (t * count + i) * NW);
    fxp_node_g_elem<NL, NW>(ow, g1, dw, ew, aw, bw, abw, P);
    store_words<NW>(g + (j * count + i) * NW, ow);
    if (y < G) return;
    t++;
    fxp_load_once<NW>(dw, opened + ((2 * t) * count + i) * NW); fxp_load_once<NW>(ew, opened + ((2 * t + 1) * count + i) * NW);
    fxp_load_once<NW>(aw, ta + (t * count + i) * NW); fxp_load_once<NW>(bw, tb + (t * count + i) * NW); fxp_load_once<NW>(abw, tab + (t * count + i) * NW);
    ew_beaver_elem<NL, NW>(ow, dw, ew, aw, bw, abw, P);
    store_words<NW>(p + (j * count + i) * NW, ow);
}

// triple t = blockIdx.y, the product of bit t + 1: the leaf's p_{t+1} times the carry g[t]
template <int NL, int NW>
__global__ void __launch_bounds__(256) k_bd_sum_mask(const FpParams<NL> P, const uint32_t *__restrict__ c, const uint32_t *__restrict__ bits,
                                                     const uint32_t *__restrict__ g, const uint32_t *__restrict__ ta, const uint32_t *__restrict__ tb,
                                                     uint32_t *__restrict__ masked, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int64_t t = blockIdx.y;
    uint32_t cw[NW], xw[NW], pw[NW], aw[NW], bw[NW], o0[NW], o1[NW];
    load_words<NW>(cw, c + i * NW);
    fxp_load_once<NW>(xw, bits + ((t + 1) * count + i) * NW);
    bd_leaf_p_elem<NL, NW>(pw, fxp_bit<NW>(cw, (int)t + 1), xw, P);
    load_words<NW>(xw, g + (t * count + i) * NW);
    fxp_load_once<NW>(aw, ta + (t * count + i) * NW);
    fxp_load_once<NW>(bw, tb + (t * count + i) * NW);
    fxp_diff_elem<NL, NW>(o0, pw, aw, P);
    fxp_diff_elem<NL, NW>(o1, xw, bw, P);
    store_words<NW>(masked + ((2 * t) * count + i) * NW, o0);
    store_words<NW>(masked + ((2 * t + 1) * count + i) * NW, o1);
}

// plane b = blockIdx.y of the result
template <int NL, int NW>
__global__ void __launch_bounds__(256) k_bd_sum_combine(const FpParams<NL> P, const uint32_t *__restrict__ opened, const uint32_t *__restrict__ c,
                                                        const uint32_t *__restrict__ bits, const uint32_t *__restrict__ g, const uint32_t *__restrict__ ta,
                                                        const uint32_t *__restrict__ tb, const uint32_t *__restrict__ tab, uint32_t *__restrict__ out,
                                                        int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int64_t b = blockIdx.y, t = b - 1;
    uint32_t cw[NW], xw[NW], pw[NW], gw[NW], dw[NW], ew[NW], aw[NW], bw[NW], abw[NW], ow[NW];
    load_words<NW>(cw, c + i * NW);
    fxp_load_once<NW>(xw, bits + (b * count + i) * NW);
    if (b == 0) {
        bd_sum0_elem<NL, NW>(ow, fxp_bit<NW>(cw, 0), xw, P);
        store_words<NW>(out + i * NW, ow);
        return;
    }
    bd_leaf_p_elem<NL, NW>(pw, fxp_bit<NW>(cw, (int)b), xw, P);
    fxp_load_once<NW>(gw, g + (t * count + i) * NW);
    fxp_load_once<NW>(dw, opened + ((2 * t) * count + i) * NW); fxp_load_once<NW>(ew, opened + ((2 * t + 1) * count + i) * NW);
    fxp_load_once<NW>(aw, ta + (t * count + i) * NW); fxp_load_once<NW>(bw, tb + (t * count + i) * NW); fxp_load_once<NW>(abw, tab + (t * count + i) * NW);
    bd_sum_elem<NL, NW>(ow, pw, gw, dw, ew, aw, bw, abw, P);
    store_words<NW>(out + (b * count + i) * NW, ow);
}

// ---------------------------------------------------------------- host: the same element functions over `count` elements
template <int NL, int NW>
static int selftest_bd(const uint64_t *p_limbs, int what, const uint64_t *const *ops, const int64_t *params, uint64_t *const *outs, int64_t count) {
    FpParams<NL> P;
    fp_params_from_limbs(P, p_limbs);
    const int m = (int)params[0], l = (int)params[1], n = m - 1;
    auto W = [](const uint64_t *base, int64_t i) -> const uint32_t (&)[NW] { return *reinterpret_cast<const uint32_t(*)[NW]>(reinterpret_cast<const uint32_t *>(base) + i * NW); };
    auto O = [](uint64_t *base, int64_t i) -> uint32_t * { return reinterpret_cast<uint32_t *>(base) + i * NW; };
    uint32_t r0[NW], r1[NW];
    if (what == HB_BD_SELFTEST_LEAVES) {
        for (int64_t i = 0; i < count; i++)
            for (int j = 0; j < n; j++) {
                fxp_leaf_elem<NL, NW>(r0, r1, fxp_bit<NW>(W(ops[0], i), j), W(ops[1], (int64_t)j * count + i), P);
                if (j == 0) bd_fold_elem<NL, NW>(r0, r1, P);
                memcpy(O(outs[0], (int64_t)j * count + i), r0, NW * 4);
                memcpy(O(outs[1], (int64_t)j * count + i), r1, NW * 4);
            }
    } else if (what == HB_BD_SELFTEST_PREFIX_MASK) {
        const int G = bd_g_only(n, l), triples = bd_level_triples(n, l);
        for (int64_t t = 0; t < triples; t++)
            for (int64_t i = 0; i < count; i++) {
                int second;
                const int64_t j = bd_node(bd_triple_node((int)t, G, second), l), q = bd_partner((int)j, l);
                fxp_diff_elem<NL, NW>(r0, W(ops[1], j * count + i), W(ops[2], t * count + i), P);
                fxp_diff_elem<NL, NW>(r1, W(second ? ops[1] : ops[0], q * count + i), W(ops[3], t * count + i), P);
                memcpy(O(outs[0], 2 * t * count + i), r0, NW * 4);
                memcpy(O(outs[0], (2 * t + 1) * count + i), r1, NW * 4);
            }
    } else if (what == HB_BD_SELFTEST_PREFIX_COMBINE) {
        const int G = bd_g_only(n, l), active = bd_active(n, l);
        for (int y = 0; y < active; y++)
            for (int64_t i = 0; i < count; i++) {
                const int64_t j = bd_node(y, l);
                int64_t t = bd_node_triple(y, G);
                uint32_t g1[NW];
                memcpy(g1, O(outs[0], j * count + i), NW * 4);
                fxp_node_g_elem<NL, NW>(r0, g1, W(ops[0], 2 * t * count + i), W(ops[0], (2 * t + 1) * count + i), W(ops[1], t * count + i), W(ops[2], t * count + i),
                                        W(ops[3], t * count + i), P);
                memcpy(O(outs[0], j * count + i), r0, NW * 4);
                if (y < G) continue;
                t++;
                ew_beaver_elem<NL, NW>(r1, W(ops[0], 2 * t * count + i), W(ops[0], (2 * t + 1) * count + i), W(ops[1], t * count + i), W(ops[2], t * count + i),
                                       W(ops[3], t * count + i), P);
                memcpy(O(outs[1], j * count + i), r1, NW * 4);
            }
    } else if (what == HB_BD_SELFTEST_SUM_MASK) {
        for (int64_t t = 0; t < n; t++)
            for (int64_t i = 0; i < count; i++) {
                uint32_t pw[NW];
                bd_leaf_p_elem<NL, NW>(pw, fxp_bit<NW>(W(ops[0], i), (int)t + 1), W(ops[1], (t + 1) * count + i), P);
                fxp_diff_elem<NL, NW>(r0, pw, W(ops[3], t * count + i), P);
                fxp_diff_elem<NL, NW>(r1, W(ops[2], t * count + i), W(ops[4], t * count + i), P);
                memcpy(O(outs[0], 2 * t * count + i), r0, NW * 4);
                memcpy(O(outs[0], (2 * t + 1) * count + i), r1, NW * 4);
            }
    } else {
        for (int64_t b = 0; b < m; b++)
            for (int64_t i = 0; i < count; i++) {
                if (b == 0) {
                    bd_sum0_elem<NL, NW>(r0, fxp_bit<NW>(W(ops[1], i), 0), W(ops[2], i), P);
                } else {
                    const int64_t t = b - 1;
                    uint32_t pw[NW];
                    bd_leaf_p_elem<NL, NW>(pw, fxp_bit<NW>(W(ops[1], i), (int)b), W(ops[2], b * count + i), P);
                    bd_sum_elem<NL, NW>(r0, pw, W(ops[3], t * count + i), W(ops[0], 2 * t * count + i), W(ops[0], (2 * t + 1) * count + i), W(ops[4], t * count + i),
                                        W(ops[5], t * count + i), W(ops[6], t * count + i), P);
                }
                memcpy(O(outs[0], b * count + i), r0, NW * 4);
            }
    }
    return HB_OK;
}

// m within the modulus and at most 256 planes
static bool bd_m_ok(int bits, int m) { return fxp_m_ok(bits, m) && m - 1 <= 256; }
static bool bd_level_ok(int m, int level) { return level >= 0 && level < bd_levels(m - 1); }

}  // namespace hb

extern "C" {

#define BD_BLOCKS(ctx, name)                                                                                           \
    const int64_t blocks = (count + 255) / 256;                                                                        \
    if (blocks > 0x7fffffffLL) return fail(ctx, HB_ERR_UNSUPPORTED, name ": batch too large for one launch");          \
    hipStream_t s = (hipStream_t)stream

int hb_bd_leaves(hb_ctx *ctx, const uint64_t *c_dev, const uint64_t *bits_dev, int m, uint64_t *g_dev, uint64_t *p_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0) return HB_ERR_BAD_ARG;
    if (!bd_m_ok(fxp_modulus_bits(ctx->p_limbs, ctx->n_limbs), m)) return fail(ctx, HB_ERR_BAD_ARG, "hb_bd_leaves: needs 0 < m <= bits(p) - 2 and m - 1 <= 256");
    if (count > 0 && m > 1 && (!c_dev || !bits_dev || !g_dev || !p_dev)) return HB_ERR_BAD_ARG;
    if (count == 0 || m == 1) return HB_OK;
    const int64_t eb = 8 * (int64_t)ctx->n_limbs, ob = (m - 1) * count * eb;
    if (fxp_overlap(g_dev, ob, p_dev, ob) || fxp_overlap(g_dev, ob, c_dev, count * eb) || fxp_overlap(p_dev, ob, c_dev, count * eb) ||
        fxp_overlap(g_dev, ob, bits_dev, ob) || fxp_overlap(p_dev, ob, bits_dev, ob))
        return fail(ctx, HB_ERR_BAD_ARG, "hb_bd_leaves: g and p are arrays of their own");
    BD_BLOCKS(ctx, "hb_bd_leaves");
    HB_DISPATCH(ctx,
        (k_bd_leaves<9, 8><<<(unsigned)blocks, 256, 0, s>>>(ctx->pw, (const uint32_t *)c_dev, (const uint32_t *)bits_dev, m, (uint32_t *)g_dev, (uint32_t *)p_dev, count)),
        (k_bd_leaves<3, 2><<<(unsigned)blocks, 256, 0, s>>>(ctx->pn, (const uint32_t *)c_dev, (const uint32_t *)bits_dev, m, (uint32_t *)g_dev, (uint32_t *)p_dev, count)));
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_bd_prefix_mask(hb_ctx *ctx, const uint64_t *g_dev, const uint64_t *p_dev, int m, int level, const uint64_t *ta_dev, const uint64_t *tb_dev,
                      uint64_t *masked_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0 || (count > 0 && (!g_dev || !p_dev || !ta_dev || !tb_dev || !masked_dev))) return HB_ERR_BAD_ARG;
    if (!bd_m_ok(fxp_modulus_bits(ctx->p_limbs, ctx->n_limbs), m)) return fail(ctx, HB_ERR_BAD_ARG, "hb_bd_prefix_mask: needs 0 < m <= bits(p) - 2 and m - 1 <= 256");
    if (!bd_level_ok(m, level)) return fail(ctx, HB_ERR_BAD_ARG, "hb_bd_prefix_mask: no such level");
    if (count == 0) return HB_OK;
    const int n = m - 1, G = bd_g_only(n, level), triples = bd_level_triples(n, level);
    const int64_t eb = 8 * (int64_t)ctx->n_limbs, ib = (int64_t)n * count * eb, mb = 2 * (int64_t)triples * count * eb;
    if (fxp_overlap(masked_dev, mb, g_dev, ib) || fxp_overlap(masked_dev, mb, p_dev, ib) || fxp_overlap(masked_dev, mb, ta_dev, mb / 2) ||
        fxp_overlap(masked_dev, mb, tb_dev, mb / 2))
        return fail(ctx, HB_ERR_BAD_ARG, "hb_bd_prefix_mask: masked is an array of its own");
    BD_BLOCKS(ctx, "hb_bd_prefix_mask");
    const dim3 grid((unsigned)blocks, (unsigned)triples);
    HB_DISPATCH(ctx,
        (k_bd_prefix_mask<9, 8><<<grid, 256, 0, s>>>(ctx->pw, (const uint32_t *)g_dev, (const uint32_t *)p_dev, level, G, (const uint32_t *)ta_dev, (const uint32_t *)tb_dev,
                                                    (uint32_t *)masked_dev, count)),
        (k_bd_prefix_mask<3, 2><<<grid, 256, 0, s>>>(ctx->pn, (const uint32_t *)g_dev, (const uint32_t *)p_dev, level, G, (const uint32_t *)ta_dev, (const uint32_t *)tb_dev,
                                                    (uint32_t *)masked_dev, count)));
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_bd_prefix_combine(hb_ctx *ctx, const uint64_t *opened_dev, uint64_t *g_dev, uint64_t *p_dev, int m, int level, const uint64_t *ta_dev,
                         const uint64_t *tb_dev, const uint64_t *tab_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0 || (count > 0 && (!opened_dev || !g_dev || !p_dev || !ta_dev || !tb_dev || !tab_dev))) return HB_ERR_BAD_ARG;
    if (!bd_m_ok(fxp_modulus_bits(ctx->p_limbs, ctx->n_limbs), m)) return fail(ctx, HB_ERR_BAD_ARG, "hb_bd_prefix_combine: needs 0 < m <= bits(p) - 2 and m - 1 <= 256");
    if (!bd_level_ok(m, level)) return fail(ctx, HB_ERR_BAD_ARG, "hb_bd_prefix_combine: no such level");
    if (count == 0) return HB_OK;
    const int n = m - 1, G = bd_g_only(n, level), active = bd_active(n, level), triples = bd_level_triples(n, level);
    const int64_t eb = 8 * (int64_t)ctx->n_limbs, ib = (int64_t)n * count * eb, tb_ = (int64_t)triples * count * eb;
    const uint64_t *planes[2] = {g_dev, p_dev};
    for (const uint64_t *o : planes)
        if (fxp_overlap(o, ib, opened_dev, 2 * tb_) || fxp_overlap(o, ib, ta_dev, tb_) || fxp_overlap(o, ib, tb_dev, tb_) || fxp_overlap(o, ib, tab_dev, tb_))
            return fail(ctx, HB_ERR_BAD_ARG, "hb_bd_prefix_combine: g and p are arrays of their own");
    if (fxp_overlap(g_dev, ib, p_dev, ib)) return fail(ctx, HB_ERR_BAD_ARG, "hb_bd_prefix_combine: g overlaps p");
    BD_BLOCKS(ctx, "hb_bd_prefix_combine");
    const dim3 grid((unsigned)blocks, (unsigned)active);
    HB_DISPATCH(ctx,
        (k_bd_prefix_combine<9, 8><<<grid, 256, 0, s>>>(ctx->pw, (const uint32_t *)opened_dev, (uint32_t *)g_dev, (uint32_t *)p_dev, level, G, (const uint32_t *)ta_dev,
                                                       (const uint32_t *)tb_dev, (const uint32_t *)tab_dev, count)),
        (k_bd_prefix_combine<3, 2><<<grid, 256, 0, s>>>(ctx->pn, (const uint32_t *)opened_dev, (uint32_t *)g_dev, (uint32_t *)p_dev, level, G, (const uint32_t *)ta_dev,
                                                       (const uint32_t *)tb_dev, (const uint32_t *)tab_dev, count)));
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_bd_sum_mask(hb_ctx *ctx, const uint64_t *c_dev, const uint64_t *bits_dev, const uint64_t *g_dev, int m, const uint64_t *ta_dev, const uint64_t *tb_dev,
                   uint64_t *masked_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0) return HB_ERR_BAD_ARG;
    if (!bd_m_ok(fxp_modulus_bits(ctx->p_limbs, ctx->n_limbs), m)) return fail(ctx, HB_ERR_BAD_ARG, "hb_bd_sum_mask: needs 0 < m <= bits(p) - 2 and m - 1 <= 256");
    if (count > 0 && m > 1 && (!c_dev || !bits_dev || !g_dev || !ta_dev || !tb_dev || !masked_dev)) return HB_ERR_BAD_ARG;
    if (count == 0 || m == 1) return HB_OK;
    const int64_t eb = 8 * (int64_t)ctx->n_limbs, ib = (int64_t)(m - 1) * count * eb, mb = 2 * ib;
    if (fxp_overlap(masked_dev, mb, c_dev, count * eb) || fxp_overlap(masked_dev, mb, bits_dev, ib + count * eb) || fxp_overlap(masked_dev, mb, g_dev, ib) ||
        fxp_overlap(masked_dev, mb, ta_dev, ib) || fxp_overlap(masked_dev, mb, tb_dev, ib))
        return fail(ctx, HB_ERR_BAD_ARG, "hb_bd_sum_mask: masked is an array of its own");
    BD_BLOCKS(ctx, "hb_bd_sum_mask");
    const dim3 grid((unsigned)blocks, (unsigned)(m - 1));
    HB_DISPATCH(ctx,
        (k_bd_sum_mask<9, 8><<<grid, 256, 0, s>>>(ctx->pw, (const uint32_t *)c_dev, (const uint32_t *)bits_dev, (const uint32_t *)g_dev, (const uint32_t *)ta_dev,
                                                 (const uint32_t *)tb_dev, (uint32_t *)masked_dev, count)),
        (k_bd_sum_mask<3, 2><<<grid, 256, 0, s>>>(ctx->pn, (const uint32_t *)c_dev, (const uint32_t *)bits_dev, (const uint32_t *)g_dev, (const uint32_t *)ta_dev,
                                                 (const uint32_t *)tb_dev, (uint32_t *)masked_dev, count)));
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_bd_sum_combine(hb_ctx *ctx, const uint64_t *opened_dev, const uint64_t *c_dev, const uint64_t *bits_dev, const uint64_t *g_dev, int m, const uint64_t *ta_dev,
                      const uint64_t *tb_dev, const uint64_t *tab_dev, uint64_t *out_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0) return HB_ERR_BAD_ARG;
    if (!bd_m_ok(fxp_modulus_bits(ctx->p_limbs, ctx->n_limbs), m)) return fail(ctx, HB_ERR_BAD_ARG, "hb_bd_sum_combine: needs 0 < m <= bits(p) - 2 and m - 1 <= 256");
    if (count > 0 && (!c_dev || !bits_dev || !out_dev || (m > 1 && (!opened_dev || !g_dev || !ta_dev || !tb_dev || !tab_dev)))) return HB_ERR_BAD_ARG;
    if (count == 0) return HB_OK;
    const int64_t eb = 8 * (int64_t)ctx->n_limbs, ib = (int64_t)(m - 1) * count * eb, ob = ib + count * eb;
    if (fxp_overlap(out_dev, ob, c_dev, count * eb) || fxp_overlap(out_dev, ob, bits_dev, ob) ||
        (m > 1 && (fxp_overlap(out_dev, ob, opened_dev, 2 * ib) || fxp_overlap(out_dev, ob, g_dev, ib) || fxp_overlap(out_dev, ob, ta_dev, ib) ||
                   fxp_overlap(out_dev, ob, tb_dev, ib) || fxp_overlap(out_dev, ob, tab_dev, ib))))
        return fail(ctx, HB_ERR_BAD_ARG, "hb_bd_sum_combine: out is an array of its own");
    BD_BLOCKS(ctx, "hb_bd_sum_combine");
    const dim3 grid((unsigned)blocks, (unsigned)m);
    HB_DISPATCH(ctx,
        (k_bd_sum_combine<9, 8><<<grid, 256, 0, s>>>(ctx->pw, (const uint32_t *)opened_dev, (const uint32_t *)c_dev, (const uint32_t *)bits_dev, (const uint32_t *)g_dev,
                                                    (const uint32_t *)ta_dev, (const uint32_t *)tb_dev, (const uint32_t *)tab_dev, (uint32_t *)out_dev, count)),
        (k_bd_sum_combine<3, 2><<<grid, 256, 0, s>>>(ctx->pn, (const uint32_t *)opened_dev, (const uint32_t *)c_dev, (const uint32_t *)bits_dev, (const uint32_t *)g_dev,
                                                    (const uint32_t *)ta_dev, (const uint32_t *)tb_dev, (const uint32_t *)tab_dev, (uint32_t *)out_dev, count)));
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_selftest_bd(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *operands, const int64_t *params, uint64_t *const *outs, int64_t count) {
    if (!p_limbs || !operands || !params || !outs || count < 0 || (n_limbs != 1 && n_limbs != 4)) return HB_ERR_BAD_ARG;
    for (int i = 0; i < 2; i++) if (params[i] < -(1 << 30) || params[i] > (1 << 30)) return HB_ERR_BAD_ARG;
    const int m = (int)params[0], level = (int)params[1];
    if (!bd_m_ok(fxp_modulus_bits(p_limbs, n_limbs), m)) return HB_ERR_BAD_ARG;
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

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

// ---------------------------------------------------------------- host side
// One step function a step (hb_rows.hpp): its checks, Args fill and row count run under a DeviceRun in the entry point, a HostRun in hb_selftest_bd.
// m within the modulus and at most 256 planes
static bool bd_m_ok(int bits, int m) { return fxp_m_ok(bits, m) && m - 1 <= 256; }
static bool bd_level_ok(int m, int level) { return level >= 0 && level < bd_levels(m - 1); }

template <class Run> static int bd_leaves_step(const Run &run, const uint64_t *c, const uint64_t *bits, int m, uint64_t *g, uint64_t *p, int64_t count) {
    if (count < 0) return HB_ERR_BAD_ARG;
    if (!bd_m_ok(run.bits(), m)) return run.fail(HB_ERR_BAD_ARG, "hb_bd_leaves: needs 0 < m <= bits(p) - 2 and m - 1 <= 256");
    if (count > 0 && m > 1 && (!c || !bits || !g || !p)) return HB_ERR_BAD_ARG;
    if (count == 0 || m == 1) return HB_OK;
    const RowSpan outs[2] = {{g, m - 1}, {p, m - 1}}, ins[2] = {{c, 1}, {bits, m - 1}};
    if (!outputs_apart(outs, 2, ins, 2, run.elem_bytes() * count)) return run.fail(HB_ERR_BAD_ARG, "hb_bd_leaves: g and p are arrays of their own");
    return run_leaves<BdLeavesRow>(run, {u32(c), u32(bits), u32(g), u32(p), m}, count);
}

template <class Run> static int bd_prefix_mask_step(const Run &run, const uint64_t *g, const uint64_t *p, int m, int level, const uint64_t *ta, const uint64_t *tb,
                                                    uint64_t *masked, int64_t count) {
    if (count < 0 || (count > 0 && (!g || !p || !ta || !tb || !masked))) return HB_ERR_BAD_ARG;
    if (!bd_m_ok(run.bits(), m)) return run.fail(HB_ERR_BAD_ARG, "hb_bd_prefix_mask: needs 0 < m <= bits(p) - 2 and m - 1 <= 256");
    if (!bd_level_ok(m, level)) return run.fail(HB_ERR_BAD_ARG, "hb_bd_prefix_mask: no such level");
    if (count == 0) return HB_OK;
    const int n = m - 1, triples = bd_level_triples(n, level);
    const RowSpan outs[1] = {{masked, 2 * triples}}, ins[4] = {{g, n}, {p, n}, {ta, triples}, {tb, triples}};
    if (!outputs_apart(outs, 1, ins, 4, run.elem_bytes() * count)) return run.fail(HB_ERR_BAD_ARG, "hb_bd_prefix_mask: masked is an array of its own");
    const BdPrefixArgs A = {nullptr, u32(ta), u32(tb), nullptr, const_cast<uint32_t *>(u32(g)), const_cast<uint32_t *>(u32(p)), u32(masked), level,
                            bd_g_only(n, level)};
    return run.template rows<BdPrefixMaskRow>(A, triples, count);
}

template <class Run> static int bd_prefix_combine_step(const Run &run, const uint64_t *opened, uint64_t *g, uint64_t *p, int m, int level, const uint64_t *ta,
                                                       const uint64_t *tb, const uint64_t *tab, int64_t count) {
    if (count < 0 || (count > 0 && (!opened || !g || !p || !ta || !tb || !tab))) return HB_ERR_BAD_ARG;
    if (!bd_m_ok(run.bits(), m)) return run.fail(HB_ERR_BAD_ARG, "hb_bd_prefix_combine: needs 0 < m <= bits(p) - 2 and m - 1 <= 256");
    if (!bd_level_ok(m, level)) return run.fail(HB_ERR_BAD_ARG, "hb_bd_prefix_combine: no such level");
    if (count == 0) return HB_OK;
    const int n = m - 1, triples = bd_level_triples(n, level);
    const RowSpan outs[2] = {{g, n}, {p, n}}, ins[4] = {{opened, 2 * triples}, {ta, triples}, {tb, triples}, {tab, triples}};
    if (!outputs_apart(outs, 2, ins, 4, run.elem_bytes() * count)) return run.fail(HB_ERR_BAD_ARG, "hb_bd_prefix_combine: g and p are arrays of their own");
    const BdPrefixArgs A = {u32(opened), u32(ta), u32(tb), u32(tab), u32(g), u32(p), nullptr, level, bd_g_only(n, level)};
    return run.template rows<BdPrefixCombineRow>(A, bd_active(n, level), count);
}

template <class Run> static int bd_sum_mask_step(const Run &run, const uint64_t *c, const uint64_t *bits, const uint64_t *g, int m, const uint64_t *ta,
                                                 const uint64_t *tb, uint64_t *masked, int64_t count) {
    if (count < 0) return HB_ERR_BAD_ARG;
    if (!bd_m_ok(run.bits(), m)) return run.fail(HB_ERR_BAD_ARG, "hb_bd_sum_mask: needs 0 < m <= bits(p) - 2 and m - 1 <= 256");
    if (count > 0 && m > 1 && (!c || !bits || !g || !ta || !tb || !masked)) return HB_ERR_BAD_ARG;
    if (count == 0 || m == 1) return HB_OK;
    const RowSpan outs[1] = {{masked, 2 * (m - 1)}}, ins[5] = {{c, 1}, {bits, m}, {g, m - 1}, {ta, m - 1}, {tb, m - 1}};
    if (!outputs_apart(outs, 1, ins, 5, run.elem_bytes() * count)) return run.fail(HB_ERR_BAD_ARG, "hb_bd_sum_mask: masked is an array of its own");
    const BdSumArgs A = {nullptr, u32(c), u32(bits), u32(g), u32(ta), u32(tb), nullptr, u32(masked), nullptr};
    return run.template rows<BdSumMaskRow>(A, m - 1, count);
}

template <class Run> static int bd_sum_combine_step(const Run &run, const uint64_t *opened, const uint64_t *c, const uint64_t *bits, const uint64_t *g, int m,
                                                    const uint64_t *ta, const uint64_t *tb, const uint64_t *tab, uint64_t *out, int64_t count) {
    if (count < 0) return HB_ERR_BAD_ARG;
    if (!bd_m_ok(run.bits(), m)) return run.fail(HB_ERR_BAD_ARG, "hb_bd_sum_combine: needs 0 < m <= bits(p) - 2 and m - 1 <= 256");
    if (count > 0 && (!c || !bits || !out || (m > 1 && (!opened || !g || !ta || !tb || !tab)))) return HB_ERR_BAD_ARG;
    if (count == 0) return HB_OK;
    const bool prod = m > 1;                                                    // with m == 1 there is no product: its operands are not looked at
    const RowSpan outs[1] = {{out, m}};
    const RowSpan ins[7] = {{c, 1}, {bits, m}, {prod ? opened : nullptr, 2 * (m - 1)}, {prod ? g : nullptr, m - 1}, {prod ? ta : nullptr, m - 1},
                            {prod ? tb : nullptr, m - 1}, {prod ? tab : nullptr, m - 1}};
    if (!outputs_apart(outs, 1, ins, 7, run.elem_bytes() * count)) return run.fail(HB_ERR_BAD_ARG, "hb_bd_sum_combine: out is an array of its own");
    const BdSumArgs A = {u32(opened), u32(c), u32(bits), u32(g), u32(ta), u32(tb), u32(tab), nullptr, u32(out)};
    return run.template rows<BdSumCombineRow>(A, m, count);
}

}  // namespace hb

extern "C" {

int hb_bd_leaves(hb_ctx *ctx, const uint64_t *c_dev, const uint64_t *bits_dev, int m, uint64_t *g_dev, uint64_t *p_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : bd_leaves_step(DeviceRun{ctx, (hipStream_t)stream, "hb_bd_leaves"}, c_dev, bits_dev, m, g_dev, p_dev, count);
}

int hb_bd_prefix_mask(hb_ctx *ctx, const uint64_t *g_dev, const uint64_t *p_dev, int m, int level, const uint64_t *ta_dev, const uint64_t *tb_dev,
                      uint64_t *masked_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : bd_prefix_mask_step(DeviceRun{ctx, (hipStream_t)stream, "hb_bd_prefix_mask"}, g_dev, p_dev, m, level, ta_dev, tb_dev, masked_dev,
                                                       count);
}

int hb_bd_prefix_combine(hb_ctx *ctx, const uint64_t *opened_dev, uint64_t *g_dev, uint64_t *p_dev, int m, int level, const uint64_t *ta_dev,
                         const uint64_t *tb_dev, const uint64_t *tab_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : bd_prefix_combine_step(DeviceRun{ctx, (hipStream_t)stream, "hb_bd_prefix_combine"}, opened_dev, g_dev, p_dev, m, level, ta_dev,
                                                          tb_dev, tab_dev, count);
}

int hb_bd_sum_mask(hb_ctx *ctx, const uint64_t *c_dev, const uint64_t *bits_dev, const uint64_t *g_dev, int m, const uint64_t *ta_dev, const uint64_t *tb_dev,
                   uint64_t *masked_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : bd_sum_mask_step(DeviceRun{ctx, (hipStream_t)stream, "hb_bd_sum_mask"}, c_dev, bits_dev, g_dev, m, ta_dev, tb_dev, masked_dev, count);
}

int hb_bd_sum_combine(hb_ctx *ctx, const uint64_t *opened_dev, const uint64_t *c_dev, const uint64_t *bits_dev, const uint64_t *g_dev, int m, const uint64_t *ta_dev,
                      const uint64_t *tb_dev, const uint64_t *tab_dev, uint64_t *out_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : bd_sum_combine_step(DeviceRun{ctx, (hipStream_t)stream, "hb_bd_sum_combine"}, opened_dev, c_dev, bits_dev, g_dev, m, ta_dev, tb_dev,
                                                       tab_dev, out_dev, count);
}

// params: m, level
int hb_selftest_bd(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *ops, const int64_t *params, uint64_t *const *outs, int64_t count) {
    if (!p_limbs || !ops || !params || !outs || (n_limbs != 1 && n_limbs != 4)) return HB_ERR_BAD_ARG;
    for (int i = 0; i < 2; i++) if (params[i] < -(1 << 30) || params[i] > (1 << 30)) return HB_ERR_BAD_ARG;
    const HostRun run = {p_limbs, n_limbs};
    const int m = (int)params[0], level = (int)params[1];
    switch (what) {
    case HB_BD_SELFTEST_LEAVES: return bd_leaves_step(run, ops[0], ops[1], m, outs[0], outs[1], count);
    case HB_BD_SELFTEST_PREFIX_MASK: return bd_prefix_mask_step(run, ops[0], ops[1], m, level, ops[2], ops[3], outs[0], count);
    case HB_BD_SELFTEST_PREFIX_COMBINE: return bd_prefix_combine_step(run, ops[0], outs[0], outs[1], m, level, ops[1], ops[2], ops[3], count);
    case HB_BD_SELFTEST_SUM_MASK: return bd_sum_mask_step(run, ops[0], ops[1], ops[2], m, ops[3], ops[4], outs[0], count);
    case HB_BD_SELFTEST_SUM_COMBINE: return bd_sum_combine_step(run, ops[0], ops[1], ops[2], ops[3], m, ops[4], ops[5], ops[6], outs[0], count);
    default: return HB_ERR_BAD_ARG;
    }
}

}  // extern "C"

// hb_fxp.hip -- fixed-point arithmetic on share arrays, the reference's progs/fixedpoint.py ("Secure Computation With Fixed-Point
// Numbers", Catrina and Saxena): random2m (:91-98), trunc_pr (:108-120), get_carry_bit / bit_ltl (:131-172), div2m (:184-193), trunc
// (:208-211) and FixedPoint.ltz (:266-268) for arrays of values -- restated on fp29.hpp, not translated.
//
// A value x has k bits (signed: |x| < 2^(k-1)), m of them are cut off, kappa is the statistical security parameter.  The protocol
// opens c = x + 2^(k-1) + r1 + 2^m r2 with r1 < 2^m, r2 < 2^(k+kappa-m) made of k + kappa preprocessed random bit shares, takes
// c2 = c mod 2^m in the clear and corrects it by the borrow of c2 - r1, the carry bit of c2 + (2^m - 1 - r1) + 1 out of a prefix tree.
// The bit shares arrive as planes: row i of `bits` holds [b_i] of every element, so a wave's loads of a plane cover consecutive elements.
//
// k_fxp_mask       r1 = sum_{i<m} 2^i b_i and r1 + 2^m r2 = sum_{i<k+kappa} 2^i b_i by Horner from the top plane down: one modular
//                  doubling and one addition a plane, no product (the planes below m feed two accumulators).  Writes x + 2^(k-1) + r1 +
//                  2^m r2 and r1; without x (random2m alone) r2 and r1.  k + kappa + 1 reads and two writes an element.
// k_fxp_trunc_pr   after the open: (x - (c mod 2^m) + r1) 2^(-m); c mod 2^m is a mask on the packed words, 2^(-m) a kernel argument in
//                  Montgomery form (wave-uniform, SGPRs: the `a` operand of mac), so the scaling is ONE product.
// k_fxp_leaves     the tree's leaves with no product: a_i, bit i of c2, is public, so carry_i = a_i (1 - b_i) and all_one_i = a_i +
//                  (1 - b_i) - 2 carry_i are selects: a_i = 1 -> (g, p) = (1 - b_i, b_i), a_i = 0 -> (0, 1 - b_i).  m + 1 leaf planes, most
//                  significant bit first, the low carry (1, 0) last.  (The reference spends a triple and an open on each of these.)
// k_fxp_carry_mask / k_fxp_carry_combine   one level of the tree, (g1, p1) o (g2, p2) = (g1 + p1 g2, p1 p2) on adjacent planes: the mask
//                  writes the two masked differences of every Beaver product of the level into one array (one thread a triple), the
//                  combine takes that array opened and writes the next level's planes (one thread a node, ew_beaver_elem twice; an odd
//                  last plane is copied).  At the root only g is computed.
// k_fxp_finish     u = 1 - carry, a2 = c2 - r1 + 2^m u = [x mod 2^m]; or (x - a2) 2^(-m) = [floor(x / 2^m)]; or its negation (ltz).
//
// Operands and results are packed canonical residues.  The per-element bodies are HB_HD functions: the __global__ wrappers only
// load, call them and store, and hb_selftest_fxp runs the very same functions on the host.
//
// Launch shape (all kernels): 256-thread workgroups, one element a thread in x; the tree's kernels take the triple / node in
// blockIdx.y.  No LDS, no grid stride, one launch a call.  Planes, triples and opened values are read once: the 32-byte width takes
// the non-temporal loads, as k_ew_beaver.
// Compiler's report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; scratch = 0 bytes for every kernel):
//   k_fxp_mask<9, 8>           83 VGPRs with x (5 waves a SIMD), 68 without (7)     k_fxp_mask<3, 2>           34 / 27 VGPRs: 8 waves
//   k_fxp_trunc_pr<9, 8>       45 VGPRs: 8 waves                                   k_fxp_trunc_pr<3, 2>       15 VGPRs: 8 waves
//   k_fxp_leaves<9, 8>         69 VGPRs: 7 waves                                   k_fxp_leaves<3, 2>         49 VGPRs: 8 waves
//   k_fxp_carry_mask<9, 8>     40 VGPRs: 8 waves                                   k_fxp_carry_mask<3, 2>     15 VGPRs: 8 waves
//   k_fxp_carry_combine<9, 8>  67 VGPRs: 7 waves                                   k_fxp_carry_combine<3, 2>  28 VGPRs: 8 waves
//   k_fxp_finish<9, 8>         64 VGPRs: 8 waves                                   k_fxp_finish<3, 2>         27 VGPRs: 8 waves
// (DESIGN.md section 3m has the schedule and the counts.)
#include "hb_common.hpp"
#include "hb_fxp_elem.hpp"

using namespace hb;

namespace hb {

// what the finish needs: 2^m (canonical), 2^m and 2^(-m) (Montgomery)
template <int NL> struct FxpFinishConsts { uint32_t pow2[NL], pow2m[NL], inv2m[NL]; };

// ---------------------------------------------------------------- per-element bodies (host and device)
// (FxpConst, fxp_horner, fxp_mask_elem, fxp_low_bits, fxp_trunc_pr_elem, fxp_bit, fxp_leaf_elem, fxp_diff_elem, fxp_node_g_elem and the host
// helpers fxp_params_ok, fxp_pow2, fxp_host_mont: hb_fxp_elem.hpp, shared with hb_bd.hip and hb_div.hip)

// mode HB_FXP_MOD: a2 = c2 - r1 + 2^m (1 - carry);  HB_FXP_TRUNC: (x - a2) 2^(-m);  HB_FXP_NEG_TRUNC: (a2 - x) 2^(-m)
template <int NL, int NW>
HB_HD void fxp_finish_elem(uint32_t (&o)[NW], const uint32_t (&xw)[NW], const uint32_t (&cw)[NW], const uint32_t (&r1w)[NW], const uint32_t (&carryw)[NW], int m,
                           int mode, const FxpFinishConsts<NL> &K, const FpParams<NL> &P) {
    uint32_t c2w[NW], a[NL], b[NL], t[NL], a2[NL];
    fxp_low_bits<NW>(c2w, cw, m);
    unpack<NL, NW>(a, c2w);
    fp_add<NL>(t, a, K.pow2, P);
    unpack<NL, NW>(b, r1w);
    fp_sub<NL>(a, t, b, P);
    unpack<NL, NW>(b, carryw);
    mont_mul<NL>(t, K.pow2m, b, P);
    fp_sub<NL>(a2, a, t, P);
    if (mode == HB_FXP_MOD) { pack<NL, NW>(o, a2); return; }
    unpack<NL, NW>(b, xw);
    if (mode == HB_FXP_TRUNC) fp_sub<NL>(t, b, a2, P); else fp_sub<NL>(t, a2, b, P);
    mont_mul<NL>(a, K.inv2m, t, P);
    pack<NL, NW>(o, a);
}

// ---------------------------------------------------------------- kernels
// No __restrict__ where the header allows an output to be an input (a thread reads its element before it writes it).
template <int NL, int NW, bool HAS_X>
__global__ void __launch_bounds__(256) k_fxp_mask(const FpParams<NL> P, const uint32_t *x, const uint32_t *bits, int nbits, int m, const FxpConst<NL> half,
                                                  uint32_t *masked, uint32_t *r1, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    uint32_t xw[NW], o0[NW], o1[NW];
    if constexpr (HAS_X) load_words<NW>(xw, x + i * NW);
    fxp_mask_elem<NL, NW, HAS_X>(o0, o1, xw, [&](uint32_t (&w)[NW], int row) { fxp_load_once<NW>(w, bits + ((int64_t)row * count + i) * NW); }, nbits, m, half.d, P);
    store_words<NW>(masked + i * NW, o0);
    store_words<NW>(r1 + i * NW, o1);
}

template <int NL, int NW>
__global__ void __launch_bounds__(256) k_fxp_trunc_pr(const FpParams<NL> P, const uint32_t *x, const uint32_t *c, const uint32_t *r1, int m, const FxpConst<NL> invm,
                                                      uint32_t *out, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    uint32_t xw[NW], cw[NW], rw[NW], ow[NW];
    load_words<NW>(xw, x + i * NW); fxp_load_once<NW>(cw, c + i * NW); fxp_load_once<NW>(rw, r1 + i * NW);
    fxp_trunc_pr_elem<NL, NW>(ow, xw, cw, rw, m, invm.d, P);
    store_words<NW>(out + i * NW, ow);
}

// g, p: m + 1 planes each, distinct from c and bits
template <int NL, int NW>
__global__ void __launch_bounds__(256) k_fxp_leaves(const FpParams<NL> P, const uint32_t *__restrict__ c, const uint32_t *__restrict__ bits, int m,
                                                    uint32_t *__restrict__ g, uint32_t *__restrict__ p, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    uint32_t cw[NW], bw[NW], gw[NW], pw[NW];
    load_words<NW>(cw, c + i * NW);
#pragma unroll 4
    for (int j = 0; j < m; j++) {
        const int bit = m - 1 - j;
        fxp_load_once<NW>(bw, bits + ((int64_t)bit * count + i) * NW);
        fxp_leaf_elem<NL, NW>(gw, pw, fxp_bit<NW>(cw, bit), bw, P);
        store_words<NW>(g + ((int64_t)j * count + i) * NW, gw);
        store_words<NW>(p + ((int64_t)j * count + i) * NW, pw);
    }
#pragma unroll
    for (int q = 0; q < NW; q++) { gw[q] = q == 0 ? 1u : 0u; pw[q] = 0u; }
    store_words<NW>(g + ((int64_t)m * count + i) * NW, gw);
    store_words<NW>(p + ((int64_t)m * count + i) * NW, pw);
}

// triple t = blockIdx.y of the level: node t / 2; its first factor is p1, its second g2 (t even) or p2 (t odd)
template <int NL, int NW>
__global__ void __launch_bounds__(256) k_fxp_carry_mask(const FpParams<NL> P, const uint32_t *__restrict__ g, const uint32_t *__restrict__ p,
                                                        const uint32_t *__restrict__ ta, const uint32_t *__restrict__ tb, uint32_t *__restrict__ masked, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int64_t t = blockIdx.y, node = t >> 1;
    uint32_t p1[NW], y[NW], aw[NW], bw[NW], o0[NW], o1[NW];
    load_words<NW>(p1, p + ((2 * node) * count + i) * NW);
    load_words<NW>(y, ((t & 1) ? p : g) + ((2 * node + 1) * count + i) * NW);
    fxp_load_once<NW>(aw, ta + (t * count + i) * NW);
    fxp_load_once<NW>(bw, tb + (t * count + i) * NW);
    fxp_diff_elem<NL, NW>(o0, p1, aw, P);
    fxp_diff_elem<NL, NW>(o1, y, bw, P);
    store_words<NW>(masked + ((2 * t) * count + i) * NW, o0);
    store_words<NW>(masked + ((2 * t + 1) * count + i) * NW, o1);
}

// node j = blockIdx.y of the next level: from planes 2j, 2j + 1, or plane 2j alone moved up (an odd count of planes)
template <int NL, int NW>
__global__ void __launch_bounds__(256) k_fxp_carry_combine(const FpParams<NL> P, const uint32_t *__restrict__ opened, const uint32_t *__restrict__ g,
                                                           const uint32_t *__restrict__ p, int pairs, int root, const uint32_t *__restrict__ ta,
                                                           const uint32_t *__restrict__ tb, const uint32_t *__restrict__ tab, uint32_t *__restrict__ g_out,
                                                           uint32_t *__restrict__ p_out, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int64_t j = blockIdx.y;
    uint32_t g1[NW], dw[NW], ew[NW], aw[NW], bw[NW], abw[NW], ow[NW];
    if (j >= pairs) {
        load_words<NW>(g1, g + ((2 * j) * count + i) * NW);
        store_words<NW>(g_out + (j * count + i) * NW, g1);
        load_words<NW>(g1, p + ((2 * j) * count + i) * NW);
        store_words<NW>(p_out + (j * count + i) * NW, g1);
        return;
    }
    int64_t t = 2 * j;
    load_words<NW>(g1, g + ((2 * j) * count + i) * NW);
    fxp_load_once<NW>(dw, opened + ((2 * t) * count + i) * NW); fxp_load_once<NW>(ew, opened + ((2 * t + 1) * count + i) * NW);
    fxp_load_once<NW>(aw, ta + (t * count + i) * NW); fxp_load_once<NW>(bw, tb + (t * count + i) * NW); fxp_load_once<NW>(abw, tab + (t * count + i) * NW);
    fxp_node_g_elem<NL, NW>(ow, g1, dw, ew, aw, bw, abw, P);
    store_words<NW>(g_out + (j * count + i) * NW, ow);
    if (root) return;
    t = 2 * j + 1;
    fxp_load_once<NW>(dw, opened + ((2 * t) * count + i) * NW); fxp_load_once<NW>(ew, opened + ((2 * t + 1) * count + i) * NW);
    fxp_load_once<NW>(aw, ta + (t * count + i) * NW); fxp_load_once<NW>(bw, tb + (t * count + i) * NW); fxp_load_once<NW>(abw, tab + (t * count + i) * NW);
    ew_beaver_elem<NL, NW>(ow, dw, ew, aw, bw, abw, P);
    store_words<NW>(p_out + (j * count + i) * NW, ow);
}

template <int NL, int NW>
__global__ void __launch_bounds__(256) k_fxp_finish(const FpParams<NL> P, const uint32_t *x, const uint32_t *c, const uint32_t *r1, const uint32_t *carry, int m, int mode,
                                                    const FxpFinishConsts<NL> K, uint32_t *out, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    uint32_t xw[NW], cw[NW], rw[NW], kw[NW], ow[NW];
    if (mode != HB_FXP_MOD) load_words<NW>(xw, x + i * NW);
    else {
#pragma unroll
        for (int q = 0; q < NW; q++) xw[q] = 0;
    }
    fxp_load_once<NW>(cw, c + i * NW); fxp_load_once<NW>(rw, r1 + i * NW); fxp_load_once<NW>(kw, carry + i * NW);
    fxp_finish_elem<NL, NW>(ow, xw, cw, rw, kw, m, mode, K, P);
    store_words<NW>(out + i * NW, ow);
}

// ---------------------------------------------------------------- host side
template <int NL, int NW> static bool fxp_finish_consts(FxpFinishConsts<NL> &K, const FpParams<NL> &P, int m, const uint64_t *inv2m_host, bool need_inv) {
    fxp_pow2<NL>(K.pow2, m, false, P);
    fxp_pow2<NL>(K.pow2m, m, true, P);
    for (int q = 0; q < NL; q++) K.inv2m[q] = 0;
    return need_inv ? fxp_host_mont<NL, NW>(K.inv2m, P, inv2m_host) : true;
}

template <int NL, int NW>
static void launch_fxp_mask(const FpParams<NL> &P, const uint32_t *x, const uint32_t *bits, int k, int m, int kappa, uint32_t *masked, uint32_t *r1, int64_t count,
                            unsigned blocks, hipStream_t s) {
    FxpConst<NL> half;
    fxp_pow2<NL>(half.d, k - 1, false, P);
    if (x) k_fxp_mask<NL, NW, true><<<blocks, 256, 0, s>>>(P, x, bits, k + kappa, m, half, masked, r1, count);
    else k_fxp_mask<NL, NW, false><<<blocks, 256, 0, s>>>(P, nullptr, bits, k + kappa, m, half, masked, r1, count);
}
template <int NL, int NW>
static bool launch_fxp_trunc_pr(const FpParams<NL> &P, const uint32_t *x, const uint32_t *c, const uint32_t *r1, int m, const uint64_t *inv2m_host, uint32_t *out,
                                int64_t count, unsigned blocks, hipStream_t s) {
    FxpConst<NL> invm;
    if (!fxp_host_mont<NL, NW>(invm.d, P, inv2m_host)) return false;
    if (count) k_fxp_trunc_pr<NL, NW><<<blocks, 256, 0, s>>>(P, x, c, r1, m, invm, out, count);
    return true;
}
template <int NL, int NW>
static bool launch_fxp_finish(const FpParams<NL> &P, const uint32_t *x, const uint32_t *c, const uint32_t *r1, const uint32_t *carry, int m, const uint64_t *inv2m_host,
                              int mode, uint32_t *out, int64_t count, unsigned blocks, hipStream_t s) {
    FxpFinishConsts<NL> K;
    if (!fxp_finish_consts<NL, NW>(K, P, m, inv2m_host, mode != HB_FXP_MOD)) return false;
    if (count) k_fxp_finish<NL, NW><<<blocks, 256, 0, s>>>(P, x, c, r1, carry, m, mode, K, out, count);
    return true;
}

// host: the same element functions over `count` elements
template <int NL, int NW>
static int selftest_fxp(const uint64_t *p_limbs, int what, const uint64_t *const *ops, const int64_t *params, uint64_t *const *outs, int64_t count) {
    FpParams<NL> P;
    fp_params_from_limbs(P, p_limbs);
    const int k = (int)params[0], m = (int)params[1], kappa = (int)params[2], aux = (int)params[3], root = (int)params[4];
    auto W = [](const uint64_t *base, int64_t i) -> const uint32_t (&)[NW] { return *reinterpret_cast<const uint32_t(*)[NW]>(reinterpret_cast<const uint32_t *>(base) + i * NW); };
    auto O = [](uint64_t *base, int64_t i) -> uint32_t * { return reinterpret_cast<uint32_t *>(base) + i * NW; };
    const uint32_t none[NW] = {};
    uint32_t r0[NW], r1[NW];
    if (what == HB_FXP_SELFTEST_MASK) {
        FxpConst<NL> half;
        fxp_pow2<NL>(half.d, k - 1, false, P);
        for (int64_t i = 0; i < count; i++) {
            auto plane = [&](uint32_t (&w)[NW], int row) { memcpy(w, W(ops[1], (int64_t)row * count + i), NW * 4); };
            if (ops[0]) fxp_mask_elem<NL, NW, true>(r0, r1, W(ops[0], i), plane, k + kappa, m, half.d, P);
            else fxp_mask_elem<NL, NW, false>(r0, r1, none, plane, k + kappa, m, half.d, P);
            memcpy(O(outs[0], i), r0, NW * 4);
            memcpy(O(outs[1], i), r1, NW * 4);
        }
    } else if (what == HB_FXP_SELFTEST_TRUNC_PR) {
        FxpConst<NL> invm;
        if (!fxp_host_mont<NL, NW>(invm.d, P, ops[3])) return HB_ERR_BAD_ARG;
        for (int64_t i = 0; i < count; i++) {
            fxp_trunc_pr_elem<NL, NW>(r0, W(ops[0], i), W(ops[1], i), W(ops[2], i), m, invm.d, P);
            memcpy(O(outs[0], i), r0, NW * 4);
        }
    } else if (what == HB_FXP_SELFTEST_LEAVES) {
        for (int64_t i = 0; i < count; i++) {
            for (int j = 0; j < m; j++) {
                const int bit = m - 1 - j;
                fxp_leaf_elem<NL, NW>(r0, r1, fxp_bit<NW>(W(ops[0], i), bit), W(ops[1], (int64_t)bit * count + i), P);
                memcpy(O(outs[0], (int64_t)j * count + i), r0, NW * 4);
                memcpy(O(outs[1], (int64_t)j * count + i), r1, NW * 4);
            }
            uint32_t one[NW] = {1u};
            memcpy(O(outs[0], (int64_t)m * count + i), one, NW * 4);
            memcpy(O(outs[1], (int64_t)m * count + i), none, NW * 4);
        }
    } else if (what == HB_FXP_SELFTEST_CARRY_MASK) {
        const int64_t triples = root ? 1 : 2 * (aux / 2);
        for (int64_t t = 0; t < triples; t++)
            for (int64_t i = 0; i < count; i++) {
                const int64_t node = t >> 1;
                fxp_diff_elem<NL, NW>(r0, W(ops[1], 2 * node * count + i), W(ops[2], t * count + i), P);
                fxp_diff_elem<NL, NW>(r1, W((t & 1) ? ops[1] : ops[0], (2 * node + 1) * count + i), W(ops[3], t * count + i), P);
                memcpy(O(outs[0], 2 * t * count + i), r0, NW * 4);
                memcpy(O(outs[0], (2 * t + 1) * count + i), r1, NW * 4);
            }
    } else if (what == HB_FXP_SELFTEST_CARRY_COMBINE) {
        const int64_t pairs = aux / 2, out_nodes = (aux + 1) / 2;
        for (int64_t j = 0; j < out_nodes; j++)
            for (int64_t i = 0; i < count; i++) {
                if (j >= pairs) {
                    memcpy(O(outs[0], j * count + i), W(ops[1], 2 * j * count + i), NW * 4);
                    memcpy(O(outs[1], j * count + i), W(ops[2], 2 * j * count + i), NW * 4);
                    continue;
                }
                int64_t t = 2 * j;
                fxp_node_g_elem<NL, NW>(r0, W(ops[1], 2 * j * count + i), W(ops[0], 2 * t * count + i), W(ops[0], (2 * t + 1) * count + i), W(ops[3], t * count + i),
                                        W(ops[4], t * count + i), W(ops[5], t * count + i), P);
                memcpy(O(outs[0], j * count + i), r0, NW * 4);
                if (root) continue;
                t = 2 * j + 1;
                ew_beaver_elem<NL, NW>(r1, W(ops[0], 2 * t * count + i), W(ops[0], (2 * t + 1) * count + i), W(ops[3], t * count + i), W(ops[4], t * count + i),
                                       W(ops[5], t * count + i), P);
                memcpy(O(outs[1], j * count + i), r1, NW * 4);
            }
    } else {
        FxpFinishConsts<NL> K;
        if (!fxp_finish_consts<NL, NW>(K, P, m, ops[4], aux != HB_FXP_MOD)) return HB_ERR_BAD_ARG;
        for (int64_t i = 0; i < count; i++) {
            fxp_finish_elem<NL, NW>(r0, aux == HB_FXP_MOD ? none : W(ops[0], i), W(ops[1], i), W(ops[2], i), W(ops[3], i), m, aux, K, P);
            memcpy(O(outs[0], i), r0, NW * 4);
        }
    }
    return HB_OK;
}

}  // namespace hb

extern "C" {

#define FXP_BLOCKS(ctx, name)                                                                                          \
    const int64_t blocks = (count + 255) / 256;                                                                        \
    if (blocks > 0x7fffffffLL) return fail(ctx, HB_ERR_UNSUPPORTED, name ": batch too large for one launch");          \
    hipStream_t s = (hipStream_t)stream

int hb_fxp_mask(hb_ctx *ctx, const uint64_t *x_dev, const uint64_t *bits_dev, int k, int m, int kappa, uint64_t *masked_dev, uint64_t *r1_dev, int64_t count,
                void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0 || (count > 0 && (!bits_dev || !masked_dev || !r1_dev))) return HB_ERR_BAD_ARG;
    if (!fxp_params_ok(fxp_modulus_bits(ctx->p_limbs, ctx->n_limbs), k, m, kappa))
        return fail(ctx, HB_ERR_BAD_ARG, "hb_fxp_mask: needs 0 < m < k, kappa >= 0 and k + kappa + 1 <= bits(p) - 1");
    if (count > 0 && masked_dev == r1_dev) return fail(ctx, HB_ERR_BAD_ARG, "hb_fxp_mask: masked and r1 are one array");
    if (count == 0) return HB_OK;
    FXP_BLOCKS(ctx, "hb_fxp_mask");
    HB_DISPATCH(ctx,
        (launch_fxp_mask<9, 8>(ctx->pw, (const uint32_t *)x_dev, (const uint32_t *)bits_dev, k, m, kappa, (uint32_t *)masked_dev, (uint32_t *)r1_dev, count, (unsigned)blocks, s)),
        (launch_fxp_mask<3, 2>(ctx->pn, (const uint32_t *)x_dev, (const uint32_t *)bits_dev, k, m, kappa, (uint32_t *)masked_dev, (uint32_t *)r1_dev, count, (unsigned)blocks, s)));
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_fxp_trunc_pr(hb_ctx *ctx, const uint64_t *x_dev, const uint64_t *c_dev, const uint64_t *r1_dev, int m, const uint64_t *inv2m_host, uint64_t *out_dev,
                    int64_t count, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0 || !inv2m_host || (count > 0 && (!x_dev || !c_dev || !r1_dev || !out_dev))) return HB_ERR_BAD_ARG;
    if (!fxp_m_ok(fxp_modulus_bits(ctx->p_limbs, ctx->n_limbs), m)) return fail(ctx, HB_ERR_BAD_ARG, "hb_fxp_trunc_pr: needs 0 < m <= bits(p) - 2");
    FXP_BLOCKS(ctx, "hb_fxp_trunc_pr");
    bool ok;
    HB_DISPATCH(ctx,
        (ok = launch_fxp_trunc_pr<9, 8>(ctx->pw, (const uint32_t *)x_dev, (const uint32_t *)c_dev, (const uint32_t *)r1_dev, m, inv2m_host, (uint32_t *)out_dev, count, (unsigned)blocks, s)),
        (ok = launch_fxp_trunc_pr<3, 2>(ctx->pn, (const uint32_t *)x_dev, (const uint32_t *)c_dev, (const uint32_t *)r1_dev, m, inv2m_host, (uint32_t *)out_dev, count, (unsigned)blocks, s)));
    if (!ok) return fail(ctx, HB_ERR_BAD_ARG, "hb_fxp_trunc_pr: inv2m is not below the modulus");
    if (count) HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_fxp_ltl_leaves(hb_ctx *ctx, const uint64_t *c_dev, const uint64_t *bits_dev, int m, uint64_t *g_dev, uint64_t *p_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0 || (count > 0 && (!c_dev || !bits_dev || !g_dev || !p_dev))) return HB_ERR_BAD_ARG;
    if (!fxp_m_ok(fxp_modulus_bits(ctx->p_limbs, ctx->n_limbs), m)) return fail(ctx, HB_ERR_BAD_ARG, "hb_fxp_ltl_leaves: needs 0 < m <= bits(p) - 2");
    if (count == 0) return HB_OK;
    const int64_t eb = 8 * (int64_t)ctx->n_limbs, ob = (m + 1) * count * eb;
    if (fxp_overlap(g_dev, ob, p_dev, ob) || fxp_overlap(g_dev, ob, c_dev, count * eb) || fxp_overlap(p_dev, ob, c_dev, count * eb) ||
        fxp_overlap(g_dev, ob, bits_dev, m * count * eb) || fxp_overlap(p_dev, ob, bits_dev, m * count * eb))
        return fail(ctx, HB_ERR_BAD_ARG, "hb_fxp_ltl_leaves: g and p are arrays of their own");
    FXP_BLOCKS(ctx, "hb_fxp_ltl_leaves");
    HB_DISPATCH(ctx,
        (k_fxp_leaves<9, 8><<<(unsigned)blocks, 256, 0, s>>>(ctx->pw, (const uint32_t *)c_dev, (const uint32_t *)bits_dev, m, (uint32_t *)g_dev, (uint32_t *)p_dev, count)),
        (k_fxp_leaves<3, 2><<<(unsigned)blocks, 256, 0, s>>>(ctx->pn, (const uint32_t *)c_dev, (const uint32_t *)bits_dev, m, (uint32_t *)g_dev, (uint32_t *)p_dev, count)));
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

// nodes planes of a level; root: the level of two planes whose p is not wanted
static bool fxp_level_ok(int nodes, int root) { return nodes >= 2 && nodes <= 257 && (!root || nodes == 2); }

int hb_fxp_carry_mask(hb_ctx *ctx, const uint64_t *g_dev, const uint64_t *p_dev, int nodes, int root, const uint64_t *ta_dev, const uint64_t *tb_dev,
                      uint64_t *masked_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0 || (count > 0 && (!g_dev || !p_dev || !ta_dev || !tb_dev || !masked_dev))) return HB_ERR_BAD_ARG;
    if (!fxp_level_ok(nodes, root)) return fail(ctx, HB_ERR_BAD_ARG, "hb_fxp_carry_mask: needs 2 <= nodes <= 257, and nodes == 2 at the root");
    if (count == 0) return HB_OK;
    const int triples = root ? 1 : 2 * (nodes / 2);
    const int64_t eb = 8 * (int64_t)ctx->n_limbs, ib = (int64_t)nodes * count * eb, mb = 2 * (int64_t)triples * count * eb;
    if (fxp_overlap(masked_dev, mb, g_dev, ib) || fxp_overlap(masked_dev, mb, p_dev, ib) || fxp_overlap(masked_dev, mb, ta_dev, mb / 2) ||
        fxp_overlap(masked_dev, mb, tb_dev, mb / 2))
        return fail(ctx, HB_ERR_BAD_ARG, "hb_fxp_carry_mask: masked is an array of its own");
    FXP_BLOCKS(ctx, "hb_fxp_carry_mask");
    const dim3 grid((unsigned)blocks, (unsigned)triples);
    HB_DISPATCH(ctx,
        (k_fxp_carry_mask<9, 8><<<grid, 256, 0, s>>>(ctx->pw, (const uint32_t *)g_dev, (const uint32_t *)p_dev, (const uint32_t *)ta_dev, (const uint32_t *)tb_dev, (uint32_t *)masked_dev, count)),
        (k_fxp_carry_mask<3, 2><<<grid, 256, 0, s>>>(ctx->pn, (const uint32_t *)g_dev, (const uint32_t *)p_dev, (const uint32_t *)ta_dev, (const uint32_t *)tb_dev, (uint32_t *)masked_dev, count)));
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_fxp_carry_combine(hb_ctx *ctx, const uint64_t *opened_dev, const uint64_t *g_dev, const uint64_t *p_dev, int nodes, int root, const uint64_t *ta_dev,
                         const uint64_t *tb_dev, const uint64_t *tab_dev, uint64_t *g_out_dev, uint64_t *p_out_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0 || (count > 0 && (!opened_dev || !g_dev || !p_dev || !ta_dev || !tb_dev || !tab_dev || !g_out_dev || (!root && !p_out_dev)))) return HB_ERR_BAD_ARG;
    if (!fxp_level_ok(nodes, root)) return fail(ctx, HB_ERR_BAD_ARG, "hb_fxp_carry_combine: needs 2 <= nodes <= 257, and nodes == 2 at the root");
    if (count == 0) return HB_OK;
    const int pairs = nodes / 2, out_nodes = (nodes + 1) / 2, triples = root ? 1 : 2 * pairs;
    const int64_t eb = 8 * (int64_t)ctx->n_limbs, ib = (int64_t)nodes * count * eb, ob = (int64_t)out_nodes * count * eb, tb_ = (int64_t)triples * count * eb;
    const uint64_t *outs[2] = {g_out_dev, root ? nullptr : p_out_dev};
    for (const uint64_t *o : outs)
        if (fxp_overlap(o, ob, g_dev, ib) || fxp_overlap(o, ob, p_dev, ib) || fxp_overlap(o, ob, opened_dev, 2 * tb_) || fxp_overlap(o, ob, ta_dev, tb_) ||
            fxp_overlap(o, ob, tb_dev, tb_) || fxp_overlap(o, ob, tab_dev, tb_))
            return fail(ctx, HB_ERR_BAD_ARG, "hb_fxp_carry_combine: the outputs are arrays of their own");
    if (fxp_overlap(outs[0], ob, outs[1], ob)) return fail(ctx, HB_ERR_BAD_ARG, "hb_fxp_carry_combine: g_out overlaps p_out");
    FXP_BLOCKS(ctx, "hb_fxp_carry_combine");
    const dim3 grid((unsigned)blocks, (unsigned)out_nodes);
    HB_DISPATCH(ctx,
        (k_fxp_carry_combine<9, 8><<<grid, 256, 0, s>>>(ctx->pw, (const uint32_t *)opened_dev, (const uint32_t *)g_dev, (const uint32_t *)p_dev, pairs, root, (const uint32_t *)ta_dev,
                                                       (const uint32_t *)tb_dev, (const uint32_t *)tab_dev, (uint32_t *)g_out_dev, (uint32_t *)p_out_dev, count)),
        (k_fxp_carry_combine<3, 2><<<grid, 256, 0, s>>>(ctx->pn, (const uint32_t *)opened_dev, (const uint32_t *)g_dev, (const uint32_t *)p_dev, pairs, root, (const uint32_t *)ta_dev,
                                                       (const uint32_t *)tb_dev, (const uint32_t *)tab_dev, (uint32_t *)g_out_dev, (uint32_t *)p_out_dev, count)));
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_fxp_div2m_finish(hb_ctx *ctx, const uint64_t *x_dev, const uint64_t *c_dev, const uint64_t *r1_dev, const uint64_t *carry_dev, int m, const uint64_t *inv2m_host,
                        int mode, uint64_t *out_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0) return HB_ERR_BAD_ARG;
    if (mode != HB_FXP_MOD && mode != HB_FXP_TRUNC && mode != HB_FXP_NEG_TRUNC) return fail(ctx, HB_ERR_BAD_ARG, "hb_fxp_div2m_finish: unknown mode");
    if ((mode != HB_FXP_MOD && !inv2m_host) || (count > 0 && (!c_dev || !r1_dev || !carry_dev || !out_dev || (mode != HB_FXP_MOD && !x_dev)))) return HB_ERR_BAD_ARG;
    if (!fxp_m_ok(fxp_modulus_bits(ctx->p_limbs, ctx->n_limbs), m)) return fail(ctx, HB_ERR_BAD_ARG, "hb_fxp_div2m_finish: needs 0 < m <= bits(p) - 2");
    FXP_BLOCKS(ctx, "hb_fxp_div2m_finish");
    bool ok;
    HB_DISPATCH(ctx,
        (ok = launch_fxp_finish<9, 8>(ctx->pw, (const uint32_t *)x_dev, (const uint32_t *)c_dev, (const uint32_t *)r1_dev, (const uint32_t *)carry_dev, m, inv2m_host, mode,
                                      (uint32_t *)out_dev, count, (unsigned)blocks, s)),
        (ok = launch_fxp_finish<3, 2>(ctx->pn, (const uint32_t *)x_dev, (const uint32_t *)c_dev, (const uint32_t *)r1_dev, (const uint32_t *)carry_dev, m, inv2m_host, mode,
                                      (uint32_t *)out_dev, count, (unsigned)blocks, s)));
    if (!ok) return fail(ctx, HB_ERR_BAD_ARG, "hb_fxp_div2m_finish: inv2m is not below the modulus");
    if (count) HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_selftest_fxp(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *operands, const int64_t *params, uint64_t *const *outs, int64_t count) {
    if (!p_limbs || !operands || !params || !outs || count < 0 || (n_limbs != 1 && n_limbs != 4)) return HB_ERR_BAD_ARG;
    for (int i = 0; i < 5; i++) if (params[i] < -(1 << 30) || params[i] > (1 << 30)) return HB_ERR_BAD_ARG;
    const int bits = fxp_modulus_bits(p_limbs, n_limbs);
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

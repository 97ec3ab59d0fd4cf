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
// One step function a step (hb_rows.hpp): its checks, Args fill and row count run under a DeviceRun in the entry point, a HostRun in hb_selftest_fxp.
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

template <class Run> static int fxp_mask_step(const Run &run, const uint64_t *x, const uint64_t *bits, int k, int m, int kappa, uint64_t *masked, uint64_t *r1,
                                              int64_t count) {
    if (count < 0 || (count > 0 && (!bits || !masked || !r1))) return HB_ERR_BAD_ARG;
    if (!fxp_params_ok(run.bits(), k, m, kappa))
        return run.fail(HB_ERR_BAD_ARG, "hb_fxp_mask: needs 0 < m < k, kappa >= 0 and k + kappa + 1 <= bits(p) - 1");
    if (count > 0 && masked == r1) return run.fail(HB_ERR_BAD_ARG, "hb_fxp_mask: masked and r1 are one array");
    if (count == 0) return HB_OK;
    const auto fill = [&](auto &A, const auto &P) {
        A.x = u32(x); A.bits = u32(bits); A.masked = u32(masked); A.r1 = u32(r1);
        return fxp_mask_consts(A, P, k, m, kappa);
    };
    if (x) return run.template rows<FxpMaskRow<true>, FxpMaskArgs>(fill, 1, count);
    return run.template rows<FxpMaskRow<false>, FxpMaskArgs>(fill, 1, count);
}

template <class Run> static int fxp_trunc_pr_step(const Run &run, const uint64_t *x, const uint64_t *c, const uint64_t *r1, int m, const uint64_t *inv2m_host,
                                                  uint64_t *out, int64_t count) {
    if (count < 0 || !inv2m_host || (count > 0 && (!x || !c || !r1 || !out))) return HB_ERR_BAD_ARG;
    if (!fxp_m_ok(run.bits(), m)) return run.fail(HB_ERR_BAD_ARG, "hb_fxp_trunc_pr: needs 0 < m <= bits(p) - 2");
    const int rc = run.template rows<FxpTruncPrRow, FxpTruncPrArgs>([&](auto &A, const auto &P) {
        A.x = u32(x); A.c = u32(c); A.r1 = u32(r1); A.out = u32(out);
        return fxp_trunc_pr_consts(A, P, m, inv2m_host);
    }, 1, count);
    return rc == HB_ERR_BAD_ARG ? run.fail(rc, "hb_fxp_trunc_pr: inv2m is not below the modulus") : rc;
}

template <class Run> static int fxp_ltl_leaves_step(const Run &run, const uint64_t *c, const uint64_t *bits, int m, uint64_t *g, uint64_t *p, int64_t count) {
    if (count < 0 || (count > 0 && (!c || !bits || !g || !p))) return HB_ERR_BAD_ARG;
    if (!fxp_m_ok(run.bits(), m)) return run.fail(HB_ERR_BAD_ARG, "hb_fxp_ltl_leaves: needs 0 < m <= bits(p) - 2");
    if (count == 0) return HB_OK;
    const RowSpan outs[2] = {{g, m + 1}, {p, m + 1}}, ins[2] = {{c, 1}, {bits, m}};
    if (!outputs_apart(outs, 2, ins, 2, run.elem_bytes() * count)) return run.fail(HB_ERR_BAD_ARG, "hb_fxp_ltl_leaves: g and p are arrays of their own");
    return run_leaves<FxpLeavesRow>(run, {u32(c), u32(bits), u32(g), u32(p), m}, count);
}

template <class Run> static int fxp_carry_mask_step(const Run &run, const uint64_t *g, const uint64_t *p, int nodes, int root, const uint64_t *ta, const uint64_t *tb,
                                                    uint64_t *masked, int64_t count) {
    if (count < 0 || (count > 0 && (!g || !p || !ta || !tb || !masked))) return HB_ERR_BAD_ARG;
    if (!fxp_level_ok(nodes, root)) return run.fail(HB_ERR_BAD_ARG, "hb_fxp_carry_mask: needs 2 <= nodes <= 257, and nodes == 2 at the root");
    if (count == 0) return HB_OK;
    const int triples = fxp_level_triples(nodes, root);
    const RowSpan outs[1] = {{masked, 2 * triples}}, ins[4] = {{g, nodes}, {p, nodes}, {ta, triples}, {tb, triples}};
    if (!outputs_apart(outs, 1, ins, 4, run.elem_bytes() * count)) return run.fail(HB_ERR_BAD_ARG, "hb_fxp_carry_mask: masked is an array of its own");
    const FxpCarryMaskArgs A = {u32(g), u32(p), u32(ta), u32(tb), u32(masked)};
    return run.template rows<FxpCarryMaskRow>(A, triples, count);
}

template <class Run> static int fxp_carry_combine_step(const Run &run, const uint64_t *opened, const uint64_t *g, const uint64_t *p, int nodes, int root,
                                                       const uint64_t *ta, const uint64_t *tb, const uint64_t *tab, uint64_t *g_out, uint64_t *p_out, int64_t count) {
    if (count < 0 || (count > 0 && (!opened || !g || !p || !ta || !tb || !tab || !g_out || (!root && !p_out)))) return HB_ERR_BAD_ARG;
    if (!fxp_level_ok(nodes, root)) return run.fail(HB_ERR_BAD_ARG, "hb_fxp_carry_combine: needs 2 <= nodes <= 257, and nodes == 2 at the root");
    if (count == 0) return HB_OK;
    const int pairs = nodes / 2, out_nodes = (nodes + 1) / 2, triples = fxp_level_triples(nodes, root);
    const RowSpan outs[2] = {{g_out, out_nodes}, {root ? nullptr : p_out, out_nodes}};
    const RowSpan ins[6] = {{g, nodes}, {p, nodes}, {opened, 2 * triples}, {ta, triples}, {tb, triples}, {tab, triples}};
    if (!outputs_apart(outs, 2, ins, 6, run.elem_bytes() * count)) return run.fail(HB_ERR_BAD_ARG, "hb_fxp_carry_combine: the outputs are arrays of their own");
    const FxpCarryCombineArgs A = {u32(opened), u32(g), u32(p), u32(ta), u32(tb), u32(tab), u32(g_out), u32(p_out), pairs, root};
    return run.template rows<FxpCarryCombineRow>(A, out_nodes, count);
}

template <class Run> static int fxp_div2m_finish_step(const Run &run, const uint64_t *x, const uint64_t *c, const uint64_t *r1, const uint64_t *carry, int m,
                                                      const uint64_t *inv2m_host, int mode, uint64_t *out, int64_t count) {
    if (count < 0) return HB_ERR_BAD_ARG;
    if (mode != HB_FXP_MOD && mode != HB_FXP_TRUNC && mode != HB_FXP_NEG_TRUNC) return run.fail(HB_ERR_BAD_ARG, "hb_fxp_div2m_finish: unknown mode");
    if ((mode != HB_FXP_MOD && !inv2m_host) || (count > 0 && (!c || !r1 || !carry || !out || (mode != HB_FXP_MOD && !x)))) return HB_ERR_BAD_ARG;
    if (!fxp_m_ok(run.bits(), m)) return run.fail(HB_ERR_BAD_ARG, "hb_fxp_div2m_finish: needs 0 < m <= bits(p) - 2");
    const int rc = run.template rows<FxpFinishRow, FxpFinishArgs>([&](auto &A, const auto &P) {
        A.x = u32(x); A.c = u32(c); A.r1 = u32(r1); A.carry = u32(carry); A.out = u32(out);
        return fxp_finish_consts(A, P, m, mode, inv2m_host);
    }, 1, count);
    return rc == HB_ERR_BAD_ARG ? run.fail(rc, "hb_fxp_div2m_finish: inv2m is not below the modulus") : rc;
}

}  // namespace hb

extern "C" {

int hb_fxp_mask(hb_ctx *ctx, const uint64_t *x_dev, const uint64_t *bits_dev, int k, int m, int kappa, uint64_t *masked_dev, uint64_t *r1_dev, int64_t count,
                void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : fxp_mask_step(DeviceRun{ctx, (hipStream_t)stream, "hb_fxp_mask"}, x_dev, bits_dev, k, m, kappa, masked_dev, r1_dev, count);
}

int hb_fxp_trunc_pr(hb_ctx *ctx, const uint64_t *x_dev, const uint64_t *c_dev, const uint64_t *r1_dev, int m, const uint64_t *inv2m_host, uint64_t *out_dev,
                    int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : fxp_trunc_pr_step(DeviceRun{ctx, (hipStream_t)stream, "hb_fxp_trunc_pr"}, x_dev, c_dev, r1_dev, m, inv2m_host, out_dev, count);
}

int hb_fxp_ltl_leaves(hb_ctx *ctx, const uint64_t *c_dev, const uint64_t *bits_dev, int m, uint64_t *g_dev, uint64_t *p_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : fxp_ltl_leaves_step(DeviceRun{ctx, (hipStream_t)stream, "hb_fxp_ltl_leaves"}, c_dev, bits_dev, m, g_dev, p_dev, count);
}

int hb_fxp_carry_mask(hb_ctx *ctx, const uint64_t *g_dev, const uint64_t *p_dev, int nodes, int root, const uint64_t *ta_dev, const uint64_t *tb_dev,
                      uint64_t *masked_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : fxp_carry_mask_step(DeviceRun{ctx, (hipStream_t)stream, "hb_fxp_carry_mask"}, g_dev, p_dev, nodes, root, ta_dev, tb_dev, masked_dev,
                                                       count);
}

int hb_fxp_carry_combine(hb_ctx *ctx, const uint64_t *opened_dev, const uint64_t *g_dev, const uint64_t *p_dev, int nodes, int root, const uint64_t *ta_dev,
                         const uint64_t *tb_dev, const uint64_t *tab_dev, uint64_t *g_out_dev, uint64_t *p_out_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : fxp_carry_combine_step(DeviceRun{ctx, (hipStream_t)stream, "hb_fxp_carry_combine"}, opened_dev, g_dev, p_dev, nodes, root, ta_dev,
                                                          tb_dev, tab_dev, g_out_dev, p_out_dev, count);
}

int hb_fxp_div2m_finish(hb_ctx *ctx, const uint64_t *x_dev, const uint64_t *c_dev, const uint64_t *r1_dev, const uint64_t *carry_dev, int m, const uint64_t *inv2m_host,
                        int mode, uint64_t *out_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : fxp_div2m_finish_step(DeviceRun{ctx, (hipStream_t)stream, "hb_fxp_div2m_finish"}, x_dev, c_dev, r1_dev, carry_dev, m, inv2m_host,
                                                         mode, out_dev, count);
}

// params: k, m, kappa, aux (nodes of a level, the finish's mode), root
int hb_selftest_fxp(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *ops, const int64_t *params, uint64_t *const *outs, int64_t count) {
    if (!p_limbs || !ops || !params || !outs || (n_limbs != 1 && n_limbs != 4)) return HB_ERR_BAD_ARG;
    for (int i = 0; i < 5; i++) if (params[i] < -(1 << 30) || params[i] > (1 << 30)) return HB_ERR_BAD_ARG;
    const HostRun run = {p_limbs, n_limbs};
    const int k = (int)params[0], m = (int)params[1], kappa = (int)params[2], aux = (int)params[3], root = (int)params[4];
    switch (what) {
    case HB_FXP_SELFTEST_MASK: return fxp_mask_step(run, ops[0], ops[1], k, m, kappa, outs[0], outs[1], count);
    case HB_FXP_SELFTEST_TRUNC_PR: return fxp_trunc_pr_step(run, ops[0], ops[1], ops[2], m, ops[3], outs[0], count);
    case HB_FXP_SELFTEST_LEAVES: return fxp_ltl_leaves_step(run, ops[0], ops[1], m, outs[0], outs[1], count);
    case HB_FXP_SELFTEST_CARRY_MASK: return fxp_carry_mask_step(run, ops[0], ops[1], aux, root, ops[2], ops[3], outs[0], count);
    case HB_FXP_SELFTEST_CARRY_COMBINE: return fxp_carry_combine_step(run, ops[0], ops[1], ops[2], aux, root, ops[3], ops[4], ops[5], outs[0], outs[1], count);
    case HB_FXP_SELFTEST_FINISH: return fxp_div2m_finish_step(run, ops[0], ops[1], ops[2], ops[3], m, ops[4], aux, outs[0], count);
    default: return HB_ERR_BAD_ARG;
    }
}

}  // extern "C"

// hb_fxp_elem.hpp -- the per-element bodies of the fixed-point steps, shared by hb_fxp.hip (masks, truncation, and the carry tree of
// div2m / ltz: only the root is kept), hb_bd.hip (the prefix network of the bit decomposition: every carry is kept), hb_div.hip
// (division: the prefix OR and the fused Goldschmidt steps) and hb_sort.hip (the comparison of a compare-exchange: the mask and the
// finish), with the Sklansky wiring the two networks share and the argument checks the files' entry points make, and the leaves'
// kernel k_leaves.  Host and device: a step's row (hb_rows.hpp) loads, calls these and
// stores, and the host self tests run the same rows.
#pragma once
#include <cstdint>
#include <cstring>
#include "hb_ew_elem.hpp"
#include "hb_rows.hpp"

namespace hb {

// the leaf of bit a (public) against the share bw of the mask's bit: a = 1 -> (1 - b, b); a = 0 -> (0, 1 - b)
template <int NL, int NW>
HB_HD void fxp_leaf_elem(uint32_t (&gw)[NW], uint32_t (&pw)[NW], uint32_t a, const uint32_t (&bw)[NW], const FpParams<NL> &P) {
    uint32_t b[NL], one[NL], nb[NL], g[NL], p[NL];
    unpack<NL, NW>(b, bw);
    small_digits<NL>(one, 1);
    fp_sub<NL>(nb, one, b, P);
#pragma unroll
    for (int q = 0; q < NL; q++) { g[q] = a ? nb[q] : 0u; p[q] = a ? b[q] : nb[q]; }
    pack<NL, NW>(gw, g);
    pack<NL, NW>(pw, p);
}

// g = g1 + [p1 g2], the product by the fused Beaver step of hb_ew_elem.hpp
template <int NL, int NW>
HB_HD void fxp_node_g_elem(uint32_t (&o)[NW], const uint32_t (&g1w)[NW], const uint32_t (&dw)[NW], const uint32_t (&ew)[NW], const uint32_t (&aw)[NW],
                           const uint32_t (&bw)[NW], const uint32_t (&abw)[NW], const FpParams<NL> &P) {
    uint32_t mw[NW], mm[NL], g1[NL], r[NL];
    ew_beaver_elem<NL, NW>(mw, dw, ew, aw, bw, abw, P);
    unpack<NL, NW>(mm, mw);
    unpack<NL, NW>(g1, g1w);
    fp_add<NL>(r, g1, mm, P);
    pack<NL, NW>(o, r);
}

// acc = 2 acc + b: one Horner step over a bit plane
template <int NL, int NW> HB_HD void fxp_horner(uint32_t (&acc)[NL], const uint32_t (&bw)[NW], const FpParams<NL> &P) {
    uint32_t b[NL], t[NL];
    unpack<NL, NW>(b, bw);
    fp_add<NL>(t, acc, acc, P);
    fp_add<NL>(acc, t, b, P);
}

// plane(w, i) loads this element's word of bit plane i.  HAS_X: o0 = x + half + sum_{i<nbits} 2^i b_i (half = 2^(k-1)), o1 = r1 =
// sum_{i<m} 2^i b_i;  else o0 = r2 = sum_{i<nbits-m} 2^i b_{m+i}, o1 = r1.
template <int NL, int NW, bool HAS_X, class Load>
HB_HD void fxp_mask_elem(uint32_t (&o0)[NW], uint32_t (&o1)[NW], const uint32_t (&xw)[NW], Load &&plane, int nbits, int m, const uint32_t (&half)[NL],
                         const FpParams<NL> &P) {
    uint32_t hi[NL], lo[NL], bw[NW];
#pragma unroll
    for (int q = 0; q < NL; q++) { hi[q] = 0; lo[q] = 0; }
#pragma unroll 4
    for (int i = nbits - 1; i >= m; i--) { plane(bw, i); fxp_horner<NL, NW>(hi, bw, P); }
#pragma unroll 4
    for (int i = m - 1; i >= 0; i--) {
        plane(bw, i);
        fxp_horner<NL, NW>(lo, bw, P);
        if constexpr (HAS_X) fxp_horner<NL, NW>(hi, bw, P);
    }
    if constexpr (HAS_X) {
        uint32_t x[NL], t[NL];
        unpack<NL, NW>(x, xw);
        fp_add<NL>(t, x, half, P);
        fp_add<NL>(x, t, hi, P);
        pack<NL, NW>(o0, x);
    } else {
        pack<NL, NW>(o0, hi);
    }
    pack<NL, NW>(o1, lo);
}

// o = c mod 2^m on packed words (0 < m < 32 NW)
template <int NW> HB_HD void fxp_low_bits(uint32_t (&o)[NW], const uint32_t (&cw)[NW], int m) {
#pragma unroll
    for (int q = 0; q < NW; q++) {
        const int rem = m - 32 * q;
        o[q] = rem >= 32 ? cw[q] : (rem <= 0 ? 0u : (cw[q] & ((1u << rem) - 1u)));
    }
}
// o = (x - (c mod 2^m) + r1) 2^(-m); invm = 2^(-m) R mod p
template <int NL, int NW>
HB_HD void fxp_trunc_pr_elem(uint32_t (&o)[NW], const uint32_t (&xw)[NW], const uint32_t (&cw)[NW], const uint32_t (&r1w)[NW], int m, const uint32_t (&invm)[NL],
                             const FpParams<NL> &P) {
    uint32_t c2w[NW], x[NL], c2[NL], t[NL], u[NL];
    fxp_low_bits<NW>(c2w, cw, m);
    unpack<NL, NW>(x, xw);
    unpack<NL, NW>(c2, c2w);
    fp_sub<NL>(t, x, c2, P);
    unpack<NL, NW>(c2, r1w);
    fp_add<NL>(u, t, c2, P);
    mont_mul<NL>(t, invm, u, P);
    pack<NL, NW>(o, t);
}

// what the finish needs: 2^m (canonical), 2^m and 2^(-m) (Montgomery)
template <int NL> struct FxpFinishConsts { uint32_t pow2[NL], pow2m[NL], inv2m[NL]; };

// mode HB_FXP_MOD: a2 = c2 - r1 + 2^m (1 - carry);  HB_FXP_TRUNC: (x - a2) 2^(-m);  HB_FXP_NEG_TRUNC: (a2 - x) 2^(-m)
// (hb_fxp.hip's finish; hb_sort.hip's swap mask takes the NEG_TRUNC result, the comparison's bit, without storing it)
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

// ---------------------------------------------------------------- the Sklansky wiring of hb_bd.hip and hb_div.hip (host and device)
// plane of node y of level l, and its partner
HB_HD int bd_node(int y, int l) { return ((y >> l) << (l + 1)) | (1 << l) | (y & ((1 << l) - 1)); }
HB_HD int bd_partner(int j, int l) { return ((j >> l) << l) - 1; }
// levels over n planes: ceil(log2 n), none for n <= 1
static inline int bd_levels(int n) {
    int l = 0;
    while ((1 << l) < n) l++;
    return l;
}
// planes j < n with bit l set: the nodes of level l
static inline int bd_active(int n, int l) {
    const int rest = (n & ((1 << (l + 1)) - 1)) - (1 << l);
    return ((n >> (l + 1)) << l) + (rest > 0 ? rest : 0);
}

// ---------------------------------------------------------------- the leaves steps of hb_fxp.hip and hb_bd.hip
// c (one row) and bits in, g and p out: arrays of their own
struct LeavesArgs { const uint32_t *c, *bits; uint32_t *g, *p; int m; };

// A leaves row walks the planes in the thread: a plane's load, then its two stores.  The loads of the next planes go out ahead of
// those stores only where the compiler knows the arrays apart, and at the 32-byte width it takes __restrict__ on the kernel's own
// parameters to tell it (pointers in an argument struct carry none, and on an inlined function's parameters it restores the 8-byte
// width's schedule alone).  So these two steps keep explicit pointers around the row's body, Row::planes; the host runs the same
// body through Row::run and host_rows.
template <class Row, int NL, int NW>
__global__ void __launch_bounds__(256) k_leaves(const FpParams<NL> P, const uint32_t *__restrict__ c, const uint32_t *__restrict__ bits, int m, uint32_t *__restrict__ g,
                                                uint32_t *__restrict__ p, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    Row::template planes<NL, NW>(c, bits, g, p, m, i, count, DeviceMem<NW>(), P);
}
template <class Row> int launch_leaves(hb_ctx *ctx, const LeavesArgs &A, unsigned blocks, hipStream_t s, int64_t count) {
    if (ctx->n_limbs == 4) k_leaves<Row, 9, 8><<<blocks, 256, 0, s>>>(ctx->pw, A.c, A.bits, A.m, A.g, A.p, count);
    else k_leaves<Row, 3, 2><<<blocks, 256, 0, s>>>(ctx->pn, A.c, A.bits, A.m, A.g, A.p, count);
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}
// the last line of a leaves step function (hb_rows.hpp): k_leaves on the device, the row's run on the host
template <class Row> int run_leaves(const DeviceRun &run, const LeavesArgs &A, int64_t count) {
    if (!run.fits(count)) return run.too_large();
    return launch_leaves<Row>(run.ctx, A, (unsigned)run.blocks(count), run.s, count);
}
template <class Row> int run_leaves(const HostRun &run, const LeavesArgs &A, int64_t count) { return run.template rows<Row>(A, 1, count); }

// ---------------------------------------------------------------- host side: argument checks
static inline bool fxp_m_ok(int bits, int m) { return m > 0 && m <= bits - 2; }

// the masked value c < 2^(k + kappa + 1) must stay below p
static inline bool fxp_params_ok(int bits, int k, int m, int kappa) { return m > 0 && m < k && kappa >= 0 && k <= 256 && kappa <= 256 && k + kappa + 1 <= bits - 1; }
// 2^e mod p, canonical digits (mont: times R)
template <int NL> static void fxp_pow2(uint32_t (&r)[NL], int e, bool mont, const FpParams<NL> &P) {
    if (mont) fp_set<NL>(r, P.one);
    else small_digits<NL>(r, 1);
    for (int i = 0; i < e; i++) { uint32_t t[NL]; fp_add<NL>(t, r, r, P); fp_set<NL>(r, t); }
}
// the finish's constants from m; inv2m_host (one canonical element in host memory) is read unless mode is HB_FXP_MOD: false if it is
// not below the modulus
template <int NL> static bool fxp_finish_fill(FxpFinishConsts<NL> &K, const FpParams<NL> &P, int m, int mode, const uint64_t *inv2m_host) {
    fxp_pow2<NL>(K.pow2, m, false, P);
    fxp_pow2<NL>(K.pow2m, m, true, P);
    for (int q = 0; q < NL; q++) K.inv2m[q] = 0;
    return mode != HB_FXP_MOD ? host_mont<NL, words_of(NL)>(K.inv2m, P, inv2m_host) : true;
}

}  // namespace hb

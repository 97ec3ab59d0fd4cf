// hb_fxp_elem.hpp -- the per-element bodies of the carry networks over (generate, propagate) planes, shared by hb_fxp.hip (the carry
// tree of div2m / ltz: only the root is kept) and hb_bd.hip (the prefix network of the bit decomposition: every carry is kept), with
// the argument checks both files' entry points make.  Host and device: the kernels only load, call and store, and the host self
// tests run the same functions.
#pragma once
#include <cstdint>
#include "hb_ew_elem.hpp"

namespace hb {

// bit i of the packed words (a chain of selects: the words stay in registers)
template <int NW> HB_HD uint32_t fxp_bit(const uint32_t (&cw)[NW], int i) {
    uint32_t w = 0;
#pragma unroll
    for (int q = 0; q < NW; q++) w = (q == (i >> 5)) ? cw[q] : w;
    return (w >> (i & 31)) & 1u;
}

// the leaf of bit a (public) against the share bw of the mask's bit: a = 1 -> (1 - b, b); a = 0 -> (0, 1 - b)
template <int NL, int NW>
HB_HD void fxp_leaf_elem(uint32_t (&gw)[NW], uint32_t (&pw)[NW], uint32_t a, const uint32_t (&bw)[NW], const FpParams<NL> &P) {
    uint32_t b[NL], one[NL], nb[NL], g[NL], p[NL];
    unpack<NL, NW>(b, bw);
#pragma unroll
    for (int q = 0; q < NL; q++) one[q] = q == 0 ? 1u : 0u;
    fp_sub<NL>(nb, one, b, P);
#pragma unroll
    for (int q = 0; q < NL; q++) { g[q] = a ? nb[q] : 0u; p[q] = a ? b[q] : nb[q]; }
    pack<NL, NW>(gw, g);
    pack<NL, NW>(pw, p);
}

// o = v - a: a masked difference
template <int NL, int NW> HB_HD void fxp_diff_elem(uint32_t (&o)[NW], const uint32_t (&vw)[NW], const uint32_t (&aw)[NW], const FpParams<NL> &P) {
    uint32_t v[NL], a[NL], r[NL];
    unpack<NL, NW>(v, vw);
    unpack<NL, NW>(a, aw);
    fp_sub<NL>(r, v, a, P);
    pack<NL, NW>(o, r);
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

// read-once operands (bit planes, triples, what was just opened)
template <int NW> __device__ __forceinline__ void fxp_load_once(uint32_t (&w)[NW], const uint32_t *p) {
    if constexpr (NW % 4 == 0) load_words_nt<NW>(w, p); else load_words<NW>(w, p);
}

// ---------------------------------------------------------------- host side: argument checks
static inline int fxp_modulus_bits(const uint64_t *p_limbs, int n_limbs) {
    for (int l = n_limbs - 1; l >= 0; l--)
        if (p_limbs[l]) return 64 * l + 64 - __builtin_clzll(p_limbs[l]);
    return 0;
}
static inline bool fxp_m_ok(int bits, int m) { return m > 0 && m <= bits - 2; }
static inline bool fxp_overlap(const void *x, int64_t x_bytes, const void *y, int64_t y_bytes) {
    const uintptr_t a = (uintptr_t)x, b = (uintptr_t)y;
    return x && y && a < b + (uintptr_t)y_bytes && b < a + (uintptr_t)x_bytes;
}

}  // namespace hb

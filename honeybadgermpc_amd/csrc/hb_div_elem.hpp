// hb_div_elem.hpp -- the per-element bodies of the division's steps (hb_div.hip), which the square root's steps (hb_fxsqrt.hip) call
// too: the prefix OR's node, the scale's Horner, the affine map after a Beaver combine, the truncation mask that keeps product + r1,
// and the truncation from it.  Host and device: a step's row (hb_rows.hpp) loads, calls these and stores.
#pragma once
#include "hb_fxp_elem.hpp"

namespace hb {

// ---------------------------------------------------------------- per-element bodies (host and device)
// y_j + y_q - [y_j y_q], the product by the fused Beaver step of hb_ew_elem.hpp
template <int NL, int NW>
HB_HD void div_or_elem(uint32_t (&o)[NW], const uint32_t (&yjw)[NW], const uint32_t (&yqw)[NW], const uint32_t (&dw)[NW], const uint32_t (&ew)[NW],
                       const uint32_t (&aw)[NW], const uint32_t (&bw)[NW], const uint32_t (&abw)[NW], const FpParams<NL> &P) {
    uint32_t mw[NW], mm[NL], a[NL], b[NL], t[NL];
    ew_beaver_elem<NL, NW>(mw, dw, ew, aw, bw, abw, P);
    unpack<NL, NW>(mm, mw);
    unpack<NL, NW>(a, yjw);
    unpack<NL, NW>(b, yqw);
    fp_add<NL>(t, a, b, P);
    fp_sub<NL>(a, t, mm, P);
    pack<NL, NW>(o, a);
}

// v = 2^(n-1) y_0 - sum_{i>=1} 2^(n-1-i) y_i: plane(w, i) loads this element's word of plane i
template <int NL, int NW, class Load> HB_HD void div_scale_elem(uint32_t (&vw)[NW], Load &&plane, int n, const FpParams<NL> &P) {
    uint32_t acc[NL], y[NL], t[NL], w[NW];
    plane(w, 0);
    unpack<NL, NW>(acc, w);
#pragma unroll 4
    for (int i = 1; i < n; i++) {
        plane(w, i);
        unpack<NL, NW>(y, w);
        fp_add<NL>(t, acc, acc, P);
        fp_sub<NL>(acc, t, y, P);
    }
    pack<NL, NW>(vw, acc);
}

// o = cst + aux + coef prod, coef = 1, -1 or -2
template <int NL, int NW>
HB_HD void div_affine_elem(uint32_t (&o)[NW], const uint32_t (&prodw)[NW], int coef, const uint32_t (&cst)[NL], const uint32_t (&auxw)[NW], const FpParams<NL> &P) {
    uint32_t pr[NL], a[NL], t[NL];
    unpack<NL, NW>(pr, prodw);
    unpack<NL, NW>(a, auxw);
    fp_add<NL>(t, a, cst, P);
    if (coef > 0) fp_add<NL>(a, t, pr, P); else fp_sub<NL>(a, t, pr, P);
    if (coef == -2) { fp_sub<NL>(t, a, pr, P); fp_set<NL>(a, t); }
    pack<NL, NW>(o, a);
}

// the truncation mask of v: masked = v + half + r1 + 2^m r2 (half = 2^(width-1)), s = v + r1
template <int NL, int NW, class Load>
HB_HD void div_trunc_mask_elem(uint32_t (&masked)[NW], uint32_t (&sw)[NW], const uint32_t (&vw)[NW], Load &&plane, int nbits, int m, const uint32_t (&half)[NL],
                               const FpParams<NL> &P) {
    uint32_t r1w[NW], v[NL], r1[NL], t[NL];
    fxp_mask_elem<NL, NW, true>(masked, r1w, vw, plane, nbits, m, half, P);
    unpack<NL, NW>(v, vw);
    unpack<NL, NW>(r1, r1w);
    fp_add<NL>(t, v, r1, P);
    pack<NL, NW>(sw, t);
}

// o = (s - (c mod 2^m)) 2^(-m); invm = 2^(-m) R mod p
template <int NL, int NW>
HB_HD void div_trunc_elem(uint32_t (&o)[NW], const uint32_t (&sw)[NW], const uint32_t (&cw)[NW], int m, const uint32_t (&invm)[NL], const FpParams<NL> &P) {
    uint32_t c2w[NW], s[NL], c2[NL], t[NL];
    fxp_low_bits<NW>(c2w, cw, m);
    unpack<NL, NW>(s, sw);
    unpack<NL, NW>(c2, c2w);
    fp_sub<NL>(t, s, c2, P);
    mont_mul<NL>(s, invm, t, P);
    pack<NL, NW>(o, s);
}

}  // namespace hb

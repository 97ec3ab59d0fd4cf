// hb_lt_elem.hpp -- the leaf of the comparison against a public value, shared by the two files whose leaves it is: hb_lt.hip (LtLeavesRow:
// the public bit comes from the opened c of every element) and hb_offsb.hip (SbLeavesRow: the public bit comes from one bound held by
// value).  The leaf is affine in the bit share because the other bit is public; the tree over the leaves is hb_fxp.hip's.
#pragma once
#include "hb_common.hpp"
#include "hb_rows.hpp"

namespace hb {

// the leaf of the public bit a of c against the share bw of the same bit of r
template <int NL, int NW>
HB_HD void lt_leaf_elem(uint32_t (&gw)[NW], uint32_t (&pw)[NW], uint32_t a, const uint32_t (&bw)[NW], int mode, const FpParams<NL> &P) {
    uint32_t b[NL], k[NL], t[NL], w[NL], g[NL], p[NL];
    unpack<NL, NW>(b, bw);
    if (mode == HB_LT_DIRECT) {                        // mode is the same for every lane; the bit a selects
        small_digits<NL>(k, 1);
        fp_sub<NL>(t, k, b, P);                        // 1 - r_i
#pragma unroll
        for (int q = 0; q < NL; q++) p[q] = a ? b[q] : t[q];
    } else {
        small_digits<NL>(k, 2);
        fp_sub<NL>(t, k, b, P);                        // 2 - r_i
        small_digits<NL>(k, 1);
        fp_add<NL>(w, k, b, P);                        // 1 + r_i
#pragma unroll
        for (int q = 0; q < NL; q++) p[q] = a ? t[q] : w[q];
    }
#pragma unroll
    for (int q = 0; q < NL; q++) g[q] = a ? 0u : b[q];
    pack<NL, NW>(gw, g);
    pack<NL, NW>(pw, p);
}

}  // namespace hb

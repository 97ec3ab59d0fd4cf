// hb_ew_elem.hpp -- the per-element bodies that several files share: the fused Beaver step (hb_ew.hip's EwBeaverRow, hb_bf.hip's
// BfSwitchRow and every other step that multiplies shares) and the masked product a b + c of the offline phase (hb_off.hip's OffMulAddRow, hb_offpow.hip's
// PowMaskRow).  Host and device: the rows only load, call and store, and the host self tests run the same functions.
#pragma once
#include "fp29.hpp"

namespace hb {

// o = d e + d q + e p + pq  (share_arithmetic.py:43) as d (e + q) + e p + pq: 3 mac + 2 redc.
// Bounds.  s = e + q is taken digit by digit with no carry and no reduction: s[i] <= 2 (2^29 - 1).  Column k of d * s + e * p
// then holds at most NL products of (2^29 - 1) * 2 (2^29 - 1) and NL of (2^29 - 1)^2, below 3 NL 2^58 -- three of the
// Lazy<NL>::GROUP = 7 (NL = 9) products a column may take (fp29.hpp:8).  REDC adds NL more products and its neighbour's carry
// (< 2^35): 4 NL 2^58 + 2^35 < 2^64 for NL <= 9, so, as in mont_mul, no carry pass is needed in front of REDC (it moves carries
// itself and only reads the low 29 bits of a column).  The value T = d (e + q) + e p < 3 p^2, so REDC returns
// u < p (1 + 3 p / R) < 2 p (R = 2^(29 NL) >= 32 p) with a top digit below 2^26: one conditional subtraction.  u = T / R; the
// product by R^2 gives T mod p, canonical; + pq with its conditional subtraction ends it.  p = 2^256 - 189 with every operand
// p - 1 is the largest case (tests/test_share_arithmetic_host.py).
template <int NL, int NW>
HB_HD void ew_beaver_elem(uint32_t (&o)[NW], const uint32_t (&dw)[NW], const uint32_t (&ew)[NW], const uint32_t (&pw)[NW],
                          const uint32_t (&qw)[NW], const uint32_t (&pqw)[NW], const FpParams<NL> &P) {
    uint32_t d[NL], e[NL], x[NL], s[NL];
    uint64_t c[2 * NL];
    unpack<NL, NW>(d, dw);
    unpack<NL, NW>(e, ew);
    unpack<NL, NW>(x, qw);
#pragma unroll
    for (int i = 0; i < NL; i++) s[i] = e[i] + x[i];
    col_zero(c);
    mac<NL>(c, d, s);
    unpack<NL, NW>(x, pw);
    mac<NL>(c, e, x);
    redc<NL>(s, c, P);
    cond_sub_p<NL>(s, P);
    mont_mul<NL>(d, P.r2, s, P);
    unpack<NL, NW>(x, pqw);
    fp_add<NL>(s, d, x, P);
    pack<NL, NW>(o, s);
}

// o = a b + c on packed words (the product as ew_binary_elem's MUL: ab / R, then times R^2)
template <int NL, int NW>
HB_HD void ew_mul_add_elem(uint32_t (&o)[NW], const uint32_t (&a)[NW], const uint32_t (&b)[NW], const uint32_t (&c)[NW], const FpParams<NL> &P) {
    uint32_t ad[NL], bd[NL], cd[NL], t[NL], r[NL];
    unpack<NL, NW>(ad, a);
    unpack<NL, NW>(bd, b);
    unpack<NL, NW>(cd, c);
    mont_mul<NL>(t, bd, ad, P);
    mont_mul<NL>(r, P.r2, t, P);
    fp_add<NL>(t, r, cd, P);
    pack<NL, NW>(o, t);
}

}  // namespace hb

// hb_sort_elem.hpp -- the per-slot bodies of the compare-exchange steps of hb_sort.hip: where a comparator's two rows lie, the bit
// that decides the swap and the swap itself.  Host and device: a step's row (hb_rows.hpp) loads, calls these and stores, and
// hb_selftest_sort runs the same rows.  The mask of the comparison is fxp_mask_elem, the comparison's bit fxp_finish_elem
// (hb_fxp_elem.hpp) and the product ew_beaver_elem (hb_ew_elem.hpp): called here, not restated.
#pragma once
#include "hb_fxp_elem.hpp"

namespace hb {

// One layer of the merge exchange over `batch` arrays of n rows: comparator e < cnt of an array compares rows lo(e) and lo(e) + d,
// lo(e) = ((e >> a) << (a + 1)) | (e & (2^a - 1)) | r -- the e-th index whose bit a equals r's.  plane = batch n, the elements of a column.
struct SortLayer { int64_t n, plane; uint32_t cnt, a, r, d; };

// slot s = array s / cnt, comparator s % cnt -> its two rows within a column
HB_HD void sort_slot_rows(const SortLayer &L, int64_t s, int64_t &lo, int64_t &hi) {
    const int64_t b = s / (int64_t)L.cnt;
    const uint32_t e = (uint32_t)(s - b * (int64_t)L.cnt);
    const uint32_t l = ((e >> L.a) << (L.a + 1)) | (e & ((1u << L.a) - 1u)) | L.r;
    lo = b * L.n + (int64_t)l;
    hi = lo + (int64_t)L.d;
}

// u = 1 - [key_lo < key_hi], the share of "swap": d = key_lo - key_hi, c the opened mask of d, r1 and the carry as hb_fxp_div2m_finish
// takes them; [d < 0] is its HB_FXP_NEG_TRUNC result at m = k - 1
template <int NL, int NW>
HB_HD void sort_swap_bit_elem(uint32_t (&uw)[NW], const uint32_t (&dw)[NW], const uint32_t (&cw)[NW], const uint32_t (&r1w)[NW], const uint32_t (&carryw)[NW], int m,
                              const FxpFinishConsts<NL> &K, const FpParams<NL> &P) {
    uint32_t bw[NW], b[NL], one[NL], u[NL];
    fxp_finish_elem<NL, NW>(bw, dw, cw, r1w, carryw, m, HB_FXP_NEG_TRUNC, K, P);
    unpack<NL, NW>(b, bw);
    small_digits<NL>(one, 1);
    fp_sub<NL>(u, one, b, P);
    pack<NL, NW>(uw, u);
}

// lo -= m, hi += m: with m = u (lo - hi) the pair is swapped where u = 1 and kept where u = 0
template <int NL, int NW>
HB_HD void sort_exchange_elem(uint32_t (&low)[NW], uint32_t (&hiw)[NW], const uint32_t (&mw)[NW], const FpParams<NL> &P) {
    uint32_t m[NL], x[NL], r[NL];
    unpack<NL, NW>(m, mw);
    unpack<NL, NW>(x, low);
    fp_sub<NL>(r, x, m, P);
    pack<NL, NW>(low, r);
    unpack<NL, NW>(x, hiw);
    fp_add<NL>(r, x, m, P);
    pack<NL, NW>(hiw, r);
}

// ---------------------------------------------------------------- host side: argument checks
// A layer the steps accept: 2 <= n <= 2^31, batch >= 1, a <= 30, r = 0 or 2^a, d a positive odd multiple of 2^a (so bit a of
// lo + d differs from bit a of lo: no row is the low row of one comparator and the high row of another -- the layer is a matching),
// and every comparator inside its array: lo(cnt - 1) + d < n.  slots = batch cnt and plane = batch n stay below 2^40.
static inline bool sort_layer_ok(SortLayer &L, int64_t n, int64_t batch, int a, int64_t r, int64_t d, int64_t cnt) {
    const int64_t top = (int64_t)1 << 40;
    if (n < 2 || n > ((int64_t)1 << 31) || batch < 1 || batch > top || a < 0 || a > 30) return false;
    const int64_t p = (int64_t)1 << a;
    if ((r != 0 && r != p) || d <= 0 || d >= n || (d & (p - 1)) != 0 || ((d >> a) & 1) == 0 || cnt < 0 || cnt > n) return false;
    if (batch > top / n) return false;
    L.n = n; L.plane = batch * n; L.cnt = (uint32_t)cnt; L.a = (uint32_t)a; L.r = (uint32_t)r; L.d = (uint32_t)d;
    if (cnt == 0) return true;
    const int64_t e = cnt - 1, lo = ((e >> a) << (a + 1)) | (e & (p - 1)) | r;
    return lo + d < n;
}

}  // namespace hb

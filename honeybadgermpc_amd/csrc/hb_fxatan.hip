// hb_fxatan.hip -- arctangent and atan2 of shared fixed-point numbers (signed k-bit values with f fractional bits), for arrays of pairs
// (y, x): the glue between the opens of the comparison (hb_fxp.hip), the division (hb_div.hip) and "products to truncation masks"
// (hb_fxexp_products_trunc).  (The reference has no arctangent: nothing here is a translation.)  A sign bit s stands for sigma = 1 - 2 s.
// With sx = [x < 0], sy = [y < 0], w = |x| - |y|, c = [w < 0], q = min(|x|, |y|) / max(|x|, |y|) in [0, 1] and a = atan q:
//     atan2(y, x) = pi g + (pi / 2) h + E a,   g = sigma_y sx,   h = sigma_y sigma_x c,   E = sigma_y sigma_x sigma_c = +-1
// and h = (sigma_y - 2 g - E) / 2, so the three bit products g, e1 = sigma_c sigma_x and E = sigma_y e1 are all the octant costs, and
// each rides in an open that exists anyway.  a is an ODD polynomial of degree d in t = 2^(N-f) q, N = k - 1, at scale beta = 2^N; with J =
// (d - 1) / 2 it needs the odd powers t^(2j+1), j <= J, and the squares u^(2^l), u = t^2:
//     level 0                     u = [t t]
//     level l = 1 .. levels       t^(2j+1) = [t^(2j+1-2^l) u^(2^(l-1))], 2^(l-1) <= j < min(2^l, J + 1): product q = j - 2^(l-1), whose first
//                                 operand is odd power q; then, last and only while a later level needs it (l < levels = bit_length(J)),
//                                 u^(2^l) = [u^(2^(l-1)) u^(2^(l-1))]
// every product truncated by N bits: 15 products at d = 23 where the powers 2 .. 23 would take 22.  A closed form, so no index list travels.
//
// FxAtanSignMaskRow    after the comparison of (x, y) against 0: the masked pairs of [sx x], [sy y] and [sigma_y sx], blockIdx.y the product.
// FxAtanAbsRow         after their open: |x| = x - 2 [sx x], |y| = y - 2 [sy y], g, w = |x| - |y| and the mask of the comparison of w against
//                      0 from k + kappa bit planes (fxp_mask_elem, the body of hb_fxp_mask); kept: |x|, |y|, g, w, r1.
// FxAtanSelectMaskRow  after that comparison: the masked pairs of [c w] and [sigma_c sigma_x], blockIdx.y the product.
// FxAtanSelectRow      after their open: num = |y| + [c w], den = |x| - [c w], e1 = [sigma_c sigma_x].
// FxAtanFirstRow       after the division: t = 2^(N-f) q, row 0 of `powers` ([J + 1][count]); the masked pairs of [t t] and of E = [sigma_y e1].
// FxAtanLevelRow       after the open of level l's masked truncations, 0 <= l < levels: the odd powers of level l go to their rows of
//                      `powers`, and the masked pairs of level l + 1 are formed.  blockIdx.y = q over max(level l's truncations, level l +
//                      1's products).  u^(2^l) and, for q >= 2^(l-1), odd power q are values this very launch finishes: the thread
//                      recomputes them from (s, opened) -- a truncation is one subtraction and one product -- and waits for nobody; the
//                      older odd powers are read from `powers`, rows below 2^(l-1), which this launch does not write.  A square is never
//                      stored: only the launch that finishes it reads it.
// FxAtanPolyMaskRow    after the open of the LAST level's masked truncations: finishes them, L = sum_j A_j t^(2j+1) in one walk (A_j PUBLIC,
//                      wave-uniform, 64-bit columns with one reduction every 7 terms, as FxLogPolyMaskRow does) and L's truncation mask
//                      (div_trunc_mask_elem).
// FxAtanAssembleRow    after L's open: a = the truncation, E by the Beaver combine of the pair the FIRST step's open carried, the masked
//                      pair of [E a], and C = A g + B (sigma_y - E) with A = Pi - H, B = H / 2 in the field (H stands for pi / 2 at the
//                      result's scale: sigma_y - 2 g - E is twice a bit, so the field's inverse of 2 halves it exactly).
// FxAtanFinishRow      after the last open: C + [E a].  E = +-1: no truncation follows.
// hb_div_product_step(SIGN) is the |b| of ONE product; the three of the abs step and its mask are one launch here.  "Products to
// truncation masks" is hb_fxexp_products_trunc as it stands, the leaves, the carry tree and the finish of the comparisons hb_fxp.hip's.
//
// Operands and results are packed canonical residues.  A step's row is an HB_HD function over a memory policy (hb_rows.hpp): k_rows runs
// it on the device, host_rows the very same row in hb_selftest_fxatan, and each step is ONE step function behind both.
//
// Launch shape (all kernels): 256-thread workgroups, one element a thread in x, the product in blockIdx.y where a step has several.  No
// LDS, no grid stride, one launch a call.  Planes, triples, opened and kept values are read once (load_once); the older powers take the
// plain load; the coefficients are one address a wave (same) and sit in SGPRs.
// Compiler's report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; scratch = 0 bytes, LDS = 0 for every kernel):
//   FxAtanSignMaskRow<9, 8>    39 VGPRs: 8 waves a SIMD                                  FxAtanSignMaskRow<3, 2>    15 VGPRs: 8 waves
//   FxAtanAbsRow<9, 8>         84 VGPRs: 5 waves                                         FxAtanAbsRow<3, 2>         44 VGPRs: 8 waves
//   FxAtanSelectMaskRow<9, 8>  47 VGPRs: 8 waves                                         FxAtanSelectMaskRow<3, 2>  23 VGPRs: 8 waves
//   FxAtanSelectRow<9, 8>      72 VGPRs: 7 waves                                         FxAtanSelectRow<3, 2>      38 VGPRs: 8 waves
//   FxAtanFirstRow<9, 8>       50 VGPRs: 8 waves                                         FxAtanFirstRow<3, 2>       22 VGPRs: 8 waves
//   FxAtanLevelRow<9, 8>       57 VGPRs: 8 waves                                         FxAtanLevelRow<3, 2>       16 VGPRs: 8 waves
//   FxAtanPolyMaskRow<9, 8>    98 VGPRs: 4 waves                                         FxAtanPolyMaskRow<3, 2>    35 VGPRs: 8 waves
//   FxAtanAssembleRow<9, 8>    72 VGPRs: 7 waves                                         FxAtanAssembleRow<3, 2>    36 VGPRs: 8 waves
//   FxAtanFinishRow<9, 8>      71 VGPRs: 7 waves                                         FxAtanFinishRow<3, 2>      25 VGPRs: 8 waves
// (DESIGN.md section 3af has the series, the error and width derivations and the counts.)
#include "hb_common.hpp"
#include "hb_div_elem.hpp"

using namespace hb;

namespace hb {

constexpr int FXATAN_MAX_DEGREE = 63;

// ---------------------------------------------------------------- the shape of a level (host and device)
HB_HD int fxatan_levels(int J) { int l = 0; while ((J >> l) != 0) l++; return l; }
// odd powers level l >= 1 forms: 2^(l-1) <= j < min(2^l, J + 1)
HB_HD int fxatan_level_odd(int level, int J) {
    if (level < 1) return 0;
    const int lo = 1 << (level - 1), hi = (2 * lo < J + 1) ? 2 * lo : J + 1;
    return hi > lo ? hi - lo : 0;
}
// products of level l: u alone at level 0; the odd powers and, while a later level needs it, the square
HB_HD int fxatan_level_products(int level, int J) {
    if (level == 0) return 1;
    const int n = fxatan_level_odd(level, J);
    return n == 0 ? 0 : n + (level < fxatan_levels(J) ? 1 : 0);
}

// ---------------------------------------------------------------- per-element bodies (host and device)
// sigma = 1 - 2 s
template <int NL, int NW> HB_HD void fxatan_sigma_elem(uint32_t (&o)[NW], const uint32_t (&sw)[NW], const FpParams<NL> &P) {
    uint32_t s[NL], one[NL], t[NL], u[NL];
    unpack<NL, NW>(s, sw);
    small_digits<NL>(one, 1);
    fp_sub<NL>(t, one, s, P);
    fp_sub<NL>(u, t, s, P);
    pack<NL, NW>(o, u);
}

// o = a + b or a - b
template <int NL, int NW> HB_HD void fxatan_addsub_elem(uint32_t (&o)[NW], const uint32_t (&aw)[NW], const uint32_t (&bw)[NW], bool add, const FpParams<NL> &P) {
    uint32_t a[NL], b[NL], t[NL];
    unpack<NL, NW>(a, aw);
    unpack<NL, NW>(b, bw);
    if (add) fp_add<NL>(t, a, b, P); else fp_sub<NL>(t, a, b, P);
    pack<NL, NW>(o, t);
}

// o = cm v, cm a constant in Montgomery form
template <int NL, int NW> HB_HD void fxatan_scale_elem(uint32_t (&o)[NW], const uint32_t (&vw)[NW], const uint32_t (&cm)[NL], const FpParams<NL> &P) {
    uint32_t v[NL], t[NL];
    unpack<NL, NW>(v, vw);
    mont_mul<NL>(t, cm, v, P);
    pack<NL, NW>(o, t);
}

// sum_{i < n} coef_i value_i (fxlog_poly_elem's scheme: a column takes GROUP products before carries must move; a reduced group sum is
// below 2 p; the sum of them is the sum / R, and the product by R^2 at the end makes it the sum)
template <int NL, int NW, class Value, class Coef>
HB_HD void fxatan_poly_elem(uint32_t (&o)[NW], Value &&value, Coef &&coef, int n, const FpParams<NL> &P) {
    constexpr int GROUP = Lazy<NL>::GROUP;
    uint32_t y[NL], a[NL], t[NL], g[NL], sum[NL], w[NW];
    uint64_t c[2 * NL];
#pragma unroll
    for (int q = 0; q < NL; q++) sum[q] = 0u;
    for (int base = 0; base < n; base += GROUP) {
        col_zero(c);
        const int end = base + GROUP < n ? base + GROUP : n;
        for (int i = base; i < end; i++) {
            value(w, i);
            unpack<NL, NW>(y, w);
            coef(w, i);
            unpack<NL, NW>(a, w);
            mac<NL>(c, a, y);
        }
        finish<NL>(g, c, P, 1);
        fp_add<NL>(t, sum, g, P);
        fp_set<NL>(sum, t);
    }
    mont_mul<NL>(t, P.r2, sum, P);
    pack<NL, NW>(o, t);
}

// truncation r of the level whose masks were just opened
template <int NL, int NW, class Mem>
HB_HD void fxatan_trunc_row(uint32_t (&o)[NW], const uint32_t *s, const uint32_t *opened, int r, int64_t i, int64_t count, int m, const uint32_t (&invm)[NL], const Mem &mem,
                            const FpParams<NL> &P) {
    uint32_t sw[NW], cw[NW];
    mem.once(sw, s, (int64_t)r * count + i); mem.once(cw, opened, (int64_t)r * count + i);
    div_trunc_elem<NL, NW>(o, sw, cw, m, invm, P);
}

// the Beaver combine of product r of an opened array of pairs
template <int NL, int NW, class Mem>
HB_HD void fxatan_beaver_row(uint32_t (&o)[NW], const uint32_t *opened, const uint32_t *ta, const uint32_t *tb, const uint32_t *tab, int r, int64_t i, int64_t count,
                             const Mem &mem, const FpParams<NL> &P) {
    uint32_t dw[NW], ew[NW], aw[NW], bw[NW], abw[NW];
    mem.once(dw, opened, (int64_t)(2 * r) * count + i); mem.once(ew, opened, (int64_t)(2 * r + 1) * count + i);
    mem.once(aw, ta, (int64_t)r * count + i); mem.once(bw, tb, (int64_t)r * count + i); mem.once(abw, tab, (int64_t)r * count + i);
    ew_beaver_elem<NL, NW>(o, dw, ew, aw, bw, abw, P);
}

// masked rows 2 r, 2 r + 1 = first - ta[r], second - tb[r]
template <int NL, int NW, class Mem>
HB_HD void fxatan_mask_pair(uint32_t *masked, const uint32_t (&first)[NW], const uint32_t (&second)[NW], const uint32_t *ta, const uint32_t *tb, int r, int64_t i,
                            int64_t count, const Mem &mem, const FpParams<NL> &P) {
    uint32_t aw[NW], o[NW];
    mem.once(aw, ta, (int64_t)r * count + i);
    diff_elem<NL, NW>(o, first, aw, P);
    mem.store(masked, (int64_t)(2 * r) * count + i, o);
    mem.once(aw, tb, (int64_t)r * count + i);
    diff_elem<NL, NW>(o, second, aw, P);
    mem.store(masked, (int64_t)(2 * r + 1) * count + i, o);
}

// ---------------------------------------------------------------- the steps' rows (host and device, over a memory policy)
struct FxAtanSignMaskArgs { const uint32_t *s, *x, *y, *ta, *tb; uint32_t *masked; };

struct FxAtanSignMaskRow {
template <int NL, int NW, class Mem>
HB_HD static void run(const FxAtanSignMaskArgs &A, int r, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
    uint32_t first[NW], second[NW];
    if (r == 0) { mem.once(first, A.s, i); mem.once(second, A.x, i); }
    else if (r == 1) { mem.once(first, A.s, count + i); mem.once(second, A.y, i); }
    else {
        mem.once(second, A.s, count + i);
        fxatan_sigma_elem<NL, NW>(first, second, P);
        mem.once(second, A.s, i);
    }
    fxatan_mask_pair<NL, NW>(A.masked, first, second, A.ta, A.tb, r, i, count, mem, P);
}
};

template <int NL> struct FxAtanAbsArgs {
    const uint32_t *opened, *ta, *tb, *tab, *x, *y, *bits;
    uint32_t *masked, *kept;
    int nbits, m;
    FpConst<NL> halfw;
};

struct FxAtanAbsRow {
template <int NL, int NW, class Mem>
HB_HD static void run(const FxAtanAbsArgs<NL> &A, int, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
    uint32_t pw[NW], vw[NW], ax[NW], ay[NW], ww[NW], o0[NW], o1[NW], zero[NL];
#pragma unroll
    for (int q = 0; q < NL; q++) zero[q] = 0u;
    fxatan_beaver_row<NL, NW>(pw, A.opened, A.ta, A.tb, A.tab, 0, i, count, mem, P);
    mem.once(vw, A.x, i);
    div_affine_elem<NL, NW>(ax, pw, -2, zero, vw, P);
    mem.store(A.kept, i, ax);
    fxatan_beaver_row<NL, NW>(pw, A.opened, A.ta, A.tb, A.tab, 1, i, count, mem, P);
    mem.once(vw, A.y, i);
    div_affine_elem<NL, NW>(ay, pw, -2, zero, vw, P);
    mem.store(A.kept, count + i, ay);
    fxatan_beaver_row<NL, NW>(pw, A.opened, A.ta, A.tb, A.tab, 2, i, count, mem, P);
    mem.store(A.kept, 2 * count + i, pw);
    fxatan_addsub_elem<NL, NW>(ww, ax, ay, false, P);
    mem.store(A.kept, 3 * count + i, ww);
    fxp_mask_elem<NL, NW, true>(o0, o1, ww, [&](uint32_t (&bw)[NW], int row) { mem.once(bw, A.bits, (int64_t)row * count + i); }, A.nbits, A.m, A.halfw.d, P);
    mem.store(A.masked, i, o0);
    mem.store(A.kept, 4 * count + i, o1);
}
};

struct FxAtanSelectMaskArgs { const uint32_t *c, *w, *sx, *ta, *tb; uint32_t *masked; };

struct FxAtanSelectMaskRow {
template <int NL, int NW, class Mem>
HB_HD static void run(const FxAtanSelectMaskArgs &A, int r, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
    uint32_t first[NW], second[NW], t[NW];
    if (r == 0) { mem.once(first, A.c, i); mem.once(second, A.w, i); }
    else {
        mem.once(t, A.c, i);
        fxatan_sigma_elem<NL, NW>(first, t, P);
        mem.once(t, A.sx, i);
        fxatan_sigma_elem<NL, NW>(second, t, P);
    }
    fxatan_mask_pair<NL, NW>(A.masked, first, second, A.ta, A.tb, r, i, count, mem, P);
}
};

struct FxAtanSelectArgs { const uint32_t *opened, *ta, *tb, *tab, *ax, *ay; uint32_t *out; };

struct FxAtanSelectRow {
template <int NL, int NW, class Mem>
HB_HD static void run(const FxAtanSelectArgs &A, int, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
    uint32_t pw[NW], vw[NW], o[NW];
    fxatan_beaver_row<NL, NW>(pw, A.opened, A.ta, A.tb, A.tab, 0, i, count, mem, P);
    mem.once(vw, A.ay, i);
    fxatan_addsub_elem<NL, NW>(o, vw, pw, true, P);
    mem.store(A.out, i, o);
    mem.once(vw, A.ax, i);
    fxatan_addsub_elem<NL, NW>(o, vw, pw, false, P);
    mem.store(A.out, count + i, o);
    fxatan_beaver_row<NL, NW>(pw, A.opened, A.ta, A.tb, A.tab, 1, i, count, mem, P);
    mem.store(A.out, 2 * count + i, pw);
}
};

template <int NL> struct FxAtanFirstArgs {
    const uint32_t *q, *sy, *e1, *ta, *tb;
    uint32_t *masked, *powers;
    FpConst<NL> scale;
};

struct FxAtanFirstRow {
template <int NL, int NW, class Mem>
HB_HD static void run(const FxAtanFirstArgs<NL> &A, int r, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
    uint32_t first[NW], second[NW], t[NW];
    if (r == 0) {
        mem.once(t, A.q, i);
        fxatan_scale_elem<NL, NW>(first, t, A.scale.d, P);
        mem.store(A.powers, i, first);
        fxatan_mask_pair<NL, NW>(A.masked, first, first, A.ta, A.tb, 0, i, count, mem, P);
    } else {
        mem.once(t, A.sy, i);
        fxatan_sigma_elem<NL, NW>(first, t, P);
        mem.once(second, A.e1, i);
        fxatan_mask_pair<NL, NW>(A.masked, first, second, A.ta, A.tb, 1, i, count, mem, P);
    }
}
};

template <int NL> struct FxAtanLevelArgs {
    const uint32_t *opened, *s, *ta, *tb;
    uint32_t *masked, *powers;
    int level, J, m;
    FpConst<NL> invm;
};

struct FxAtanLevelRow {
template <int NL, int NW, class Mem>
HB_HD static void run(const FxAtanLevelArgs<NL> &A, int q, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
    const int half = A.level ? 1 << (A.level - 1) : 0;                            // level l's odd powers are rows half .. of `powers`
    const int done = fxatan_level_products(A.level, A.J), odd = fxatan_level_odd(A.level + 1, A.J), next = fxatan_level_products(A.level + 1, A.J);
    uint32_t first[NW], square[NW];
    if (q < done - 1) {                                                           // the last truncation of a level before the last is the square
        fxatan_trunc_row<NL, NW>(first, A.s, A.opened, q, i, count, A.m, A.invm.d, mem, P);
        mem.store(A.powers, (int64_t)(half + q) * count + i, first);
    }
    if (q >= next) return;
    fxatan_trunc_row<NL, NW>(square, A.s, A.opened, done - 1, i, count, A.m, A.invm.d, mem, P);
    if (q >= odd) {                                                               // the next square
#pragma unroll
        for (int w = 0; w < NW; w++) first[w] = square[w];
    } else if (A.level && q >= half) fxatan_trunc_row<NL, NW>(first, A.s, A.opened, q - half, i, count, A.m, A.invm.d, mem, P);
    else mem.load(first, A.powers, (int64_t)q * count + i);
    fxatan_mask_pair<NL, NW>(A.masked, first, square, A.ta, A.tb, q, i, count, mem, P);
}
};

template <int NL> struct FxAtanPolyArgs {
    const uint32_t *opened, *s, *powers, *coef, *bits;
    uint32_t *masked, *s_out;
    int J, half, m_in, nbits, m_out;
    FpConst<NL> invm, halfw;
};

struct FxAtanPolyMaskRow {
template <int NL, int NW, class Mem>
HB_HD static void run(const FxAtanPolyArgs<NL> &A, int, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
    uint32_t lw[NW], o0[NW], o1[NW];
    fxatan_poly_elem<NL, NW>(lw, [&](uint32_t (&w)[NW], int j) {                      // term j is t^(2j+1)
        if (j < A.half) mem.once(w, A.powers, (int64_t)j * count + i);
        else fxatan_trunc_row<NL, NW>(w, A.s, A.opened, j - A.half, i, count, A.m_in, A.invm.d, mem, P);
    }, [&](uint32_t (&w)[NW], int j) { mem.same(w, A.coef + (int64_t)j * NW); }, A.J + 1, P);
    div_trunc_mask_elem<NL, NW>(o0, o1, lw, [&](uint32_t (&bw)[NW], int row) { mem.once(bw, A.bits, (int64_t)row * count + i); }, A.nbits, A.m_out, A.halfw.d, P);
    mem.store(A.masked, i, o0);
    mem.store(A.s_out, i, o1);
}
};

template <int NL> struct FxAtanAssembleArgs {
    const uint32_t *opened, *s, *eopened, *ea, *eb, *eab, *sy, *g, *ta, *tb;
    uint32_t *masked, *c;
    int m;
    FpConst<NL> invm, ca, cb;                                                   // ca, cb: A, B in Montgomery form
};

struct FxAtanAssembleRow {
template <int NL, int NW, class Mem>
HB_HD static void run(const FxAtanAssembleArgs<NL> &A, int, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
    uint32_t aw[NW], ew[NW], tw[NW], uw[NW], vw[NW];
    fxatan_trunc_row<NL, NW>(aw, A.s, A.opened, 0, i, count, A.m, A.invm.d, mem, P);
    fxatan_beaver_row<NL, NW>(ew, A.eopened, A.ea, A.eb, A.eab, 0, i, count, mem, P);
    fxatan_mask_pair<NL, NW>(A.masked, ew, aw, A.ta, A.tb, 0, i, count, mem, P);
    mem.once(tw, A.sy, i);
    fxatan_sigma_elem<NL, NW>(uw, tw, P);
    fxatan_addsub_elem<NL, NW>(tw, uw, ew, false, P);                               // sigma_y - E
    fxatan_scale_elem<NL, NW>(uw, tw, A.cb.d, P);
    mem.once(tw, A.g, i);
    fxatan_scale_elem<NL, NW>(vw, tw, A.ca.d, P);
    fxatan_addsub_elem<NL, NW>(tw, vw, uw, true, P);
    mem.store(A.c, i, tw);
}
};

struct FxAtanFinishArgs { const uint32_t *opened, *ta, *tb, *tab, *c; uint32_t *out; };

struct FxAtanFinishRow {
template <int NL, int NW, class Mem>
HB_HD static void run(const FxAtanFinishArgs &A, int, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
    uint32_t pw[NW], cw[NW], o[NW];
    fxatan_beaver_row<NL, NW>(pw, A.opened, A.ta, A.tb, A.tab, 0, i, count, mem, P);
    mem.once(cw, A.c, i);
    fxatan_addsub_elem<NL, NW>(o, cw, pw, true, P);
    mem.store(A.out, i, o);
}
};

// ---------------------------------------------------------------- host side
// One step function a step (hb_rows.hpp): a DeviceRun in the entry point, a HostRun in hb_selftest_fxatan.
static bool fxatan_degree_ok(int d) { return d >= 3 && d <= FXATAN_MAX_DEGREE && (d & 1); }

template <class Run> static int fxatan_sign_mask_step(const Run &run, const uint64_t *s, const uint64_t *x, const uint64_t *y, const uint64_t *ta, const uint64_t *tb,
                                                      uint64_t *masked, int64_t count) {
    if (count < 0 || (count > 0 && (!s || !x || !y || !ta || !tb || !masked))) return HB_ERR_BAD_ARG;
    if (count == 0) return HB_OK;
    const int64_t rb = run.elem_bytes() * count;
    const RowSpan outs[1] = {{masked, 6}}, ins[5] = {{s, 2}, {x, 1}, {y, 1}, {ta, 3}, {tb, 3}};
    if (!outputs_apart(outs, 1, ins, 5, rb)) return run.fail(HB_ERR_BAD_ARG, "hb_fxatan_sign_mask: masked is an array of its own");
    const FxAtanSignMaskArgs A = {u32(s), u32(x), u32(y), u32(ta), u32(tb), u32(masked)};
    return run.template rows<FxAtanSignMaskRow>(A, 3, count);
}

template <class Run> static int fxatan_abs_step(const Run &run, const uint64_t *opened, const uint64_t *ta, const uint64_t *tb, const uint64_t *tab, const uint64_t *x,
                                                const uint64_t *y, const uint64_t *bits, int k, int kappa, uint64_t *masked, uint64_t *kept, int64_t count) {
    if (count < 0) return HB_ERR_BAD_ARG;
    if (k < 2 || !fxp_params_ok(run.bits(), k, k - 1, kappa)) return run.fail(HB_ERR_BAD_ARG, "hb_fxatan_abs: needs a comparison the modulus has room for");
    if (count > 0 && (!opened || !ta || !tb || !tab || !x || !y || !bits || !masked || !kept)) return HB_ERR_BAD_ARG;
    const int64_t rb = run.elem_bytes() * count;
    const RowSpan outs[2] = {{masked, 1}, {kept, 5}}, ins[7] = {{opened, 6}, {ta, 3}, {tb, 3}, {tab, 3}, {x, 1}, {y, 1}, {bits, k + kappa}};
    if (count > 0 && !outputs_apart(outs, 2, ins, 7, rb)) return run.fail(HB_ERR_BAD_ARG, "hb_fxatan_abs: masked and kept are arrays of their own");
    return run.template rows<FxAtanAbsRow, FxAtanAbsArgs>([&](auto &A, const auto &P) {
        A.opened = u32(opened); A.ta = u32(ta); A.tb = u32(tb); A.tab = u32(tab); A.x = u32(x); A.y = u32(y); A.bits = u32(bits);
        A.masked = u32(masked); A.kept = u32(kept); A.nbits = k + kappa; A.m = k - 1;
        constexpr int NL = sizeof(A.halfw.d) / sizeof(uint32_t);
        fxp_pow2<NL>(A.halfw.d, k - 1, false, P);
        return true;
    }, 1, count);
}

template <class Run> static int fxatan_select_mask_step(const Run &run, const uint64_t *c, const uint64_t *w, const uint64_t *sx, const uint64_t *ta, const uint64_t *tb,
                                                        uint64_t *masked, int64_t count) {
    if (count < 0 || (count > 0 && (!c || !w || !sx || !ta || !tb || !masked))) return HB_ERR_BAD_ARG;
    if (count == 0) return HB_OK;
    const int64_t rb = run.elem_bytes() * count;
    const RowSpan outs[1] = {{masked, 4}}, ins[5] = {{c, 1}, {w, 1}, {sx, 1}, {ta, 2}, {tb, 2}};
    if (!outputs_apart(outs, 1, ins, 5, rb)) return run.fail(HB_ERR_BAD_ARG, "hb_fxatan_select_mask: masked is an array of its own");
    const FxAtanSelectMaskArgs A = {u32(c), u32(w), u32(sx), u32(ta), u32(tb), u32(masked)};
    return run.template rows<FxAtanSelectMaskRow>(A, 2, count);
}

template <class Run> static int fxatan_select_step(const Run &run, const uint64_t *opened, const uint64_t *ta, const uint64_t *tb, const uint64_t *tab, const uint64_t *ax,
                                                   const uint64_t *ay, uint64_t *out, int64_t count) {
    if (count < 0 || (count > 0 && (!opened || !ta || !tb || !tab || !ax || !ay || !out))) return HB_ERR_BAD_ARG;
    if (count == 0) return HB_OK;
    const int64_t rb = run.elem_bytes() * count;
    const RowSpan outs[1] = {{out, 3}}, ins[6] = {{opened, 4}, {ta, 2}, {tb, 2}, {tab, 2}, {ax, 1}, {ay, 1}};
    if (!outputs_apart(outs, 1, ins, 6, rb)) return run.fail(HB_ERR_BAD_ARG, "hb_fxatan_select: out is an array of its own");
    const FxAtanSelectArgs A = {u32(opened), u32(ta), u32(tb), u32(tab), u32(ax), u32(ay), u32(out)};
    return run.template rows<FxAtanSelectRow>(A, 1, count);
}

template <class Run> static int fxatan_first_step(const Run &run, const uint64_t *q, int shift, const uint64_t *sy, const uint64_t *e1, const uint64_t *ta, const uint64_t *tb,
                                                  uint64_t *masked, uint64_t *powers, int64_t count) {
    if (count < 0) return HB_ERR_BAD_ARG;
    if (shift < 0 || shift > 255) return run.fail(HB_ERR_BAD_ARG, "hb_fxatan_first: needs 0 <= shift <= 255");
    if (count > 0 && (!q || !sy || !e1 || !ta || !tb || !masked || !powers)) return HB_ERR_BAD_ARG;
    const int64_t rb = run.elem_bytes() * count;
    const RowSpan outs[2] = {{masked, 4}, {powers, 1}}, ins[5] = {{q, 1}, {sy, 1}, {e1, 1}, {ta, 2}, {tb, 2}};
    if (count > 0 && !outputs_apart(outs, 2, ins, 5, rb)) return run.fail(HB_ERR_BAD_ARG, "hb_fxatan_first: masked and powers are arrays of their own");
    return run.template rows<FxAtanFirstRow, FxAtanFirstArgs>([&](auto &A, const auto &P) {
        A.q = u32(q); A.sy = u32(sy); A.e1 = u32(e1); A.ta = u32(ta); A.tb = u32(tb); A.masked = u32(masked); A.powers = u32(powers);
        constexpr int NL = sizeof(A.scale.d) / sizeof(uint32_t);
        fxp_pow2<NL>(A.scale.d, shift, true, P);
        return true;
    }, 2, count);
}

template <class Run> static int fxatan_level_step(const Run &run, int level, int d, const uint64_t *opened, const uint64_t *s, int m, const uint64_t *inv2m_host,
                                                  const uint64_t *ta, const uint64_t *tb, uint64_t *masked, uint64_t *powers, int64_t count) {
    if (count < 0) return HB_ERR_BAD_ARG;
    if (!fxatan_degree_ok(d) || level < 0 || level >= fxatan_levels((d - 1) / 2) || !fxp_m_ok(run.bits(), m))
        return run.fail(HB_ERR_BAD_ARG, "hb_fxatan_level: needs 3 <= d <= 63 odd, 0 <= level < bit_length((d - 1) / 2) and 0 < m <= bits(p) - 2");
    if (!inv2m_host || (count > 0 && (!opened || !s || !ta || !tb || !masked || !powers))) return HB_ERR_BAD_ARG;
    const int J = (d - 1) / 2, done = fxatan_level_products(level, J), next = fxatan_level_products(level + 1, J);
    const int64_t rb = run.elem_bytes() * count;
    const RowSpan outs[2] = {{masked, 2 * next}, {powers, J + 1}}, ins[4] = {{opened, done}, {s, done}, {ta, next}, {tb, next}};
    if (count > 0 && !outputs_apart(outs, 2, ins, 4, rb)) return run.fail(HB_ERR_BAD_ARG, "hb_fxatan_level: masked and powers are arrays of their own");
    const int rc = run.template rows<FxAtanLevelRow, FxAtanLevelArgs>([&](auto &A, const auto &P) {
        A.opened = u32(opened); A.s = u32(s); A.ta = u32(ta); A.tb = u32(tb); A.masked = u32(masked); A.powers = u32(powers);
        A.level = level; A.J = J; A.m = m;
        constexpr int NL = sizeof(A.invm.d) / sizeof(uint32_t);
        return host_mont<NL, words_of(NL)>(A.invm.d, P, inv2m_host);
    }, done > next ? done : next, count);
    return rc == HB_ERR_BAD_ARG ? run.fail(rc, "hb_fxatan_level: a constant is not below the modulus") : rc;
}

template <class Run> static int fxatan_poly_mask_step(const Run &run, int d, const uint64_t *opened, const uint64_t *s, int m_in, const uint64_t *inv2m_host,
                                                      const uint64_t *powers, const uint64_t *coef, const uint64_t *bits, int width, int m_out, int kappa, uint64_t *masked,
                                                      uint64_t *s_out, int64_t count) {
    if (count < 0) return HB_ERR_BAD_ARG;
    if (!fxatan_degree_ok(d) || !fxp_m_ok(run.bits(), m_in) || !fxp_params_ok(run.bits(), width, m_out, kappa))
        return run.fail(HB_ERR_BAD_ARG, "hb_fxatan_poly_mask: needs 3 <= d <= 63 odd, 0 < m_in <= bits(p) - 2 and a truncation the modulus has room for");
    if (!inv2m_host || !coef || (count > 0 && (!opened || !s || !powers || !bits || !masked || !s_out))) return HB_ERR_BAD_ARG;
    const int J = (d - 1) / 2, last = fxatan_levels(J), half = 1 << (last - 1), done = fxatan_level_products(last, J);
    const int64_t rb = run.elem_bytes() * count, cb = run.elem_bytes() * (J + 1);
    const RowSpan outs[2] = {{masked, 1}, {s_out, 1}}, ins[4] = {{opened, done}, {s, done}, {powers, half}, {bits, width + kappa}};
    if (count > 0 && (!outputs_apart(outs, 2, ins, 4, rb) || overlap(coef, cb, masked, rb) || overlap(coef, cb, s_out, rb)))
        return run.fail(HB_ERR_BAD_ARG, "hb_fxatan_poly_mask: masked and s_out are arrays of their own");
    const int rc = run.template rows<FxAtanPolyMaskRow, FxAtanPolyArgs>([&](auto &A, const auto &P) {
        A.opened = u32(opened); A.s = u32(s); A.powers = u32(powers); A.coef = u32(coef); A.bits = u32(bits);
        A.masked = u32(masked); A.s_out = u32(s_out);
        A.J = J; A.half = half; A.m_in = m_in; A.nbits = width + kappa; A.m_out = m_out;
        constexpr int NL = sizeof(A.invm.d) / sizeof(uint32_t);
        fxp_pow2<NL>(A.halfw.d, width - 1, false, P);
        return host_mont<NL, words_of(NL)>(A.invm.d, P, inv2m_host);
    }, 1, count);
    return rc == HB_ERR_BAD_ARG ? run.fail(rc, "hb_fxatan_poly_mask: a constant is not below the modulus") : rc;
}

template <class Run> static int fxatan_assemble_step(const Run &run, const uint64_t *opened, const uint64_t *s, int m, const uint64_t *inv2m_host, const uint64_t *eopened,
                                                     const uint64_t *ea, const uint64_t *eb, const uint64_t *eab, const uint64_t *sy, const uint64_t *g,
                                                     const uint64_t *cst_host, const uint64_t *ta, const uint64_t *tb, uint64_t *masked, uint64_t *c, int64_t count) {
    if (count < 0) return HB_ERR_BAD_ARG;
    if (!fxp_m_ok(run.bits(), m)) return run.fail(HB_ERR_BAD_ARG, "hb_fxatan_assemble: needs 0 < m <= bits(p) - 2");
    if (!inv2m_host || !cst_host || (count > 0 && (!opened || !s || !eopened || !ea || !eb || !eab || !sy || !g || !ta || !tb || !masked || !c))) return HB_ERR_BAD_ARG;
    const int64_t rb = run.elem_bytes() * count;
    const RowSpan outs[2] = {{masked, 2}, {c, 1}}, ins[10] = {{opened, 1}, {s, 1}, {eopened, 2}, {ea, 1}, {eb, 1}, {eab, 1}, {sy, 1}, {g, 1}, {ta, 1}, {tb, 1}};
    if (count > 0 && !outputs_apart(outs, 2, ins, 10, rb)) return run.fail(HB_ERR_BAD_ARG, "hb_fxatan_assemble: masked and c are arrays of their own");
    const int limbs = run.limbs();
    const int rc = run.template rows<FxAtanAssembleRow, FxAtanAssembleArgs>([&](auto &A, const auto &P) {
        A.opened = u32(opened); A.s = u32(s); A.eopened = u32(eopened); A.ea = u32(ea); A.eb = u32(eb); A.eab = u32(eab); A.sy = u32(sy); A.g = u32(g);
        A.ta = u32(ta); A.tb = u32(tb); A.masked = u32(masked); A.c = u32(c); A.m = m;
        constexpr int NL = sizeof(A.invm.d) / sizeof(uint32_t);
        return host_mont<NL, words_of(NL)>(A.invm.d, P, inv2m_host) && host_mont<NL, words_of(NL)>(A.ca.d, P, cst_host) &&
               host_mont<NL, words_of(NL)>(A.cb.d, P, cst_host + limbs);
    }, 1, count);
    return rc == HB_ERR_BAD_ARG ? run.fail(rc, "hb_fxatan_assemble: a constant is not below the modulus") : rc;
}

template <class Run> static int fxatan_finish_step(const Run &run, const uint64_t *opened, const uint64_t *ta, const uint64_t *tb, const uint64_t *tab, const uint64_t *c,
                                                   uint64_t *out, int64_t count) {
    if (count < 0 || (count > 0 && (!opened || !ta || !tb || !tab || !c || !out))) return HB_ERR_BAD_ARG;
    if (count == 0) return HB_OK;
    const int64_t rb = run.elem_bytes() * count;
    const RowSpan outs[1] = {{out, 1}}, ins[5] = {{opened, 2}, {ta, 1}, {tb, 1}, {tab, 1}, {c, 1}};
    if (!outputs_apart(outs, 1, ins, 5, rb)) return run.fail(HB_ERR_BAD_ARG, "hb_fxatan_finish: out is an array of its own");
    const FxAtanFinishArgs A = {u32(opened), u32(ta), u32(tb), u32(tab), u32(c), u32(out)};
    return run.template rows<FxAtanFinishRow>(A, 1, count);
}

}  // namespace hb

extern "C" {

int hb_fxatan_sign_mask(hb_ctx *ctx, const uint64_t *s_dev, const uint64_t *x_dev, const uint64_t *y_dev, const uint64_t *ta_dev, const uint64_t *tb_dev,
                        uint64_t *masked_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : fxatan_sign_mask_step(DeviceRun{ctx, (hipStream_t)stream, "hb_fxatan_sign_mask"}, s_dev, x_dev, y_dev, ta_dev, tb_dev, masked_dev, count);
}

int hb_fxatan_abs(hb_ctx *ctx, const uint64_t *opened_dev, const uint64_t *ta_dev, const uint64_t *tb_dev, const uint64_t *tab_dev, const uint64_t *x_dev,
                  const uint64_t *y_dev, const uint64_t *bits_dev, int k, int kappa, uint64_t *masked_dev, uint64_t *kept_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : fxatan_abs_step(DeviceRun{ctx, (hipStream_t)stream, "hb_fxatan_abs"}, opened_dev, ta_dev, tb_dev, tab_dev, x_dev, y_dev, bits_dev, k, kappa,
                                                   masked_dev, kept_dev, count);
}

int hb_fxatan_select_mask(hb_ctx *ctx, const uint64_t *c_dev, const uint64_t *w_dev, const uint64_t *sx_dev, const uint64_t *ta_dev, const uint64_t *tb_dev,
                          uint64_t *masked_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : fxatan_select_mask_step(DeviceRun{ctx, (hipStream_t)stream, "hb_fxatan_select_mask"}, c_dev, w_dev, sx_dev, ta_dev, tb_dev, masked_dev, count);
}

int hb_fxatan_select(hb_ctx *ctx, const uint64_t *opened_dev, const uint64_t *ta_dev, const uint64_t *tb_dev, const uint64_t *tab_dev, const uint64_t *ax_dev,
                     const uint64_t *ay_dev, uint64_t *out_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : fxatan_select_step(DeviceRun{ctx, (hipStream_t)stream, "hb_fxatan_select"}, opened_dev, ta_dev, tb_dev, tab_dev, ax_dev, ay_dev, out_dev, count);
}

int hb_fxatan_first(hb_ctx *ctx, const uint64_t *q_dev, int shift, const uint64_t *sy_dev, const uint64_t *e1_dev, const uint64_t *ta_dev, const uint64_t *tb_dev,
                    uint64_t *masked_dev, uint64_t *powers_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : fxatan_first_step(DeviceRun{ctx, (hipStream_t)stream, "hb_fxatan_first"}, q_dev, shift, sy_dev, e1_dev, ta_dev, tb_dev, masked_dev, powers_dev,
                                                     count);
}

int hb_fxatan_level(hb_ctx *ctx, int level, int d, const uint64_t *opened_dev, const uint64_t *s_dev, int m, const uint64_t *inv2m_host, const uint64_t *ta_dev,
                    const uint64_t *tb_dev, uint64_t *masked_dev, uint64_t *powers_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : fxatan_level_step(DeviceRun{ctx, (hipStream_t)stream, "hb_fxatan_level"}, level, d, opened_dev, s_dev, m, inv2m_host, ta_dev, tb_dev,
                                                     masked_dev, powers_dev, count);
}

int hb_fxatan_poly_mask(hb_ctx *ctx, int d, const uint64_t *opened_dev, const uint64_t *s_dev, int m_in, const uint64_t *inv2m_host, const uint64_t *powers_dev,
                        const uint64_t *coef_dev, const uint64_t *bits_dev, int width, int m_out, int kappa, uint64_t *masked_dev, uint64_t *s_out_dev, int64_t count,
                        void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : fxatan_poly_mask_step(DeviceRun{ctx, (hipStream_t)stream, "hb_fxatan_poly_mask"}, d, opened_dev, s_dev, m_in, inv2m_host, powers_dev, coef_dev,
                                                         bits_dev, width, m_out, kappa, masked_dev, s_out_dev, count);
}

int hb_fxatan_assemble(hb_ctx *ctx, const uint64_t *opened_dev, const uint64_t *s_dev, int m, const uint64_t *inv2m_host, const uint64_t *eopened_dev,
                       const uint64_t *ea_dev, const uint64_t *eb_dev, const uint64_t *eab_dev, const uint64_t *sy_dev, const uint64_t *g_dev, const uint64_t *cst_host,
                       const uint64_t *ta_dev, const uint64_t *tb_dev, uint64_t *masked_dev, uint64_t *c_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : fxatan_assemble_step(DeviceRun{ctx, (hipStream_t)stream, "hb_fxatan_assemble"}, opened_dev, s_dev, m, inv2m_host, eopened_dev, ea_dev, eb_dev,
                                                        eab_dev, sy_dev, g_dev, cst_host, ta_dev, tb_dev, masked_dev, c_dev, count);
}

int hb_fxatan_finish(hb_ctx *ctx, const uint64_t *opened_dev, const uint64_t *ta_dev, const uint64_t *tb_dev, const uint64_t *tab_dev, const uint64_t *c_dev,
                     uint64_t *out_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : fxatan_finish_step(DeviceRun{ctx, (hipStream_t)stream, "hb_fxatan_finish"}, opened_dev, ta_dev, tb_dev, tab_dev, c_dev, out_dev, count);
}

// params: as the header lists them for each step
int hb_selftest_fxatan(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *ops, const int64_t *params, uint64_t *const *outs, int64_t count) {
    if (!p_limbs || !ops || !params || !outs || (n_limbs != 1 && n_limbs != 4)) return HB_ERR_BAD_ARG;
    for (int i = 0; i < 5; i++) if (params[i] < -(1 << 30) || params[i] > (1 << 30)) return HB_ERR_BAD_ARG;
    const HostRun run = {p_limbs, n_limbs};
    const int a = (int)params[0], b = (int)params[1], c = (int)params[2], d = (int)params[3], e = (int)params[4];
    switch (what) {
    case HB_FXATAN_SELFTEST_SIGN_MASK: return fxatan_sign_mask_step(run, ops[0], ops[1], ops[2], ops[3], ops[4], outs[0], count);
    case HB_FXATAN_SELFTEST_ABS:                                                 // k, kappa
        return fxatan_abs_step(run, ops[0], ops[1], ops[2], ops[3], ops[4], ops[5], ops[6], a, b, outs[0], outs[1], count);
    case HB_FXATAN_SELFTEST_SELECT_MASK: return fxatan_select_mask_step(run, ops[0], ops[1], ops[2], ops[3], ops[4], outs[0], count);
    case HB_FXATAN_SELFTEST_SELECT: return fxatan_select_step(run, ops[0], ops[1], ops[2], ops[3], ops[4], ops[5], outs[0], count);
    case HB_FXATAN_SELFTEST_FIRST:                                               // shift
        return fxatan_first_step(run, ops[0], a, ops[1], ops[2], ops[3], ops[4], outs[0], outs[1], count);
    case HB_FXATAN_SELFTEST_LEVEL:                                               // level, d, m
        return fxatan_level_step(run, a, b, ops[0], ops[1], c, ops[2], ops[3], ops[4], outs[0], outs[1], count);
    case HB_FXATAN_SELFTEST_POLY_MASK:                                           // d, m_in, width, m_out, kappa
        return fxatan_poly_mask_step(run, a, ops[0], ops[1], b, ops[2], ops[3], ops[4], ops[5], c, d, e, outs[0], outs[1], count);
    case HB_FXATAN_SELFTEST_ASSEMBLE:                                            // m
        return fxatan_assemble_step(run, ops[0], ops[1], a, ops[2], ops[3], ops[4], ops[5], ops[6], ops[7], ops[8], ops[9], ops[10], ops[11], outs[0], outs[1], count);
    case HB_FXATAN_SELFTEST_FINISH: return fxatan_finish_step(run, ops[0], ops[1], ops[2], ops[3], ops[4], outs[0], count);
    default: return HB_ERR_BAD_ARG;
    }
}

}  // extern "C"

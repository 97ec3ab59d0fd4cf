// hb_fxsqrt.hip -- square root and inverse square root of shared fixed-point numbers (unsigned k-bit values with f fractional bits),
// for arrays of values: the steps that hb_div.hip does not already have.  (hb_sqrt.hip is the FIELD square root of the G1
// decompression; this file is the real-number one.  The reference has no square root: nothing here is a translation.)  Everything
// between two opens is ONE launch.  With N = k - 1, beta = 2^N, y the prefix OR from the top of the bits of x:
//
// FxSqrtNormMaskRow   v = sum_i 2^(N-1-i) (y_i - y_{i+1}) by hb_div.hip's Horner, and T = sum_i W_i (y_i - y_{i+1}) = sum_i D_i y_i with
//                      the PUBLIC D_i = W_i - W_{i-1} (one or two sets of weights: the root's, the inverse root's), in the one walk over
//                      the planes: each is read once.  D_i is the same for every element, so a plane costs one product by a
//                      wave-uniform constant a set (81 v_mad_u64_u32 with an SGPR operand), accumulated in 64-bit columns with ONE
//                      reduction every 7 planes (fp29.hpp's Lazy) and one product by R^2 at the end.  The alternative -- the even and the
//                      odd exponents as two doubling chains and one constant product -- costs two additions and two conditional
//                      subtractions a plane a chain, about 4 x 27 instructions against 81 + 300 / 7, and cannot give W_i =
//                      floor(2^(e_i / 2)) at every odd e_i, only floor(sqrt(2) 2^q) 2^(e_i / 2 - q - 1/2): so the products it is.
//                      Writes kept = (v, T[, T']) and the masked pair of [x v] as one array to open.
// FxSqrtFirstRow      after the scale's open: c = [x v] by the Beaver combine, y0 = A - B c (A, B constants: the linear first
//                      approximation of c^(-1/2), scaled), the masked pair of [c y0] as one array to open, and h = y0 kept.
// FxSqrtTruncRow      after an open of masked truncations: t = (s - (c mod 2^m)) 2^(-m) for one or two values, and what the next open needs.
//                      blockIdx.y = the product the thread masks.
//                        HB_FXSQRT_GH   g = t_0, h = t_1 (two rows) or the h kept by FxSqrtFirstRow (one row): kept = (g, h), and the
//                                       masked pair of [g h]
//                        HB_FXSQRT_R    r = cst - t_0 (cst = 3 beta); (g - a0, r - b0) and / or (h - a1, r - b1): the pairs of [g r], [h r],
//                                       `which` says which (bit 0: g, bit 1: h)
//                        HB_FXSQRT_OUT  (t_q - a_q, w_q - b_q) for one or two values: the pairs of [g T], [h T'], w the kept weights
// "Products to truncation mask" between them is hb_div_product_step(HB_DIV_TRUNC) and the last step hb_div_trunc_step(HB_DIV_T_RESULT),
// as they stand; the per-element bodies both files call are in hb_div_elem.hpp.
//
// Operands and results are packed canonical residues.  A step's row is an HB_HD function over a memory policy (hb_rows.hpp): k_rows runs
// it on the device, host_rows the very same row in hb_selftest_fxsqrt, and each step is ONE step function behind both.
//
// Launch shape (all kernels): 256-thread workgroups, one element a thread in x, the product in blockIdx.y (FxSqrtNormMaskRow walks
// the planes in the thread, FxSqrtFirstRow has one row).  No LDS, no grid stride, one launch a call.  Planes, triples, opened and kept
// values are read once and take the non-temporal loads (load_once); x takes the plain one; the weights are one address a wave (same).
// Compiler's report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; scratch = 0 bytes for every kernel):
//   FxSqrtNormMaskRow<9, 8>   131 VGPRs: 3 waves a SIMD                           FxSqrtNormMaskRow<3, 2>   46 VGPRs: 8 waves
//   FxSqrtFirstRow<9, 8>      74 VGPRs: 6 waves                                   FxSqrtFirstRow<3, 2>      29 VGPRs: 8 waves
//   FxSqrtTruncRow<9, 8>      72 VGPRs: 7 waves                                   FxSqrtTruncRow<3, 2>      22 VGPRs: 8 waves
// (FxSqrtNormMaskRow holds two sets of 18 64-bit columns, 72 registers, beside the Horner value and a plane's digits.)
// (DESIGN.md section 3ab has the schedule, the error and width derivations and the counts.)
#include "hb_common.hpp"
#include "hb_div_elem.hpp"

using namespace hb;

namespace hb {

// ---------------------------------------------------------------- per-element bodies (host and device)
// One walk over the n planes: v = 2^(n-1) y_0 - sum_{i>=1} 2^(n-1-i) y_i (div_scale_elem's Horner) and t_s = sum_i D_{s,i} y_i for
// sets = 1 or 2 sets of weights.  plane(w, i) loads this element's word of plane i, weight(w, s, i) the canonical D_{s,i}.  A column
// takes GROUP products before carries must move; the reduced group sums are below 2 p (GROUP p^2 / R < p), one conditional
// subtraction each; the sum of them is sum D y / R, and the product by R^2 at the end makes it sum D y.
template <int NL, int NW, class Load, class Weight>
HB_HD void fxsqrt_scale_elem(uint32_t (&vw)[NW], uint32_t (&t0w)[NW], uint32_t (&t1w)[NW], Load &&plane, Weight &&weight, int n, int sets, const FpParams<NL> &P) {
    constexpr int GROUP = Lazy<NL>::GROUP;
    uint32_t acc[NL], y[NL], t[NL], d[NL], s0[NL], s1[NL], w[NW];
    uint64_t c0[2 * NL], c1[2 * NL];
#pragma unroll
    for (int q = 0; q < NL; q++) { acc[q] = 0u; s0[q] = 0u; s1[q] = 0u; }
    for (int base = 0; base < n; base += GROUP) {
        col_zero(c0);
        col_zero(c1);
        const int end = base + GROUP < n ? base + GROUP : n;
        for (int i = base; i < end; i++) {
            plane(w, i);
            unpack<NL, NW>(y, w);
            fp_add<NL>(t, acc, acc, P);
            if (i == 0) fp_set<NL>(acc, y); else fp_sub<NL>(acc, t, y, P);
            weight(w, 0, i);
            unpack<NL, NW>(d, w);
            mac<NL>(c0, d, y);
            if (sets == 2) {
                weight(w, 1, i);
                unpack<NL, NW>(d, w);
                mac<NL>(c1, d, y);
            }
        }
        finish<NL>(d, c0, P, 1);
        fp_add<NL>(t, s0, d, P);
        fp_set<NL>(s0, t);
        if (sets == 2) {
            finish<NL>(d, c1, P, 1);
            fp_add<NL>(t, s1, d, P);
            fp_set<NL>(s1, t);
        }
    }
    pack<NL, NW>(vw, acc);
    mont_mul<NL>(t, P.r2, s0, P);
    pack<NL, NW>(t0w, t);
    if (sets == 2) mont_mul<NL>(t, P.r2, s1, P);
    pack<NL, NW>(t1w, t);
}

// y0 = a - b c; bm = b R mod p
template <int NL, int NW>
HB_HD void fxsqrt_first_elem(uint32_t (&o)[NW], const uint32_t (&cw)[NW], const uint32_t (&a)[NL], const uint32_t (&bm)[NL], const FpParams<NL> &P) {
    uint32_t c[NL], t[NL], r[NL];
    unpack<NL, NW>(c, cw);
    mont_mul<NL>(t, bm, c, P);
    fp_sub<NL>(r, a, t, P);
    pack<NL, NW>(o, r);
}

// ---------------------------------------------------------------- the steps' rows (host and device, over a memory policy)
struct FxSqrtNormArgs { const uint32_t *x, *y, *wts, *ta, *tb; uint32_t *masked, *kept; int n, sets; };

struct FxSqrtNormMaskRow {
template <int NL, int NW, class Mem>
HB_HD static void run(const FxSqrtNormArgs &A, int, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
    uint32_t vw[NW], t0[NW], t1[NW], w[NW], aw[NW], o[NW];
    fxsqrt_scale_elem<NL, NW>(vw, t0, t1, [&](uint32_t (&pw)[NW], int row) { mem.once(pw, A.y, (int64_t)row * count + i); },
                              [&](uint32_t (&ww)[NW], int set, int row) { mem.same(ww, A.wts + ((int64_t)set * A.n + row) * NW); }, A.n, A.sets, P);
    mem.store(A.kept, i, vw);
    mem.store(A.kept, count + i, t0);
    if (A.sets == 2) mem.store(A.kept, 2 * count + i, t1);
    mem.load(w, A.x, i); mem.once(aw, A.ta, i);
    diff_elem<NL, NW>(o, w, aw, P);
    mem.store(A.masked, i, o);
    mem.once(aw, A.tb, i);
    diff_elem<NL, NW>(o, vw, aw, P);
    mem.store(A.masked, count + i, o);
}
};

template <int NL> struct FxSqrtFirstArgs {
    const uint32_t *opened, *ta, *tb, *tab, *nxt_a, *nxt_b;
    uint32_t *masked, *h;
    FpConst<NL> a, bm;
};

struct FxSqrtFirstRow {
template <int NL, int NW, class Mem>
HB_HD static void run(const FxSqrtFirstArgs<NL> &A, int, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
    uint32_t dw[NW], ew[NW], aw[NW], bw[NW], abw[NW], cw[NW], yw[NW], o[NW];
    mem.once(dw, A.opened, i); mem.once(ew, A.opened, count + i);
    mem.once(aw, A.ta, i); mem.once(bw, A.tb, i); mem.once(abw, A.tab, i);
    ew_beaver_elem<NL, NW>(cw, dw, ew, aw, bw, abw, P);
    fxsqrt_first_elem<NL, NW>(yw, cw, A.a.d, A.bm.d, P);
    mem.store(A.h, i, yw);
    mem.once(aw, A.nxt_a, i);
    diff_elem<NL, NW>(o, cw, aw, P);
    mem.store(A.masked, i, o);
    mem.once(aw, A.nxt_b, i);
    diff_elem<NL, NW>(o, yw, aw, P);
    mem.store(A.masked, count + i, o);
}
};

template <int NL> struct FxSqrtTruncArgs {
    const uint32_t *opened, *s, *kept_in, *ta, *tb;
    uint32_t *masked, *kept_out;
    int mode, rows, which, m;
    FpConst<NL> invm, cst;
};

struct FxSqrtTruncRow {
template <int NL, int NW, class Mem>
HB_HD static void run(const FxSqrtTruncArgs<NL> &A, int q, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
    uint32_t sw[NW], cw[NW], first[NW], second[NW], aw[NW], o[NW];
    if (A.mode == HB_FXSQRT_GH) {
        mem.once(sw, A.s, i); mem.once(cw, A.opened, i);
        div_trunc_elem<NL, NW>(first, sw, cw, A.m, A.invm.d, P);
        if (A.rows == 2) {
            mem.once(sw, A.s, count + i); mem.once(cw, A.opened, count + i);
            div_trunc_elem<NL, NW>(second, sw, cw, A.m, A.invm.d, P);
        } else {
            mem.once(second, A.kept_in, i);
        }
        mem.store(A.kept_out, i, first);
        mem.store(A.kept_out, count + i, second);
    } else if (A.mode == HB_FXSQRT_R) {
        uint32_t t0[NW], zero[NW];
#pragma unroll
        for (int w = 0; w < NW; w++) zero[w] = 0u;
        mem.once(sw, A.s, i); mem.once(cw, A.opened, i);
        div_trunc_elem<NL, NW>(t0, sw, cw, A.m, A.invm.d, P);
        div_affine_elem<NL, NW>(second, t0, -1, A.cst.d, zero, P);
        const int from = (A.which & 1) && q == 0 ? 0 : 1;                      // g for the first product where g is asked for, else h
        mem.once(first, A.kept_in, (int64_t)from * count + i);
    } else {
        mem.once(sw, A.s, (int64_t)q * count + i); mem.once(cw, A.opened, (int64_t)q * count + i);
        div_trunc_elem<NL, NW>(first, sw, cw, A.m, A.invm.d, P);
        mem.once(second, A.kept_in, (int64_t)q * count + i);
    }
    mem.once(aw, A.ta, (int64_t)q * count + i);
    diff_elem<NL, NW>(o, first, aw, P);
    mem.store(A.masked, (int64_t)(2 * q) * count + i, o);
    mem.once(aw, A.tb, (int64_t)q * count + i);
    diff_elem<NL, NW>(o, second, aw, P);
    mem.store(A.masked, (int64_t)(2 * q + 1) * count + i, o);
}
};

// ---------------------------------------------------------------- host side
// One step function a step (hb_rows.hpp): a DeviceRun in the entry point, a HostRun in hb_selftest_fxsqrt.
static int fxsqrt_products(int mode, int rows, int which) { return mode == HB_FXSQRT_GH ? 1 : (mode == HB_FXSQRT_R ? (which == 3 ? 2 : 1) : rows); }
static int fxsqrt_kept_in_rows(int mode, int rows) { return mode == HB_FXSQRT_GH ? (rows == 1 ? 1 : 0) : (mode == HB_FXSQRT_R ? 2 : rows); }
static bool fxsqrt_trunc_ok(int bits, int mode, int rows, int which, int m) {
    if (!fxp_m_ok(bits, m)) return false;
    switch (mode) {
    case HB_FXSQRT_GH: return (rows == 1 || rows == 2) && which == 3;
    case HB_FXSQRT_R: return rows == 1 && which >= 1 && which <= 3;
    case HB_FXSQRT_OUT: return (rows == 1 || rows == 2) && which >= 1 && which <= 3 && rows == (which == 3 ? 2 : 1);
    default: return false;
    }
}

template <class Run> static int fxsqrt_norm_mask_step(const Run &run, const uint64_t *x, const uint64_t *y, int n_planes, const uint64_t *wts, int sets,
                                                      const uint64_t *ta, const uint64_t *tb, uint64_t *masked, uint64_t *kept, int64_t count) {
    if (count < 0 || !wts || (count > 0 && (!x || !y || !ta || !tb || !masked || !kept))) return HB_ERR_BAD_ARG;
    if (n_planes < 1 || n_planes > 256 || sets < 1 || sets > 2) return run.fail(HB_ERR_BAD_ARG, "hb_fxsqrt_norm_mask: needs 1 <= n_planes <= 256 and one or two sets of weights");
    if (count == 0) return HB_OK;
    const int64_t rb = run.elem_bytes() * count;
    const RowSpan outs[2] = {{masked, 2}, {kept, 1 + sets}}, ins[4] = {{x, 1}, {y, n_planes}, {ta, 1}, {tb, 1}};
    if (!outputs_apart(outs, 2, ins, 4, rb) || overlap(wts, run.elem_bytes() * sets * n_planes, masked, 2 * rb) ||
        overlap(wts, run.elem_bytes() * sets * n_planes, kept, (1 + sets) * rb))
        return run.fail(HB_ERR_BAD_ARG, "hb_fxsqrt_norm_mask: masked and kept are arrays of their own");
    const FxSqrtNormArgs A = {u32(x), u32(y), u32(wts), u32(ta), u32(tb), u32(masked), u32(kept), n_planes, sets};
    return run.template rows<FxSqrtNormMaskRow>(A, 1, count);
}

template <class Run> static int fxsqrt_first_step(const Run &run, const uint64_t *opened, const uint64_t *ta, const uint64_t *tb, const uint64_t *tab,
                                                  const uint64_t *a_host, const uint64_t *b_host, const uint64_t *nxt_a, const uint64_t *nxt_b, uint64_t *masked,
                                                  uint64_t *h, int64_t count) {
    if (count < 0 || !a_host || !b_host || (count > 0 && (!opened || !ta || !tb || !tab || !nxt_a || !nxt_b || !masked || !h))) return HB_ERR_BAD_ARG;
    const int64_t rb = run.elem_bytes() * count;
    const RowSpan outs[2] = {{masked, 2}, {h, 1}}, ins[6] = {{opened, 2}, {ta, 1}, {tb, 1}, {tab, 1}, {nxt_a, 1}, {nxt_b, 1}};
    if (count > 0 && !outputs_apart(outs, 2, ins, 6, rb)) return run.fail(HB_ERR_BAD_ARG, "hb_fxsqrt_first: masked and h are arrays of their own");
    const int rc = run.template rows<FxSqrtFirstRow, FxSqrtFirstArgs>([&](auto &A, const auto &P) {
        A.opened = u32(opened); A.ta = u32(ta); A.tb = u32(tb); A.tab = u32(tab); A.nxt_a = u32(nxt_a); A.nxt_b = u32(nxt_b);
        A.masked = u32(masked); A.h = u32(h);
        constexpr int NL = sizeof(A.a.d) / sizeof(uint32_t);
        return host_digits<NL, words_of(NL)>(A.a.d, P, a_host) && host_mont<NL, words_of(NL)>(A.bm.d, P, b_host);
    }, 1, count);
    return rc == HB_ERR_BAD_ARG ? run.fail(rc, "hb_fxsqrt_first: a constant is not below the modulus") : rc;
}

template <class Run> static int fxsqrt_trunc_step(const Run &run, int mode, int rows, int which, const uint64_t *opened, const uint64_t *s, int m,
                                                  const uint64_t *inv2m_host, const uint64_t *cst_host, const uint64_t *kept_in, const uint64_t *ta, const uint64_t *tb,
                                                  uint64_t *masked, uint64_t *kept_out, int64_t count) {
    if (count < 0) return HB_ERR_BAD_ARG;
    if (!fxsqrt_trunc_ok(run.bits(), mode, rows, which, m))
        return run.fail(HB_ERR_BAD_ARG, "hb_fxsqrt_trunc_step: unknown mode, a row count or `which` the mode does not take, or m outside 0 < m <= bits(p) - 2");
    const int products = fxsqrt_products(mode, rows, which), kin = fxsqrt_kept_in_rows(mode, rows), kout = mode == HB_FXSQRT_GH ? 2 : 0;
    if (!inv2m_host || (mode == HB_FXSQRT_R && !cst_host)) return HB_ERR_BAD_ARG;
    if (count > 0 && (!opened || !s || !ta || !tb || !masked || (kin && !kept_in) || (kout && !kept_out))) return HB_ERR_BAD_ARG;
    const int64_t rb = run.elem_bytes() * count;
    const RowSpan outs[2] = {{masked, 2 * products}, {kout ? kept_out : nullptr, kout}};
    const RowSpan ins[5] = {{opened, rows}, {s, rows}, {kin ? kept_in : nullptr, kin}, {ta, products}, {tb, products}};
    if (count > 0 && !outputs_apart(outs, 2, ins, 5, rb)) return run.fail(HB_ERR_BAD_ARG, "hb_fxsqrt_trunc_step: the outputs are arrays of their own");
    const int rc = run.template rows<FxSqrtTruncRow, FxSqrtTruncArgs>([&](auto &A, const auto &P) {
        A.opened = u32(opened); A.s = u32(s); A.kept_in = kin ? u32(kept_in) : nullptr; A.ta = u32(ta); A.tb = u32(tb);
        A.masked = u32(masked); A.kept_out = kout ? u32(kept_out) : nullptr;
        A.mode = mode; A.rows = rows; A.which = which; A.m = m;
        constexpr int NL = sizeof(A.cst.d) / sizeof(uint32_t);
        for (int q = 0; q < NL; q++) A.cst.d[q] = 0;
        if (!host_mont<NL, words_of(NL)>(A.invm.d, P, inv2m_host)) return false;
        return mode == HB_FXSQRT_R ? host_digits<NL, words_of(NL)>(A.cst.d, P, cst_host) : true;
    }, products, count);
    return rc == HB_ERR_BAD_ARG ? run.fail(rc, "hb_fxsqrt_trunc_step: a constant is not below the modulus") : rc;
}

}  // namespace hb

extern "C" {

int hb_fxsqrt_norm_mask(hb_ctx *ctx, const uint64_t *x_dev, const uint64_t *y_dev, int n_planes, const uint64_t *weights_dev, int sets, const uint64_t *ta_dev,
                        const uint64_t *tb_dev, uint64_t *masked_dev, uint64_t *kept_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : fxsqrt_norm_mask_step(DeviceRun{ctx, (hipStream_t)stream, "hb_fxsqrt_norm_mask"}, x_dev, y_dev, n_planes, weights_dev, sets, ta_dev,
                                                         tb_dev, masked_dev, kept_dev, count);
}

int hb_fxsqrt_first(hb_ctx *ctx, const uint64_t *opened_dev, const uint64_t *ta_dev, const uint64_t *tb_dev, const uint64_t *tab_dev, const uint64_t *a_host,
                    const uint64_t *b_host, const uint64_t *nxt_a_dev, const uint64_t *nxt_b_dev, uint64_t *masked_dev, uint64_t *h_dev, int64_t count, void *stream) {
    HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : fxsqrt_first_step(DeviceRun{ctx, (hipStream_t)stream, "hb_fxsqrt_first"}, opened_dev, ta_dev, tb_dev, tab_dev, a_host, b_host, nxt_a_dev,
                                                     nxt_b_dev, masked_dev, h_dev, count);
}

int hb_fxsqrt_trunc_step(hb_ctx *ctx, int mode, int rows, int which, const uint64_t *opened_dev, const uint64_t *s_dev, int m, const uint64_t *inv2m_host,
                         const uint64_t *cst_host, const uint64_t *kept_in_dev, const uint64_t *ta_dev, const uint64_t *tb_dev, uint64_t *masked_dev,
                         uint64_t *kept_out_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : fxsqrt_trunc_step(DeviceRun{ctx, (hipStream_t)stream, "hb_fxsqrt_trunc_step"}, mode, rows, which, opened_dev, s_dev, m, inv2m_host,
                                                     cst_host, kept_in_dev, ta_dev, tb_dev, masked_dev, kept_out_dev, count);
}

// params: as the header lists them for each step
int hb_selftest_fxsqrt(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *ops, const int64_t *params, uint64_t *const *outs, int64_t count) {
    if (!p_limbs || !ops || !params || !outs || (n_limbs != 1 && n_limbs != 4)) return HB_ERR_BAD_ARG;
    for (int i = 0; i < 4; i++) if (params[i] < -(1 << 30) || params[i] > (1 << 30)) return HB_ERR_BAD_ARG;
    const HostRun run = {p_limbs, n_limbs};
    const int a = (int)params[0], b = (int)params[1], c = (int)params[2], d = (int)params[3];
    switch (what) {
    case HB_FXSQRT_SELFTEST_NORM_MASK:                                          // n_planes, sets
        return fxsqrt_norm_mask_step(run, ops[0], ops[1], a, ops[2], b, ops[3], ops[4], outs[0], outs[1], count);
    case HB_FXSQRT_SELFTEST_FIRST: return fxsqrt_first_step(run, ops[0], ops[1], ops[2], ops[3], ops[4], ops[5], ops[6], ops[7], outs[0], outs[1], count);
    case HB_FXSQRT_SELFTEST_TRUNC_STEP:                                         // mode, rows, which, m
        return fxsqrt_trunc_step(run, a, b, c, ops[0], ops[1], d, ops[2], ops[3], ops[4], ops[5], ops[6], outs[0], outs[1], count);
    default: return HB_ERR_BAD_ARG;
    }
}

}  // extern "C"

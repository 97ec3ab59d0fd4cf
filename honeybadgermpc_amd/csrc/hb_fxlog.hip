// hb_fxlog.hip -- base-2, natural and any-public-base logarithm of shared fixed-point numbers (unsigned k-bit values with f fractional
// bits), for arrays of values: the steps that hb_div.hip, hb_fxsqrt.hip and hb_fxexp.hip do not already have.  (The reference has no
// logarithm: nothing here is a translation.)  Everything between two opens is ONE launch.  With N = k - 1, beta = 2^N, c = [x v] the
// mantissa in [beta / 2, beta), Y = beta [x != 0] and t = 4 c - 3 Y in [-beta, beta), the logarithm of the mantissa is a polynomial of
// degree d in t / beta, and the steps evaluate it: the powers t^2 .. t^d by doubling, each at scale beta, then a linear combination.
// Level l = 1, 2, .. forms t^j, 2^(l-1) < j <= min(2^l, d), as [t^(2^(l-1)) t^(j - 2^(l-1))] truncated by N bits; product q of a level
// has the operands t^(half) and t^(q+1), half = 2^(l-1): a closed form, so no index list travels.
//
// FxLogFirstRow       after the scale's open: c = [x v] by the Beaver combine, t = 4 c - 3 Y; t is row 0 of `powers` ([d][count]) and
//                      the masked pair of [t t] is the array to open.
// FxLogLevelRow       after the open of level l's masked truncations: t^(half + 1 + q) = (s_q - (opened_q mod 2^m)) 2^(-m), stored as row
//                      half + q of `powers`, and the masked pairs of level l + 1: (t^(2 half) - ta_q, t^(q+1) - tb_q).  blockIdx.y = q, over
//                      max(level l's truncations, level l + 1's products).  t^(2 half) and, for q >= half, t^(q+1) are powers this very
//                      launch finishes: the thread recomputes them from (s, opened) -- a truncation is one subtraction and one product --
//                      and waits for nobody; the older powers are read from `powers`, rows below half, which this launch does not write.
// FxLogPolyMaskRow    after the open of the LAST level's masked truncations: finishes them, L = A_0 Y + sum_{j=1..d} A_j t^j in one walk
//                      (A_j PUBLIC, the same for every element: one product by a wave-uniform constant a term, accumulated in 64-bit
//                      columns with one reduction every 7 terms -- fp29.hpp's Lazy, as FxSqrtNormMaskRow does), and the truncation mask
//                      of L from width + kappa bit planes (div_trunc_mask_elem, the body of hb_div_product_step(HB_DIV_TRUNC)): masked to
//                      open and s = L + r1 kept.
// FxLogFinishRow      after the last open: (s - (opened mod 2^m)) 2^(-m) + I, I the integer part the scale step kept.
// "Products to truncation masks" between the opens of a level is hb_fxexp_products_trunc, as it stands (hb_div_product_step takes two
// products at the most; a level has up to d / 2).
//
// Operands and results are packed canonical residues.  A step's row is an HB_HD function over a memory policy (hb_rows.hpp): k_rows runs
// it on the device, host_rows the very same row in hb_selftest_fxlog, and each step is ONE step function behind both.
//
// Launch shape (all kernels): 256-thread workgroups, one element a thread in x, the product in blockIdx.y (FxLogPolyMaskRow walks the
// powers and the planes in the thread; FxLogFirstRow and FxLogFinishRow have one row).  No LDS, no grid stride, one launch a call.
// Planes, triples, opened and kept values are read once and take the non-temporal loads (load_once); the older powers take the plain
// one (`powers` is written by the same launch, other rows); the coefficients are one address a wave (same) and sit in SGPRs.
// Compiler's report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; scratch = 0 bytes for every kernel):
//   FxLogFirstRow<9, 8>       74 VGPRs: 6 waves a SIMD                                   FxLogFirstRow<3, 2>       27 VGPRs: 8 waves
//   FxLogLevelRow<9, 8>       63 VGPRs: 8 waves                                          FxLogLevelRow<3, 2>       22 VGPRs: 8 waves
//   FxLogPolyMaskRow<9, 8>    104 VGPRs: 4 waves                                         FxLogPolyMaskRow<3, 2>    39 VGPRs: 8 waves
//   FxLogFinishRow<9, 8>      49 VGPRs: 8 waves                                          FxLogFinishRow<3, 2>      16 VGPRs: 8 waves
// (DESIGN.md section 3ad has the series, the error and width derivations and the counts.)
#include "hb_common.hpp"
#include "hb_div_elem.hpp"

using namespace hb;

namespace hb {

constexpr int FXLOG_MAX_DEGREE = 64;

// ---------------------------------------------------------------- the shape of a level (host and device)
// level l >= 1 forms the powers half < j <= min(2 half, d), half = 2^(l-1)
HB_HD int fxlog_half(int level) { return 1 << (level - 1); }
HB_HD int fxlog_level_powers(int level, int d) { const int h = fxlog_half(level); return d <= h ? 0 : ((2 * h < d ? 2 * h : d) - h); }
static int fxlog_levels(int d) { int l = 0; while ((1 << l) < d) l++; return l; }

// ---------------------------------------------------------------- per-element bodies (host and device)
// t = 4 c - 3 y
template <int NL, int NW>
HB_HD void fxlog_first_elem(uint32_t (&o)[NW], const uint32_t (&cw)[NW], const uint32_t (&yw)[NW], const FpParams<NL> &P) {
    uint32_t c[NL], y[NL], t[NL], u[NL];
    unpack<NL, NW>(c, cw);
    unpack<NL, NW>(y, yw);
    fp_add<NL>(t, c, c, P);
    fp_add<NL>(c, t, t, P);
    fp_add<NL>(t, y, y, P);
    fp_add<NL>(u, t, y, P);
    fp_sub<NL>(t, c, u, P);
    pack<NL, NW>(o, t);
}

// sum_{i < n} coef_i value_i: value(w, i) loads this element's word of term i, coef(w, i) the canonical coefficient.  A column takes GROUP
// products before carries must move; a reduced group sum is below 2 p, one conditional subtraction; the sum of them is the sum / R, and the
// product by R^2 at the end makes it the sum (fxsqrt_scale_elem's scheme).
template <int NL, int NW, class Value, class Coef>
HB_HD void fxlog_poly_elem(uint32_t (&o)[NW], Value &&value, Coef &&coef, int n, const FpParams<NL> &P) {
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

// ---------------------------------------------------------------- the steps' rows (host and device, over a memory policy)
struct FxLogFirstArgs { const uint32_t *opened, *ta, *tb, *tab, *ybig, *nxt_a, *nxt_b; uint32_t *masked, *powers; };

struct FxLogFirstRow {
template <int NL, int NW, class Mem>
HB_HD static void run(const FxLogFirstArgs &A, int, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
    uint32_t dw[NW], ew[NW], aw[NW], bw[NW], abw[NW], cw[NW], tw[NW], o[NW];
    mem.once(dw, A.opened, i); mem.once(ew, A.opened, count + i);
    mem.once(aw, A.ta, i); mem.once(bw, A.tb, i); mem.once(abw, A.tab, i);
    ew_beaver_elem<NL, NW>(cw, dw, ew, aw, bw, abw, P);
    mem.once(aw, A.ybig, i);
    fxlog_first_elem<NL, NW>(tw, cw, aw, P);
    mem.store(A.powers, i, tw);
    mem.once(aw, A.nxt_a, i);
    diff_elem<NL, NW>(o, tw, aw, P);
    mem.store(A.masked, i, o);
    mem.once(aw, A.nxt_b, i);
    diff_elem<NL, NW>(o, tw, aw, P);
    mem.store(A.masked, count + i, o);
}
};

template <int NL> struct FxLogLevelArgs {
    const uint32_t *opened, *s, *ta, *tb;
    uint32_t *masked, *powers;
    int level, d, m;
    FpConst<NL> invm;
};

// truncation r of the level whose masks were just opened
template <int NL, int NW, class Mem>
HB_HD void fxlog_trunc_row(uint32_t (&o)[NW], const uint32_t *s, const uint32_t *opened, int r, int64_t i, int64_t count, int m, const uint32_t (&invm)[NL], const Mem &mem,
                           const FpParams<NL> &P) {
    uint32_t sw[NW], cw[NW];
    mem.once(sw, s, (int64_t)r * count + i); mem.once(cw, opened, (int64_t)r * count + i);
    div_trunc_elem<NL, NW>(o, sw, cw, m, invm, P);
}

struct FxLogLevelRow {
template <int NL, int NW, class Mem>
HB_HD static void run(const FxLogLevelArgs<NL> &A, int q, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
    const int half = fxlog_half(A.level), done = fxlog_level_powers(A.level, A.d), next = fxlog_level_powers(A.level + 1, A.d);
    uint32_t first[NW], second[NW], aw[NW], o[NW];
    if (q < done) {
        fxlog_trunc_row<NL, NW>(second, A.s, A.opened, q, i, count, A.m, A.invm.d, mem, P);
        mem.store(A.powers, (int64_t)(half + q) * count + i, second);
    }
    if (q >= next) return;
    fxlog_trunc_row<NL, NW>(first, A.s, A.opened, done - 1, i, count, A.m, A.invm.d, mem, P);          // t^(2 half): a next level means done == half
    if (q >= half) fxlog_trunc_row<NL, NW>(second, A.s, A.opened, q - half, i, count, A.m, A.invm.d, mem, P);
    else mem.load(second, A.powers, (int64_t)q * count + i);
    mem.once(aw, A.ta, (int64_t)q * count + i);
    diff_elem<NL, NW>(o, first, aw, P);
    mem.store(A.masked, (int64_t)(2 * q) * count + i, o);
    mem.once(aw, A.tb, (int64_t)q * count + i);
    diff_elem<NL, NW>(o, second, aw, P);
    mem.store(A.masked, (int64_t)(2 * q + 1) * count + i, o);
}
};

template <int NL> struct FxLogPolyArgs {
    const uint32_t *opened, *s, *powers, *ybig, *coef, *bits;
    uint32_t *masked, *s_out;
    int d, half, m_in, nbits, m_out;
    FpConst<NL> invm, halfw;
};

struct FxLogPolyMaskRow {
template <int NL, int NW, class Mem>
HB_HD static void run(const FxLogPolyArgs<NL> &A, int, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
    uint32_t lw[NW], o0[NW], o1[NW];
    fxlog_poly_elem<NL, NW>(lw, [&](uint32_t (&w)[NW], int j) {                       // term 0 is Y, term j >= 1 the power t^j
        if (j == 0) mem.once(w, A.ybig, i);
        else if (j - 1 < A.half) mem.once(w, A.powers, (int64_t)(j - 1) * count + i);
        else fxlog_trunc_row<NL, NW>(w, A.s, A.opened, j - 1 - A.half, i, count, A.m_in, A.invm.d, mem, P);
    }, [&](uint32_t (&w)[NW], int j) { mem.same(w, A.coef + (int64_t)j * NW); }, A.d + 1, P);
    div_trunc_mask_elem<NL, NW>(o0, o1, lw, [&](uint32_t (&bw)[NW], int row) { mem.once(bw, A.bits, (int64_t)row * count + i); }, A.nbits, A.m_out, A.halfw.d, P);
    mem.store(A.masked, i, o0);
    mem.store(A.s_out, i, o1);
}
};

template <int NL> struct FxLogFinishArgs {
    const uint32_t *opened, *s, *ipart;
    uint32_t *out;
    int m;
    FpConst<NL> invm;
};

struct FxLogFinishRow {
template <int NL, int NW, class Mem>
HB_HD static void run(const FxLogFinishArgs<NL> &A, int, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
    uint32_t tw[NW], iw[NW], o[NW], zero[NL];
#pragma unroll
    for (int q = 0; q < NL; q++) zero[q] = 0u;
    fxlog_trunc_row<NL, NW>(tw, A.s, A.opened, 0, i, count, A.m, A.invm.d, mem, P);
    mem.once(iw, A.ipart, i);
    div_affine_elem<NL, NW>(o, tw, 1, zero, iw, P);
    mem.store(A.out, i, o);
}
};

// ---------------------------------------------------------------- host side
// One step function a step (hb_rows.hpp): a DeviceRun in the entry point, a HostRun in hb_selftest_fxlog.
static bool fxlog_degree_ok(int d) { return d >= 2 && d <= FXLOG_MAX_DEGREE; }

template <class Run> static int fxlog_first_step(const Run &run, const uint64_t *opened, const uint64_t *ta, const uint64_t *tb, const uint64_t *tab, const uint64_t *ybig,
                                                 const uint64_t *nxt_a, const uint64_t *nxt_b, uint64_t *masked, uint64_t *powers, int64_t count) {
    if (count < 0 || (count > 0 && (!opened || !ta || !tb || !tab || !ybig || !nxt_a || !nxt_b || !masked || !powers))) return HB_ERR_BAD_ARG;
    if (count == 0) return HB_OK;
    const int64_t rb = run.elem_bytes() * count;
    const RowSpan outs[2] = {{masked, 2}, {powers, 1}}, ins[7] = {{opened, 2}, {ta, 1}, {tb, 1}, {tab, 1}, {ybig, 1}, {nxt_a, 1}, {nxt_b, 1}};
    if (!outputs_apart(outs, 2, ins, 7, rb)) return run.fail(HB_ERR_BAD_ARG, "hb_fxlog_first: masked and powers are arrays of their own");
    const FxLogFirstArgs A = {u32(opened), u32(ta), u32(tb), u32(tab), u32(ybig), u32(nxt_a), u32(nxt_b), u32(masked), u32(powers)};
    return run.template rows<FxLogFirstRow>(A, 1, count);
}

template <class Run> static int fxlog_level_step(const Run &run, int level, int d, const uint64_t *opened, const uint64_t *s, int m, const uint64_t *inv2m_host,
                                                 const uint64_t *ta, const uint64_t *tb, uint64_t *masked, uint64_t *powers, int64_t count) {
    if (count < 0) return HB_ERR_BAD_ARG;
    if (!fxlog_degree_ok(d) || level < 1 || level >= fxlog_levels(d) || !fxp_m_ok(run.bits(), m))
        return run.fail(HB_ERR_BAD_ARG, "hb_fxlog_level: needs 2 <= d <= 64, 1 <= level < ceil(log2 d) and 0 < m <= bits(p) - 2");
    if (!inv2m_host || (count > 0 && (!opened || !s || !ta || !tb || !masked || !powers))) return HB_ERR_BAD_ARG;
    const int done = fxlog_level_powers(level, d), next = fxlog_level_powers(level + 1, d);
    const int64_t rb = run.elem_bytes() * count;
    const RowSpan outs[2] = {{masked, 2 * next}, {powers, d}}, ins[4] = {{opened, done}, {s, done}, {ta, next}, {tb, next}};
    if (count > 0 && !outputs_apart(outs, 2, ins, 4, rb)) return run.fail(HB_ERR_BAD_ARG, "hb_fxlog_level: masked and powers are arrays of their own");
    const int rc = run.template rows<FxLogLevelRow, FxLogLevelArgs>([&](auto &A, const auto &P) {
        A.opened = u32(opened); A.s = u32(s); A.ta = u32(ta); A.tb = u32(tb); A.masked = u32(masked); A.powers = u32(powers);
        A.level = level; A.d = d; A.m = m;
        constexpr int NL = sizeof(A.invm.d) / sizeof(uint32_t);
        return host_mont<NL, words_of(NL)>(A.invm.d, P, inv2m_host);
    }, done > next ? done : next, count);
    return rc == HB_ERR_BAD_ARG ? run.fail(rc, "hb_fxlog_level: a constant is not below the modulus") : rc;
}

template <class Run> static int fxlog_poly_mask_step(const Run &run, int d, const uint64_t *opened, const uint64_t *s, int m_in, const uint64_t *inv2m_host,
                                                     const uint64_t *powers, const uint64_t *ybig, const uint64_t *coef, const uint64_t *bits, int width, int m_out, int kappa,
                                                     uint64_t *masked, uint64_t *s_out, int64_t count) {
    if (count < 0) return HB_ERR_BAD_ARG;
    if (!fxlog_degree_ok(d) || !fxp_m_ok(run.bits(), m_in) || !fxp_params_ok(run.bits(), width, m_out, kappa))
        return run.fail(HB_ERR_BAD_ARG, "hb_fxlog_poly_mask: needs 2 <= d <= 64, 0 < m_in <= bits(p) - 2 and a truncation the modulus has room for");
    if (!inv2m_host || !coef || (count > 0 && (!opened || !s || !powers || !ybig || !bits || !masked || !s_out))) return HB_ERR_BAD_ARG;
    const int last = fxlog_levels(d), half = fxlog_half(last), done = fxlog_level_powers(last, d);
    const int64_t rb = run.elem_bytes() * count, cb = run.elem_bytes() * (d + 1);
    const RowSpan outs[2] = {{masked, 1}, {s_out, 1}}, ins[5] = {{opened, done}, {s, done}, {powers, half}, {ybig, 1}, {bits, width + kappa}};
    if (count > 0 && (!outputs_apart(outs, 2, ins, 5, rb) || overlap(coef, cb, masked, rb) || overlap(coef, cb, s_out, rb)))
        return run.fail(HB_ERR_BAD_ARG, "hb_fxlog_poly_mask: masked and s_out are arrays of their own");
    const int rc = run.template rows<FxLogPolyMaskRow, FxLogPolyArgs>([&](auto &A, const auto &P) {
        A.opened = u32(opened); A.s = u32(s); A.powers = u32(powers); A.ybig = u32(ybig); A.coef = u32(coef); A.bits = u32(bits);
        A.masked = u32(masked); A.s_out = u32(s_out);
        A.d = d; A.half = half; A.m_in = m_in; A.nbits = width + kappa; A.m_out = m_out;
        constexpr int NL = sizeof(A.invm.d) / sizeof(uint32_t);
        fxp_pow2<NL>(A.halfw.d, width - 1, false, P);
        return host_mont<NL, words_of(NL)>(A.invm.d, P, inv2m_host);
    }, 1, count);
    return rc == HB_ERR_BAD_ARG ? run.fail(rc, "hb_fxlog_poly_mask: a constant is not below the modulus") : rc;
}

template <class Run> static int fxlog_finish_step(const Run &run, const uint64_t *opened, const uint64_t *s, int m, const uint64_t *inv2m_host, const uint64_t *ipart,
                                                  uint64_t *out, int64_t count) {
    if (count < 0) return HB_ERR_BAD_ARG;
    if (!fxp_m_ok(run.bits(), m)) return run.fail(HB_ERR_BAD_ARG, "hb_fxlog_finish: needs 0 < m <= bits(p) - 2");
    if (!inv2m_host || (count > 0 && (!opened || !s || !ipart || !out))) return HB_ERR_BAD_ARG;
    const int64_t rb = run.elem_bytes() * count;
    const RowSpan outs[1] = {{out, 1}}, ins[3] = {{opened, 1}, {s, 1}, {ipart, 1}};
    if (count > 0 && !outputs_apart(outs, 1, ins, 3, rb)) return run.fail(HB_ERR_BAD_ARG, "hb_fxlog_finish: out is an array of its own");
    const int rc = run.template rows<FxLogFinishRow, FxLogFinishArgs>([&](auto &A, const auto &P) {
        A.opened = u32(opened); A.s = u32(s); A.ipart = u32(ipart); A.out = u32(out); A.m = m;
        constexpr int NL = sizeof(A.invm.d) / sizeof(uint32_t);
        return host_mont<NL, words_of(NL)>(A.invm.d, P, inv2m_host);
    }, 1, count);
    return rc == HB_ERR_BAD_ARG ? run.fail(rc, "hb_fxlog_finish: a constant is not below the modulus") : rc;
}

}  // namespace hb

extern "C" {

int hb_fxlog_first(hb_ctx *ctx, const uint64_t *opened_dev, const uint64_t *ta_dev, const uint64_t *tb_dev, const uint64_t *tab_dev, const uint64_t *ybig_dev,
                   const uint64_t *nxt_a_dev, const uint64_t *nxt_b_dev, uint64_t *masked_dev, uint64_t *powers_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : fxlog_first_step(DeviceRun{ctx, (hipStream_t)stream, "hb_fxlog_first"}, opened_dev, ta_dev, tb_dev, tab_dev, ybig_dev, nxt_a_dev, nxt_b_dev,
                                                    masked_dev, powers_dev, count);
}

int hb_fxlog_level(hb_ctx *ctx, int level, int d, const uint64_t *opened_dev, const uint64_t *s_dev, int m, const uint64_t *inv2m_host, const uint64_t *ta_dev,
                   const uint64_t *tb_dev, uint64_t *masked_dev, uint64_t *powers_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : fxlog_level_step(DeviceRun{ctx, (hipStream_t)stream, "hb_fxlog_level"}, level, d, opened_dev, s_dev, m, inv2m_host, ta_dev, tb_dev,
                                                    masked_dev, powers_dev, count);
}

int hb_fxlog_poly_mask(hb_ctx *ctx, int d, const uint64_t *opened_dev, const uint64_t *s_dev, int m_in, const uint64_t *inv2m_host, const uint64_t *powers_dev,
                       const uint64_t *ybig_dev, const uint64_t *coef_dev, const uint64_t *bits_dev, int width, int m_out, int kappa, uint64_t *masked_dev,
                       uint64_t *s_out_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : fxlog_poly_mask_step(DeviceRun{ctx, (hipStream_t)stream, "hb_fxlog_poly_mask"}, d, opened_dev, s_dev, m_in, inv2m_host, powers_dev,
                                                        ybig_dev, coef_dev, bits_dev, width, m_out, kappa, masked_dev, s_out_dev, count);
}

int hb_fxlog_finish(hb_ctx *ctx, const uint64_t *opened_dev, const uint64_t *s_dev, int m, const uint64_t *inv2m_host, const uint64_t *ipart_dev, uint64_t *out_dev,
                    int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : fxlog_finish_step(DeviceRun{ctx, (hipStream_t)stream, "hb_fxlog_finish"}, opened_dev, s_dev, m, inv2m_host, ipart_dev, out_dev, count);
}

// params: as the header lists them for each step
int hb_selftest_fxlog(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *ops, const int64_t *params, uint64_t *const *outs, int64_t count) {
    if (!p_limbs || !ops || !params || !outs || (n_limbs != 1 && n_limbs != 4)) return HB_ERR_BAD_ARG;
    for (int i = 0; i < 5; i++) if (params[i] < -(1 << 30) || params[i] > (1 << 30)) return HB_ERR_BAD_ARG;
    const HostRun run = {p_limbs, n_limbs};
    const int a = (int)params[0], b = (int)params[1], c = (int)params[2], d = (int)params[3], e = (int)params[4];
    switch (what) {
    case HB_FXLOG_SELFTEST_FIRST: return fxlog_first_step(run, ops[0], ops[1], ops[2], ops[3], ops[4], ops[5], ops[6], outs[0], outs[1], count);
    case HB_FXLOG_SELFTEST_LEVEL:                                               // level, d, m
        return fxlog_level_step(run, a, b, ops[0], ops[1], c, ops[2], ops[3], ops[4], outs[0], outs[1], count);
    case HB_FXLOG_SELFTEST_POLY_MASK:                                           // d, m_in, width, m_out, kappa
        return fxlog_poly_mask_step(run, a, ops[0], ops[1], b, ops[2], ops[3], ops[4], ops[5], ops[6], c, d, e, outs[0], outs[1], count);
    case HB_FXLOG_SELFTEST_FINISH:                                              // m
        return fxlog_finish_step(run, ops[0], ops[1], a, ops[2], ops[3], outs[0], count);
    default: return HB_ERR_BAD_ARG;
    }
}

}  // extern "C"

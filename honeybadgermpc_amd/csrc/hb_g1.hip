// hb_g1.hip -- the group G1 of BLS12-381, E: y^2 = x^3 + 4 over GF(Q), and on it the linear (Pedersen) polynomial commitment of the
// reference's poly_commit_lin.py (commit :12-19, verify_eval :24-29, batch_verify_eval :31-37), which costs an AVSS dealer one
// g^a h^b a coefficient and a recipient a (t + 1)-term product of powers a share (hbavss.py) -- restated on fp29.hpp, not translated.
//
// Field.  Fq = FpParams<14>, 12 words: fourteen 29-bit digits, Montgomery's R = 2^406 over the 381-bit Q.  The modulus is fixed, so its
// digits, R mod Q, R^2 mod Q and n0 are literals (fq_params); g1_consts_ok re-derives every one of them from Q's words with plain
// shifts and subtractions and is asked once a process and by every self test.  make_params of hb_core.hip (a 320-bit integer) is not
// used and no instantiation for <9> or <3> changes.  Lazy<NL> is not used either: no dot products here.
//   One product needs no carry pass before REDC: a column holds at most 14 products of two 29-bit digits and, during REDC, 14 more and
//   its neighbour's carry: 28 (2^29 - 1)^2 + 2^35 < 2^63.
//   LAZY SUMS.  fq_add_lazy adds without the conditional subtraction.  mont_mul takes operands with a b < 2^24 Q^2 and digits below
//   2^29 (but the top one: 4 bits in Q, 7 in whatever twelve words hold): REDC gives a b / R + Q < Q (1 + 2^24 Q / 2^406) < 3 Q / 2, so
//   ONE conditional subtraction leaves the canonical residue.  Twelve words of HBM hold less than 10 Q (g1_load reduces what it is
//   given).  The only lazy values are X + Y^2 < 2 Q and 3 X^2 < 3 Q in g1_double; each is used as a factor and nothing else.  Every
//   other sum and difference is fp_add / fp_sub on canonical residues, so is_zero and equality are exact.
//
// Points.  HBM: (count, 2, 6) 64-bit words, x then y, little-endian canonical residues below Q; the identity is all zeros ((0, 0) is not
// on the curve).  Registers: Jacobian (X : Y : Z), x = X / Z^2, y = Y / Z^3, Montgomery residues, Z = 0 the identity.
//   g1_double      A = X^2, B = Y^2, C = B^2, D = 2 ((X + B)^2 - A - C), E = 3 A, F = E^2;
//                  X' = F - 2 D, Y' = E (D - X') - 8 C, Z' = 2 Y Z                                        (a = 0; 7 products)
//                  Complete: #E = H R is odd, so no point has y = 0, and Z = 0 stays Z' = 0.
//   g1_add_mixed   second operand affine:  U2 = x2 Z1^2, S2 = y2 Z1^3, H = U2 - X1, r = S2 - Y1;
//                  X' = r^2 - H^3 - 2 X1 H^2, Y' = r (X1 H^2 - X') - Y1 H^3, Z' = Z1 H                   (11 products)
//   g1_add         both Jacobian: U1 = X1 Z2^2, U2 = X2 Z1^2, S1 = Y1 Z2^3, S2 = Y2 Z1^3, H = U2 - U1, r = S2 - S1;
//                  X' = r^2 - H^3 - 2 U1 H^2, Y' = r (U1 H^2 - X') - S1 H^3, Z' = Z1 Z2 H                 (16 products)
//   Both additions are complete by three rarely entered branches, not by computing two results a lane: an identity operand returns
//   the other one; H = 0 with r = 0 (equal points) runs g1_double; H = 0 with r != 0 (opposite points) gives the identity.  For
//   finite operands H = 0 iff the x coordinates agree, and then y2 = +-y1: nothing else can make a denominator vanish.
//   g1_eq          X1 Z2^2 = X2 Z1^2 and Y1 Z2^3 = Y2 Z1^3, identities apart: no inversion                (8 products)
//   to affine      one fq_inv (Z^(Q - 2): the exponent's words are shifted out a bit a round) and 4 products; 0^(Q - 2) = 0 maps Z = 0 to (0, 0).
//
// Kernels: 256-thread workgroups, one item a thread, grid = ceil(count / 256), no LDS, no grid stride, every lane checked against
// count, the caller's stream, nothing waits for another workgroup.
//   k_g1_scalar_mul   k_i P_i, k a plain 256-bit integer: left to right, a doubling a bit once the first set bit has passed and a mixed
//                     addition a set bit; scalar and point: one for all (element 0) or one an element
//   k_g1_add          P_i +- Q_i (mixed addition of two affine operands)
//   k_g1_check        flag_i = identity, or (coordinates below Q and on the curve)
//   k_g1_table        fixed-base windows of ONE base, width c in {4, 8}, W = 256 / c windows of n = 2^c - 1 entries: entry (w, j) =
//                     j 2^(c w) base, affine.  One thread a WINDOW: c w doublings, n - 1 complete additions of B_w (the first of them is
//                     the doubling branch), then Montgomery's trick: one inversion a window for all its entries.  Serial in a lane
//                     (W lanes work): a table is built once a common reference string.
//                     Layout: entry e = w n + (j - 1) at 32 words: x's 14 Montgomery digits, 2 words of padding, y's 14, 2 of padding
//                     (eight dwordx4 loads an entry); behind the W n entries 2 x 16 words an entry of scratch (Z and prefix products), then the base.
//   k_g1_commit       a_i g + b_i h from the two tables: the window digits of a and b from the bottom, a mixed addition a non-zero
//                     digit (2 W at most), no doubling
//   k_g1_eval         sum_j idx^j C_bj by Horner's rule: acc = C_t; acc = idx acc + C_j.  idx acc is a left-to-right double-and-add
//                     over the bits of idx (wave-uniform: floor(log2 idx) doublings, popcount(idx) - 1 complete additions of the old acc)
//   k_g1_verify       per item: the Horner side with an on-curve check of each commitment as it is loaded, s_b g + w_b h from the
//                     tables, g1_eq; verdict_b = 1 accepted / 0 rejected, rejected items counted into *rejected (atomicAdd)
// The per-element bodies are HB_HD functions (as hb_jj.hip): the __global__ wrappers only find the index and call them, and
// hb_selftest_g1 runs the very same bodies over host memory.
// mont_mul<14> is NOT inlined on the device (fq_mul_call: operands and result by value in VGPRs, no stack): inlined, k_g1_verify
// held ~110 copies of a 4.4 KB product against a 64 KB instruction cache; called, it is 63 KB.  Compiler's report: profiles/g1.txt.
#include "hb_g1_elem.hpp"

using namespace hb;

namespace hb {

// ---------------------------------------------------------------- per-item bodies (host and device)
HB_HD void g1_scalar_mul_elem(uint32_t *out, const uint32_t *k, const uint32_t *p, const FpParams<QL> &P) {
    uint32_t kw[SW];
    G1Aff a;
    G1Jac acc;
    g1_load_scalar(kw, k);
    g1_load(a, p, P);
    g1_mul_affine(acc, kw, a, P);
    g1_store(out, acc, P);
}
HB_HD void g1_add_elem(uint32_t *out, const uint32_t *p, const uint32_t *q, int subtract, const FpParams<QL> &P) {
    G1Aff a, b;
    G1Jac acc;
    g1_load(a, p, P);
    g1_load(b, q, P);
    if (subtract) fp_neg<QL>(b.y, b.y, P);
    g1_from_affine(acc, a, P);
    g1_add_mixed(acc, b, P);
    g1_store(out, acc, P);
}
HB_HD int32_t g1_check_elem(const uint32_t *p, const FpParams<QL> &P) {
    G1Aff a;
    const bool below = g1_load(a, p, P);
    if (a.inf) return 1;
    return (below && g1_on_curve(a, P)) ? 1 : 0;
}
// (g1_table_window, the body of k_g1_table, lives in hb_g1_elem.hpp: k_g1_crs_table of hb_crs.hip runs it a base a workgroup)
// acc = ka g + kb h from the two tables
HB_HD void g1_comb(G1Jac &acc, const uint32_t (&kaw)[SW], const uint32_t (&kbw)[SW], const uint32_t *tg, const uint32_t *th, int c, const FpParams<QL> &P) {
    const int n = (1 << c) - 1, W = 256 / c;
    uint32_t ka[SW], kb[SW];
#pragma unroll
    for (int q = 0; q < SW; q++) { ka[q] = kaw[q]; kb[q] = kbw[q]; }
    g1_set_identity(acc, P);
#pragma unroll 1
    for (int w = 0; w < W; w++) {
#pragma unroll 1
        for (int s = 0; s < 2; s++) {
            const uint32_t d = (s ? kb[0] : ka[0]) & (uint32_t)n;
            if (d) {
                G1Aff e;
                g1_load_entry(e, (s ? th : tg) + ((int64_t)w * n + (d - 1)) * G1_ENT);
                g1_add_mixed(acc, e, P);
            }
        }
#pragma unroll
        for (int q = 0; q < SW; q++) {
            ka[q] = (ka[q] >> c) | (q + 1 < SW ? ka[q + 1] << (32 - c) : 0u);
            kb[q] = (kb[q] >> c) | (q + 1 < SW ? kb[q + 1] << (32 - c) : 0u);
        }
    }
}
HB_HD void g1_commit_elem(uint32_t *out, const uint32_t *a, const uint32_t *b, const uint32_t *tg, const uint32_t *th, int c, const FpParams<QL> &P) {
    uint32_t ka[SW], kb[SW];
    G1Jac acc;
    g1_load_scalar(ka, a);
    g1_load_scalar(kb, b);
    g1_comb(acc, ka, kb, tg, th, c, P);
    g1_store(out, acc, P);
}
// acc = sum_j idx^j C_j over the item's n_coef commitments at cs; returns whether every one of them passed g1_check_elem's test
HB_HD bool g1_horner(G1Jac &acc, const uint32_t *cs, int n_coef, uint32_t idx, bool check, const FpParams<QL> &P) {
    G1Aff cj;
    bool ok = g1_load(cj, cs + (int64_t)(n_coef - 1) * G1_PT, P);
    if (check && !cj.inf) ok = ok && g1_on_curve(cj, P);
    g1_from_affine(acc, cj, P);
    const int top = idx ? 31 - __builtin_clz(idx) : 0;
#pragma unroll 1
    for (int j = n_coef - 2; j >= 0; j--) {
        if (idx == 0) g1_set_identity(acc, P);
        else if (idx > 1) {
            const G1Jac base = acc;
#pragma unroll 1
            for (int b = top - 1; b >= 0; b--) {
                g1_double(acc, acc, P);
                if ((idx >> b) & 1u) g1_add(acc, base, P);
            }
        }
        bool below = g1_load(cj, cs + (int64_t)j * G1_PT, P);
        if (check && !cj.inf) below = below && g1_on_curve(cj, P);
        ok = ok && below;
        g1_add_mixed(acc, cj, P);
    }
    return ok;
}
HB_HD void g1_eval_elem(uint32_t *out, const uint32_t *cs, int n_coef, uint32_t idx, const FpParams<QL> &P) {
    G1Jac acc;
    g1_horner(acc, cs, n_coef, idx, false, P);
    g1_store(out, acc, P);
}
HB_HD int32_t g1_verify_elem(const uint32_t *cs, int n_coef, uint32_t idx, const uint32_t *s, const uint32_t *wt, const uint32_t *tg, const uint32_t *th, int c,
                             const FpParams<QL> &P) {
    uint32_t ka[SW], kb[SW];
    G1Jac lhs, rhs;
    const bool ok = g1_horner(lhs, cs, n_coef, idx, true, P);
    g1_load_scalar(ka, s);
    g1_load_scalar(kb, wt);
    g1_comb(rhs, ka, kb, tg, th, c, P);
    return (ok && g1_eq(lhs, rhs, P)) ? 1 : 0;
}

// ---------------------------------------------------------------- kernels
__global__ void __launch_bounds__(256) k_g1_scalar_mul(const uint32_t *k, int k_bcast, const uint32_t *p, int p_bcast, uint32_t *out, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const FpParams<QL> P = fq_params();
    g1_scalar_mul_elem(out + i * G1_PT, k + (k_bcast ? 0 : i) * SW, p + (p_bcast ? 0 : i) * G1_PT, P);
}
__global__ void __launch_bounds__(256) k_g1_add(const uint32_t *p, const uint32_t *q, int subtract, uint32_t *out, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const FpParams<QL> P = fq_params();
    g1_add_elem(out + i * G1_PT, p + i * G1_PT, q + i * G1_PT, subtract, P);
}
__global__ void __launch_bounds__(256) k_g1_check(const uint32_t *p, int32_t *flags, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const FpParams<QL> P = fq_params();
    flags[i] = g1_check_elem(p + i * G1_PT, P);
}
__global__ void __launch_bounds__(256) k_g1_table(const uint32_t *base, int c, uint32_t *table) {
    const int w = blockIdx.x * 256 + threadIdx.x;
    if (w >= 256 / c) return;
    const FpParams<QL> P = fq_params();
    g1_table_window(table, base, c, w, P);
}
__global__ void __launch_bounds__(256) k_g1_commit(const uint32_t *tg, const uint32_t *th, int c, const uint32_t *a, const uint32_t *b, uint32_t *out, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const FpParams<QL> P = fq_params();
    g1_commit_elem(out + i * G1_PT, a + i * SW, b + i * SW, tg, th, c, P);
}
__global__ void __launch_bounds__(256) k_g1_eval(const uint32_t *cs, int n_coef, uint32_t idx, uint32_t *out, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const FpParams<QL> P = fq_params();
    g1_eval_elem(out + i * G1_PT, cs + i * n_coef * G1_PT, n_coef, idx, P);
}
__global__ void __launch_bounds__(256) k_g1_verify(const uint32_t *tg, const uint32_t *th, int c, const uint32_t *cs, int n_coef, uint32_t idx, const uint32_t *s,
                                                   const uint32_t *wt, int32_t *verdict, int32_t *rejected, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const FpParams<QL> P = fq_params();
    const int32_t v = g1_verify_elem(cs + i * n_coef * G1_PT, n_coef, idx, s + i * SW, wt + i * SW, tg, th, c, P);
    verdict[i] = v;
    if (!v) atomicAdd(rejected, 1);
}

// ---------------------------------------------------------------- host side
static bool g1_window_ok(int c) { return c == 4 || c == 8; }
static int64_t g1_table_words(int c) { return (int64_t)(256 / c) * ((1 << c) - 1) * (G1_ENT + G1_SCR) + G1_SCR; }   // + the base, for the build

}  // namespace hb

extern "C" {

int hb_g1_scalar_mul(hb_ctx *ctx, const uint64_t *k_dev, int k_broadcast, const uint64_t *p_dev, int point_broadcast, uint64_t *out_dev, int64_t count, void *stream) {
    G1_ENTER("hb_g1_scalar_mul", count, !k_dev || !p_dev || !out_dev);
    if (count > 1 && ((k_broadcast && (const uint64_t *)out_dev == k_dev) || (point_broadcast && (const uint64_t *)out_dev == p_dev)))
        return fail(ctx, HB_ERR_BAD_ARG, "hb_g1_scalar_mul: out aliases a broadcast operand");
    if (count == 0) return HB_OK;
    k_g1_scalar_mul<<<blocks, 256, 0, s>>>((const uint32_t *)k_dev, k_broadcast != 0, (const uint32_t *)p_dev, point_broadcast != 0, (uint32_t *)out_dev, count);
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_g1_add(hb_ctx *ctx, const uint64_t *p_dev, const uint64_t *q_dev, int subtract, uint64_t *out_dev, int64_t count, void *stream) {
    G1_ENTER("hb_g1_add", count, !p_dev || !q_dev || !out_dev);
    if (count == 0) return HB_OK;
    k_g1_add<<<blocks, 256, 0, s>>>((const uint32_t *)p_dev, (const uint32_t *)q_dev, subtract != 0, (uint32_t *)out_dev, count);
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_g1_check(hb_ctx *ctx, const uint64_t *p_dev, int32_t *flags_dev, int64_t count, void *stream) {
    G1_ENTER("hb_g1_check", count, !p_dev || !flags_dev);
    if (count == 0) return HB_OK;
    k_g1_check<<<blocks, 256, 0, s>>>((const uint32_t *)p_dev, flags_dev, count);
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int64_t hb_g1_table_bytes(int window) { return g1_window_ok(window) ? g1_table_words(window) * 4 : 0; }

int hb_g1_table(hb_ctx *ctx, const uint64_t *base_host, int window, void *table_dev, void *stream) {
    const int64_t one = 1;
    G1_ENTER("hb_g1_table", one, !base_host || !table_dev);
    if (!g1_window_ok(window)) return fail(ctx, HB_ERR_BAD_ARG, "hb_g1_table: the window width is 4 or 8");
    const FpParams<QL> P = fq_params();
    G1Aff a;
    const bool below = g1_load(a, (const uint32_t *)base_host, P);
    if (a.inf) return fail(ctx, HB_ERR_BAD_ARG, "hb_g1_table: the base is the identity");
    if (!below || !g1_on_curve(a, P)) return fail(ctx, HB_ERR_BAD_ARG, "hb_g1_table: the base is not on the curve");
    // the base rides behind the table's scratch: no allocation, no lifetime to keep
    uint32_t *table = (uint32_t *)table_dev;
    uint32_t *base_dev = table + g1_table_words(window) - G1_SCR;
    HB_HIP(ctx, hipMemcpyAsync(base_dev, base_host, G1_PT * 4, hipMemcpyHostToDevice, s));
    HB_HIP(ctx, hipStreamSynchronize(s));                       // base_host is the caller's again on return
    k_g1_table<<<1, 256, 0, s>>>(base_dev, window, table);
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_g1_commit(hb_ctx *ctx, const void *tg_dev, const void *th_dev, int window, const uint64_t *a_dev, const uint64_t *b_dev, uint64_t *out_dev, int64_t count,
                 void *stream) {
    G1_ENTER("hb_g1_commit", count, !a_dev || !b_dev || !out_dev);
    if (!tg_dev || !th_dev || !g1_window_ok(window)) return fail(ctx, HB_ERR_BAD_ARG, "hb_g1_commit: two tables of window width 4 or 8");
    if (count == 0) return HB_OK;
    k_g1_commit<<<blocks, 256, 0, s>>>((const uint32_t *)tg_dev, (const uint32_t *)th_dev, window, (const uint32_t *)a_dev, (const uint32_t *)b_dev, (uint32_t *)out_dev, count);
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_g1_eval(hb_ctx *ctx, const uint64_t *cs_dev, int n_coef, uint64_t index, uint64_t *out_dev, int64_t count, void *stream) {
    G1_ENTER("hb_g1_eval", count, !cs_dev || !out_dev);
    if (n_coef < 1 || n_coef > (1 << 20)) return fail(ctx, HB_ERR_BAD_ARG, "hb_g1_eval: between 1 and 2^20 commitments an item");
    if (index >> 32) return fail(ctx, HB_ERR_BAD_ARG, "hb_g1_eval: the index must be below 2^32");
    if ((const uint64_t *)out_dev == cs_dev && count > 0 && n_coef > 1) return fail(ctx, HB_ERR_BAD_ARG, "hb_g1_eval: out aliases the commitments");
    if (count > (1LL << 40) / n_coef) return fail(ctx, HB_ERR_UNSUPPORTED, "hb_g1_eval: batch too large for one launch");
    if (count == 0) return HB_OK;
    k_g1_eval<<<blocks, 256, 0, s>>>((const uint32_t *)cs_dev, n_coef, (uint32_t)index, (uint32_t *)out_dev, count);
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_g1_verify(hb_ctx *ctx, const void *tg_dev, const void *th_dev, int window, const uint64_t *cs_dev, int n_coef, uint64_t index, const uint64_t *s_dev,
                 const uint64_t *w_dev, int32_t *verdict_dev, int32_t *rejected_dev, int64_t count, void *stream) {
    G1_ENTER("hb_g1_verify", count, !cs_dev || !s_dev || !w_dev || !verdict_dev);
    if (!rejected_dev) return fail(ctx, HB_ERR_BAD_ARG, "hb_g1_verify: the counter is missing");
    if (!tg_dev || !th_dev || !g1_window_ok(window)) return fail(ctx, HB_ERR_BAD_ARG, "hb_g1_verify: two tables of window width 4 or 8");
    if (n_coef < 1 || n_coef > (1 << 20)) return fail(ctx, HB_ERR_BAD_ARG, "hb_g1_verify: between 1 and 2^20 commitments an item");
    if (index >> 32) return fail(ctx, HB_ERR_BAD_ARG, "hb_g1_verify: the index must be below 2^32");
    if (count > (1LL << 40) / n_coef) return fail(ctx, HB_ERR_UNSUPPORTED, "hb_g1_verify: batch too large for one launch");
    if (count == 0) return HB_OK;
    k_g1_verify<<<blocks, 256, 0, s>>>((const uint32_t *)tg_dev, (const uint32_t *)th_dev, window, (const uint32_t *)cs_dev, n_coef, (uint32_t)index, (const uint32_t *)s_dev,
                                       (const uint32_t *)w_dev, verdict_dev, rejected_dev, count);
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_selftest_g1(int what, const uint64_t *const *operands, int flags, int64_t arg, uint64_t *out, int64_t count) {
    if (!operands || count < 0 || !out || !g1_consts_ok()) return HB_ERR_BAD_ARG;
    const FpParams<QL> P = fq_params();
    auto U = [&](int k) { return reinterpret_cast<const uint32_t *>(operands[k]); };
    auto need = [&](int n) { for (int k = 0; k < n; k++) if (!operands[k]) return false; return true; };
    uint32_t *o = reinterpret_cast<uint32_t *>(out);
    switch (what) {
    case HB_G1_SELFTEST_FQ_MUL: {
        if (!need(2) || flags || arg) return HB_ERR_BAD_ARG;
        for (int64_t i = 0; i < count; i++) {
            uint32_t a[QL], b[QL];
            load_digits<QL, QW>(a, U(0) + i * QW);
            load_digits<QL, QW>(b, U(1) + i * QW);
            if (!fq_below_q(a, P) || !fq_below_q(b, P)) return HB_ERR_BAD_ARG;
            fq_to_mont(a, a, P);
            fq_to_mont(b, b, P);
            fq_mul(a, a, b, P);
            fq_from_mont(b, a, P);
            store_digits<QL, QW>(o + i * QW, b);
        }
        return HB_OK;
    }
    case HB_G1_SELFTEST_SCALAR_MUL: {
        if (!need(2) || (flags & ~(HB_G1_SCALAR_BROADCAST | HB_G1_POINT_BROADCAST)) || arg) return HB_ERR_BAD_ARG;
        const bool kb = (flags & HB_G1_SCALAR_BROADCAST) != 0, pb = (flags & HB_G1_POINT_BROADCAST) != 0;
        for (int64_t i = 0; i < count; i++) g1_scalar_mul_elem(o + i * G1_PT, U(0) + (kb ? 0 : i) * SW, U(1) + (pb ? 0 : i) * G1_PT, P);
        return HB_OK;
    }
    case HB_G1_SELFTEST_ADD: {
        if (!need(flags & HB_G1_DOUBLE ? 1 : 2) || (flags & ~(HB_G1_SUBTRACT | HB_G1_GENERAL | HB_G1_DOUBLE)) || arg) return HB_ERR_BAD_ARG;
        for (int64_t i = 0; i < count; i++) {
            if (!(flags & (HB_G1_GENERAL | HB_G1_DOUBLE))) { g1_add_elem(o + i * G1_PT, U(0) + i * G1_PT, U(1) + i * G1_PT, flags & HB_G1_SUBTRACT, P); continue; }
            // the formulas a kernel reaches only inside a loop, on operands moved off Z = 1: (X, Y, Z) -> (X z^2, Y z^3, Z z)
            auto lift = [&](G1Jac &j, const uint32_t *p, const uint32_t (&z)[QL], bool negate) {
                G1Aff a;
                uint32_t z2[QL];
                g1_load(a, p, P);
                if (negate) fp_neg<QL>(a.y, a.y, P);
                g1_from_affine(j, a, P);
                fq_mul(z2, z, z, P);
                fq_mul(j.X, j.X, z2, P);
                fq_mul(j.Y, j.Y, z2, P);
                fq_mul(j.Y, j.Y, z, P);
                fq_mul(j.Z, j.Z, z, P);
            };
            G1Jac a, b;
            lift(a, U(0) + i * G1_PT, P.r2, false);
            if (flags & HB_G1_DOUBLE) g1_double(a, a, P);
            else {
                uint32_t z[QL];
                fp_add<QL>(z, P.r2, P.one, P);
                lift(b, U(1) + i * G1_PT, z, (flags & HB_G1_SUBTRACT) != 0);
                g1_add(a, b, P);
            }
            g1_store(o + i * G1_PT, a, P);
        }
        return HB_OK;
    }
    case HB_G1_SELFTEST_CHECK: {
        if (!need(1) || flags || arg) return HB_ERR_BAD_ARG;
        for (int64_t i = 0; i < count; i++) reinterpret_cast<int32_t *>(out)[i] = g1_check_elem(U(0) + i * G1_PT, P);
        return HB_OK;
    }
    case HB_G1_SELFTEST_TABLE: {
        if (!need(1) || flags || !g1_window_ok((int)arg) || count != 1) return HB_ERR_BAD_ARG;
        G1Aff a;
        if (!g1_load(a, U(0), P) || a.inf || !g1_on_curve(a, P)) return HB_ERR_BAD_ARG;
        for (int w = 0; w < 256 / (int)arg; w++) g1_table_window(o, U(0), (int)arg, w, P);
        return HB_OK;
    }
    case HB_G1_SELFTEST_COMMIT: {
        if (!need(4) || flags || !g1_window_ok((int)arg)) return HB_ERR_BAD_ARG;
        for (int64_t i = 0; i < count; i++) g1_commit_elem(o + i * G1_PT, U(0) + i * SW, U(1) + i * SW, U(2), U(3), (int)arg, P);
        return HB_OK;
    }
    case HB_G1_SELFTEST_EVAL: {
        if (!need(1) || flags < 1 || arg < 0 || (arg >> 32)) return HB_ERR_BAD_ARG;
        for (int64_t i = 0; i < count; i++) g1_eval_elem(o + i * G1_PT, U(0) + i * flags * G1_PT, flags, (uint32_t)arg, P);
        return HB_OK;
    }
    case HB_G1_SELFTEST_VERIFY: {
        const int n_coef = flags & 0xffff, c = flags >> 16;
        if (!need(5) || n_coef < 1 || !g1_window_ok(c) || arg < 0 || (arg >> 32)) return HB_ERR_BAD_ARG;
        int32_t *v = reinterpret_cast<int32_t *>(out);
        v[count] = 0;
        for (int64_t i = 0; i < count; i++) {
            v[i] = g1_verify_elem(U(0) + i * n_coef * G1_PT, n_coef, (uint32_t)arg, U(1) + i * SW, U(2) + i * SW, U(3), U(4), c, P);
            if (!v[i]) v[count]++;
        }
        return HB_OK;
    }
    default: return HB_ERR_BAD_ARG;
    }
}

}  // extern "C"

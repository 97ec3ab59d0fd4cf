// hb_crs.hip -- the prover of the constant-size (KZG) polynomial commitment of the reference's poly_commit_const.py in BLS12-381 G1:
// commit (:20-27) and create_witness (:29-45) are sums of powers of the FIXED bases of a common reference string, gs[j] = alpha^j g and
// hs[j] = alpha^j h, and HbAvssBatch._get_dealer_msg (hbavss.py:567-598) runs secret_count commits and n secret_count witnesses of them.
// (verify_eval and batch_verify_eval need a pairing -- G2, Fq12 -- and are NOT here.)  Built from the bodies of hb_g1_elem.hpp.
//
//   k_g1_crs_table   the window tables of N bases in one launch: workgroup k builds base k with g1_table_window, a window a lane (W =
//                    256 / c lanes work).  Table k stands at tables + k hb_g1_table_bytes(c) in the single-base layout of hb_g1.hip, its
//                    base behind its scratch: every one of the N tables is also an argument of hb_g1_commit and hb_g1_verify.
//   k_kzg_quotient   synthetic division in Fr, one lane a (polynomial b, point i):  q[t-1] = phi[t];  q[j-1] = phi[j] + x_i q[j],
//                    j = t-1 .. 1;  rem = phi[0] + x_i q[0] = phi_b(x_i): (phi_b(X) - phi_b(x_i)) / (X - x_i) = sum_j q[j] X^j, the
//                    exponents of a witness, and the share (or, from the blinding polynomial, the aux value) out of the same pass.
//                    x_i is kept as a Montgomery residue, so one mont_mul a step returns the canonical product of canonical q[j]: t
//                    products and t additions a lane.  Inputs canonical (below R), outputs canonical.
//   k_g1_crs_msm     out[m] = sum_{k < terms} a[m][k] G_k (+ b[m][k] H_k) from one or two families of tables, F = 1 or 2.  Scalars are
//                    plain 256-bit integers; digit w of a scalar is its byte (c = 8) or nibble (c = 4) w, read from the scalar's word.
//                    A row is U = F terms W units u = (f terms + k) W + w; a unit with a non-zero digit d is one g1_load_entry of entry
//                    (w, d) of base k's table and one complete g1_add_mixed: no doubling anywhere.  S lanes share a row (split), lane s
//                    takes the units [s U / S, (s + 1) U / S) and a workgroup holds 256 / S rows.
//                      S = 1   no LDS, no barrier: k_g1_commit for terms bases a family.
//                      S > 1   each lane parks its Jacobian sum as a tree node in LDS (43 words a node, 43 KB), log2 S tree steps
//                              (msm_tree_step, g1_add) run inside each group of S nodes, the group's first lane stores the affine
//                              result: one inversion a row.  Every lane of the workgroup reaches every barrier: lanes of rows beyond
//                              `rows` and lanes without units hold the identity.
//                    Products a row: 11 U for the additions (2 K W 11 = 15 488 at K = 22, c = 8) + 16 (S - 1) for the tree +
//                    ~640 for the inversion.  At S = 1 the lanes of a wave read the same (base, window) of the tables at the same time.
// 256-thread workgroups (64 for the tables), every lane checked against its count, nothing waits for another workgroup, the caller's
// stream, nothing allocated.  The per-row, quotient and table bodies are HB_HD: hb_selftest_g1_crs runs the very same functions over host
// memory and drives the split path lane by lane with an array in place of LDS.  fq_mul stays the called function (hb_g1_elem.hpp).
// Compiler's report and timings: profiles/g1_crs.txt.
#include <vector>

#include "hb_g1_elem.hpp"

using namespace hb;

namespace hb {

constexpr int RL = 9, RW = 8;                            // Fr digits and words (the four-limb context of R)
constexpr int CRS_WG = 256;
constexpr int CRS_MAX_BASES = 4096;
// split = 0: the smallest power of two S with rows S >= CRS_FILL_LANES, S <= U and S <= 256.  The starting point was one wave a SIMD of an
// MI355X (256 CUs x 4 SIMDs x 64 lanes = 65 536 lanes).  The sweep of profiles/g1_crs.txt (t = 21, window 8, two families) moved it to FOUR
// times that -- the two waves a SIMD these kernels run at, twice over:
//   rows =     16  S = 64: 3.16 ms   S = 256: 1.41 ms                      (the cap; U = 1408)
//   rows =  1 024  S = 64: 3.42 ms   S = 256: 3.18 ms                      (65 536 lanes against 262 144)
//   rows = 65 536  S =  1: 23.4 ms   S = 4: 20.2 ms   S = 16: 29.5 ms      (262 144 lanes again; beyond them the trees only cost)
// Window 4 has its best split at the same places.
constexpr int64_t CRS_FILL_LANES = 262144;

static bool crs_window_ok(int c) { return c == 4 || c == 8; }
static bool crs_split_ok(int S) { return S >= 1 && S <= CRS_WG && (S & (S - 1)) == 0; }
static int crs_auto_split(int64_t rows, int64_t U) {
    int S = 1;
    while (S < CRS_WG && rows * S < CRS_FILL_LANES && 2 * S <= U) S *= 2;
    return S;
}

// ---------------------------------------------------------------- bodies (host and device)
HB_HD void kzg_quotient_elem(uint32_t *q, uint32_t *rem, const uint32_t *phi, const uint32_t *x, int n_coef, const FpParams<RL> &P) {
    uint32_t xm[RL], acc[RL], c[RL], t[RL];
    load_digits<RL, RW>(c, x);
    to_mont(xm, c, P);
    load_digits<RL, RW>(acc, phi + (int64_t)(n_coef - 1) * RW);
#pragma unroll 1
    for (int j = n_coef - 2; j >= 0; j--) {
        store_digits<RL, RW>(q + (int64_t)j * RW, acc);          // q[j] = phi[j + 1] + x q[j + 1]
        mont_mul(t, xm, acc, P);
        load_digits<RL, RW>(c, phi + (int64_t)j * RW);
        fp_add(acc, c, t, P);
    }
    store_digits<RL, RW>(rem, acc);
}
// window digit w of the scalar at s: its byte (c = 8) or nibble (c = 4) w
HB_HD uint32_t crs_digit(const uint32_t *s, int c, int w) { return c == 8 ? (s[w >> 2] >> (8 * (w & 3))) & 255u : (s[w >> 3] >> (4 * (w & 7))) & 15u; }
// acc = the units [u0, u1) of one row: a, b its scalars (b and th unused when every unit lies in the first family)
HB_HD void crs_msm_lane(G1Jac &acc, const uint32_t *tg, const uint32_t *th, int64_t tab_words, int c, const uint32_t *a, const uint32_t *b, int terms, int64_t u0, int64_t u1,
                        const FpParams<QL> &P) {
    const int n = (1 << c) - 1, W = 256 / c;
    g1_set_identity(acc, P);
    int fk = (int)(u0 / W), w = (int)(u0 % W);
#pragma unroll 1
    for (int64_t u = u0; u < u1; u++) {
        const bool second = fk >= terms;
        const int k = second ? fk - terms : fk;
        const uint32_t d = crs_digit((second ? b : a) + (int64_t)k * SW, c, w);
        if (d) {
            G1Aff e;
            g1_load_entry(e, (second ? th : tg) + (int64_t)k * tab_words + ((int64_t)w * n + (d - 1)) * G1_ENT);
            g1_add_mixed(acc, e, P);
        }
        if (++w == W) { w = 0; fk++; }
    }
}
// lane s of S of a row of U units
HB_HD void crs_units(int64_t U, int S, int s, int64_t &u0, int64_t &u1) {
    u0 = (int64_t)s * U / S;
    u1 = (int64_t)(s + 1) * U / S;
}

// ---------------------------------------------------------------- kernels
__global__ void __launch_bounds__(64) k_g1_crs_table(uint32_t *tables, int64_t tab_words, int c) {
    const int w = threadIdx.x;
    if (w >= 256 / c) return;
    const FpParams<QL> P = fq_params();
    uint32_t *table = tables + (int64_t)blockIdx.x * tab_words;
    g1_table_window(table, table + tab_words - G1_SCR, c, w, P);
}
__global__ void __launch_bounds__(256) k_kzg_quotient(const FpParams<RL> P, const uint32_t *phi, int n_coef, const uint32_t *xs, int64_t n_points, uint32_t *q, uint32_t *rem,
                                                      int64_t lanes) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= lanes) return;
    const int64_t b = e / n_points, i = e - b * n_points;
    kzg_quotient_elem(q + e * (n_coef - 1) * RW, rem + e * RW, phi + b * n_coef * RW, xs + i * RW, n_coef, P);
}
template <bool SPLIT>
__global__ void __launch_bounds__(256) k_g1_crs_msm(const uint32_t *tg, const uint32_t *th, int64_t tab_words, int c, const uint32_t *a, const uint32_t *b, int terms, int F,
                                                    int S, uint32_t *out, int64_t rows) {
    const int tid = threadIdx.x, s = tid & (S - 1);
    const int64_t m = ((int64_t)blockIdx.x * CRS_WG + tid) / S;
    if (!SPLIT && m >= rows) return;
    const FpParams<QL> P = fq_params();
    const bool live = m < rows;
    const int64_t row = live ? m : 0;                            // an idle group reads nothing: its lanes get no units
    int64_t u0 = 0, u1 = 0;
    if (live) crs_units((int64_t)F * terms * (256 / c), S, s, u0, u1);
    G1Jac acc;
    crs_msm_lane(acc, tg, th, tab_words, c, a + row * terms * SW, b ? b + row * terms * SW : nullptr, terms, u0, u1, P);
    if constexpr (SPLIT) {
        __shared__ uint32_t nodes[CRS_WG * MSM_NODE];
        msm_node_store(nodes, tid, acc);
        __syncthreads();
#pragma unroll 1
        for (int half = S / 2; half >= 1; half >>= 1) {
            msm_tree_step(nodes + (tid - s) * MSM_NODE, s, half, P);
            __syncthreads();
        }
        if (s != 0 || !live) return;
        msm_node_load(acc, nodes, tid);
    }
    g1_store(out + m * G1_PT, acc, P);
}

// ---------------------------------------------------------------- host side
// the bases as hb_g1_table takes one: 0 fine, 1 an identity, 2 a point off the curve
static int crs_bases_check(const uint32_t *bases, int64_t n, const FpParams<QL> &P) {
    for (int64_t k = 0; k < n; k++) {
        G1Aff a;
        const bool below = g1_load(a, bases + k * G1_PT, P);
        if (a.inf) return 1;
        if (!below || !g1_on_curve(a, P)) return 2;
    }
    return 0;
}
static bool crs_overlap(const void *p, int64_t pbytes, const void *q, int64_t qbytes) {
    const char *a = (const char *)p, *b = (const char *)q;
    return p && q && pbytes > 0 && qbytes > 0 && a < b + qbytes && b < a + pbytes;
}
// a workgroup of k_g1_crs_msm<true> on the host: an array in place of LDS, the lanes one after another between what are barriers on the device
static void crs_host_workgroup(int64_t wg, const uint32_t *tg, const uint32_t *th, int64_t tab_words, int c, const uint32_t *a, const uint32_t *b, int terms, int F, int S,
                               uint32_t *out, int64_t rows, const FpParams<QL> &P) {
    std::vector<uint32_t> nodes(CRS_WG * MSM_NODE);
    for (int tid = 0; tid < CRS_WG; tid++) {
        const int s = tid & (S - 1);
        const int64_t m = (wg * CRS_WG + tid) / S, row = m < rows ? m : 0;
        int64_t u0 = 0, u1 = 0;
        if (m < rows) crs_units((int64_t)F * terms * (256 / c), S, s, u0, u1);
        G1Jac acc;
        crs_msm_lane(acc, tg, th, tab_words, c, a + row * terms * SW, b ? b + row * terms * SW : nullptr, terms, u0, u1, P);
        msm_node_store(nodes.data(), tid, acc);
    }
    for (int half = S / 2; half >= 1; half >>= 1)
        for (int tid = 0; tid < CRS_WG; tid++) msm_tree_step(nodes.data() + (tid - (tid & (S - 1))) * MSM_NODE, tid & (S - 1), half, P);
    for (int tid = 0; tid < CRS_WG; tid += S) {
        const int64_t m = (wg * CRS_WG + tid) / S;
        if (m >= rows) break;
        G1Jac acc;
        msm_node_load(acc, nodes.data(), tid);
        g1_store(out + m * G1_PT, acc, P);
    }
}

}  // namespace hb

extern "C" {

int hb_g1_crs_table(hb_ctx *ctx, const uint64_t *bases_host, int64_t n_bases, int window, void *tables_dev, void *stream) {
    G1_ENTER("hb_g1_crs_table", n_bases, !bases_host || !tables_dev);
    (void)blocks;
    if (!crs_window_ok(window)) return fail(ctx, HB_ERR_BAD_ARG, "hb_g1_crs_table: the window width is 4 or 8");
    if (n_bases > CRS_MAX_BASES) return fail(ctx, HB_ERR_BAD_ARG, "hb_g1_crs_table: at most 4096 bases");
    if (n_bases == 0) return HB_OK;
    const FpParams<QL> P = fq_params();
    const uint32_t *bases = (const uint32_t *)bases_host;
    const int bad = crs_bases_check(bases, n_bases, P);
    if (bad == 1) return fail(ctx, HB_ERR_BAD_ARG, "hb_g1_crs_table: a base is the identity");
    if (bad == 2) return fail(ctx, HB_ERR_BAD_ARG, "hb_g1_crs_table: a base is not on the curve");
    // each base rides behind its table's scratch, as hb_g1_table's does
    const int64_t tab_words = hb_g1_table_bytes(window) / 4;
    uint32_t *tables = (uint32_t *)tables_dev;
    for (int64_t k = 0; k < n_bases; k++)
        HB_HIP(ctx, hipMemcpyAsync(tables + (k + 1) * tab_words - G1_SCR, bases + k * G1_PT, G1_PT * 4, hipMemcpyHostToDevice, s));
    HB_HIP(ctx, hipStreamSynchronize(s));                       // bases_host is the caller's again on return
    k_g1_crs_table<<<(unsigned)n_bases, 64, 0, s>>>(tables, tab_words, window);
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_kzg_quotient(hb_ctx *ctx, const uint64_t *phi_dev, int n_coef, const uint64_t *xs_dev, int64_t n_points, uint64_t *q_dev, uint64_t *rem_dev, int64_t count_polys,
                    void *stream) {
    G1_ENTER("hb_kzg_quotient", count_polys, !phi_dev);
    if (n_points < 0 || (count_polys > 0 && n_points > 0 && (!xs_dev || !rem_dev || (n_coef > 1 && !q_dev))))
        return fail(ctx, HB_ERR_BAD_ARG, "hb_kzg_quotient: a null pointer or a negative count");
    if (n_coef < 1 || n_coef > (1 << 20)) return fail(ctx, HB_ERR_BAD_ARG, "hb_kzg_quotient: between 1 and 2^20 coefficients a polynomial");
    if (n_points > 0 && count_polys > (1LL << 36) / n_points / n_coef) return fail(ctx, HB_ERR_UNSUPPORTED, "hb_kzg_quotient: batch too large for one launch");
    const int64_t lanes = count_polys * n_points, eb = RW * 4;
    const int64_t phi_b = count_polys * n_coef * eb, xs_b = n_points * eb, q_b = lanes * (n_coef - 1) * eb, rem_b = lanes * eb;
    if (crs_overlap(q_dev, q_b, phi_dev, phi_b) || crs_overlap(q_dev, q_b, xs_dev, xs_b) || crs_overlap(rem_dev, rem_b, phi_dev, phi_b) || crs_overlap(rem_dev, rem_b, xs_dev, xs_b) ||
        crs_overlap(q_dev, q_b, rem_dev, rem_b))
        return fail(ctx, HB_ERR_BAD_ARG, "hb_kzg_quotient: an output aliases an input or the other output");
    if (lanes == 0) return HB_OK;
    k_kzg_quotient<<<(unsigned)((lanes + 255) / 256), 256, 0, s>>>(ctx->pw, (const uint32_t *)phi_dev, n_coef, (const uint32_t *)xs_dev, n_points, (uint32_t *)q_dev,
                                                                    (uint32_t *)rem_dev, lanes);
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_g1_crs_msm(hb_ctx *ctx, const void *tg_dev, const void *th_dev, int64_t n_bases, int window, const uint64_t *a_dev, const uint64_t *b_dev, int64_t terms, int split,
                  uint64_t *out_dev, int64_t rows, void *stream) {
    G1_ENTER("hb_g1_crs_msm", rows, !out_dev || (terms > 0 && (!tg_dev || !a_dev)));
    if (rows > 0 && terms > 0 && (th_dev == nullptr) != (b_dev == nullptr)) return fail(ctx, HB_ERR_BAD_ARG, "hb_g1_crs_msm: the second family needs both its tables and its scalars");
    if (!crs_window_ok(window)) return fail(ctx, HB_ERR_BAD_ARG, "hb_g1_crs_msm: the window width is 4 or 8");
    if (n_bases < 0 || n_bases > CRS_MAX_BASES || terms < 0 || terms > n_bases) return fail(ctx, HB_ERR_BAD_ARG, "hb_g1_crs_msm: 0 <= terms <= n_bases <= 4096");
    if (split != 0 && !crs_split_ok(split)) return fail(ctx, HB_ERR_BAD_ARG, "hb_g1_crs_msm: split is 0 (the library's rule) or a power of two in [1, 256]");
    const int64_t tab_bytes = hb_g1_table_bytes(window), out_b = rows * G1_PT * 4, sc_b = rows * terms * SW * 4;
    if (crs_overlap(out_dev, out_b, a_dev, sc_b) || crs_overlap(out_dev, out_b, b_dev, sc_b) || crs_overlap(out_dev, out_b, tg_dev, n_bases * tab_bytes) ||
        crs_overlap(out_dev, out_b, th_dev, n_bases * tab_bytes))
        return fail(ctx, HB_ERR_BAD_ARG, "hb_g1_crs_msm: out aliases an input");
    if (rows == 0) return HB_OK;
    if (terms == 0) {
        HB_HIP(ctx, hipMemsetAsync(out_dev, 0, out_b, s));
        return HB_OK;
    }
    const int F = th_dev ? 2 : 1;
    const int S = split ? split : crs_auto_split(rows, (int64_t)F * terms * (256 / window));
    const int64_t wgs = (rows * S + CRS_WG - 1) / CRS_WG;
    if (wgs > 0x7fffffffLL) return fail(ctx, HB_ERR_UNSUPPORTED, "hb_g1_crs_msm: batch too large for one launch");
    if (S == 1)
        k_g1_crs_msm<false><<<(unsigned)wgs, 256, 0, s>>>((const uint32_t *)tg_dev, (const uint32_t *)th_dev, tab_bytes / 4, window, (const uint32_t *)a_dev, (const uint32_t *)b_dev,
                                                         (int)terms, F, 1, (uint32_t *)out_dev, rows);
    else
        k_g1_crs_msm<true><<<(unsigned)wgs, 256, 0, s>>>((const uint32_t *)tg_dev, (const uint32_t *)th_dev, tab_bytes / 4, window, (const uint32_t *)a_dev, (const uint32_t *)b_dev,
                                                        (int)terms, F, S, (uint32_t *)out_dev, rows);
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_selftest_g1_crs(int what, const uint64_t *const *operands, int flags, int64_t arg, uint64_t *out, int64_t count) {
    if (!operands || count < 0 || !out || !g1_consts_ok()) return HB_ERR_BAD_ARG;
    const FpParams<QL> P = fq_params();
    auto U = [&](int k) { return reinterpret_cast<const uint32_t *>(operands[k]); };
    uint32_t *o = reinterpret_cast<uint32_t *>(out);
    switch (what) {
    case HB_G1_CRS_SELFTEST_TABLE: {
        const int c = (int)arg;
        if (!operands[0] || flags || !crs_window_ok(c) || count > CRS_MAX_BASES) return HB_ERR_BAD_ARG;
        if (crs_bases_check(U(0), count, P)) return HB_ERR_BAD_ARG;
        const int64_t tab_words = hb_g1_table_bytes(c) / 4;
        for (int64_t k = 0; k < count; k++) {
            for (int w = 0; w < 256 / c; w++) g1_table_window(o + k * tab_words, U(0) + k * G1_PT, c, w, P);   // (the base's place behind the scratch is left alone)
        }
        return HB_OK;
    }
    case HB_G1_CRS_SELFTEST_QUOTIENT: {
        // flags = n_coef, arg = n_points, count = polynomials; out = q (count * n_points * (n_coef - 1) elements), then rem
        const int n_coef = flags;
        const int64_t n = arg;
        if (!operands[0] || n_coef < 1 || n < 0 || (n > 0 && !operands[1])) return HB_ERR_BAD_ARG;
        FpParams<RL> PR;
        fp_params_from_limbs(PR, G1_ORDER);
        uint32_t *rem = o + count * n * (n_coef - 1) * RW;
        for (int64_t e = 0; e < count * n; e++)
            kzg_quotient_elem(o + e * (n_coef - 1) * RW, rem + e * RW, U(0) + (e / n) * n_coef * RW, U(1) + (e % n) * RW, n_coef, PR);
        return HB_OK;
    }
    case HB_G1_CRS_SELFTEST_MSM: {
        // operands = tables of G, tables of H or null, a, b or null; flags = window | split << 8 (0: the rule); arg = terms | n_bases << 32
        const int c = flags & 255, split = flags >> 8;
        const int64_t terms = arg & 0xffffffffLL, n_bases = arg >> 32;
        if (!crs_window_ok(c) || (split != 0 && !crs_split_ok(split)) || n_bases < 0 || n_bases > CRS_MAX_BASES || terms > n_bases) return HB_ERR_BAD_ARG;
        if (terms > 0 && count > 0 && ((operands[1] == nullptr) != (operands[3] == nullptr) || !operands[0] || !operands[2])) return HB_ERR_BAD_ARG;
        if (terms == 0) {
            memset(o, 0, count * G1_PT * 4);
            return HB_OK;
        }
        const int F = operands[1] ? 2 : 1;
        const int S = split ? split : crs_auto_split(count, (int64_t)F * terms * (256 / c));
        const int64_t tab_words = hb_g1_table_bytes(c) / 4;
        if (S == 1) {
            for (int64_t m = 0; m < count; m++) {
                G1Jac acc;
                crs_msm_lane(acc, U(0), U(1), tab_words, c, U(2) + m * terms * SW, F == 2 ? U(3) + m * terms * SW : nullptr, (int)terms, 0, (int64_t)F * terms * (256 / c), P);
                g1_store(o + m * G1_PT, acc, P);
            }
            return HB_OK;
        }
        for (int64_t wg = 0; wg < (count * S + CRS_WG - 1) / CRS_WG; wg++) crs_host_workgroup(wg, U(0), U(1), tab_words, c, U(2), U(3), (int)terms, F, S, o, count, P);
        return HB_OK;
    }
    default: return HB_ERR_BAD_ARG;
    }
}

}  // extern "C"

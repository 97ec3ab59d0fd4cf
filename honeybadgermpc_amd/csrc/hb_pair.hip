// hb_pair.hip -- products of BLS12-381 pairings against PREPARED G2 points: the verifier's half of the KZG commitment
// (poly_commit_const.py).  Both G2 arguments of a check are fixed by the CRS, so their line coefficients are computed once on the host
// (bls12_381_pairing.prepare_g2) and the device does no G2 arithmetic: it needs the tower of hb_fq12_elem.hpp, a Miller loop that reads
// the lines, and the final exponentiation.
//
//   out[m] = FE(prod_k ML(P[m][k], Q_k)),  k < K <= 4,  Q_k a prepared table shared by every item
//
// The loop is the reference's: for each bit of |x| / 2 below the leading one, the K lines are folded into f by fq12_mul_by_014, a set
// bit folds K more, then one squaring; a last round of lines; conjugation (x < 0); the final exponentiation by the reference's chain,
// which is the power 3 (Q^12 - 1) / R.  An identity P[m][k] contributes 1 (its lines are skipped).
//
// Table layout (the library's own): 68 entries of three Fq2 (the crate's coeffs.0, .1, .2), each 2 x 14 Montgomery digits: 84 words an
// entry, 22 848 bytes a point.  The entry's address depends on the loop counter alone.
//
// Products of Fq an item (hb_fq12_elem.hpp counts the bodies): the loop 68 K lines of 43 and 62 squarings of 36 = 2 924 K + 2 232
// (K = 2: 8 080); the final exponentiation 5 powers by |x| (63 cyclotomic squarings of 18 and 5 products: 1 404 each; |x| / 2 one
// squaring less), 10 products, 4 Frobenius maps, one squaring and one inversion (72 + 33 + 4 + about 570): about 8 350.  With the
// plain complex squaring in the powers it was about 14 000.
//
// One lane an item, 64 lanes a workgroup.  An Fq12 is 168 words; the loop holds one, the final exponentiation five, and the Fq12
// products are real calls (hb_fq12_elem.hpp), so these values live in private memory.  DESIGN 3x has the compiler's figures.
//
// k_pair_op (hb_debug_pair_op, hbmpc_hip_debug.h) is the tests' door to the same bodies: ONE tower or Fq operation a launch on the
// caller's operands (pair_tower_elem, which the self test's tower case runs on the host), same geometry, a status an item.
#include "hb_fq12_elem.hpp"

using namespace hb;

namespace hb {

constexpr int PAIR_WG = 64;

__global__ void __launch_bounds__(PAIR_WG) k_pair_product(const uint32_t *__restrict__ t0, const uint32_t *__restrict__ t1, const uint32_t *__restrict__ t2,
                                                           const uint32_t *__restrict__ t3, int K, const uint32_t *__restrict__ points, int mode, uint32_t *out,
                                                           int32_t *verdict, int32_t *rejected, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * PAIR_WG + threadIdx.x;
    if (i >= count) return;
    const FpParams<QL> P = fq_params();
    const PairTables T = {{t0, t1, t2, t3}};
    Fq12E f;
    const bool ok = pair_product_elem(f, T, K, points + i * K * G1_PT, P);
    if (mode == HB_PAIR_GT) fq12_store(out + i * GT_WORDS, f, P);
    else {
        const int32_t v = (ok && fq12_is_one(f, P)) ? 1 : 0;
        verdict[i] = v;
        if (!v) atomicAdd(rejected, 1);
    }
}

// One operation of the tower on given operands (hb_debug_pair_op): load, pair_tower_elem, store.  `two` and the validity of op and arg
// are the host's; a lane whose residues are not all below Q computes on the reduced words, as k_pair_product does, and stores zeros.
__global__ void __launch_bounds__(PAIR_WG) k_pair_op(int op, int64_t arg, int two, const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, uint32_t *__restrict__ out,
                                                      int32_t *__restrict__ status, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * PAIR_WG + threadIdx.x;
    if (i >= count) return;
    const FpParams<QL> P = fq_params();
    Fq12E x, y, r;
    bool ok = fq12_load(x, a + i * GT_WORDS, P);
    if (two) ok = fq12_load(y, b + i * GT_WORDS, P) && ok;
    else fq12_set(y, x);
    ok = pair_tower_elem(r, x, y, op, arg, P) && ok;
    if (ok) fq12_store(out + i * GT_WORDS, r, P);
    else {
        const uint32_t z[QW] = {};
#pragma unroll
        for (int k = 0; k < 12; k++) store_words<QW>(out + i * GT_WORDS + k * QW, z);
    }
    status[i] = ok ? 1 : 0;
}

static bool pair_overlap(const void *a, int64_t na, const void *b, int64_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + (uintptr_t)nb && y < x + (uintptr_t)na;
}

}  // namespace hb

extern "C" {

int64_t hb_pair_table_bytes(void) { return (int64_t)PAIR_TABLE * 4; }

int hb_pair_prepare(hb_ctx *ctx, const uint64_t *coeffs_host, int64_t n_coeffs, void *table_dev, void *stream) {
    const int64_t one = 1;
    G1_ENTER("hb_pair_prepare", one, !coeffs_host || !table_dev);
    (void)blocks;
    if (!pair_consts_ok()) return fail(ctx, HB_ERR_UNSUPPORTED, "hb_pair_prepare: the Frobenius constants do not derive from Q");
    if (n_coeffs != PAIR_LINES * 3) return fail(ctx, HB_ERR_BAD_ARG, "hb_pair_prepare: a prepared point has 68 coefficient triples");
    std::vector<uint32_t> table(PAIR_TABLE);
    if (!pair_table_fill(table.data(), (const uint32_t *)coeffs_host)) return fail(ctx, HB_ERR_BAD_ARG, "hb_pair_prepare: a coefficient is not below Q");
    HB_HIP(ctx, hipMemcpyAsync(table_dev, table.data(), (size_t)PAIR_TABLE * 4, hipMemcpyHostToDevice, s));
    HB_HIP(ctx, hipStreamSynchronize(s));
    return HB_OK;
}

int hb_pair_product(hb_ctx *ctx, const void *const *tables_dev, int K, const uint64_t *points_dev, int mode, uint64_t *out_dev, int32_t *flags_dev, int32_t *rejected_dev,
                    int64_t count, void *stream) {
    HB_API_GUARD(ctx);
    { const int rc = g1_ctx_ok(ctx, "hb_pair_product"); if (rc != HB_OK) return rc; }
    if (!pair_consts_ok()) return fail(ctx, HB_ERR_UNSUPPORTED, "hb_pair_product: the Frobenius constants do not derive from Q");
    if (K < 1 || K > 4) return fail(ctx, HB_ERR_BAD_ARG, "hb_pair_product: between 1 and 4 pairs an item");
    if (mode != HB_PAIR_GT && mode != HB_PAIR_VERDICT) return fail(ctx, HB_ERR_BAD_ARG, "hb_pair_product: mode is HB_PAIR_GT or HB_PAIR_VERDICT");
    if (count < 0 || !tables_dev) return fail(ctx, HB_ERR_BAD_ARG, "hb_pair_product: a null pointer or a negative count");
    for (int k = 0; k < K; k++) if (!tables_dev[k]) return fail(ctx, HB_ERR_BAD_ARG, "hb_pair_product: a prepared table is missing");
    if (count > 0 && (!points_dev || (mode == HB_PAIR_GT ? !out_dev : (!flags_dev || !rejected_dev))))
        return fail(ctx, HB_ERR_BAD_ARG, "hb_pair_product: a null pointer or a negative count");
    if (count > (INT64_MAX >> 20) || (count + PAIR_WG - 1) / PAIR_WG > 0x7fffffffLL) return fail(ctx, HB_ERR_UNSUPPORTED, "hb_pair_product: batch too large for one launch");
    if (count == 0) return HB_OK;
    const int64_t in_bytes = count * K * G1_PT * 4;
    const void *o = mode == HB_PAIR_GT ? (const void *)out_dev : (const void *)flags_dev;
    const int64_t o_bytes = mode == HB_PAIR_GT ? count * GT_WORDS * 4 : count * 4;
    bool clash = pair_overlap(o, o_bytes, points_dev, in_bytes);
    if (mode == HB_PAIR_VERDICT) clash = clash || pair_overlap(rejected_dev, 4, points_dev, in_bytes) || pair_overlap(rejected_dev, 4, flags_dev, o_bytes);
    for (int k = 0; k < K; k++) {
        clash = clash || pair_overlap(o, o_bytes, tables_dev[k], (int64_t)PAIR_TABLE * 4);
        if (mode == HB_PAIR_VERDICT) clash = clash || pair_overlap(rejected_dev, 4, tables_dev[k], (int64_t)PAIR_TABLE * 4);
    }
    if (clash) return fail(ctx, HB_ERR_BAD_ARG, "hb_pair_product: an output overlaps an input");
    hipStream_t s = (hipStream_t)stream;
    const uint32_t *t[4];
    for (int k = 0; k < 4; k++) t[k] = (const uint32_t *)tables_dev[k < K ? k : 0];
    k_pair_product<<<(unsigned)((count + PAIR_WG - 1) / PAIR_WG), PAIR_WG, 0, s>>>(t[0], t[1], t[2], t[3], K, (const uint32_t *)points_dev, mode, (uint32_t *)out_dev, flags_dev,
                                                                                    rejected_dev, count);
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

// hbmpc_hip_debug.h: one tower or Fq operation on the device at the caller's operands; the checks are hb_pair_product's
int hb_debug_pair_op(hb_ctx *ctx, int op, int64_t arg, const uint64_t *a_dev, const uint64_t *b_dev, uint64_t *out_dev, int32_t *status_dev, int64_t count, void *stream) {
    HB_API_GUARD(ctx);
    { const int rc = g1_ctx_ok(ctx, "hb_debug_pair_op"); if (rc != HB_OK) return rc; }
    if (!pair_consts_ok()) return fail(ctx, HB_ERR_UNSUPPORTED, "hb_debug_pair_op: the Frobenius constants do not derive from Q");
    if (op < 0 || op > HB_PAIR_OP_FQ_INV || !pair_op_arg_ok(op, arg)) return fail(ctx, HB_ERR_BAD_ARG, "hb_debug_pair_op: an unknown operation or an arg it does not take");
    const bool two = pair_op_two(op);
    if (count < 0 || (count > 0 && (!a_dev || (two && !b_dev) || !out_dev || !status_dev))) return fail(ctx, HB_ERR_BAD_ARG, "hb_debug_pair_op: a null pointer or a negative count");
    if (count > (INT64_MAX >> 20) || (count + PAIR_WG - 1) / PAIR_WG > 0x7fffffffLL) return fail(ctx, HB_ERR_UNSUPPORTED, "hb_debug_pair_op: batch too large for one launch");
    if (count == 0) return HB_OK;
    if ((((uintptr_t)a_dev | (uintptr_t)(two ? b_dev : nullptr) | (uintptr_t)out_dev) & 15u) || ((uintptr_t)status_dev & 3u))
        return fail(ctx, HB_ERR_BAD_ARG, "hb_debug_pair_op: the operands and the output must be aligned to 16 bytes");
    const int64_t bytes = count * GT_WORDS * 4;
    bool clash = pair_overlap(out_dev, bytes, a_dev, bytes) || pair_overlap(status_dev, count * 4, a_dev, bytes) || pair_overlap(status_dev, count * 4, out_dev, bytes);
    if (two) clash = clash || pair_overlap(out_dev, bytes, b_dev, bytes) || pair_overlap(status_dev, count * 4, b_dev, bytes);
    if (clash) return fail(ctx, HB_ERR_BAD_ARG, "hb_debug_pair_op: an output overlaps an input or the other output");
    k_pair_op<<<(unsigned)((count + PAIR_WG - 1) / PAIR_WG), PAIR_WG, 0, (hipStream_t)stream>>>(op, arg, two ? 1 : 0, (const uint32_t *)a_dev, (const uint32_t *)(two ? b_dev : a_dev),
                                                                                                 (uint32_t *)out_dev, status_dev, count);
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_selftest_pairing(int what, const uint64_t *const *operands, int flags, int64_t arg, uint64_t *out, int64_t count) {
    if (!operands || count < 0 || !out || !pair_consts_ok()) return HB_ERR_BAD_ARG;
    const FpParams<QL> P = fq_params();
    auto U = [&](int k) { return reinterpret_cast<const uint32_t *>(operands[k]); };
    auto need = [&](int n) { for (int k = 0; k < n; k++) if (!operands[k]) return false; return true; };
    uint32_t *o = reinterpret_cast<uint32_t *>(out);
    switch (what) {
    case HB_PAIR_SELFTEST_TOWER: {
        // operands[0..1] = a, b: Fq12 elements, twelve residues each; an operation on a smaller field takes the leading coordinates and
        // copies the rest of a through; flags also takes the Fq operations of hbmpc_hip_debug.h (pair_tower_elem, which k_pair_op runs too)
        const bool two = pair_op_two(flags);
        if (!need(two ? 2 : 1) || !pair_op_arg_ok(flags, arg)) return HB_ERR_BAD_ARG;
        for (int64_t i = 0; i < count; i++) {
            Fq12E a, b, r;
            if (!fq12_load(a, U(0) + i * GT_WORDS, P)) return HB_ERR_BAD_ARG;
            if (two) { if (!fq12_load(b, U(1) + i * GT_WORDS, P)) return HB_ERR_BAD_ARG; }
            else fq12_set(b, a);
            if (!pair_tower_elem(r, a, b, flags, arg, P)) return HB_ERR_BAD_ARG;
            fq12_store(o + i * GT_WORDS, r, P);
        }
        return HB_OK;
    }
    case HB_PAIR_SELFTEST_PREPARE: {
        if (!need(1) || flags || arg || count != 1) return HB_ERR_BAD_ARG;
        return pair_table_fill(o, U(0)) ? HB_OK : HB_ERR_BAD_ARG;
    }
    case HB_PAIR_SELFTEST_PRODUCT: {
        // operands[0] = points (count, K, 12 words), operands[1..K] = tables; flags = K; arg = mode
        const int K = flags;
        if (K < 1 || K > 4 || !need(K + 1) || (arg != HB_PAIR_GT && arg != HB_PAIR_VERDICT)) return HB_ERR_BAD_ARG;
        PairTables T;
        for (int k = 0; k < 4; k++) T.t[k] = U(1 + (k < K ? k : 0));
        int32_t *v = reinterpret_cast<int32_t *>(out);
        if (arg == HB_PAIR_VERDICT) v[count] = 0;
        for (int64_t i = 0; i < count; i++) {
            Fq12E f;
            const bool ok = pair_product_elem(f, T, K, U(0) + i * K * G1_PT, P);
            if (arg == HB_PAIR_GT) fq12_store(o + i * GT_WORDS, f, P);
            else {
                v[i] = (ok && fq12_is_one(f, P)) ? 1 : 0;
                if (!v[i]) v[count]++;
            }
        }
        return HB_OK;
    }
    default: return HB_ERR_BAD_ARG;
    }
}

}  // extern "C"

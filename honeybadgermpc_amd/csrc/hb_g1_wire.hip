// hb_g1_wire.hip -- G1 points as they arrive from another party: the 48-byte compressed encoding of the reference's Rust crate (the
// format of G1.__getstate__ / __setstate__ in betterpairing.py, pinned by the crate's test vectors) unpacked and packed on the device,
// and membership in the subgroup of order R decided by the curve's endomorphism where g1.in_subgroup pays a full-width scalar
// multiplication.  Built from the bodies of hb_g1_elem.hpp; the bodies here are in hb_g1_wire_elem.hpp.
//
// Square root.  Q = 3 mod 4, so y = a^((Q + 1) / 4) is a root of a whenever a has one, and y^2 == a tells.  The exponent has 379 bits,
//   229 of them set.  The host derives ONE sliding-window schedule of width 3 from it (the odd powers a, a^3, a^5, a^7 in registers,
//   picked by chains of selects on a wave-uniform index, as hb_legendre of hb_eq.hip): 4 products for the table, 377 squarings and 106
//   products for the power (106 steps, 9 squarings in the longest), one squaring for the test: 488 products, the same in every lane.
//   Width 4 would save some twenty products and hold 4 x 14 more registers.
// Membership.  phi(x, y) = (beta x, y), beta a cube root of unity in Fq, acts on the subgroup of order R as multiplication by an
//   eigenvalue lambda with lambda = -x^2 mod R for the curve's parameter x = -0xd201000000010000, and phi(P) = -[x^2] P holds for NO
//   point of the curve outside that subgroup (Scott, eprint 2021/1130, section 6; El Housni, Guillevic and Piellard, eprint 2022/352).
//   [x]([x] P) is two left-to-right double-and-add passes over the 64-bit constant (Hamming weight 6: 63 doublings and 5 complete
//   Jacobian additions each), Jacobian throughout; the comparison is cross-multiplied (beta x Z^2 == X, y Z^3 == -Y, Z != 0): no
//   inversion.  The additions are g1_add_base: g1_add's formulas ordered so that the accumulator's X and Y die before the base's side
//   is computed (nine field elements live at the peak, not twelve: two waves a SIMD for k_g1_subgroup where g1_add left one).
//   2 (63 x 7 + 5 x 16) + 6 = 1048 products against the 3805 of a multiplication by R with its inversion
//   (profiles/g1.txt).  Of the two non-trivial cube roots of unity only one matches -x^2: the load-time check on the generator tells them apart.
// Encoding.  Big-endian x in 48 bytes; in byte 0: 0x80 compressed (always), 0x40 the identity (x = 0, no sign), 0x20 y > (Q - 1) / 2.
//   The statuses follow the host model's checks in their order (bls12_381.G1.decompress), the first failed one wins.
//
// Kernels: 256-thread workgroups, one item a lane, grid = ceil(count / 256), no LDS, every lane checked against count, nothing waits for
// another workgroup, the caller's stream.  An encoding is read as three dwordx4 and a point written as six.
//   k_g1_subgroup     flag_i = hb_g1_check's test and (identity or phi(P_i) == -[x^2] P_i)
//   k_g1_decompress   bytes -> words -> digits -> Montgomery; rhs = x^3 + 4; y = rhs^((Q + 1) / 4); the sign; with check_subgroup the
//                     body of k_g1_subgroup on the point in registers; x and y back to canonical words (after the test: they are not
//                     held across it); status_i, the point or zeros, rejected items counted (atomicAdd).
//                     Every lane runs the whole chain whatever its flags say: the loops are wave-uniform.
//   k_g1_compress     words -> bytes and two comparisons: no field product
//   k_g1_wire_op      hb_debug_g1_wire_op (hbmpc_hip_debug.h): the bare root (wire_sqrt_elem) or phi (g1_phi_elem) on the caller's operands,
//                     the per-item functions of the self test's SQRT and PHI cases: for the tests
// Compiler's report and timings: profiles/g1_wire.txt.
#include "hb_g1_wire_elem.hpp"
#include "../../include/hbmpc_hip_debug.h"

using namespace hb;

namespace hb {

// ---------------------------------------------------------------- kernels
__global__ void __launch_bounds__(256) k_g1_subgroup(const WireConsts K, const uint32_t *p, int32_t *flags, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const FpParams<QL> P = fq_params();
    flags[i] = g1_subgroup_elem(p + i * G1_PT, K, P);
}
__global__ void __launch_bounds__(256) k_g1_decompress(const WireConsts K, const uint32_t *enc, int check_subgroup, uint32_t *out, int32_t *status, int32_t *rejected,
                                                       int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const FpParams<QL> P = fq_params();
    const int32_t st = g1_decompress_elem(out + i * G1_PT, enc + i * G1_ENC_WORDS, check_subgroup, K, P);
    status[i] = st;
    if (st) atomicAdd(rejected, 1);
}
__global__ void __launch_bounds__(256) k_g1_compress(const WireConsts K, const uint32_t *p, uint32_t *enc, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    g1_compress_elem(enc + i * G1_ENC_WORDS, p + i * G1_PT, K);
}

// the bare root or phi on given operands (hb_debug_g1_wire_op): the per-item functions of the self test's SQRT and PHI cases
__global__ void __launch_bounds__(256) k_g1_wire_op(const WireConsts K, int what, const uint32_t *__restrict__ in, uint32_t *__restrict__ out, int32_t *__restrict__ flags,
                                                    int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const FpParams<QL> P = fq_params();
    if (what == HB_G1_WIRE_SELFTEST_SQRT) {
        const int32_t f = wire_sqrt_elem(out + i * QW, in + i * QW, K, P);
        if (f < 0) {
            const uint32_t z[QW] = {};
            store_words<QW>(out + i * QW, z);
        }
        flags[i] = f;
    } else g1_phi_elem(out + i * G1_PT, in + i * G1_PT, K, P);
}

// ---------------------------------------------------------------- host side
// beta, the cube root of unity with phi(P) = -[x^2] P on the subgroup, and the generator the load-time check runs on
static const uint32_t WIRE_BETA[QW] = {0xfffefffeu, 0x2e01ffffu, 0x620a0002u, 0xde17d813u, 0xe6f89688u, 0xddb3a93bu, 0x6a0f77eau, 0xba69c607u, 0xdf76ce51u, 0x5f19672fu, 0u, 0u};
alignas(16) static const uint64_t WIRE_GEN[12] = {0xfb3af00adb22c6bbull, 0x6c55e83ff97a1aefull, 0xa14e3a3f171bac58ull, 0xc3688c4f9774b905ull, 0x2695638c4fa9ac0full, 0x17f1d3a73197d794ull,
                                                  0x0caa232946c5e7e1ull, 0xd03cc744a2888ae4ull, 0x00db18cb2c04b3edull, 0xfcf5e095d5d00af6ull, 0xa09e30ed741d8ae4ull, 0x08b3f481e3aaa0f1ull};

// the sliding-window schedule of the exponent in e's words (eq_make_sched of hb_eq.hip, over twelve words)
static bool wire_make_sched(WireSched &S, const uint32_t (&e)[QW]) {
    auto bit = [&](int i) { return (e[i >> 5] >> (i & 31)) & 1u; };
    int top = 32 * QW - 1;
    while (top >= 0 && !bit(top)) top--;
    if (top < 0) return false;
    S.first = 0;
    S.n = 0;
    bool started = false;
    uint32_t pending = 0;
    auto push = [&](uint32_t nsq, uint32_t m) {
        if (S.n >= (uint32_t)WIRE_MAX_STEPS || nsq > 255u) return false;
        S.step[S.n++] = (uint16_t)(nsq << 8 | m);
        return true;
    };
    for (int i = top; i >= 0;) {
        if (!bit(i)) { pending++; i--; continue; }
        int l = i - WIRE_WINDOW + 1 > 0 ? i - WIRE_WINDOW + 1 : 0;
        while (!bit(l)) l++;
        uint32_t v = 0;
        for (int b = i; b >= l; b--) v = (v << 1) | bit(b);
        if (!started) { S.first = (v - 1) / 2; started = true; }
        else if (!push(pending + (uint32_t)(i - l + 1), (v - 1) / 2 + 1)) return false;
        pending = 0;
        i = l - 1;
    }
    if (pending && !push(pending, 0)) return false;
    for (uint32_t s = S.n; s < (uint32_t)WIRE_MAX_STEPS; s++) S.step[s] = 0;
    return true;
}
// (Q + 1) / 4 and (Q - 1) / 2 from Q's words by shifts; beta and the schedule checked by what they must satisfy
static bool g1_wire_derive(WireConsts &K) {
    if (!g1_consts_ok()) return false;
    static const uint32_t qm2[QW] = G1_QM2_WORDS;
    const FpParams<QL> P = fq_params();
    uint32_t q1[QW], e[QW], h[QW], bw[QW];
    for (int i = 0; i < QW; i++) q1[i] = qm2[i];
    if ((q1[0] & 0xffu) != 0xa9u) return false;                 // Q - 2 ends in ...a9: neither step below carries
    q1[0] += 3;                                                 // Q + 1
    for (int i = 0; i < QW; i++) e[i] = (q1[i] >> 2) | (i + 1 < QW ? q1[i + 1] << 30 : 0u);
    for (int i = 0; i < QW; i++) if (((e[i] << 2) | (i ? e[i - 1] >> 30 : 0u)) != q1[i]) return false;   // 4 e == Q + 1
    if (e[QW - 1] >> 30) return false;
    q1[0] -= 2;                                                 // Q - 1
    for (int i = 0; i < QW; i++) h[i] = (q1[i] >> 1) | (i + 1 < QW ? q1[i + 1] << 31 : 0u);
    unpack<QL, QW>(K.half, h);
    if (!wire_make_sched(K.S, e)) return false;
    // beta^3 == 1, beta != 1
    uint32_t b2[QL], b3[QL];
    for (int i = 0; i < QW; i++) bw[i] = WIRE_BETA[i];
    unpack<QL, QW>(b2, bw);
    if (!fq_below_q(b2, P)) return false;
    fq_to_mont(K.beta, b2, P);
    fq_mul(b2, K.beta, K.beta, P);
    fq_mul(b3, b2, K.beta, P);
    if (!fp_eq<QL>(b3, P.one) || fp_eq<QL>(K.beta, P.one)) return false;
    // phi(G) == -[x^2] G: this beta and not its square
    G1Aff g;
    if (!g1_load(g, reinterpret_cast<const uint32_t *>(WIRE_GEN), P) || g.inf || !g1_on_curve(g, P) || !g1_endo_member(g, K.beta, P)) return false;
    // the schedule: sqrt(4) == +-2
    uint32_t two[QL], four[QL], y[QL], ny[QL];
    fp_add<QL>(two, P.one, P.one, P);
    fp_add<QL>(four, two, two, P);
    if (!fq_sqrt(y, four, K.S, P)) return false;
    fp_neg<QL>(ny, y, P);
    return fp_eq<QL>(y, two) || fp_eq<QL>(ny, two);
}
static const WireConsts *g1_wire_consts() {
    static WireConsts K;
    static const bool ok = g1_wire_derive(K);
    return ok ? &K : nullptr;
}
static bool wire_aligned(const void *p) { return ((uintptr_t)p & 15u) == 0; }
static bool wire_overlap(const void *p, int64_t pbytes, const void *q, int64_t qbytes) {
    const char *a = (const char *)p, *b = (const char *)q;
    return pbytes > 0 && qbytes > 0 && a < b + qbytes && b < a + pbytes;
}

}  // namespace hb

#define G1_WIRE_ENTER(name, count, nullcheck)                                                                         \
    G1_ENTER(name, count, nullcheck);                                                                                 \
    const WireConsts *K = g1_wire_consts();                                                                           \
    if (!K) return fail(ctx, HB_ERR_UNSUPPORTED, name ": the exponent of the square root or beta fails its check against Q")

extern "C" {

int hb_g1_subgroup(hb_ctx *ctx, const uint64_t *p_dev, int32_t *flags_dev, int64_t count, void *stream) {
    G1_WIRE_ENTER("hb_g1_subgroup", count, !p_dev || !flags_dev);
    if (wire_overlap(flags_dev, count * 4, p_dev, count * G1_PT * 4)) return fail(ctx, HB_ERR_BAD_ARG, "hb_g1_subgroup: the flags overlap the points");
    if (count == 0) return HB_OK;
    k_g1_subgroup<<<blocks, 256, 0, s>>>(*K, (const uint32_t *)p_dev, flags_dev, count);
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_g1_decompress(hb_ctx *ctx, const void *bytes_dev, int check_subgroup, uint64_t *out_dev, int32_t *status_dev, int32_t *rejected_dev, int64_t count, void *stream) {
    G1_WIRE_ENTER("hb_g1_decompress", count, !bytes_dev || !out_dev || !status_dev);
    if (!rejected_dev) return fail(ctx, HB_ERR_BAD_ARG, "hb_g1_decompress: the counter is missing");
    if (!wire_aligned(bytes_dev) || !wire_aligned(out_dev)) return fail(ctx, HB_ERR_BAD_ARG, "hb_g1_decompress: the bytes and the points must be aligned to 16 bytes");
    const int64_t enc_b = count * G1_ENC_WORDS * 4, out_b = count * G1_PT * 4;
    if (wire_overlap(out_dev, out_b, bytes_dev, enc_b) || wire_overlap(status_dev, count * 4, bytes_dev, enc_b) || wire_overlap(status_dev, count * 4, out_dev, out_b) ||
        wire_overlap(rejected_dev, 4, bytes_dev, enc_b) || wire_overlap(rejected_dev, 4, out_dev, out_b) || wire_overlap(rejected_dev, 4, status_dev, count * 4))
        return fail(ctx, HB_ERR_BAD_ARG, "hb_g1_decompress: an output overlaps the input or another output");
    if (count == 0) return HB_OK;
    k_g1_decompress<<<blocks, 256, 0, s>>>(*K, (const uint32_t *)bytes_dev, check_subgroup != 0, (uint32_t *)out_dev, status_dev, rejected_dev, count);
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_g1_compress(hb_ctx *ctx, const uint64_t *p_dev, void *bytes_dev, int64_t count, void *stream) {
    G1_WIRE_ENTER("hb_g1_compress", count, !p_dev || !bytes_dev);
    if (!wire_aligned(bytes_dev) || !wire_aligned(p_dev)) return fail(ctx, HB_ERR_BAD_ARG, "hb_g1_compress: the points and the bytes must be aligned to 16 bytes");
    if (wire_overlap(bytes_dev, count * G1_ENC_WORDS * 4, p_dev, count * G1_PT * 4)) return fail(ctx, HB_ERR_BAD_ARG, "hb_g1_compress: the bytes overlap the points");
    if (count == 0) return HB_OK;
    k_g1_compress<<<blocks, 256, 0, s>>>(*K, (const uint32_t *)p_dev, (uint32_t *)bytes_dev, count);
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

// hbmpc_hip_debug.h: the bare square root or phi on the device at the caller's operands
int hb_debug_g1_wire_op(hb_ctx *ctx, int what, const uint64_t *in_dev, uint64_t *out_dev, int32_t *flags_dev, int64_t count, void *stream) {
    const bool root = what == HB_G1_WIRE_SELFTEST_SQRT;
    G1_WIRE_ENTER("hb_debug_g1_wire_op", count, !in_dev || !out_dev || (root && !flags_dev));
    if (!root && what != HB_G1_WIRE_SELFTEST_PHI) return fail(ctx, HB_ERR_BAD_ARG, "hb_debug_g1_wire_op: what is HB_G1_WIRE_SELFTEST_SQRT or HB_G1_WIRE_SELFTEST_PHI");
    if (count == 0) return HB_OK;
    if (!wire_aligned(in_dev) || !wire_aligned(out_dev)) return fail(ctx, HB_ERR_BAD_ARG, "hb_debug_g1_wire_op: the operands and the output must be aligned to 16 bytes");
    const int64_t bytes = count * (root ? QW : G1_PT) * 4;
    if (wire_overlap(out_dev, bytes, in_dev, bytes) || (root && (wire_overlap(flags_dev, count * 4, in_dev, bytes) || wire_overlap(flags_dev, count * 4, out_dev, bytes))))
        return fail(ctx, HB_ERR_BAD_ARG, "hb_debug_g1_wire_op: an output overlaps the input or the other output");
    k_g1_wire_op<<<blocks, 256, 0, s>>>(*K, what, (const uint32_t *)in_dev, (uint32_t *)out_dev, flags_dev, count);
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_selftest_g1_wire(int what, const uint64_t *const *operands, int flags, int64_t arg, uint64_t *out, int64_t count) {
    if (!operands || !operands[0] || count < 0 || !out || arg || !wire_aligned(operands[0]) || !wire_aligned(out)) return HB_ERR_BAD_ARG;
    const WireConsts *K = g1_wire_consts();
    if (!K) return HB_ERR_UNSUPPORTED;
    const FpParams<QL> P = fq_params();
    const uint32_t *in = reinterpret_cast<const uint32_t *>(operands[0]);
    uint32_t *o = reinterpret_cast<uint32_t *>(out);
    switch (what) {
    case HB_G1_WIRE_SELFTEST_SUBGROUP: {
        if (flags) return HB_ERR_BAD_ARG;
        for (int64_t i = 0; i < count; i++) reinterpret_cast<int32_t *>(out)[i] = g1_subgroup_elem(in + i * G1_PT, *K, P);
        return HB_OK;
    }
    case HB_G1_WIRE_SELFTEST_DECOMPRESS: {
        if (flags & ~1) return HB_ERR_BAD_ARG;
        int32_t *status = reinterpret_cast<int32_t *>(o + count * G1_PT);
        status[count] = 0;
        for (int64_t i = 0; i < count; i++) {
            status[i] = g1_decompress_elem(o + i * G1_PT, in + i * G1_ENC_WORDS, flags, *K, P);
            if (status[i]) status[count]++;
        }
        return HB_OK;
    }
    case HB_G1_WIRE_SELFTEST_COMPRESS: {
        if (flags) return HB_ERR_BAD_ARG;
        for (int64_t i = 0; i < count; i++) g1_compress_elem(o + i * G1_ENC_WORDS, in + i * G1_PT, *K);
        return HB_OK;
    }
    case HB_G1_WIRE_SELFTEST_SQRT: {
        if (flags) return HB_ERR_BAD_ARG;
        int32_t *square = reinterpret_cast<int32_t *>(o + count * QW);
        for (int64_t i = 0; i < count; i++) {
            const int32_t f = wire_sqrt_elem(o + i * QW, in + i * QW, *K, P);
            if (f < 0) return HB_ERR_BAD_ARG;
            square[i] = f;
        }
        return HB_OK;
    }
    case HB_G1_WIRE_SELFTEST_PHI: {
        if (flags) return HB_ERR_BAD_ARG;
        for (int64_t i = 0; i < count; i++) g1_phi_elem(o + i * G1_PT, in + i * G1_PT, *K, P);
        return HB_OK;
    }
    default: return HB_ERR_BAD_ARG;
    }
}

}  // extern "C"

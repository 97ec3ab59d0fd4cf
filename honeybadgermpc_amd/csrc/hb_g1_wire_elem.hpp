// hb_g1_wire_elem.hpp -- the bodies of hb_g1_wire.hip: a square root in Fq, the endomorphism phi and the membership test built on it, and
// the 48-byte compressed encoding in both directions.  Host and device, on the field and point bodies of hb_g1_elem.hpp: the kernels
// only find the index and call, hb_selftest_g1_wire runs the same functions over host memory.  The head of hb_g1_wire.hip states the
// formulas and counts the products.
#pragma once
#include "hb_g1_elem.hpp"

namespace hb {

constexpr int G1_ENC_WORDS = 12;                         // 32-bit words an encoding: 48 bytes, three dwordx4
constexpr uint64_t G1_X = 0xd201000000010000ull;         // |x|, the curve's parameter: bits 63, 62, 60, 57, 48, 16
// The exponent (Q + 1) / 4 as a left-to-right sliding-window schedule of width 3, as EqSched of hb_eq.hip: acc starts as table[first];
// step s squares acc (step >> 8) times and then, if (step & 0xff) != 0, multiplies it by table[(step & 0xff) - 1]; table[k] = a^(2k + 1).
// A multiplying step consumes at least three bits (but for the last): 379 bits take at most 128 steps.
constexpr int WIRE_WINDOW = 3;
constexpr int WIRE_MAX_STEPS = 136;
struct WireSched { uint32_t first, n; uint16_t step[WIRE_MAX_STEPS]; };
// what the kernels take by value: the schedule, beta as a Montgomery residue, (Q - 1) / 2 as canonical digits
struct WireConsts { WireSched S; uint32_t beta[QL], half[QL]; };

// a < b, digits (the top one may exceed 29 bits)
HB_HD bool fq_lt(const uint32_t (&a)[QL], const uint32_t (&b)[QL]) {
    int32_t borrow = 0;
#pragma unroll
    for (int i = 0; i < QL; i++) borrow = ((int32_t)a[i] - (int32_t)b[i] + borrow) >> 31;
    return borrow != 0;
}
// r = table entry k: a chain of selects on a wave-uniform k, the table stays in registers
HB_HD void wire_pick(uint32_t (&r)[QL], const uint32_t (&t1)[QL], const uint32_t (&t3)[QL], const uint32_t (&t5)[QL], const uint32_t (&t7)[QL], uint32_t k) {
#pragma unroll
    for (int q = 0; q < QL; q++) r[q] = k == 0 ? t1[q] : (k == 1 ? t3[q] : (k == 2 ? t5[q] : t7[q]));
}
// r = a^e for the schedule's exponent e, Montgomery residues: the same squarings and products in every lane
HB_HD void fq_pow_sched(uint32_t (&r)[QL], const uint32_t (&a)[QL], const WireSched &S, const FpParams<QL> &P) {
    static_assert(WIRE_WINDOW == 3, "the table is four named arrays");
    uint32_t t1[QL], t3[QL], t5[QL], t7[QL], sq[QL], acc[QL], b[QL];
    fp_set<QL>(t1, a);
    fq_mul(sq, t1, t1, P);
    fq_mul(t3, t1, sq, P);
    fq_mul(t5, t3, sq, P);
    fq_mul(t7, t5, sq, P);
    wire_pick(acc, t1, t3, t5, t7, S.first);
#pragma unroll 1
    for (uint32_t s = 0; s < S.n; s++) {
        const uint32_t st = S.step[s], nsq = st >> 8, m = st & 0xffu;
#pragma unroll 1
        for (uint32_t j = 0; j < nsq; j++) fq_mul(acc, acc, acc, P);
        if (m) {
            wire_pick(b, t1, t3, t5, t7, m - 1);
            fq_mul(acc, acc, b, P);
        }
    }
    fp_set<QL>(r, acc);
}
// y = a^((Q + 1) / 4) for a canonical Montgomery residue a; returns y^2 == a: Q = 3 mod 4, so y is a root whenever a has one
HB_HD bool fq_sqrt(uint32_t (&y)[QL], const uint32_t (&a)[QL], const WireSched &S, const FpParams<QL> &P) {
    uint32_t t[QL];
    fq_pow_sched(y, a, S, P);
    fq_mul(t, y, y, P);
    return fp_eq<QL>(t, a);
}
// The bare root of six words of canonical residue (the self test's SQRT case and k_g1_wire_op): out = a^((Q + 1) / 4) if that squares
// to a, else zero; returns 1 a square, 0 not, -1 for a not below Q (nothing written)
HB_HD int32_t wire_sqrt_elem(uint32_t *out, const uint32_t *in, const WireConsts &K, const FpParams<QL> &P) {
    uint32_t a[QL], y[QL];
    load_digits<QL, QW>(a, in);
    if (!fq_below_q(a, P)) return -1;
    fq_to_mont(a, a, P);
    const int32_t square = fq_sqrt(y, a, K.S, P) ? 1 : 0;
    fq_from_mont(a, y, P);
    if (!square) fq_zero(a);
    store_digits<QL, QW>(out, a);
    return square;
}
// x^3 + 4, Montgomery residues
HB_HD void g1_curve_rhs(uint32_t (&r)[QL], const uint32_t (&x)[QL], const FpParams<QL> &P) {
    uint32_t four[QL];
    fq_mul(r, x, x, P);
    fq_mul(r, r, x, P);
    fp_add<QL>(four, P.one, P.one, P);
    fp_add<QL>(four, four, four, P);
    fp_add<QL>(r, r, four, P);
}

// r = r + q, both Jacobian; complete.  g1_add's formulas in an order that lets r's X and Y die before q's side is computed (q, the base
// of a pass, is live anyway): nine field elements live at the peak where g1_add holds twelve.  Equal operands double q, not r.
HB_HD void g1_add_base(G1Jac &r, const G1Jac &q, const FpParams<QL> &P) {
    if (fp_is_zero<QL>(q.Z)) return;
    if (fp_is_zero<QL>(r.Z)) { r = q; return; }
    uint32_t z[QL], U1[QL], S1[QL], H[QL], rr[QL];
    fq_mul(z, q.Z, q.Z, P);
    fq_mul(U1, r.X, z, P);
    fq_mul(S1, r.Y, q.Z, P);
    fq_mul(S1, S1, z, P);
    fq_mul(z, r.Z, r.Z, P);
    fq_mul(H, q.X, z, P);
    fq_mul(rr, q.Y, r.Z, P);
    fq_mul(rr, rr, z, P);
    fp_sub<QL>(H, H, U1, P);
    fp_sub<QL>(rr, rr, S1, P);
    if (fp_is_zero<QL>(H)) {
        if (fp_is_zero<QL>(rr)) g1_double(r, q, P);
        else g1_set_identity(r, P);
        return;
    }
    fq_mul(z, r.Z, q.Z, P);
    g1_add_tail(r, H, rr, U1, S1, z, P);
}
// r = |x| base, both Jacobian (r is not base): from the top bit down, 63 doublings and 5 complete additions, the same in every lane
HB_HD void g1_mul_x(G1Jac &r, const G1Jac &base, const FpParams<QL> &P) {
    r = base;
#pragma unroll 1
    for (int b = 62; b >= 0; b--) {
        g1_double(r, r, P);
        if ((G1_X >> b) & 1u) g1_add_base(r, base, P);
    }
}
// phi(a) == -[x^2] a for a finite point a of the curve: exactly the points of the subgroup of order R.  [x]([x] a) stays Jacobian
// between the two multiplications; the comparison is cross-multiplied: beta x Z^2 == X, y Z^3 == -Y, Z != 0 (x^2 is no multiple of R,
// so a member other than the identity does not reach Z = 0).  126 doublings, 10 additions, 6 products.
HB_HD bool g1_endo_member(const G1Aff &a, const uint32_t (&beta)[QL], const FpParams<QL> &P) {
    G1Jac q, t;
    g1_from_affine(q, a, P);
#pragma unroll 1
    for (int pass = 0; pass < 2; pass++) {
        t = q;
        g1_mul_x(q, t, P);
    }
    uint32_t zz[QL], u[QL], v[QL];
    fq_mul(zz, q.Z, q.Z, P);
    fq_mul(u, a.x, beta, P);
    fq_mul(u, u, zz, P);
    fq_mul(v, a.y, zz, P);
    fq_mul(v, v, q.Z, P);
    fp_neg<QL>(zz, q.Y, P);
    return !fp_is_zero<QL>(q.Z) && fp_eq<QL>(u, q.X) && fp_eq<QL>(v, zz);
}
// flag of hb_g1_subgroup: hb_g1_check's test, and the identity or a member
HB_HD int32_t g1_subgroup_elem(const uint32_t *p, const WireConsts &K, const FpParams<QL> &P) {
    G1Aff a;
    const bool below = g1_load(a, p, P);
    const bool curve = g1_on_curve(a, P), member = g1_endo_member(a, K.beta, P);
    return (a.inf || (below && curve && member)) ? 1 : 0;
}
// out = (beta x, y); the identity stays all zeros
HB_HD void g1_phi_elem(uint32_t *out, const uint32_t *p, const WireConsts &K, const FpParams<QL> &P) {
    uint32_t w[QW];
    G1Aff a;
    g1_load(a, p, P);
    fq_mul(a.x, a.x, K.beta, P);
    fq_from_mont(a.x, a.x, P);
    store_digits<QL, QW>(out, a.x);
    load_words<QW>(w, p + QW);
    store_words<QW>(out + QW, w);
}

// 48 bytes -> a point and its status (HB_G1_WIRE_*).  enc holds the big-endian x: word j of x is the byte-swapped word 11 - j of enc, the
// three flags are the top bits of word 11.  Every lane computes rhs, the root and (when asked) the membership test whatever its flags
// say; the status picks the first failed check in the host model's order, and a rejected item stores zeros.
HB_HD int32_t g1_decompress_elem(uint32_t *out, const uint32_t *enc, int check_subgroup, const WireConsts &K, const FpParams<QL> &P) {
    uint32_t w[G1_ENC_WORDS], xw[QW], xd[QL], rhs[QL], ym[QL], yc[QL], nm[QL];
    load_words<G1_ENC_WORDS>(w, enc);
#pragma unroll
    for (int j = 0; j < QW; j++) xw[j] = __builtin_bswap32(w[QW - 1 - j]);
    const uint32_t fl = xw[QW - 1] >> 29;
    xw[QW - 1] &= 0x1fffffffu;
    unpack<QL, QW>(xd, xw);
    const bool x_zero = fp_is_zero<QL>(xd), below = fq_below_q(xd, P);
    G1Aff a;
    fq_to_mont(a.x, xd, P);
    g1_curve_rhs(rhs, a.x, P);
    const bool square = fq_sqrt(ym, rhs, K.S, P);
    fq_from_mont(yc, ym, P);
    // the sign flag asks for the root above (Q - 1) / 2, read on the canonical value
    const bool flip = fq_lt(K.half, yc) != ((fl & 1u) != 0);
    fp_neg<QL>(nm, ym, P);
#pragma unroll
    for (int q = 0; q < QL; q++) a.y[q] = flip ? nm[q] : ym[q];
    a.inf = false;
    bool member = true;
    if (check_subgroup) member = g1_endo_member(a, K.beta, P);
    // the canonical words from the Montgomery residues, after the test: two products, and 28 registers fewer across it
    fq_from_mont(xd, a.x, P);
    fq_from_mont(yc, a.y, P);
    int32_t status;
    if (!(fl & 4u)) status = HB_G1_WIRE_NOT_COMPRESSED;
    else if (fl & 2u) status = (x_zero && !(fl & 1u)) ? HB_G1_WIRE_OK : HB_G1_WIRE_BAD_IDENTITY;
    else if (!below) status = HB_G1_WIRE_X_NOT_BELOW_Q;
    else if (!square) status = HB_G1_WIRE_NOT_ON_CURVE;
    else if (!member) status = HB_G1_WIRE_NOT_IN_SUBGROUP;
    else status = HB_G1_WIRE_OK;
    const bool keep = status == HB_G1_WIRE_OK && !(fl & 2u);
#pragma unroll
    for (int q = 0; q < QL; q++) { xd[q] = keep ? xd[q] : 0u; yc[q] = keep ? yc[q] : 0u; }
    store_digits<QL, QW>(out, xd);
    store_digits<QL, QW>(out + QW, yc);
    return status;
}
// a point -> 48 bytes: x as it stands, 0x80, 0x40 for the all-zero point, 0x20 for y > (Q - 1) / 2.  No field product.
HB_HD void g1_compress_elem(uint32_t *enc, const uint32_t *p, const WireConsts &K) {
    uint32_t xw[QW], yw[QW], yd[QL], w[G1_ENC_WORDS];
    load_words<QW>(xw, p);
    load_words<QW>(yw, p + QW);
    uint32_t any = 0;
#pragma unroll
    for (int j = 0; j < QW; j++) any |= xw[j] | yw[j];
    unpack<QL, QW>(yd, yw);
    xw[QW - 1] |= 0x80000000u | (any == 0 ? 0x40000000u : (fq_lt(K.half, yd) ? 0x20000000u : 0u));
#pragma unroll
    for (int j = 0; j < G1_ENC_WORDS; j++) w[j] = __builtin_bswap32(xw[QW - 1 - j]);
    store_words<G1_ENC_WORDS>(enc, w);
}

}  // namespace hb

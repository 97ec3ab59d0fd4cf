// hb_g1_elem.hpp -- the field and point bodies of BLS12-381 G1 (fq_*, g1_double, g1_add_mixed, g1_add, g1_eq, g1_load, g1_store,
// g1_mul_affine, g1_table_window, the tree nodes of the sums, fq_params and the non-inlined fq_mul_call) and the checks every G1 entry
// point makes (G1_ENTER), shared by hb_g1.hip, hb_msm.hip and hb_crs.hip.  Host and device: the kernels only load, call and store, and the host self tests run the same functions.  The head of
// hb_g1.hip derives the bounds (Field, LAZY SUMS) and states the formulas (Points).
#pragma once
#include "hb_common.hpp"

namespace hb {

constexpr int QL = 14, QW = 12, SW = 8;                  // Fq digits, Fq words, scalar words
constexpr int G1_PT = 2 * QW;                            // words a point in HBM
constexpr int G1_ENT = 32;                               // words a table entry
constexpr int G1_SCR = 32;                               // words of scratch a table entry (Z, prefix product)

HB_HD FpParams<QL> fq_params() {
    return FpParams<QL>{
        {0x1fffaaab, 0xff7ffff, 0x14ffffee, 0x17fffd62, 0xf6241ea, 0x9507b58, 0xafd9cc3, 0x109e70a2, 0x1764774b, 0x121a5d66, 0x12c6e9ed, 0x12ffcd34, 0x111ea3, 0xd},
        {0x15bef7ae, 0x1031cd0e, 0x2dd93e8, 0x9226323, 0xe6e2cd2, 0x11684daa, 0x1170e5db, 0x88e25b1, 0x1b366399, 0x1c536f47, 0xd1f9cbc, 0x278b67f, 0x1ea66a2b, 0xc},
        {0x3a9fb84, 0xba00690, 0x71288f1, 0xf59bcc5, 0x126cb614, 0x585bf36, 0x1b85ac3d, 0x1cf856fa, 0x1891ecbd, 0x1a7eec05, 0x155a88f0, 0x741ac6d, 0x1317c30f, 0x9},
        0x1ffcfffd, 0};
}
// Q - 2, the exponent of an inversion, and the group order R (the modulus of every context these entry points take)
#define G1_QM2_WORDS {0xffffaaa9u, 0xb9feffffu, 0xb153ffffu, 0x1eabfffeu, 0xf6b0f624u, 0x6730d2a0u, 0xf38512bfu, 0x64774b84u, 0x434bacd7u, 0x4b1ba7b6u, 0x397fe69au, 0x1a0111eau}
static const uint64_t G1_ORDER[4] = {0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull};

struct G1Jac { uint32_t X[QL], Y[QL], Z[QL]; };
struct G1Aff { uint32_t x[QL], y[QL]; bool inf; };

#if defined(__HIP_DEVICE_COMPILE__)
// operands and result as 14-lane vectors: vectors travel in VGPRs whatever their size (28 of the 31 argument registers), where a struct
// beyond 16 registers of arguments would be handed over through private memory
typedef uint32_t fq_vec __attribute__((ext_vector_type(14)));
__device__ __noinline__ fq_vec fq_mul_call(fq_vec a, fq_vec b) {
    const FpParams<QL> P = fq_params();
    uint32_t x[QL], y[QL], z[QL];
#pragma unroll
    for (int q = 0; q < QL; q++) { x[q] = a[q]; y[q] = b[q]; }
    mont_mul<QL>(z, x, y, P);
    fq_vec r;
#pragma unroll
    for (int q = 0; q < QL; q++) r[q] = z[q];
    return r;
}
#else
// the host's copy is one function too: the self test's bodies hold some 200 products
static __attribute__((noinline)) void fq_mul_host(uint32_t (&r)[QL], const uint32_t (&a)[QL], const uint32_t (&b)[QL], const FpParams<QL> &P) { mont_mul<QL>(r, a, b, P); }
#endif
// r = a b / R mod Q, canonical; operands as LAZY SUMS above allows; r may be a or b
HB_HD void fq_mul(uint32_t (&r)[QL], const uint32_t (&a)[QL], const uint32_t (&b)[QL], const FpParams<QL> &P) {
#if defined(__HIP_DEVICE_COMPILE__)
    fq_vec x, y;
#pragma unroll
    for (int q = 0; q < QL; q++) { x[q] = a[q]; y[q] = b[q]; }
    const fq_vec z = fq_mul_call(x, y);
#pragma unroll
    for (int q = 0; q < QL; q++) r[q] = z[q];
#else
    fq_mul_host(r, a, b, P);
#endif
}
HB_HD void fq_to_mont(uint32_t (&r)[QL], const uint32_t (&a)[QL], const FpParams<QL> &P) { fq_mul(r, a, P.r2, P); }
HB_HD void fq_from_mont(uint32_t (&r)[QL], const uint32_t (&a)[QL], const FpParams<QL> &P) {
    uint32_t one[QL];
#pragma unroll
    for (int q = 0; q < QL; q++) one[q] = q == 0 ? 1u : 0u;
    fq_mul(r, a, one, P);
}
// r = a + b without the conditional subtraction: digits below 2^29 but the top one
HB_HD void fq_add_lazy(uint32_t (&r)[QL], const uint32_t (&a)[QL], const uint32_t (&b)[QL]) {
    uint32_t carry_ = 0;
#pragma unroll
    for (int i = 0; i < QL; i++) {
        const uint32_t v = a[i] + b[i] + carry_;
        if (i < QL - 1) { carry_ = v >> LB; r[i] = v & DMASK; } else r[i] = v;
    }
}
HB_HD void fq_zero(uint32_t (&r)[QL]) {
#pragma unroll
    for (int q = 0; q < QL; q++) r[q] = 0;
}
// a^(Q - 2); 0 -> 0
HB_HD void fq_inv(uint32_t (&r)[QL], const uint32_t (&a)[QL], const FpParams<QL> &P) {
    uint32_t e[QW] = G1_QM2_WORDS;
    uint32_t acc[QL];
    fp_set<QL>(acc, P.one);
#pragma unroll 1
    for (int b = 0; b < 32 * QW; b++) {
        fq_mul(acc, acc, acc, P);
        const uint32_t bit = e[QW - 1] >> 31;
#pragma unroll
        for (int q = QW - 1; q > 0; q--) e[q] = (e[q] << 1) | (e[q - 1] >> 31);
        e[0] <<= 1;
        if (bit) fq_mul(acc, acc, a, P);
    }
    fp_set<QL>(r, acc);
}
// digits (top digit may exceed 29 bits) below Q?
HB_HD bool fq_below_q(const uint32_t (&v)[QL], const FpParams<QL> &P) {
    int32_t borrow = 0;
#pragma unroll
    for (int i = 0; i < QL; i++) borrow = ((int32_t)v[i] - (int32_t)P.p[i] + borrow) >> 31;
    return borrow != 0;
}

// ---------------------------------------------------------------- the group
HB_HD void g1_set_identity(G1Jac &r, const FpParams<QL> &P) {
    fp_set<QL>(r.X, P.one);
    fp_set<QL>(r.Y, P.one);
    fq_zero(r.Z);
}
HB_HD void g1_from_affine(G1Jac &r, const G1Aff &a, const FpParams<QL> &P) {
#pragma unroll
    for (int q = 0; q < QL; q++) { r.X[q] = a.inf ? P.one[q] : a.x[q]; r.Y[q] = a.inf ? P.one[q] : a.y[q]; r.Z[q] = a.inf ? 0u : P.one[q]; }
}
// r = 2 p (r may be p)
HB_HD void g1_double(G1Jac &r, const G1Jac &p, const FpParams<QL> &P) {
    uint32_t A[QL], B[QL], C[QL], D[QL], E[QL], t[QL];
    fq_mul(A, p.X, p.X, P);
    fq_mul(B, p.Y, p.Y, P);
    fq_mul(C, B, B, P);
    fq_add_lazy(t, p.X, B);                                    // < 2 Q: a factor only
    fq_mul(t, t, t, P);
    fp_sub<QL>(t, t, A, P);
    fp_sub<QL>(t, t, C, P);
    fp_add<QL>(D, t, t, P);
    fq_add_lazy(E, A, A);
    fq_add_lazy(E, E, A);                                      // < 3 Q: a factor only
    fq_mul(t, p.Y, p.Z, P);
    fp_add<QL>(r.Z, t, t, P);
    fq_mul(t, E, E, P);
    fp_sub<QL>(t, t, D, P);
    fp_sub<QL>(r.X, t, D, P);
    fp_sub<QL>(t, D, r.X, P);
    fq_mul(t, E, t, P);
    fp_add<QL>(C, C, C, P);
    fp_add<QL>(C, C, C, P);
    fp_add<QL>(C, C, C, P);
    fp_sub<QL>(r.Y, t, C, P);
}
// the common tail of both additions: from H, rr = r, U1 (X1 in the first operand's scale), S1, and zz = the product of the Zs
HB_HD void g1_add_tail(G1Jac &r, const uint32_t (&H)[QL], const uint32_t (&rr)[QL], const uint32_t (&U1)[QL], const uint32_t (&S1)[QL], const uint32_t (&zz)[QL],
                       const FpParams<QL> &P) {
    uint32_t HH[QL], HHH[QL], V[QL], t[QL];
    fq_mul(HH, H, H, P);
    fq_mul(HHH, H, HH, P);
    fq_mul(V, U1, HH, P);
    fq_mul(r.Z, zz, H, P);
    fq_mul(t, rr, rr, P);
    fp_sub<QL>(t, t, HHH, P);
    fp_sub<QL>(t, t, V, P);
    fp_sub<QL>(r.X, t, V, P);
    fq_mul(HHH, S1, HHH, P);
    fp_sub<QL>(t, V, r.X, P);
    fq_mul(t, rr, t, P);
    fp_sub<QL>(r.Y, t, HHH, P);
}
// r = r + a, a affine; complete
HB_HD void g1_add_mixed(G1Jac &r, const G1Aff &a, const FpParams<QL> &P) {
    if (a.inf) return;
    if (fp_is_zero<QL>(r.Z)) { g1_from_affine(r, a, P); return; }
    uint32_t zz[QL], U2[QL], S2[QL], H[QL], rr[QL];
    fq_mul(zz, r.Z, r.Z, P);
    fq_mul(U2, a.x, zz, P);
    fq_mul(S2, a.y, r.Z, P);
    fq_mul(S2, S2, zz, P);
    fp_sub<QL>(H, U2, r.X, P);
    fp_sub<QL>(rr, S2, r.Y, P);
    if (fp_is_zero<QL>(H)) {
        if (fp_is_zero<QL>(rr)) g1_double(r, r, P);
        else g1_set_identity(r, P);
        return;
    }
    fp_set<QL>(U2, r.X);
    fp_set<QL>(S2, r.Y);
    fp_set<QL>(zz, r.Z);
    g1_add_tail(r, H, rr, U2, S2, zz, P);
}
// r = r + q, both Jacobian; complete
HB_HD void g1_add(G1Jac &r, const G1Jac &q, const FpParams<QL> &P) {
    if (fp_is_zero<QL>(q.Z)) return;
    if (fp_is_zero<QL>(r.Z)) { r = q; return; }
    uint32_t z1[QL], z2[QL], U1[QL], U2[QL], S1[QL], S2[QL], H[QL], rr[QL];
    fq_mul(z1, r.Z, r.Z, P);
    fq_mul(z2, q.Z, q.Z, P);
    fq_mul(U1, r.X, z2, P);
    fq_mul(U2, q.X, z1, P);
    fq_mul(S1, r.Y, q.Z, P);
    fq_mul(S1, S1, z2, P);
    fq_mul(S2, q.Y, r.Z, P);
    fq_mul(S2, S2, z1, P);
    fp_sub<QL>(H, U2, U1, P);
    fp_sub<QL>(rr, S2, S1, P);
    if (fp_is_zero<QL>(H)) {
        if (fp_is_zero<QL>(rr)) g1_double(r, r, P);
        else g1_set_identity(r, P);
        return;
    }
    fq_mul(z1, r.Z, q.Z, P);
    g1_add_tail(r, H, rr, U1, S1, z1, P);
}
HB_HD bool g1_eq(const G1Jac &a, const G1Jac &b, const FpParams<QL> &P) {
    const bool az = fp_is_zero<QL>(a.Z), bz = fp_is_zero<QL>(b.Z);
    if (az || bz) return az && bz;
    uint32_t z1[QL], z2[QL], u[QL], v[QL];
    fq_mul(z1, a.Z, a.Z, P);
    fq_mul(z2, b.Z, b.Z, P);
    fq_mul(u, a.X, z2, P);
    fq_mul(v, b.X, z1, P);
    if (!fp_eq<QL>(u, v)) return false;
    fq_mul(z1, z1, a.Z, P);
    fq_mul(z2, z2, b.Z, P);
    fq_mul(u, a.Y, z2, P);
    fq_mul(v, b.Y, z1, P);
    return fp_eq<QL>(u, v);
}
// y^2 = x^3 + 4 for a finite affine point (Montgomery residues)
HB_HD bool g1_on_curve(const G1Aff &a, const FpParams<QL> &P) {
    uint32_t l[QL], r[QL], four[QL];
    fq_mul(l, a.y, a.y, P);
    fq_mul(r, a.x, a.x, P);
    fq_mul(r, r, a.x, P);
    fp_add<QL>(four, P.one, P.one, P);
    fp_add<QL>(four, four, four, P);
    fp_add<QL>(r, r, four, P);
    return fp_eq<QL>(l, r);
}

// ---------------------------------------------------------------- memory forms
// a point of HBM -> affine Montgomery; returns: the identity, or both coordinates below Q (whatever the words hold is reduced)
HB_HD bool g1_load(G1Aff &a, const uint32_t *p, const FpParams<QL> &P) {
    uint32_t d[QL];
    load_digits<QL, QW>(d, p);
    bool zero = fp_is_zero<QL>(d), below = fq_below_q(d, P);
    fq_to_mont(a.x, d, P);
    load_digits<QL, QW>(d, p + QW);
    zero = zero && fp_is_zero<QL>(d);
    below = below && fq_below_q(d, P);
    fq_to_mont(a.y, d, P);
    a.inf = zero;
    return below;
}
// Jacobian -> the affine point of HBM: one inversion; Z = 0 -> all zeros
HB_HD void g1_store(uint32_t *p, const G1Jac &j, const FpParams<QL> &P) {
    uint32_t zi[QL], zi2[QL], t[QL], d[QL];
    fq_inv(zi, j.Z, P);
    fq_mul(zi2, zi, zi, P);
    fq_mul(t, j.X, zi2, P);
    fq_from_mont(d, t, P);
    store_digits<QL, QW>(p, d);
    fq_mul(t, j.Y, zi2, P);
    fq_mul(t, t, zi, P);
    fq_from_mont(d, t, P);
    store_digits<QL, QW>(p + QW, d);
}
// 14 digits <-> 16 words of a table
HB_HD void g1_load16(uint32_t (&d)[QL], const uint32_t *p) {
    uint32_t w[16];
    load_words<16>(w, p);
#pragma unroll
    for (int q = 0; q < QL; q++) d[q] = w[q];
}
HB_HD void g1_store16(uint32_t *p, const uint32_t (&d)[QL]) {
    uint32_t w[16];
#pragma unroll
    for (int q = 0; q < 16; q++) w[q] = q < QL ? d[q] : 0u;
    store_words<16>(p, w);
}
HB_HD void g1_load_entry(G1Aff &a, const uint32_t *p) {
    g1_load16(a.x, p);
    g1_load16(a.y, p + 16);
    a.inf = fp_is_zero<QL>(a.x) && fp_is_zero<QL>(a.y);
}
HB_HD void g1_load_scalar(uint32_t (&k)[SW], const uint32_t *p) { load_words<SW>(k, p); }

// acc = k a: the scalar's bits from the top; doublings start with the first set bit
HB_HD void g1_mul_affine(G1Jac &acc, const uint32_t (&kw)[SW], const G1Aff &a, const FpParams<QL> &P) {
    uint32_t k[SW];
#pragma unroll
    for (int q = 0; q < SW; q++) k[q] = kw[q];
    g1_set_identity(acc, P);
    bool started = false;
#pragma unroll 1
    for (int b = 0; b < 32 * SW; b++) {
        const uint32_t bit = k[SW - 1] >> 31;
#pragma unroll
        for (int q = SW - 1; q > 0; q--) k[q] = (k[q] << 1) | (k[q - 1] >> 31);
        k[0] <<= 1;
        if (started) g1_double(acc, acc, P);
        if (bit) { g1_add_mixed(acc, a, P); started = true; }
    }
}

// ---------------------------------------------------------------- fixed-base tables (k_g1_table of hb_g1.hip, k_g1_crs_table of hb_crs.hip)
// window w of a base's table (the layout at the head of hb_g1.hip): entries, then scratch
HB_HD void g1_table_window(uint32_t *table, const uint32_t *base, int c, int w, const FpParams<QL> &P) {
    const int n = (1 << c) - 1, W = 256 / c;
    uint32_t *ent = table + (int64_t)w * n * G1_ENT;
    uint32_t *scr = table + (int64_t)W * n * G1_ENT + (int64_t)w * n * G1_SCR;
    G1Aff a;
    G1Jac bw, acc;
    g1_load(a, base, P);
    g1_from_affine(bw, a, P);
#pragma unroll 1
    for (int s = 0; s < c * w; s++) g1_double(bw, bw, P);
    // entry j = j B_w, Jacobian: X, Y in the entry, Z and the product of the Zs before it in the scratch
    uint32_t run[QL];
    fp_set<QL>(run, P.one);
    g1_set_identity(acc, P);
#pragma unroll 1
    for (int j = 0; j < n; j++) {
        g1_add(acc, bw, P);
        g1_store16(ent + j * G1_ENT, acc.X);
        g1_store16(ent + j * G1_ENT + 16, acc.Y);
        g1_store16(scr + j * G1_SCR, acc.Z);
        g1_store16(scr + j * G1_SCR + 16, run);
        if (!fp_is_zero<QL>(acc.Z)) fq_mul(run, run, acc.Z, P);
    }
    uint32_t inv[QL];
    fq_inv(inv, run, P);
#pragma unroll 1
    for (int j = n - 1; j >= 0; j--) {
        uint32_t z[QL], zi[QL], zi2[QL], x[QL], y[QL];
        g1_load16(z, scr + j * G1_SCR);
        g1_load16(zi, scr + j * G1_SCR + 16);
        g1_load16(x, ent + j * G1_ENT);
        g1_load16(y, ent + j * G1_ENT + 16);
        if (fp_is_zero<QL>(z)) {                               // an identity entry (a base of small order): (0, 0)
            fq_zero(x);
            fq_zero(y);
        } else {
            fq_mul(zi, zi, inv, P);                            // 1 / Z_j
            fq_mul(inv, inv, z, P);
            fq_mul(zi2, zi, zi, P);
            fq_mul(x, x, zi2, P);
            fq_mul(y, y, zi2, P);
            fq_mul(y, y, zi, P);
        }
        g1_store16(ent + j * G1_ENT, x);
        g1_store16(ent + j * G1_ENT + 16, y);
    }
}

// ---------------------------------------------------------------- the tree of hb_msm.hip and hb_crs.hip
// a node: a Jacobian point of 3 x 14 digits at a stride of 43 words (odd: lanes of a step hit distinct banks)
constexpr int MSM_NODE = 3 * QL + 1;                     // words a tree node: 42 digits, one of padding
HB_HD void msm_node_store(uint32_t *nodes, int lane, const G1Jac &j) {
    uint32_t *n = nodes + lane * MSM_NODE;
#pragma unroll
    for (int q = 0; q < QL; q++) { n[q] = j.X[q]; n[QL + q] = j.Y[q]; n[2 * QL + q] = j.Z[q]; }
}
HB_HD void msm_node_load(G1Jac &j, const uint32_t *nodes, int lane) {
    const uint32_t *n = nodes + lane * MSM_NODE;
#pragma unroll
    for (int q = 0; q < QL; q++) { j.X[q] = n[q]; j.Y[q] = n[QL + q]; j.Z[q] = n[2 * QL + q]; }
}
// one step of the tree: node lane += node lane + half
HB_HD void msm_tree_step(uint32_t *nodes, int lane, int half, const FpParams<QL> &P) {
    if (lane >= half) return;
    G1Jac a, b;
    msm_node_load(b, nodes, lane + half);
    if (fp_is_zero<QL>(b.Z)) return;
    msm_node_load(a, nodes, lane);
    g1_add(a, b, P);
    msm_node_store(nodes, lane, a);
}

// ---------------------------------------------------------------- host side
// The literals of fq_params and G1_QM2_WORDS against Q's words, by shifts and subtractions alone: R mod Q and R^2 mod Q by doubling 1
// modulo Q 406 and 812 times over 13 words, n0 by Newton's iteration.
static bool g1_consts_derive() {
    static const uint32_t qm2[QW] = G1_QM2_WORDS;
    uint32_t q[13] = {0}, v[13] = {0};
    for (int i = 0; i < QW; i++) q[i] = qm2[i];
    q[0] += 2;                                                  // Q - 2 ends in ...a9: no carry
    const FpParams<QL> P = fq_params();
    auto digit = [](const uint32_t *x, int i) {
        const int bit = LB * i, j = bit >> 5, s = bit & 31;
        const uint64_t two = (uint64_t)x[j] | ((uint64_t)(j + 1 < 13 ? x[j + 1] : 0u) << 32);
        return (uint32_t)(two >> s) & DMASK;
    };
    for (int i = 0; i < QL; i++) if (digit(q, i) != P.p[i]) return false;
    v[0] = 1;
    for (int step = 1; step <= 2 * LB * QL; step++) {
        uint32_t carry_ = 0;
        for (int i = 0; i < 13; i++) { const uint32_t nv = (v[i] << 1) | carry_; carry_ = v[i] >> 31; v[i] = nv; }
        uint32_t t[13];
        int64_t borrow = 0;
        for (int i = 0; i < 13; i++) { const int64_t d = (int64_t)v[i] - q[i] + borrow; t[i] = (uint32_t)d; borrow = d >> 32; }
        if (!borrow) memcpy(v, t, sizeof(v));
        if (step == LB * QL) for (int i = 0; i < QL; i++) if (digit(v, i) != P.one[i]) return false;
    }
    for (int i = 0; i < QL; i++) if (digit(v, i) != P.r2[i]) return false;
    uint32_t inv = 1;
    for (int it = 0; it < 5; it++) inv *= 2u - q[0] * inv;       // q^-1 mod 2^32
    return ((0u - inv) & DMASK) == P.n0;
}
static bool g1_consts_ok() {
    static const bool ok = g1_consts_derive();
    return ok;
}
static bool g1_blocks(int64_t count, unsigned *blocks) {
    const int64_t b = (count + 255) / 256;
    *blocks = (unsigned)b;
    return b <= 0x7fffffffLL;
}
// every entry point: a four-limb context over the group order
static int g1_ctx_ok(hb_ctx *ctx, const char *name) {
    if (!ctx) return HB_ERR_BAD_ARG;
    if (ctx->n_limbs != 4 || memcmp(ctx->p_limbs, G1_ORDER, sizeof(G1_ORDER)) != 0) {
        ctx->err = std::string(name) + ": the context's modulus is not the order of G1";
        return HB_ERR_BAD_ARG;
    }
    if (!g1_consts_ok()) {
        ctx->err = std::string(name) + ": the constants of Fq do not derive from Q";
        return HB_ERR_UNSUPPORTED;
    }
    return HB_OK;
}

}  // namespace hb

#define G1_ENTER(name, count, nullcheck)                                                                              \
    HB_API_GUARD(ctx);                                                                                                \
    { const int rc__ = g1_ctx_ok(ctx, name); if (rc__ != HB_OK) return rc__; }                                        \
    if ((count) < 0 || ((count) > 0 && (nullcheck))) return fail(ctx, HB_ERR_BAD_ARG, name ": a null pointer or a negative count"); \
    unsigned blocks;                                                                                                  \
    if (!g1_blocks((count), &blocks) || (count) > (INT64_MAX >> 20)) return fail(ctx, HB_ERR_UNSUPPORTED, name ": batch too large for one launch"); \
    hipStream_t s = (hipStream_t)stream

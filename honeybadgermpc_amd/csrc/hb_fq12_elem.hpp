// hb_fq12_elem.hpp -- the tower Fq2 -> Fq6 -> Fq12 of BLS12-381 over the 14-digit Fq of hb_g1_elem.hpp, the Miller loop over prepared
// G2 lines and the final exponentiation.  Host and device: k_pair_product of hb_pair.hip only loads, calls and stores, and
// hb_selftest_pairing runs the same functions over host memory.  pair_tower_elem is ONE operation of the tower or of Fq on given
// operands: the self test's tower case on the host and k_pair_op (hb_debug_pair_op) on the device both call it, so the device build of
// these bodies -- fq_mul_call, the PAIR_FN calls, Fq12 values in private memory -- is tested at chosen operands, not only inside a pairing.
//
//   Fq2 = Fq[u] / (u^2 + 1),   Fq6 = Fq2[v] / (v^3 - (1 + u)),   Fq12 = Fq6[w] / (w^2 - v)           (the reference crate's tower)
//
// Products of Fq a call (fq_mul counts one, fq_inv about 570):
//   fq2_mul 3 (Karatsuba), fq2_sqr 2, fq2_mul_fq 2, fq2_mul_nr 0 (times 1 + u: (a0 - a1, a0 + a1)), fq2_inv 4 + fq_inv
//   fq6_mul 18 (six fq2_mul), fq6_mul_by_01 15, fq6_mul_by_1 9, fq6_mul_nr 0 (times v: (xi c2, c0, c1)), fq6_inv 33 + fq2_inv
//   fq12_mul 54, fq12_sqr 36 (complex squaring: two fq6_mul), fq12_cyclo_sqr 18 (nine fq2_sqr; cyclotomic subgroup only),
//   fq12_mul_by_014 39, fq12_inv 72 + fq6_inv, fq12_frobenius 21 (seven fq2_mul)
//   a line of the loop: 4 (the coefficients times x_P, y_P) + 39
//
// LAZY SUMS (every operand pair of fq_mul has a b < 2^24 Q^2).  The ONLY sums left without their conditional subtraction
// are the operand sums of the Karatsuba products, fq2_add_lazy / fq6_add_lazy: s = a0 + a1 at the Fq12 level (< 2 Q a coordinate), of
// which fq6_mul and fq6_mul_by_01 take s1 + s2 (< 4 Q), of which fq2_mul takes c0 + c1 (< 8 Q).  Such a sum is used as a FACTOR of
// fq_mul and nothing else: 8 Q * 8 Q = 2^6 Q^2.  fq2_sqr's 2 a0 (< 2 Q) is the same.  Every fq_mul result is canonical, every
// difference and every sum that is stored is fp_sub / fp_add on canonical residues, so what is compared (fq12_is_one) or written out
// is canonical.  fq2_sqr takes canonical operands only (it subtracts them): fq4_sqr adds a + b with fp_add.
//
// Every loop over digits or coefficients is fully unrolled; the bit loops (Miller, powers by |x|) are `#pragma unroll 1` and index
// nothing but the prepared table, whose address depends on the loop counter alone (wave-uniform: scalar loads).
//
// Where an Fq12 lives.  The Fq6 and Fq12 products are functions of their own on the device (PAIR_FN: not inlined, operands by
// reference), so an Fq12 is addressed and lives in private memory; fq_mul's operands and result travel in registers as before.  See
// DESIGN 3x for the registers and bytes of scratch this costs and why it was kept.
#pragma once
#include "hb_g1_elem.hpp"
#include "../../include/hbmpc_hip_debug.h"

namespace hb {

#define PAIR_FN static __host__ __device__ __attribute__((noinline))

constexpr int PAIR_LINES = 68;                           // 63 doublings, 5 additions
constexpr int PAIR_ENT = 3 * 2 * QL;                     // words a table entry: three Fq2 in Montgomery digits (84: a multiple of four)
constexpr int PAIR_TABLE = PAIR_LINES * PAIR_ENT;        // words a prepared point
constexpr int GT_WORDS = 12 * QW;                        // 32-bit words a GT element in HBM: twelve canonical residues
constexpr uint64_t PAIR_X = 0xd201000000010000ull;       // |x|

struct Fq2E { uint32_t c0[QL], c1[QL]; };
struct Fq6E { Fq2E c0, c1, c2; };
struct Fq12E { Fq6E c0, c1; };

// gamma_i = (1 + u)^((Q^i - 1) / 6), its square and its fourth power, i = 1, 2, 3, Montgomery digits; pair_consts_derive() below
// recomputes every one of them from Q
#define PAIR_FROB12_C1_1 {{0x1000a938, 0x82633e3, 0x19f1dada, 0x14162cff, 0x1caaaa9a, 0x13b1f614, 0x11d37530, 0x322a535, 0xecf0fc0, 0x13417b68, 0x1433489f, 0xbe62c9c, 0x1257c722, 0x2}, \
    {0xfff0173, 0x7d1cc1c, 0x1b0e2514, 0x3e9d062, 0x12b79750, 0x159e8543, 0x192a2792, 0xd7bcb6c, 0x895678b, 0x1ed8e1fe, 0x1e93a14d, 0x719a097, 0xdb95781, 0xa}}
#define PAIR_FROB6_C1_1 {{0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0}, \
    {0x1195dfeb, 0x1b04e484, 0x6026044, 0x86070a2, 0x1fd68858, 0x137e9670, 0x6871e67, 0x1e736664, 0x83b24f6, 0x8a70373, 0x2a012fd, 0x112f94b, 0x18a2733c, 0x3}}
#define PAIR_FROB6_C2_1 {{0x154030c4, 0x16aceb14, 0x1814e947, 0x1fba3004, 0x2e0fc81, 0xfb3da4f, 0x170f2de1, 0xacd4cbc, 0x9689a69, 0x110b9212, 0x533b200, 0x1554d884, 0xba917a7, 0x0}, \
    {0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0}}
#define PAIR_FROB12_C1_2 {{0xe69cac0, 0x14f31b7b, 0xefd9fa9, 0xf9f8cc0, 0xf8bb992, 0x15d1e4e7, 0x4767e5b, 0x122b0a3e, 0xf295254, 0x97359f3, 0x1026d6f0, 0x11ecd3e9, 0x76eab67, 0x9}, \
    {0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0}}
#define PAIR_FROB6_C1_2 {{0xabf79e7, 0x194b14eb, 0x1ceb16a6, 0x1845cd5d, 0xc814568, 0x199ca109, 0x13ee6ee1, 0x5d123e5, 0xdfbdce2, 0x10ecb54, 0xd9337ed, 0x1daaf4b0, 0x146806fb, 0xc}, \
    {0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0}}
#define PAIR_FROB6_C2_2 {{0x1195dfeb, 0x1b04e484, 0x6026044, 0x86070a2, 0x1fd68858, 0x137e9670, 0x6871e67, 0x1e736664, 0x83b24f6, 0x8a70373, 0x2a012fd, 0x112f94b, 0x18a2733c, 0x3}, \
    {0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0}}
#define PAIR_FROB12_C1_3 {{0x99d9fee, 0x1cfab983, 0x7e0b07e, 0x1f87f0f2, 0xbc18573, 0xcdbe130, 0x10ddd19, 0x100cbeaf, 0x9169c21, 0xf93673e, 0x11de55b3, 0x97ddc84, 0x11fce827, 0xc}, \
    {0x16620abd, 0x12fd467c, 0xd1f4f6f, 0x18780c70, 0x3a0bc76, 0x1c749a28, 0x9efbfa9, 0x91b1f3, 0xe4ddb2a, 0x286f628, 0xe8943a, 0x981f0b0, 0xe14367c, 0x0}}
#define PAIR_FROB6_C1_3 {{0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0}, \
    {0x3a9fb84, 0xba00690, 0x71288f1, 0xf59bcc5, 0x126cb614, 0x585bf36, 0x1b85ac3d, 0x1cf856fa, 0x1891ecbd, 0x1a7eec05, 0x155a88f0, 0x741ac6d, 0x1317c30f, 0x9}}
#define PAIR_FROB6_C2_3 {{0x1c55af27, 0x457f96f, 0xded76fd, 0x8a6409d, 0x1cf58bd6, 0x3cabc21, 0xf77f086, 0x13a619a7, 0x1ed28a8d, 0x179b7160, 0x1d6c60fc, 0xbbe20c6, 0xcf95b94, 0x3}, \
    {0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0, 0x0}}
// (Q - 1) / 6, the exponent of gamma_1
#define PAIR_QM1_6_WORDS {0xfffff1c7u, 0x49aa7fffu, 0x72e35555u, 0x51caaaau, 0xd3c82906u, 0xe688231au, 0x7deb831fu, 0xe613e1ebu, 0xb5e1f223u, 0xc849bf3u, 0x5eeaa66fu, 0x45582fcu}

// ---------------------------------------------------------------- Fq2
HB_HD void fq2_set(Fq2E &r, const Fq2E &a) { fp_set<QL>(r.c0, a.c0); fp_set<QL>(r.c1, a.c1); }
HB_HD void fq2_zero(Fq2E &r) { fq_zero(r.c0); fq_zero(r.c1); }
HB_HD void fq2_one(Fq2E &r, const FpParams<QL> &P) { fp_set<QL>(r.c0, P.one); fq_zero(r.c1); }
HB_HD bool fq2_is_zero(const Fq2E &a) { return fp_is_zero<QL>(a.c0) && fp_is_zero<QL>(a.c1); }
HB_HD bool fq2_eq(const Fq2E &a, const Fq2E &b) { return fp_eq<QL>(a.c0, b.c0) && fp_eq<QL>(a.c1, b.c1); }
HB_HD void fq2_add(Fq2E &r, const Fq2E &a, const Fq2E &b, const FpParams<QL> &P) { fp_add<QL>(r.c0, a.c0, b.c0, P); fp_add<QL>(r.c1, a.c1, b.c1, P); }
HB_HD void fq2_sub(Fq2E &r, const Fq2E &a, const Fq2E &b, const FpParams<QL> &P) { fp_sub<QL>(r.c0, a.c0, b.c0, P); fp_sub<QL>(r.c1, a.c1, b.c1, P); }
HB_HD void fq2_neg(Fq2E &r, const Fq2E &a, const FpParams<QL> &P) { fp_neg<QL>(r.c0, a.c0, P); fp_neg<QL>(r.c1, a.c1, P); }
HB_HD void fq2_conj(Fq2E &r, const Fq2E &a, const FpParams<QL> &P) { fp_set<QL>(r.c0, a.c0); fp_neg<QL>(r.c1, a.c1, P); }
// a factor only (LAZY SUMS)
HB_HD void fq2_add_lazy(Fq2E &r, const Fq2E &a, const Fq2E &b) { fq_add_lazy(r.c0, a.c0, b.c0); fq_add_lazy(r.c1, a.c1, b.c1); }
// r = a b; a, b below 4 Q a coordinate; r may be a or b
HB_HD void fq2_mul(Fq2E &r, const Fq2E &a, const Fq2E &b, const FpParams<QL> &P) {
    uint32_t aa[QL], bb[QL], s[QL], t[QL];
    fq_add_lazy(s, a.c0, a.c1);
    fq_add_lazy(t, b.c0, b.c1);
    fq_mul(aa, a.c0, b.c0, P);
    fq_mul(bb, a.c1, b.c1, P);
    fq_mul(s, s, t, P);
    fp_sub<QL>(s, s, aa, P);
    fp_sub<QL>(r.c1, s, bb, P);
    fp_sub<QL>(r.c0, aa, bb, P);
}
// r = a^2, a canonical
HB_HD void fq2_sqr(Fq2E &r, const Fq2E &a, const FpParams<QL> &P) {
    uint32_t s[QL], t[QL], d[QL];
    fq_add_lazy(s, a.c0, a.c1);
    fp_sub<QL>(t, a.c0, a.c1, P);
    fq_add_lazy(d, a.c0, a.c0);
    fq_mul(d, d, a.c1, P);
    fq_mul(r.c0, s, t, P);
    fp_set<QL>(r.c1, d);
}
HB_HD void fq2_mul_fq(Fq2E &r, const Fq2E &a, const uint32_t (&k)[QL], const FpParams<QL> &P) {
    fq_mul(r.c0, a.c0, k, P);
    fq_mul(r.c1, a.c1, k, P);
}
// r = (1 + u) a
HB_HD void fq2_mul_nr(Fq2E &r, const Fq2E &a, const FpParams<QL> &P) {
    uint32_t t[QL];
    fp_sub<QL>(t, a.c0, a.c1, P);
    fp_add<QL>(r.c1, a.c0, a.c1, P);
    fp_set<QL>(r.c0, t);
}
// 1 / a; 0 -> 0
HB_HD void fq2_inv(Fq2E &r, const Fq2E &a, const FpParams<QL> &P) {
    uint32_t t[QL], s[QL];
    fq_mul(t, a.c0, a.c0, P);
    fq_mul(s, a.c1, a.c1, P);
    fp_add<QL>(t, t, s, P);
    fq_inv(t, t, P);
    fq_mul(r.c0, a.c0, t, P);
    fq_mul(s, a.c1, t, P);
    fp_neg<QL>(r.c1, s, P);
}

// ---------------------------------------------------------------- Fq6
HB_HD void fq6_set(Fq6E &r, const Fq6E &a) { fq2_set(r.c0, a.c0); fq2_set(r.c1, a.c1); fq2_set(r.c2, a.c2); }
HB_HD void fq6_add(Fq6E &r, const Fq6E &a, const Fq6E &b, const FpParams<QL> &P) { fq2_add(r.c0, a.c0, b.c0, P); fq2_add(r.c1, a.c1, b.c1, P); fq2_add(r.c2, a.c2, b.c2, P); }
HB_HD void fq6_sub(Fq6E &r, const Fq6E &a, const Fq6E &b, const FpParams<QL> &P) { fq2_sub(r.c0, a.c0, b.c0, P); fq2_sub(r.c1, a.c1, b.c1, P); fq2_sub(r.c2, a.c2, b.c2, P); }
HB_HD void fq6_neg(Fq6E &r, const Fq6E &a, const FpParams<QL> &P) { fq2_neg(r.c0, a.c0, P); fq2_neg(r.c1, a.c1, P); fq2_neg(r.c2, a.c2, P); }
HB_HD void fq6_add_lazy(Fq6E &r, const Fq6E &a, const Fq6E &b) { fq2_add_lazy(r.c0, a.c0, b.c0); fq2_add_lazy(r.c1, a.c1, b.c1); fq2_add_lazy(r.c2, a.c2, b.c2); }
// r = v a (a canonical)
HB_HD void fq6_mul_nr(Fq6E &r, const Fq6E &a, const FpParams<QL> &P) {
    Fq2E t;
    fq2_mul_nr(t, a.c2, P);
    fq2_set(r.c2, a.c1);
    fq2_set(r.c1, a.c0);
    fq2_set(r.c0, t);
}
// r = a b; a, b below 2 Q a coordinate; r may be a or b
PAIR_FN void fq6_mul(Fq6E &r, const Fq6E &a, const Fq6E &b, const FpParams<QL> &P) {
    Fq2E aa, bb, cc, s, t, t0, t1, t2;
    fq2_mul(aa, a.c0, b.c0, P);
    fq2_mul(bb, a.c1, b.c1, P);
    fq2_mul(cc, a.c2, b.c2, P);
    fq2_add_lazy(s, a.c1, a.c2);
    fq2_add_lazy(t, b.c1, b.c2);
    fq2_mul(t0, s, t, P);
    fq2_add_lazy(s, a.c0, a.c1);
    fq2_add_lazy(t, b.c0, b.c1);
    fq2_mul(t1, s, t, P);
    fq2_add_lazy(s, a.c0, a.c2);
    fq2_add_lazy(t, b.c0, b.c2);
    fq2_mul(t2, s, t, P);
    fq2_sub(t0, t0, bb, P);
    fq2_sub(t0, t0, cc, P);
    fq2_mul_nr(t0, t0, P);
    fq2_add(r.c0, t0, aa, P);
    fq2_sub(t1, t1, aa, P);
    fq2_sub(t1, t1, bb, P);
    fq2_mul_nr(s, cc, P);
    fq2_add(r.c1, t1, s, P);
    fq2_sub(t2, t2, aa, P);
    fq2_sub(t2, t2, cc, P);
    fq2_add(r.c2, t2, bb, P);
}
// r = a (c0 + c1 v); a below 2 Q a coordinate, c0 canonical, c1 below 2 Q; r may be a
PAIR_FN void fq6_mul_by_01(Fq6E &r, const Fq6E &a, const Fq2E &c0, const Fq2E &c1, const FpParams<QL> &P) {
    Fq2E aa, bb, s, t, t1, t2, t3;
    fq2_mul(aa, a.c0, c0, P);
    fq2_mul(bb, a.c1, c1, P);
    fq2_mul(t1, a.c2, c1, P);
    fq2_mul(t3, a.c2, c0, P);
    fq2_add_lazy(s, c0, c1);
    fq2_add_lazy(t, a.c0, a.c1);
    fq2_mul(t2, s, t, P);
    fq2_mul_nr(t1, t1, P);
    fq2_add(r.c0, t1, aa, P);
    fq2_sub(t2, t2, aa, P);
    fq2_sub(r.c1, t2, bb, P);
    fq2_add(r.c2, t3, bb, P);
}
// r = a (c1 v); r may be a
PAIR_FN void fq6_mul_by_1(Fq6E &r, const Fq6E &a, const Fq2E &c1, const FpParams<QL> &P) {
    Fq2E t0, t1, t2;
    fq2_mul(t0, a.c2, c1, P);
    fq2_mul(t1, a.c0, c1, P);
    fq2_mul(t2, a.c1, c1, P);
    fq2_mul_nr(r.c0, t0, P);
    fq2_set(r.c1, t1);
    fq2_set(r.c2, t2);
}
// 1 / a, a canonical; 0 -> 0
PAIR_FN void fq6_inv(Fq6E &r, const Fq6E &a, const FpParams<QL> &P) {
    Fq2E c0, c1, c2, t, s;
    fq2_mul(t, a.c1, a.c2, P);
    fq2_mul_nr(t, t, P);
    fq2_sqr(c0, a.c0, P);
    fq2_sub(c0, c0, t, P);
    fq2_sqr(c1, a.c2, P);
    fq2_mul_nr(c1, c1, P);
    fq2_mul(t, a.c0, a.c1, P);
    fq2_sub(c1, c1, t, P);
    fq2_sqr(c2, a.c1, P);
    fq2_mul(t, a.c0, a.c2, P);
    fq2_sub(c2, c2, t, P);
    fq2_mul(t, a.c2, c1, P);
    fq2_mul(s, a.c1, c2, P);
    fq2_add(t, t, s, P);
    fq2_mul_nr(t, t, P);
    fq2_mul(s, a.c0, c0, P);
    fq2_add(t, t, s, P);
    fq2_inv(t, t, P);
    fq2_mul(r.c0, t, c0, P);
    fq2_mul(r.c1, t, c1, P);
    fq2_mul(r.c2, t, c2, P);
}

// ---------------------------------------------------------------- Fq12
HB_HD void fq12_set(Fq12E &r, const Fq12E &a) { fq6_set(r.c0, a.c0); fq6_set(r.c1, a.c1); }
HB_HD void fq12_one(Fq12E &r, const FpParams<QL> &P) {
    fq2_one(r.c0.c0, P);
    fq2_zero(r.c0.c1);
    fq2_zero(r.c0.c2);
    fq2_zero(r.c1.c0);
    fq2_zero(r.c1.c1);
    fq2_zero(r.c1.c2);
}
HB_HD bool fq12_is_one(const Fq12E &a, const FpParams<QL> &P) {
    return fp_eq<QL>(a.c0.c0.c0, P.one) && fp_is_zero<QL>(a.c0.c0.c1) && fq2_is_zero(a.c0.c1) && fq2_is_zero(a.c0.c2) && fq2_is_zero(a.c1.c0) && fq2_is_zero(a.c1.c1) &&
           fq2_is_zero(a.c1.c2);
}
HB_HD bool fq12_is_zero(const Fq12E &a) {
    return fq2_is_zero(a.c0.c0) && fq2_is_zero(a.c0.c1) && fq2_is_zero(a.c0.c2) && fq2_is_zero(a.c1.c0) && fq2_is_zero(a.c1.c1) && fq2_is_zero(a.c1.c2);
}
// r = a b (canonical operands); r may be a or b
PAIR_FN void fq12_mul(Fq12E &r, const Fq12E &a, const Fq12E &b, const FpParams<QL> &P) {
    Fq6E aa, bb, s, t;
    fq6_mul(aa, a.c0, b.c0, P);
    fq6_mul(bb, a.c1, b.c1, P);
    fq6_add_lazy(s, a.c0, a.c1);
    fq6_add_lazy(t, b.c0, b.c1);
    fq6_mul(s, s, t, P);
    fq6_sub(s, s, aa, P);
    fq6_sub(r.c1, s, bb, P);
    fq6_mul_nr(bb, bb, P);
    fq6_add(r.c0, bb, aa, P);
}
// r = a^2 (canonical); r may be a.  c0 = (c0 + c1)(c0 + v c1) - ab - v ab, c1 = 2 ab, ab = c0 c1
PAIR_FN void fq12_sqr(Fq12E &r, const Fq12E &a, const FpParams<QL> &P) {
    Fq6E ab, s, t;
    fq6_mul(ab, a.c0, a.c1, P);
    fq6_add_lazy(s, a.c0, a.c1);
    fq6_mul_nr(t, a.c1, P);
    fq6_add_lazy(t, t, a.c0);
    fq6_mul(s, s, t, P);
    fq6_sub(s, s, ab, P);
    fq6_add(r.c1, ab, ab, P);
    fq6_mul_nr(ab, ab, P);
    fq6_sub(r.c0, s, ab, P);
}
// r = a (c0 + c1 v + c4 v w), the shape of a line; r may be a
PAIR_FN void fq12_mul_by_014(Fq12E &r, const Fq12E &a, const Fq2E &c0, const Fq2E &c1, const Fq2E &c4, const FpParams<QL> &P) {
    Fq6E aa, bb, s;
    Fq2E o;
    fq6_mul_by_01(aa, a.c0, c0, c1, P);
    fq6_mul_by_1(bb, a.c1, c4, P);
    fq2_add_lazy(o, c1, c4);
    fq6_add_lazy(s, a.c1, a.c0);
    fq6_mul_by_01(s, s, c0, o, P);
    fq6_sub(s, s, aa, P);
    fq6_sub(r.c1, s, bb, P);
    fq6_mul_nr(bb, bb, P);
    fq6_add(r.c0, bb, aa, P);
}
HB_HD void fq12_conj(Fq12E &r, const Fq12E &a, const FpParams<QL> &P) {
    fq6_set(r.c0, a.c0);
    fq6_neg(r.c1, a.c1, P);
}
// r = a^(Q^PW), PW = 1, 2, 3; r may be a
template <int PW> PAIR_FN void fq12_frobenius(Fq12E &r, const Fq12E &a, const FpParams<QL> &P) {
    static_assert(PW >= 1 && PW <= 3, "powers 1, 2 and 3");
    const Fq2E g12 = PW == 1 ? Fq2E PAIR_FROB12_C1_1 : PW == 2 ? Fq2E PAIR_FROB12_C1_2 : Fq2E PAIR_FROB12_C1_3;
    const Fq2E g61 = PW == 1 ? Fq2E PAIR_FROB6_C1_1 : PW == 2 ? Fq2E PAIR_FROB6_C1_2 : Fq2E PAIR_FROB6_C1_3;
    const Fq2E g62 = PW == 1 ? Fq2E PAIR_FROB6_C2_1 : PW == 2 ? Fq2E PAIR_FROB6_C2_2 : Fq2E PAIR_FROB6_C2_3;
    Fq12E t;
    if (PW & 1) {
        fq2_conj(t.c0.c0, a.c0.c0, P);
        fq2_conj(t.c0.c1, a.c0.c1, P);
        fq2_conj(t.c0.c2, a.c0.c2, P);
        fq2_conj(t.c1.c0, a.c1.c0, P);
        fq2_conj(t.c1.c1, a.c1.c1, P);
        fq2_conj(t.c1.c2, a.c1.c2, P);
    } else fq12_set(t, a);
    fq2_set(r.c0.c0, t.c0.c0);
    fq2_mul(r.c0.c1, t.c0.c1, g61, P);
    fq2_mul(r.c0.c2, t.c0.c2, g62, P);
    fq2_mul(t.c1.c1, t.c1.c1, g61, P);
    fq2_mul(t.c1.c2, t.c1.c2, g62, P);
    fq2_mul(r.c1.c0, t.c1.c0, g12, P);
    fq2_mul(r.c1.c1, t.c1.c1, g12, P);
    fq2_mul(r.c1.c2, t.c1.c2, g12, P);
}
// 1 / a down the tower to one fq_inv; 0 -> 0
PAIR_FN void fq12_inv(Fq12E &r, const Fq12E &a, const FpParams<QL> &P) {
    Fq6E t, s;
    fq6_mul(t, a.c0, a.c0, P);
    fq6_mul(s, a.c1, a.c1, P);
    fq6_mul_nr(s, s, P);
    fq6_sub(t, t, s, P);
    fq6_inv(t, t, P);
    fq6_mul(r.c0, a.c0, t, P);
    fq6_mul(s, a.c1, t, P);
    fq6_neg(r.c1, s, P);
}
// (c0, c1) = (a + b s)^2 in Fq4 = Fq2[s] / (s^2 - (1 + u)): three squarings
HB_HD void fq4_sqr(Fq2E &c0, Fq2E &c1, const Fq2E &a, const Fq2E &b, const FpParams<QL> &P) {
    Fq2E t0, t1, t2;
    fq2_sqr(t0, a, P);
    fq2_sqr(t1, b, P);
    fq2_add(t2, a, b, P);
    fq2_sqr(t2, t2, P);
    fq2_sub(t2, t2, t0, P);
    fq2_sub(c1, t2, t1, P);
    fq2_mul_nr(t2, t1, P);
    fq2_add(c0, t2, t0, P);
}
// r = 3 t - 2 z (plus: r = 3 t + 2 z)
HB_HD void fq2_cyclo_mix(Fq2E &r, const Fq2E &t, const Fq2E &z, bool plus, const FpParams<QL> &P) {
    Fq2E d;
    if (plus) fq2_add(d, t, z, P);
    else fq2_sub(d, t, z, P);
    fq2_add(d, d, d, P);
    fq2_add(r, d, t, P);
}
// r = a^2 for a in the cyclotomic subgroup (a^(Q^6 + 1) = 1 and a^(Q^4 - Q^2 + 1) = 1: everything after the easy part of the final
// exponentiation), Granger and Scott's squaring: 18 products where fq12_sqr takes 36; canonical; r may be a.  NOT a squaring elsewhere.
PAIR_FN void fq12_cyclo_sqr(Fq12E &r, const Fq12E &a, const FpParams<QL> &P) {
    Fq2E t0, t1, t2, t3, t4, t5;
    fq4_sqr(t0, t1, a.c0.c0, a.c1.c1, P);
    fq4_sqr(t2, t3, a.c1.c0, a.c0.c2, P);
    fq4_sqr(t4, t5, a.c0.c1, a.c1.c2, P);
    fq2_mul_nr(t5, t5, P);
    Fq12E o;
    fq2_cyclo_mix(o.c0.c0, t0, a.c0.c0, false, P);
    fq2_cyclo_mix(o.c1.c1, t1, a.c1.c1, true, P);
    fq2_cyclo_mix(o.c0.c1, t2, a.c0.c1, false, P);
    fq2_cyclo_mix(o.c1.c2, t3, a.c1.c2, true, P);
    fq2_cyclo_mix(o.c1.c0, t5, a.c1.c0, true, P);
    fq2_cyclo_mix(o.c0.c2, t4, a.c0.c2, false, P);
    fq12_set(r, o);
}
// r = conj(a^|x|) = a^x for a in the cyclotomic subgroup (half: |x| / 2); r must not be a
PAIR_FN void fq12_exp_x(Fq12E &r, const Fq12E &a, bool half, const FpParams<QL> &P) {
    uint64_t e = PAIR_X << 1;                                  // the bits below the leading one, at the top
    const int n = half ? 62 : 63;                              // |x| / 2 drops the last of them
    fq12_set(r, a);
#pragma unroll 1
    for (int b = 0; b < n; b++) {
        fq12_cyclo_sqr(r, r, P);
        if (e >> 63) fq12_mul(r, r, a, P);
        e <<= 1;
    }
    fq12_conj(r, r, P);
}
// f^(3 (Q^12 - 1) / R) by the reference's chain: the easy part, then five powers by |x|.  f = 0 -> 0 (never a Miller value)
PAIR_FN void fq12_final_exp(Fq12E &out, const Fq12E &f, const FpParams<QL> &P) {
    Fq12E r, y0, y1, y2, y3;
    fq12_inv(y0, f, P);
    fq12_conj(y1, f, P);
    fq12_mul(y1, y1, y0, P);
    fq12_frobenius<2>(r, y1, P);
    fq12_mul(r, r, y1, P);
    fq12_sqr(y0, r, P);
    fq12_exp_x(y1, y0, false, P);
    fq12_exp_x(y2, y1, true, P);
    fq12_conj(y3, r, P);
    fq12_mul(y1, y1, y3, P);
    fq12_conj(y1, y1, P);
    fq12_mul(y1, y1, y2, P);
    fq12_exp_x(y2, y1, false, P);
    fq12_exp_x(y3, y2, false, P);
    fq12_conj(y1, y1, P);
    fq12_mul(y3, y3, y1, P);
    fq12_conj(y1, y1, P);
    fq12_frobenius<3>(y1, y1, P);
    fq12_frobenius<2>(y2, y2, P);
    fq12_mul(y1, y1, y2, P);
    fq12_exp_x(y2, y3, false, P);
    fq12_mul(y2, y2, y0, P);
    fq12_mul(y2, y2, r, P);
    fq12_mul(y1, y1, y2, P);
    fq12_frobenius<1>(y2, y3, P);
    fq12_mul(out, y1, y2, P);
}

// ---------------------------------------------------------------- memory forms
// twelve words of canonical residue <-> Montgomery digits; returns whether the residue was below Q
HB_HD bool fq_load_mont(uint32_t (&r)[QL], const uint32_t *p, const FpParams<QL> &P) {
    uint32_t d[QL];
    load_digits<QL, QW>(d, p);
    const bool below = fq_below_q(d, P);
    fq_to_mont(r, d, P);
    return below;
}
HB_HD void fq_store_canon(uint32_t *p, const uint32_t (&a)[QL], const FpParams<QL> &P) {
    uint32_t d[QL];
    fq_from_mont(d, a, P);
    store_digits<QL, QW>(p, d);
}
HB_HD bool fq2_load(Fq2E &r, const uint32_t *p, const FpParams<QL> &P) {
    const bool a = fq_load_mont(r.c0, p, P), b = fq_load_mont(r.c1, p + QW, P);
    return a && b;
}
HB_HD void fq2_store(uint32_t *p, const Fq2E &a, const FpParams<QL> &P) {
    fq_store_canon(p, a.c0, P);
    fq_store_canon(p + QW, a.c1, P);
}
HB_HD bool fq12_load(Fq12E &r, const uint32_t *p, const FpParams<QL> &P) {
    bool ok = fq2_load(r.c0.c0, p, P);
    ok = fq2_load(r.c0.c1, p + 2 * QW, P) && ok;
    ok = fq2_load(r.c0.c2, p + 4 * QW, P) && ok;
    ok = fq2_load(r.c1.c0, p + 6 * QW, P) && ok;
    ok = fq2_load(r.c1.c1, p + 8 * QW, P) && ok;
    ok = fq2_load(r.c1.c2, p + 10 * QW, P) && ok;
    return ok;
}
HB_HD void fq12_store(uint32_t *p, const Fq12E &a, const FpParams<QL> &P) {
    fq2_store(p, a.c0.c0, P);
    fq2_store(p + 2 * QW, a.c0.c1, P);
    fq2_store(p + 4 * QW, a.c0.c2, P);
    fq2_store(p + 6 * QW, a.c1.c0, P);
    fq2_store(p + 8 * QW, a.c1.c1, P);
    fq2_store(p + 10 * QW, a.c1.c2, P);
}
// an Fq2 of a table entry: 28 Montgomery digits
HB_HD void pair_load_coef(Fq2E &r, const uint32_t *__restrict__ p) {
#pragma unroll
    for (int q = 0; q < QL; q++) { r.c0[q] = p[q]; r.c1[q] = p[QL + q]; }
}

// ---------------------------------------------------------------- one operation of the tower, for the self test and k_pair_op
// Does the operation read b?  And does it take this arg: the Frobenius power 1..3, the two shift counts of FQ_MUL_LAZY, else 0.
HB_HD bool pair_op_two(int op) {
    return op == HB_PAIR_OP_FQ2_MUL || op == HB_PAIR_OP_FQ6_MUL || op == HB_PAIR_OP_FQ12_MUL || op == HB_PAIR_OP_FQ6_MUL_BY_01 || op == HB_PAIR_OP_FQ6_MUL_BY_1 ||
           op == HB_PAIR_OP_FQ12_MUL_BY_014 || op == HB_PAIR_OP_FQ_MUL || op == HB_PAIR_OP_FQ_MUL_LAZY;
}
HB_HD bool pair_op_arg_ok(int op, int64_t arg) {
    if (op == HB_PAIR_OP_FQ12_FROBENIUS) return arg >= 1 && arg <= 3;
    if (op == HB_PAIR_OP_FQ_MUL_LAZY) return arg >= 0 && (arg & ~0x33ll) == 0;
    return arg == 0;
}
// r = k a, k = 2^sh, by doublings without the conditional subtraction: what the Karatsuba operand sums are made of (LAZY SUMS)
HB_HD void fq_shift_lazy(uint32_t (&r)[QL], const uint32_t (&a)[QL], int sh) {
    fp_set<QL>(r, a);
#pragma unroll 1
    for (int k = 0; k < sh; k++) fq_add_lazy(r, r, r);
}
// r = op(a, b): HB_PAIR_OP_* of hbmpc_hip.h and the Fq operations of hbmpc_hip_debug.h.  An operation on a smaller field takes the
// leading coordinates and copies the rest of a through; MUL_BY_01 / MUL_BY_1 / MUL_BY_014 take their sparse factor from the head of b.
// Returns false (r = a) for an unknown op or an arg the op does not take.  r is neither a nor b.
HB_HD bool pair_tower_elem(Fq12E &r, const Fq12E &a, const Fq12E &b, int op, int64_t arg, const FpParams<QL> &P) {
    fq12_set(r, a);
    if (!pair_op_arg_ok(op, arg)) return false;
    switch (op) {
    case HB_PAIR_OP_FQ2_MUL: fq2_mul(r.c0.c0, a.c0.c0, b.c0.c0, P); break;
    case HB_PAIR_OP_FQ2_SQR: fq2_sqr(r.c0.c0, a.c0.c0, P); break;
    case HB_PAIR_OP_FQ2_MUL_NR: fq2_mul_nr(r.c0.c0, a.c0.c0, P); break;
    case HB_PAIR_OP_FQ2_INV: fq2_inv(r.c0.c0, a.c0.c0, P); break;
    case HB_PAIR_OP_FQ6_MUL: fq6_mul(r.c0, a.c0, b.c0, P); break;
    case HB_PAIR_OP_FQ6_MUL_BY_01: fq6_mul_by_01(r.c0, a.c0, b.c0.c0, b.c0.c1, P); break;
    case HB_PAIR_OP_FQ6_MUL_BY_1: fq6_mul_by_1(r.c0, a.c0, b.c0.c0, P); break;
    case HB_PAIR_OP_FQ6_MUL_NR: fq6_mul_nr(r.c0, a.c0, P); break;
    case HB_PAIR_OP_FQ6_INV: fq6_inv(r.c0, a.c0, P); break;
    case HB_PAIR_OP_FQ12_MUL: fq12_mul(r, a, b, P); break;
    case HB_PAIR_OP_FQ12_SQR: fq12_sqr(r, a, P); break;
    case HB_PAIR_OP_FQ12_MUL_BY_014: fq12_mul_by_014(r, a, b.c0.c0, b.c0.c1, b.c0.c2, P); break;
    case HB_PAIR_OP_FQ12_CONJ: fq12_conj(r, a, P); break;
    case HB_PAIR_OP_FQ12_FROBENIUS:
        if (arg == 1) fq12_frobenius<1>(r, a, P);
        else if (arg == 2) fq12_frobenius<2>(r, a, P);
        else fq12_frobenius<3>(r, a, P);
        break;
    case HB_PAIR_OP_FQ12_INV: fq12_inv(r, a, P); break;
    case HB_PAIR_OP_FQ12_FINAL_EXP: fq12_final_exp(r, a, P); break;
    case HB_PAIR_OP_FQ12_CYCLO_SQR: fq12_cyclo_sqr(r, a, P); break;
    case HB_PAIR_OP_FQ_MUL: fq_mul(r.c0.c0.c0, a.c0.c0.c0, b.c0.c0.c0, P); break;
    case HB_PAIR_OP_FQ_MUL_LAZY: {
        uint32_t s[QL], t[QL];
        fq_shift_lazy(s, a.c0.c0.c0, (int)(arg >> 4));
        fq_shift_lazy(t, b.c0.c0.c0, (int)(arg & 3));
        fq_mul(r.c0.c0.c0, s, t, P);
        break;
    }
    case HB_PAIR_OP_FQ_INV: fq_inv(r.c0.c0.c0, a.c0.c0.c0, P); break;
    default: return false;
    }
    return true;
}

// ---------------------------------------------------------------- the loop
struct PairTables { const uint32_t *__restrict__ t[4]; };

// f *= the line `line` of every live pair, evaluated at its point
HB_HD void pair_lines(Fq12E &f, const PairTables &T, int K, int line, const G1Aff (&pt)[4], const FpParams<QL> &P) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (k < K && !pt[k].inf) {
            const uint32_t *__restrict__ e = T.t[k] + line * PAIR_ENT;
            Fq2E c0, c1, c2;
            pair_load_coef(c0, e);
            pair_load_coef(c1, e + 2 * QL);
            pair_load_coef(c2, e + 4 * QL);
            fq2_mul_fq(c0, c0, pt[k].y, P);
            fq2_mul_fq(c1, c1, pt[k].x, P);
            fq12_mul_by_014(f, f, c2, c1, c0, P);
        }
    }
}
// out = FE(prod_k ML(P_k, Q_k)) over K pairs, the K points at `points`; an identity point contributes 1.  Returns whether every
// point is the identity or has coordinates below Q and lies on the curve (the value is computed from the reduced words regardless).
HB_HD bool pair_product_elem(Fq12E &out, const PairTables &T, int K, const uint32_t *points, const FpParams<QL> &P) {
    G1Aff pt[4];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (k < K) {
            bool good = g1_load(pt[k], points + k * G1_PT, P);
            if (!pt[k].inf) good = good && g1_on_curve(pt[k], P);
            ok = ok && good;
        } else pt[k].inf = true;
    }
    Fq12E f;
    fq12_one(f, P);
    uint64_t e = (PAIR_X >> 1) << 2;                            // the bits of |x| / 2 below the leading one (bit 62), at the top
    int line = 0;
#pragma unroll 1
    for (int b = 0; b < 62; b++) {
        pair_lines(f, T, K, line++, pt, P);
        if (e >> 63) pair_lines(f, T, K, line++, pt, P);
        e <<= 1;
        fq12_sqr(f, f, P);
    }
    pair_lines(f, T, K, line, pt, P);
    fq12_conj(f, f, P);
    fq12_final_exp(out, f, P);
    return ok;
}

// ---------------------------------------------------------------- host side
// One prepared point: 68 x 3 Fq2 of canonical words (coefficient, then c0, c1: 12 words each) -> the table's Montgomery digits.
// Returns whether every residue was below Q.
static bool pair_table_fill(uint32_t *table, const uint32_t *coeffs) {
    const FpParams<QL> P = fq_params();
    bool ok = true;
    for (int i = 0; i < PAIR_LINES * 6; i++) {
        uint32_t m[QL];
        ok = fq_load_mont(m, coeffs + (int64_t)i * QW, P) && ok;
        for (int q = 0; q < QL; q++) table[(int64_t)i * QL + q] = m[q];
    }
    return ok;
}
// The Frobenius literals from Q alone: gamma_1 = (1 + u)^((Q - 1) / 6) by square and multiply over the exponent derived from Q - 2 by
// a long division, gamma_(i + 1) = gamma_1 conj(gamma_i) (since (Q^(i+1) - 1) / 6 = (Q - 1) / 6 + Q (Q^i - 1) / 6), and their squares
// and fourth powers.
static bool pair_consts_derive() {
    if (!g1_consts_ok()) return false;
    const FpParams<QL> P = fq_params();
    static const uint32_t qm2[QW] = G1_QM2_WORDS, lit[QW] = PAIR_QM1_6_WORDS;
    uint32_t e[QW];
    uint64_t rem = 0;
    for (int i = QW - 1; i >= 0; i--) {
        const uint64_t cur = (rem << 32) | (uint64_t)(qm2[i] + (i == 0 ? 1u : 0u));   // Q - 1: Q - 2 ends in ...a9
        e[i] = (uint32_t)(cur / 6);
        rem = cur % 6;
    }
    if (rem) return false;
    for (int i = 0; i < QW; i++) if (e[i] != lit[i]) return false;
    Fq2E xi, g1, g;
    fp_set<QL>(xi.c0, P.one);
    fp_set<QL>(xi.c1, P.one);
    fq2_one(g1, P);
    for (int b = 32 * QW - 1; b >= 0; b--) {
        fq2_sqr(g1, g1, P);
        if ((e[b >> 5] >> (b & 31)) & 1u) fq2_mul(g1, g1, xi, P);
    }
    const Fq2E l12[3] = {PAIR_FROB12_C1_1, PAIR_FROB12_C1_2, PAIR_FROB12_C1_3}, l61[3] = {PAIR_FROB6_C1_1, PAIR_FROB6_C1_2, PAIR_FROB6_C1_3},
               l62[3] = {PAIR_FROB6_C2_1, PAIR_FROB6_C2_2, PAIR_FROB6_C2_3};
    fq2_set(g, g1);
    for (int i = 0; i < 3; i++) {
        Fq2E s, f;
        fq2_sqr(s, g, P);
        fq2_sqr(f, s, P);
        if (!fq2_eq(g, l12[i]) || !fq2_eq(s, l61[i]) || !fq2_eq(f, l62[i])) return false;
        fq2_conj(s, g, P);
        fq2_mul(g, g1, s, P);
    }
    return true;
}
static bool pair_consts_ok() {
    static const bool ok = pair_consts_derive();
    return ok;
}

}  // namespace hb

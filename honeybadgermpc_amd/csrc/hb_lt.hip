// hb_lt.hip -- less-than of shared field elements, the reference's LessThan mixin (progs/mixins/share_comparison.py:83-212, "An Improved
// Multiparty Protocol for Comparison of Secret-shared Values", Reistad 2007) for arrays of values -- restated on fp29.hpp, not translated.
//
// For a pair a, b < (p - 1) / 2 the protocol opens c = 2 (a - b) + r, r a dealt random residue with bit shares r_0 .. r_{L-1}, L the
// bit length of p, and [a < b] = c_0 xor r_0 xor [r > c].  The reference's x = sum_i r_i (1 - c_i) prod_{j>i} (1 + (r_j xor c_j))
// (:137-163) is the g at the root of the carry tree's operator (g1, p1) o (g2, p2) = (g1 + p1 g2, p1 p2) of hb_fxp.hip over leaves that
// are affine in [r_i], because c_i is public; its least significant bit is [r > c].  The same tree over the leaves of the comparison
// itself gives [r > c] as a bit.  The tree's levels are FxpCarryMaskRow / FxpCarryCombineRow of hb_fxp.hip, unchanged.
//
// The steps are rows under the generic kernel k_rows (hb_rows.hpp):
// LtMaskRow        2 (a - b) + r, the array to open (b may be absent: 2 a + r).
// LtLeavesRow      (g, p), L planes each, most significant bit first; bit i of c is taken from the packed words and selects:
//                     HB_LT_DIRECT     c_i = 0 -> (r_i, 1 - r_i)   c_i = 1 -> (0, r_i)         g = [r_i > c_i], p = [r_i = c_i]: root g = [r > c]
//                     HB_LT_REFERENCE  c_i = 0 -> (r_i, 1 + r_i)   c_i = 1 -> (0, 2 - r_i)     the reference's r_i (1 - c_i), 1 + (r_i xor c_i): root g = x
//                  No triple, no open.  (The reference spends a product and an open on every bit, one after the other.)
// LtXorMaskRow     DIRECT, after the tree gave w = [r > c]: u = c_0 ? 1 - r_0 : r_0 and the array to open [u - pa, w - qa].
// LtDmaskRow       REFERENCE, after the tree gave x: u, and ONE array of five planes [s + x, u - pa, s_0 - qa, s_1 - pb, s_2 - qb] with
//                  s_0, s_1, s_2 = planes 0, L - 1, L - 2 of the second mask's bit shares (:178-182): d = s + x and the masked operands of
//                  the two products that do not depend on d travel in one open.
// LtMidRow         that array opened: v = u xor s_0 and s_1 s_2 by ew_beaver_elem, d_0 by the reference's four-way select (:186-199;
//                  d < p < 2^L, so the three comparisons of d read bits L - 1 and L - 2 of d alone), the array to open [v - pc, d_0 - qc].
// LtXorFinishRow   both modes: u + v - 2 [u v], the last xor.
//
// Operands and results are packed canonical residues.  The per-element bodies are HB_HD functions; a step's row -- which operands it
// loads, which body it calls, where it stores -- is an HB_HD function over a memory policy, so hb_selftest_lt runs on the host the very
// rows, arithmetic and addressing, that k_rows runs on the device.
//
// Launch shape (all steps): 256-thread workgroups, one element a thread in x; LtLeavesRow takes the plane in blockIdx.y (c is one
// element a thread and stays in L2 for the L planes).  No LDS, no grid stride, one launch a call.  Bit planes, triples and opened
// values are read once: the 32-byte width takes the non-temporal loads, as EwBeaverRow.
// Compiler's report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; scratch = 0 bytes for every kernel):
//   LtMaskRow<9, 8>        29 VGPRs with b, 30 without: 8 waves a SIMD        LtMaskRow<3, 2>        12 VGPRs: 8 waves
//   LtLeavesRow<9, 8>      41 VGPRs: 8 waves                                  LtLeavesRow<3, 2>      17 VGPRs: 8 waves
//   LtXorMaskRow<9, 8>     56 VGPRs: 8 waves                                  LtXorMaskRow<3, 2>     24 VGPRs: 8 waves
//   LtDmaskRow<9, 8>      101 VGPRs: 4 waves                                  LtDmaskRow<3, 2>       34 VGPRs: 8 waves
//   LtMidRow<9, 8>         83 VGPRs: 5 waves                                  LtMidRow<3, 2>         56 VGPRs: 8 waves
//   LtXorFinishRow<9, 8>   73 VGPRs: 6 waves                                  LtXorFinishRow<3, 2>   29 VGPRs: 8 waves
// LtDmaskRow<9, 8> held 68 VGPRs (7 waves) while its pointers were __restrict__ kernel parameters; pointers in an argument struct
// carry none and the compiler keeps more of the 21 loads' results live.  The launch streams 17 elements an element and took the same
// time either way (profiles/less_than.txt), so it has no kernel of its own.
// (DESIGN.md section 3p has the schedule and the counts.)
#include "hb_common.hpp"
#include "hb_ew_elem.hpp"
#include "hb_lt_elem.hpp"
#include "hb_rows.hpp"

using namespace hb;

namespace hb {

// ---------------------------------------------------------------- per-element bodies (host and device)
// o = 2 (a - b) + r; HAS_B = false: 2 a + r
template <int NL, int NW, bool HAS_B>
HB_HD void lt_mask_elem(uint32_t (&o)[NW], const uint32_t (&aw)[NW], const uint32_t (&bw)[NW], const uint32_t (&rw)[NW], const FpParams<NL> &P) {
    uint32_t z[NL], t[NL], u[NL];
    unpack<NL, NW>(z, aw);
    if constexpr (HAS_B) {
        unpack<NL, NW>(t, bw);
        fp_sub<NL>(u, z, t, P);
        fp_set<NL>(z, u);
    }
    fp_add<NL>(t, z, z, P);
    unpack<NL, NW>(z, rw);
    fp_add<NL>(u, t, z, P);
    pack<NL, NW>(o, u);
}

// (the leaf of the public bit of c against the share of the same bit of r, lt_leaf_elem, is hb_lt_elem.hpp's: hb_offsb.hip makes the same leaves)

// u = c_0 xor [r_0]: c_0 ? 1 - r_0 : r_0
template <int NL, int NW> HB_HD void lt_u_elem(uint32_t (&uw)[NW], const uint32_t (&cw)[NW], const uint32_t (&r0w)[NW], const FpParams<NL> &P) {
    uint32_t b[NL], one[NL], t[NL];
    unpack<NL, NW>(b, r0w);
    small_digits<NL>(one, 1);
    fp_sub<NL>(t, one, b, P);
    const uint32_t c0 = cw[0] & 1u;
#pragma unroll
    for (int q = 0; q < NL; q++) t[q] = c0 ? t[q] : b[q];
    pack<NL, NW>(uw, t);
}

// DIRECT: u, m0 = u - pa, m1 = w - qa
template <int NL, int NW>
HB_HD void lt_xor_mask_elem(uint32_t (&uw)[NW], uint32_t (&m0)[NW], uint32_t (&m1)[NW], const uint32_t (&cw)[NW], const uint32_t (&r0w)[NW], const uint32_t (&ww)[NW],
                            const uint32_t (&paw)[NW], const uint32_t (&qaw)[NW], const FpParams<NL> &P) {
    lt_u_elem<NL, NW>(uw, cw, r0w, P);
    diff_elem<NL, NW>(m0, uw, paw, P);
    diff_elem<NL, NW>(m1, ww, qaw, P);
}

// REFERENCE: u, m0 = s + x, m1 = u - pa, m2 = s_0 - qa, m3 = s_1 - pb, m4 = s_2 - qb
template <int NL, int NW>
HB_HD void lt_dmask_elem(uint32_t (&uw)[NW], uint32_t (&m0)[NW], uint32_t (&m1)[NW], uint32_t (&m2)[NW], uint32_t (&m3)[NW], uint32_t (&m4)[NW], const uint32_t (&cw)[NW],
                         const uint32_t (&r0w)[NW], const uint32_t (&xw)[NW], const uint32_t (&sw)[NW], const uint32_t (&s0w)[NW], const uint32_t (&s1w)[NW],
                         const uint32_t (&s2w)[NW], const uint32_t (&paw)[NW], const uint32_t (&qaw)[NW], const uint32_t (&pbw)[NW], const uint32_t (&qbw)[NW],
                         const FpParams<NL> &P) {
    uint32_t s[NL], x[NL], t[NL];
    unpack<NL, NW>(s, sw);
    unpack<NL, NW>(x, xw);
    fp_add<NL>(t, s, x, P);
    pack<NL, NW>(m0, t);
    lt_u_elem<NL, NW>(uw, cw, r0w, P);
    diff_elem<NL, NW>(m1, uw, paw, P);
    diff_elem<NL, NW>(m2, s0w, qaw, P);
    diff_elem<NL, NW>(m3, s1w, pbw, P);
    diff_elem<NL, NW>(m4, s2w, qbw, P);
}

// o = x + y - 2 [x y] with [x y] the fused Beaver step over the opened masked operands d, e
template <int NL, int NW>
HB_HD void lt_xor_elem(uint32_t (&o)[NW], const uint32_t (&xw)[NW], const uint32_t (&yw)[NW], const uint32_t (&dw)[NW], const uint32_t (&ew)[NW], const uint32_t (&pw)[NW],
                       const uint32_t (&qw)[NW], const uint32_t (&pqw)[NW], const FpParams<NL> &P) {
    uint32_t mw[NW], m[NL], x[NL], y[NL], t[NL];
    ew_beaver_elem<NL, NW>(mw, dw, ew, pw, qw, pqw, P);
    unpack<NL, NW>(m, mw);
    unpack<NL, NW>(x, xw);
    unpack<NL, NW>(y, yw);
    fp_add<NL>(t, x, y, P);
    fp_sub<NL>(x, t, m, P);
    fp_sub<NL>(t, x, m, P);
    pack<NL, NW>(o, t);
}

// o0 .. o4 the array of lt_dmask_elem opened.  v = u xor s_0; d_0 = (1 - s_1 - s_2 + s_1 s_2) d0 + (s_2 - s_1 s_2) (d0 ^ [d < 2^(L-2)]) +
// (s_1 - s_1 s_2) (d0 ^ [d < 2^(L-1)]) + s_1 s_2 (d0 ^ [d < 2^(L-1) + 2^(L-2)]): every public factor is a bit, so the sum is a sum of
// selected terms; m0 = v - pc, m1 = d_0 - qc
template <int NL, int NW>
HB_HD void lt_mid_elem(uint32_t (&vw)[NW], uint32_t (&d0w)[NW], uint32_t (&m0)[NW], uint32_t (&m1)[NW], const uint32_t (&o0)[NW], const uint32_t (&o1)[NW],
                       const uint32_t (&o2)[NW], const uint32_t (&o3)[NW], const uint32_t (&o4)[NW], const uint32_t (&uw)[NW], const uint32_t (&s0w)[NW],
                       const uint32_t (&s1w)[NW], const uint32_t (&s2w)[NW], const uint32_t (&paw)[NW], const uint32_t (&qaw)[NW], const uint32_t (&pqaw)[NW],
                       const uint32_t (&pbw)[NW], const uint32_t (&qbw)[NW], const uint32_t (&pqbw)[NW], const uint32_t (&pcw)[NW], const uint32_t (&qcw)[NW], int L,
                       const FpParams<NL> &P) {
    lt_xor_elem<NL, NW>(vw, uw, s0w, o1, o2, paw, qaw, pqaw, P);
    uint32_t spw[NW], sp[NL], s1[NL], s2[NL], t[NL], w[NL], acc[NL];
    ew_beaver_elem<NL, NW>(spw, o3, o4, pbw, qbw, pqbw, P);
    unpack<NL, NW>(sp, spw);
    unpack<NL, NW>(s1, s1w);
    unpack<NL, NW>(s2, s2w);
    const uint32_t d0 = o0[0] & 1u, t1 = word_bit<NW>(o0, L - 1), t2 = word_bit<NW>(o0, L - 2);
    const uint32_t dx1 = d0 ^ (t1 ^ 1u), dx2 = d0 ^ ((t1 | t2) ^ 1u), dx12 = d0 ^ ((t1 & t2) ^ 1u);
    // (1 - s_1 - s_2 + s_1 s_2) d0
    small_digits<NL>(w, 1);
    fp_sub<NL>(t, w, s1, P);
    fp_sub<NL>(w, t, s2, P);
    fp_add<NL>(t, w, sp, P);
#pragma unroll
    for (int q = 0; q < NL; q++) acc[q] = d0 ? t[q] : 0u;
    fp_sub<NL>(t, s2, sp, P);
    fp_add<NL>(w, acc, t, P);
#pragma unroll
    for (int q = 0; q < NL; q++) acc[q] = dx2 ? w[q] : acc[q];
    fp_sub<NL>(t, s1, sp, P);
    fp_add<NL>(w, acc, t, P);
#pragma unroll
    for (int q = 0; q < NL; q++) acc[q] = dx1 ? w[q] : acc[q];
    fp_add<NL>(w, acc, sp, P);
#pragma unroll
    for (int q = 0; q < NL; q++) acc[q] = dx12 ? w[q] : acc[q];
    pack<NL, NW>(d0w, acc);
    diff_elem<NL, NW>(m0, vw, pcw, P);
    diff_elem<NL, NW>(m1, d0w, qcw, P);
}

// ---------------------------------------------------------------- the steps' rows (host and device, over a memory policy: hb_rows.hpp)
// Every output is an array of its own, and every row issues all its loads ahead of its first store.
struct LtMaskArgs { const uint32_t *a, *b, *r; uint32_t *masked; };

template <bool HAS_B> struct LtMaskRow {
    template <int NL, int NW, class Mem>
    HB_HD static void run(const LtMaskArgs &A, int, int64_t i, int64_t, const Mem &mem, const FpParams<NL> &P) {
        uint32_t aw[NW], bw[NW], rw[NW], ow[NW];
        mem.load(aw, A.a, i);
        if constexpr (HAS_B) mem.load(bw, A.b, i);
        else {
#pragma unroll
            for (int q = 0; q < NW; q++) bw[q] = 0;
        }
        mem.load(rw, A.r, i);
        lt_mask_elem<NL, NW, HAS_B>(ow, aw, bw, rw, P);
        mem.store(A.masked, i, ow);
    }
};

// g, p: L planes each; plane y holds bit L - 1 - y
struct LtLeavesArgs { const uint32_t *c, *r_bits; uint32_t *g, *p; int L, mode; };

struct LtLeavesRow {
    template <int NL, int NW, class Mem>
    HB_HD static void run(const LtLeavesArgs &A, int y, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
        const int64_t j = y;
        const int bit = A.L - 1 - y;
        uint32_t cw[NW], bw[NW], gw[NW], pw[NW];
        mem.load(cw, A.c, i);
        mem.once(bw, A.r_bits, (int64_t)bit * count + i);
        lt_leaf_elem<NL, NW>(gw, pw, word_bit<NW>(cw, bit), bw, A.mode, P);
        mem.store(A.g, j * count + i, gw);
        mem.store(A.p, j * count + i, pw);
    }
};

// masked: (2, count)
struct LtXorMaskArgs { const uint32_t *c, *r0, *w, *pa, *qa; uint32_t *u, *masked; };

struct LtXorMaskRow {
    template <int NL, int NW, class Mem>
    HB_HD static void run(const LtXorMaskArgs &A, int, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
        uint32_t cw[NW], rw[NW], ww[NW], paw[NW], qaw[NW], uw[NW], m0[NW], m1[NW];
        mem.load(cw, A.c, i); mem.load(rw, A.r0, i); mem.once(ww, A.w, i);
        mem.once(paw, A.pa, i); mem.once(qaw, A.qa, i);
        lt_xor_mask_elem<NL, NW>(uw, m0, m1, cw, rw, ww, paw, qaw, P);
        mem.store(A.u, i, uw);
        mem.store(A.masked, i, m0);
        mem.store(A.masked, count + i, m1);
    }
};

// masked: (5, count); s_0, s_1, s_2 are planes 0, L - 1, L - 2 of s_bits
struct LtDmaskArgs { const uint32_t *c, *r0, *x, *s, *s_bits, *pa, *qa, *pb, *qb; uint32_t *u, *masked; int L; };

struct LtDmaskRow {
    template <int NL, int NW, class Mem>
    HB_HD static void run(const LtDmaskArgs &A, int, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
        uint32_t cw[NW], rw[NW], xw[NW], sw[NW], s0w[NW], s1w[NW], s2w[NW], paw[NW], qaw[NW], pbw[NW], qbw[NW], uw[NW], m0[NW], m1[NW], m2[NW], m3[NW], m4[NW];
        mem.load(cw, A.c, i); mem.load(rw, A.r0, i); mem.once(xw, A.x, i); mem.load(sw, A.s, i);
        mem.load(s0w, A.s_bits, i);
        mem.load(s1w, A.s_bits, (int64_t)(A.L - 1) * count + i);
        mem.load(s2w, A.s_bits, (int64_t)(A.L - 2) * count + i);
        mem.once(paw, A.pa, i); mem.once(qaw, A.qa, i); mem.once(pbw, A.pb, i); mem.once(qbw, A.qb, i);
        lt_dmask_elem<NL, NW>(uw, m0, m1, m2, m3, m4, cw, rw, xw, sw, s0w, s1w, s2w, paw, qaw, pbw, qbw, P);
        mem.store(A.u, i, uw);
        mem.store(A.masked, i, m0);
        mem.store(A.masked, count + i, m1);
        mem.store(A.masked, 2 * count + i, m2);
        mem.store(A.masked, 3 * count + i, m3);
        mem.store(A.masked, 4 * count + i, m4);
    }
};

// opened: (5, count); masked: (2, count)
struct LtMidArgs { const uint32_t *opened, *u, *s_bits, *pa, *qa, *pqa, *pb, *qb, *pqb, *pc, *qc; uint32_t *v, *d0, *masked; int L; };

struct LtMidRow {
    template <int NL, int NW, class Mem>
    HB_HD static void run(const LtMidArgs &A, int, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
        uint32_t o0[NW], o1[NW], o2[NW], o3[NW], o4[NW], uw[NW], s0w[NW], s1w[NW], s2w[NW], paw[NW], qaw[NW], pqaw[NW], pbw[NW], qbw[NW], pqbw[NW], pcw[NW], qcw[NW];
        uint32_t vw[NW], d0w[NW], m0[NW], m1[NW];
        mem.once(o0, A.opened, i); mem.once(o1, A.opened, count + i); mem.once(o2, A.opened, 2 * count + i);
        mem.once(o3, A.opened, 3 * count + i); mem.once(o4, A.opened, 4 * count + i);
        mem.once(uw, A.u, i);
        mem.load(s0w, A.s_bits, i);
        mem.load(s1w, A.s_bits, (int64_t)(A.L - 1) * count + i);
        mem.load(s2w, A.s_bits, (int64_t)(A.L - 2) * count + i);
        mem.once(paw, A.pa, i); mem.once(qaw, A.qa, i); mem.once(pqaw, A.pqa, i);
        mem.once(pbw, A.pb, i); mem.once(qbw, A.qb, i); mem.once(pqbw, A.pqb, i);
        mem.load(pcw, A.pc, i); mem.load(qcw, A.qc, i);
        lt_mid_elem<NL, NW>(vw, d0w, m0, m1, o0, o1, o2, o3, o4, uw, s0w, s1w, s2w, paw, qaw, pqaw, pbw, qbw, pqbw, pcw, qcw, A.L, P);
        mem.store(A.v, i, vw);
        mem.store(A.d0, i, d0w);
        mem.store(A.masked, i, m0);
        mem.store(A.masked, count + i, m1);
    }
};

// opened: (2, count)
struct LtXorFinishArgs { const uint32_t *opened, *u, *v, *tp, *tq, *tpq; uint32_t *out; };

struct LtXorFinishRow {
    template <int NL, int NW, class Mem>
    HB_HD static void run(const LtXorFinishArgs &A, int, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
        uint32_t dw[NW], ew[NW], uw[NW], vw[NW], pw[NW], qw[NW], pqw[NW], ow[NW];
        mem.once(dw, A.opened, i); mem.once(ew, A.opened, count + i);
        mem.once(uw, A.u, i); mem.once(vw, A.v, i);
        mem.once(pw, A.tp, i); mem.once(qw, A.tq, i); mem.once(pqw, A.tpq, i);
        lt_xor_elem<NL, NW>(ow, uw, vw, dw, ew, pw, qw, pqw, P);
        mem.store(A.out, i, ow);
    }
};

// ---------------------------------------------------------------- host side
// One step function a step (hb_rows.hpp): its checks, Args fill and row count run under a DeviceRun in the entry point, a HostRun in hb_selftest_lt.
static bool lt_mode_ok(int mode) { return mode == HB_LT_DIRECT || mode == HB_LT_REFERENCE; }

template <class Run> static int lt_mask_step(const Run &run, const uint64_t *a, const uint64_t *b, const uint64_t *r, uint64_t *masked, int64_t count) {
    if (count < 0 || (count > 0 && (!a || !r || !masked))) return HB_ERR_BAD_ARG;
    if (count == 0) return HB_OK;
    const int64_t eb = run.elem_bytes() * count;
    const RowSpan outs[1] = {{masked, 1}}, ins[3] = {{a, 1}, {b, 1}, {r, 1}};
    if (!outputs_apart(outs, 1, ins, 3, eb)) return run.fail(HB_ERR_BAD_ARG, "hb_lt_mask: masked is an array of its own");
    const LtMaskArgs A = {u32(a), u32(b), u32(r), u32(masked)};
    if (b) return run.template rows<LtMaskRow<true>>(A, 1, count);
    return run.template rows<LtMaskRow<false>>(A, 1, count);
}

template <class Run> static int lt_leaves_step(const Run &run, const uint64_t *c, const uint64_t *r_bits, int L, int mode, uint64_t *g, uint64_t *p, int64_t count) {
    if (count < 0 || (count > 0 && (!c || !r_bits || !g || !p))) return HB_ERR_BAD_ARG;
    if (!lt_mode_ok(mode)) return run.fail(HB_ERR_BAD_ARG, "hb_lt_leaves: unknown mode");
    if (L != run.bits()) return run.fail(HB_ERR_BAD_ARG, "hb_lt_leaves: L is the bit length of the modulus");
    if (count == 0) return HB_OK;
    const int64_t eb = run.elem_bytes() * count;
    const RowSpan outs[2] = {{g, L}, {p, L}}, ins[2] = {{c, 1}, {r_bits, L}};
    if (!outputs_apart(outs, 2, ins, 2, eb)) return run.fail(HB_ERR_BAD_ARG, "hb_lt_leaves: g and p are arrays of their own");
    const LtLeavesArgs A = {u32(c), u32(r_bits), u32(g), u32(p), L, mode};
    return run.template rows<LtLeavesRow>(A, L, count);
}

template <class Run> static int lt_xor_mask_step(const Run &run, const uint64_t *c, const uint64_t *r0, const uint64_t *w, const uint64_t *pa, const uint64_t *qa,
                                                 uint64_t *u, uint64_t *masked, int64_t count) {
    if (count < 0 || (count > 0 && (!c || !r0 || !w || !pa || !qa || !u || !masked))) return HB_ERR_BAD_ARG;
    if (count == 0) return HB_OK;
    const int64_t eb = run.elem_bytes() * count;
    const RowSpan outs[2] = {{u, 1}, {masked, 2}}, ins[5] = {{c, 1}, {r0, 1}, {w, 1}, {pa, 1}, {qa, 1}};
    if (!outputs_apart(outs, 2, ins, 5, eb)) return run.fail(HB_ERR_BAD_ARG, "hb_lt_xor_mask: u and masked are arrays of their own");
    const LtXorMaskArgs A = {u32(c), u32(r0), u32(w), u32(pa), u32(qa), u32(u), u32(masked)};
    return run.template rows<LtXorMaskRow>(A, 1, count);
}

template <class Run> static int lt_dmask_step(const Run &run, const uint64_t *c, const uint64_t *r0, const uint64_t *x, const uint64_t *s, const uint64_t *s_bits, int L,
                                              const uint64_t *pa, const uint64_t *qa, const uint64_t *pb, const uint64_t *qb, uint64_t *u, uint64_t *masked,
                                              int64_t count) {
    if (count < 0 || (count > 0 && (!c || !r0 || !x || !s || !s_bits || !pa || !qa || !pb || !qb || !u || !masked)))
        return HB_ERR_BAD_ARG;
    if (L != run.bits()) return run.fail(HB_ERR_BAD_ARG, "hb_lt_dmask: L is the bit length of the modulus");
    if (count == 0) return HB_OK;
    const int64_t eb = run.elem_bytes() * count;
    const RowSpan outs[2] = {{u, 1}, {masked, 5}},
                 ins[9] = {{c, 1}, {r0, 1}, {x, 1}, {s, 1}, {s_bits, L}, {pa, 1}, {qa, 1}, {pb, 1}, {qb, 1}};
    if (!outputs_apart(outs, 2, ins, 9, eb)) return run.fail(HB_ERR_BAD_ARG, "hb_lt_dmask: u and masked are arrays of their own");
    const LtDmaskArgs A = {u32(c), u32(r0), u32(x), u32(s), u32(s_bits), u32(pa), u32(qa), u32(pb), u32(qb), u32(u), u32(masked), L};
    return run.template rows<LtDmaskRow>(A, 1, count);
}

template <class Run> static int lt_mid_step(const Run &run, const uint64_t *opened, const uint64_t *u, const uint64_t *s_bits, int L, const uint64_t *pa,
                                            const uint64_t *qa, const uint64_t *pqa, const uint64_t *pb, const uint64_t *qb, const uint64_t *pqb, const uint64_t *pc,
                                            const uint64_t *qc, uint64_t *v, uint64_t *d0, uint64_t *masked, int64_t count) {
    if (count < 0) return HB_ERR_BAD_ARG;
    const uint64_t *trip[8] = {pa, qa, pqa, pb, qb, pqb, pc, qc};
    if (count > 0) {
        for (const uint64_t *t : trip) if (!t) return HB_ERR_BAD_ARG;
        if (!opened || !u || !s_bits || !v || !d0 || !masked) return HB_ERR_BAD_ARG;
    }
    if (L != run.bits()) return run.fail(HB_ERR_BAD_ARG, "hb_lt_mid: L is the bit length of the modulus");
    if (count == 0) return HB_OK;
    const int64_t eb = run.elem_bytes() * count;
    const RowSpan outs[3] = {{v, 1}, {d0, 1}, {masked, 2}};
    RowSpan ins[11] = {{opened, 5}, {u, 1}, {s_bits, L}};
    for (int k = 0; k < 8; k++) ins[3 + k] = {trip[k], 1};
    if (!outputs_apart(outs, 3, ins, 11, eb)) return run.fail(HB_ERR_BAD_ARG, "hb_lt_mid: the outputs are arrays of their own");
    const LtMidArgs A = {u32(opened), u32(u), u32(s_bits), u32(pa), u32(qa), u32(pqa), u32(pb), u32(qb), u32(pqb), u32(pc), u32(qc),
                         u32(v), u32(d0), u32(masked), L};
    return run.template rows<LtMidRow>(A, 1, count);
}

template <class Run> static int lt_xor_finish_step(const Run &run, const uint64_t *opened, const uint64_t *u, const uint64_t *v, const uint64_t *p, const uint64_t *q,
                                                   const uint64_t *pq, uint64_t *out, int64_t count) {
    if (count < 0 || (count > 0 && (!opened || !u || !v || !p || !q || !pq || !out))) return HB_ERR_BAD_ARG;
    if (count == 0) return HB_OK;
    const int64_t eb = run.elem_bytes() * count;
    const RowSpan outs[1] = {{out, 1}}, ins[6] = {{opened, 2}, {u, 1}, {v, 1}, {p, 1}, {q, 1}, {pq, 1}};
    if (!outputs_apart(outs, 1, ins, 6, eb)) return run.fail(HB_ERR_BAD_ARG, "hb_lt_xor_finish: out is an array of its own");
    const LtXorFinishArgs A = {u32(opened), u32(u), u32(v), u32(p), u32(q), u32(pq), u32(out)};
    return run.template rows<LtXorFinishRow>(A, 1, count);
}

}  // namespace hb

extern "C" {

int hb_lt_mask(hb_ctx *ctx, const uint64_t *a_dev, const uint64_t *b_dev, const uint64_t *r_dev, uint64_t *masked_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : lt_mask_step(DeviceRun{ctx, (hipStream_t)stream, "hb_lt_mask"}, a_dev, b_dev, r_dev, masked_dev, count);
}

int hb_lt_leaves(hb_ctx *ctx, const uint64_t *c_dev, const uint64_t *r_bits_dev, int L, int mode, uint64_t *g_dev, uint64_t *p_dev, int64_t count, void *stream) {
    HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : lt_leaves_step(DeviceRun{ctx, (hipStream_t)stream, "hb_lt_leaves"}, c_dev, r_bits_dev, L, mode, g_dev, p_dev, count);
}

int hb_lt_xor_mask(hb_ctx *ctx, const uint64_t *c_dev, const uint64_t *r0_dev, const uint64_t *w_dev, const uint64_t *pa_dev, const uint64_t *qa_dev, uint64_t *u_dev,
                   uint64_t *masked_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : lt_xor_mask_step(DeviceRun{ctx, (hipStream_t)stream, "hb_lt_xor_mask"}, c_dev, r0_dev, w_dev, pa_dev, qa_dev, u_dev, masked_dev,
                                                    count);
}

int hb_lt_dmask(hb_ctx *ctx, const uint64_t *c_dev, const uint64_t *r0_dev, const uint64_t *x_dev, const uint64_t *s_dev, const uint64_t *s_bits_dev, int L,
                const uint64_t *pa_dev, const uint64_t *qa_dev, const uint64_t *pb_dev, const uint64_t *qb_dev, uint64_t *u_dev, uint64_t *masked_dev, int64_t count,
                void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : lt_dmask_step(DeviceRun{ctx, (hipStream_t)stream, "hb_lt_dmask"}, c_dev, r0_dev, x_dev, s_dev, s_bits_dev, L, pa_dev, qa_dev, pb_dev,
                                                 qb_dev, u_dev, masked_dev, count);
}

int hb_lt_mid(hb_ctx *ctx, const uint64_t *opened_dev, const uint64_t *u_dev, const uint64_t *s_bits_dev, int L, const uint64_t *pa_dev, const uint64_t *qa_dev,
              const uint64_t *pqa_dev, const uint64_t *pb_dev, const uint64_t *qb_dev, const uint64_t *pqb_dev, const uint64_t *pc_dev, const uint64_t *qc_dev,
              uint64_t *v_dev, uint64_t *d0_dev, uint64_t *masked_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : lt_mid_step(DeviceRun{ctx, (hipStream_t)stream, "hb_lt_mid"}, opened_dev, u_dev, s_bits_dev, L, pa_dev, qa_dev, pqa_dev, pb_dev,
                                               qb_dev, pqb_dev, pc_dev, qc_dev, v_dev, d0_dev, masked_dev, count);
}

int hb_lt_xor_finish(hb_ctx *ctx, const uint64_t *opened_dev, const uint64_t *u_dev, const uint64_t *v_dev, const uint64_t *p_dev, const uint64_t *q_dev,
                     const uint64_t *pq_dev, uint64_t *out_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : lt_xor_finish_step(DeviceRun{ctx, (hipStream_t)stream, "hb_lt_xor_finish"}, opened_dev, u_dev, v_dev, p_dev, q_dev, pq_dev, out_dev,
                                                      count);
}

// params: L, mode (read by the steps that take them)
int hb_selftest_lt(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *ops, const int64_t *params, uint64_t *const *outs, int64_t count) {
    if (!p_limbs || !ops || !params || !outs || (n_limbs != 1 && n_limbs != 4)) return HB_ERR_BAD_ARG;
    if (params[0] != (int)params[0] || params[1] != (int)params[1]) return HB_ERR_BAD_ARG;    // L, mode: the steps take them as int
    const HostRun run = {p_limbs, n_limbs};
    const int L = (int)params[0], mode = (int)params[1];
    switch (what) {
    case HB_LT_SELFTEST_MASK: return lt_mask_step(run, ops[0], ops[1], ops[2], outs[0], count);
    case HB_LT_SELFTEST_LEAVES: return lt_leaves_step(run, ops[0], ops[1], L, mode, outs[0], outs[1], count);
    case HB_LT_SELFTEST_XOR_MASK: return lt_xor_mask_step(run, ops[0], ops[1], ops[2], ops[3], ops[4], outs[0], outs[1], count);
    case HB_LT_SELFTEST_DMASK: return lt_dmask_step(run, ops[0], ops[1], ops[2], ops[3], ops[4], L, ops[5], ops[6], ops[7], ops[8], outs[0], outs[1], count);
    case HB_LT_SELFTEST_MID:
        return lt_mid_step(run, ops[0], ops[1], ops[2], L, ops[3], ops[4], ops[5], ops[6], ops[7], ops[8], ops[9], ops[10], outs[0], outs[1], outs[2], count);
    case HB_LT_SELFTEST_XOR_FINISH: return lt_xor_finish_step(run, ops[0], ops[1], ops[2], ops[3], ops[4], ops[5], outs[0], count);
    default: return HB_ERR_BAD_ARG;
    }
}

}  // extern "C"

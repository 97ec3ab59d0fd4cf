// hb_jj.hip -- the Jubjub twisted Edwards curve a x^2 + y^2 = 1 + d x^2 y^2 of the reference's elliptic_curve.py and progs/jubjub.py:
// batched scalar multiplication and doubling tables in the clear (Point.__mul__, elliptic_curve.py:102-122, and the p2i.double()
// chain of share_mul, progs/jubjub.py:280-286) and the addition of shared points (SharedPoint.add, progs/jubjub.py:87-113) as four
// fused passes around four opens -- restated on fp29.hpp, not translated.
//
// Cleartext.  Extended coordinates (X : Y : Z : T), x = X / Z, y = Y / Z, T = X Y / Z, every coordinate a Montgomery residue, general a
// and d (kernel arguments, Montgomery form).  With a a square and d a non-square the unified law is complete: no Z is ever zero.
//   jj_double      A = X^2, B = Y^2, C = 2 Z^2, D = a A, E = (X + Y)^2 - A - B, G = D + B, F = G - C, H = D - B;
//                  (X', Y', T', Z') = (E F, G H, E H, F G)                                                           8 products
//   jj_add_mixed   the second point affine (x2, y2, td2 = d x2 y2):  A = X x2, B = Y y2, C = T td2, E = (X + Y)(x2 + y2) - A - B,
//                  F = Z - C, G = Z + C, H = B - a A;  (X', Y', T', Z') = (E F, G H, E H, F G)                       9 products
// k_jj_scalar_mul    out_i = n_i P_i: the accumulator starts at (0 : 1 : 1 : 0) and takes the scalar's bits from the top, one
//                    doubling a bit and one mixed addition a set bit, 32 NW bits in a loop that is not unrolled (the scalar's words are
//                    shifted left a bit a round: no register array is indexed by the loop counter); one fp_inv at the end.  Everything
//                    stays in registers.  n_i = 0 leaves (0, 1).  Scalar and point: one for all (element 0) or one an element.
// k_jj_double_table  rows j < K of 2^j P_i, projective: the Montgomery residues X R, Y R, Z R of row j at [j][i] of three arrays.
//                    hb_jj_double_table then makes them affine with ONE hb_ew_inv over the K count values of Z and two hb_ew_op
//                    products ((X R) / (Z R) = x): no inversion an element and row.
//
// Shared addition (curves with a = -1, as the reference's law reads), for m independent pairs, every operand a share array:
//     x3 = (x1 y2 + y1 x2) / (1 + d x1 x2 y1 y2)          y3 = (y1 y2 + x1 x2) / (1 - d x1 x2 y1 y2)
// regrouped so that each numerator rides with the blinding of its denominator, num / den = (num r) / (den r) with den r opened:
// 9 Beaver triples and 2 random shares (rx, ry) a pair.  Triple k multiplies:  0 x1 x2,  1 y1 y2,  2 x1 y2,  3 y1 x2,  4 xp yp,
// 5 nx rx,  6 ny ry,  7 dx rx,  8 dy ry   (xp = x1 x2, yp = y1 y2, nx = x1 y2 + y1 x2, ny = yp + xp, dx = 1 + d xp yp, dy = 1 - d xp yp).
//   k_jj_add_mask     A [8][m]: rows 2k, 2k + 1 the masked factors (first - p_k, second - q_k) of products 0..3
//   k_jj_add_stage1   opened A -> xp, yp, x1 y2, y1 x2 (four Beaver steps) -> B [6][m]: the masked factors of products 4..6
//   k_jj_add_stage2   opened B -> [xp yp], u = [nx rx], v = [ny ry] (three Beaver steps); u, v kept ([2][m]); C [4][m]: the masked
//                     factors of products 7, 8.  A public 1 and d meet a share alike on every party.
//   k_jj_add_stage3   opened C -> D [2][m]: the shares of sig_x = dx rx, sig_y = dy ry (two Beaver steps)
//   hb_jj_add_finish  opened D -> hb_ew_inv over its 2 m values (batched), then k_jj_add_scale: x3 = u / sig_x, y3 = v / sig_y
// A zero sig (r = 0, or operands off the curve) is counted by hb_ew_inv's counter.  Six launches and four opens an addition.
// Every Beaver step is ew_beaver_elem of hb_ew_elem.hpp, unchanged; everything between the steps is fp_add / fp_sub / mont_mul on
// canonical residues: there is NO lazy sum in this file beyond ew_beaver_elem's own (bounds stated there), so every digit is below 2^29
// and every value below p between two calls.  p = 2^256 - 189 with every operand p - 1 is the largest case (tests/test_jubjub_host.py).
//
// The per-element bodies are HB_HD functions on pointers and an index (as ew_inv_lane of hb_ew.hip): they load what they need when
// they need it -- a stage reads up to 28 elements, more than a lane holds at once -- and store their rows; the __global__ wrappers
// only find the index and call them, and hb_selftest_jj runs the very same functions over host memory.  Outputs are distinct arrays.
// Launch shape (all kernels): 256-thread workgroups, one element (pair) a thread, grid = ceil(count / 256), no LDS, no grid stride,
// the caller's stream.  What was just opened and the preprocessing are read once: the 32-byte width takes the non-temporal loads.
// Compiler's report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): DESIGN.md section 3l and profiles/jubjub.txt.
#include "hb_common.hpp"
#include "hb_ew_elem.hpp"
#include "hb_rows.hpp"

using namespace hb;

namespace hb {

// a field element as digits, handed to a kernel by value (the curve's a and d in Montgomery form)
template <int NL> struct JjConst { uint32_t d[NL]; };
template <int NL> struct JjPoint { uint32_t X[NL], Y[NL], Z[NL], T[NL]; };
// one party's triples: row k of a component starts k * stride elements behind its base
struct JjTrip { const uint32_t *p, *q, *pq; int64_t stride; };

// ---------------------------------------------------------------- per-element bodies (host and device)
template <int NL, int NW> HB_HD void jj_digits_once(uint32_t (&d)[NL], const uint32_t *p) {
    uint32_t w[NW];
    load_once<NW>(w, p);
    unpack<NL, NW>(d, w);
}

// r = 2 p (r may be p)
template <int NL> HB_HD void jj_double(JjPoint<NL> &r, const JjPoint<NL> &p, const uint32_t (&am)[NL], const FpParams<NL> &P) {
    uint32_t A[NL], B[NL], C[NL], D[NL], E[NL], F[NL], G[NL], H[NL], t[NL];
    mont_mul<NL>(A, p.X, p.X, P);
    mont_mul<NL>(B, p.Y, p.Y, P);
    mont_mul<NL>(t, p.Z, p.Z, P);
    fp_add<NL>(C, t, t, P);
    mont_mul<NL>(D, am, A, P);
    fp_add<NL>(t, p.X, p.Y, P);
    mont_mul<NL>(E, t, t, P);
    fp_sub<NL>(t, E, A, P);
    fp_sub<NL>(E, t, B, P);
    fp_add<NL>(G, D, B, P);
    fp_sub<NL>(F, G, C, P);
    fp_sub<NL>(H, D, B, P);
    mont_mul<NL>(r.X, E, F, P);
    mont_mul<NL>(r.Y, G, H, P);
    mont_mul<NL>(r.T, E, H, P);
    mont_mul<NL>(r.Z, F, G, P);
}

// r = r + (x2, y2), the second point affine with td2 = d x2 y2
template <int NL>
HB_HD void jj_add_mixed(JjPoint<NL> &r, const uint32_t (&x2)[NL], const uint32_t (&y2)[NL], const uint32_t (&td2)[NL], const uint32_t (&am)[NL], const FpParams<NL> &P) {
    uint32_t A[NL], B[NL], C[NL], E[NL], F[NL], G[NL], H[NL], s[NL], t[NL];
    mont_mul<NL>(A, r.X, x2, P);
    mont_mul<NL>(B, r.Y, y2, P);
    mont_mul<NL>(C, r.T, td2, P);
    fp_add<NL>(s, r.X, r.Y, P);
    fp_add<NL>(t, x2, y2, P);
    mont_mul<NL>(E, s, t, P);
    fp_sub<NL>(t, E, A, P);
    fp_sub<NL>(E, t, B, P);
    fp_sub<NL>(F, r.Z, C, P);
    fp_add<NL>(G, r.Z, C, P);
    mont_mul<NL>(t, am, A, P);
    fp_sub<NL>(H, B, t, P);
    mont_mul<NL>(r.X, E, F, P);
    mont_mul<NL>(r.Y, G, H, P);
    mont_mul<NL>(r.T, E, H, P);
    mont_mul<NL>(r.Z, F, G, P);
}

// (ox, oy) = n (x, y): packed canonical words in and out; am, dm the curve's constants in Montgomery form
template <int NL, int NW>
HB_HD void jj_scalar_mul_elem(uint32_t (&ox)[NW], uint32_t (&oy)[NW], const uint32_t (&nw)[NW], const uint32_t (&xw)[NW], const uint32_t (&yw)[NW],
                              const uint32_t (&am)[NL], const uint32_t (&dm)[NL], const FpParams<NL> &P) {
    uint32_t x2[NL], y2[NL], td2[NL], t[NL], k[NW];
    JjPoint<NL> acc;
    unpack<NL, NW>(t, xw);
    to_mont<NL>(x2, t, P);
    unpack<NL, NW>(t, yw);
    to_mont<NL>(y2, t, P);
    mont_mul<NL>(t, x2, y2, P);
    mont_mul<NL>(td2, t, dm, P);
#pragma unroll
    for (int q = 0; q < NL; q++) { acc.X[q] = 0; acc.T[q] = 0; acc.Y[q] = P.one[q]; acc.Z[q] = P.one[q]; }
#pragma unroll
    for (int q = 0; q < NW; q++) k[q] = nw[q];
#pragma unroll 1
    for (int b = 0; b < 32 * NW; b++) {
        jj_double<NL>(acc, acc, am, P);
        const uint32_t bit = k[NW - 1] >> 31;
#pragma unroll
        for (int q = NW - 1; q > 0; q--) k[q] = (k[q] << 1) | (k[q - 1] >> 31);
        k[0] <<= 1;
        if (bit) jj_add_mixed<NL>(acc, x2, y2, td2, am, P);
    }
    fp_inv<NL>(t, acc.Z, P);
    mont_mul<NL>(x2, acc.X, t, P);
    mont_mul<NL>(y2, acc.Y, t, P);
    from_mont<NL>(td2, x2, P);
    pack<NL, NW>(ox, td2);
    from_mont<NL>(td2, y2, P);
    pack<NL, NW>(oy, td2);
}

// rows j < K of 2^j (x, y), projective, as the Montgomery residues of X, Y, Z: row j of element i at [(j * count + i) * NW]
template <int NL, int NW>
HB_HD void jj_double_table_elem(uint32_t *xs, uint32_t *ys, uint32_t *zs, const uint32_t (&xw)[NW], const uint32_t (&yw)[NW], const uint32_t (&am)[NL], int K,
                                int64_t i, int64_t count, const FpParams<NL> &P) {
    uint32_t t[NL];
    JjPoint<NL> acc;
    unpack<NL, NW>(t, xw);
    to_mont<NL>(acc.X, t, P);
    unpack<NL, NW>(t, yw);
    to_mont<NL>(acc.Y, t, P);
    mont_mul<NL>(acc.T, acc.X, acc.Y, P);
    fp_set<NL>(acc.Z, P.one);
#pragma unroll 1
    for (int j = 0; j < K; j++) {
        const int64_t at = ((int64_t)j * count + i) * NW;
        store_digits<NL, NW>(xs + at, acc.X);
        store_digits<NL, NW>(ys + at, acc.Y);
        store_digits<NL, NW>(zs + at, acc.Z);
        if (j + 1 < K) jj_double<NL>(acc, acc, am, P);
    }
}

// out = v - mask[i]
template <int NL, int NW> HB_HD void jj_sub_store(uint32_t *out, const uint32_t (&v)[NL], const uint32_t *mask, const FpParams<NL> &P) {
    uint32_t k[NL], r[NL];
    jj_digits_once<NL, NW>(k, mask);
    fp_sub<NL>(r, v, k, P);
    store_digits<NL, NW>(out, r);
}
// o = the Beaver step of triple k on the opened factors at dp, ep (element i of each)
template <int NL, int NW>
HB_HD void jj_beaver(uint32_t (&o)[NL], const uint32_t *dp, const uint32_t *ep, const JjTrip &t, int k, int64_t i, const FpParams<NL> &P) {
    uint32_t dw[NW], ew[NW], pw[NW], qw[NW], pqw[NW], ow[NW];
    const int64_t at = ((int64_t)k * t.stride + i) * NW;
    load_once<NW>(dw, dp + i * NW);
    load_once<NW>(ew, ep + i * NW);
    load_once<NW>(pw, t.p + at);
    load_once<NW>(qw, t.q + at);
    load_once<NW>(pqw, t.pq + at);
    ew_beaver_elem<NL, NW>(ow, dw, ew, pw, qw, pqw, P);
    unpack<NL, NW>(o, ow);
}
#define JJ_ROW(base, row) ((base) + ((int64_t)(row) * m + i) * NW)
#define JJ_TRIP(comp, k) ((comp) + ((int64_t)(k) * t.stride + i) * NW)

// A[2k] = first_k - p_k, A[2k + 1] = second_k - q_k for the products 0 x1 x2, 1 y1 y2, 2 x1 y2, 3 y1 x2
template <int NL, int NW>
HB_HD void jj_mask_elem(uint32_t *A, const uint32_t *x1, const uint32_t *y1, const uint32_t *x2, const uint32_t *y2, const JjTrip &t, int64_t i, int64_t m,
                        const FpParams<NL> &P) {
    uint32_t xa[NL], ya[NL], xb[NL], yb[NL];
    load_digits<NL, NW>(xa, x1 + i * NW);
    load_digits<NL, NW>(ya, y1 + i * NW);
    load_digits<NL, NW>(xb, x2 + i * NW);
    load_digits<NL, NW>(yb, y2 + i * NW);
    jj_sub_store<NL, NW>(JJ_ROW(A, 0), xa, JJ_TRIP(t.p, 0), P);
    jj_sub_store<NL, NW>(JJ_ROW(A, 1), xb, JJ_TRIP(t.q, 0), P);
    jj_sub_store<NL, NW>(JJ_ROW(A, 2), ya, JJ_TRIP(t.p, 1), P);
    jj_sub_store<NL, NW>(JJ_ROW(A, 3), yb, JJ_TRIP(t.q, 1), P);
    jj_sub_store<NL, NW>(JJ_ROW(A, 4), xa, JJ_TRIP(t.p, 2), P);
    jj_sub_store<NL, NW>(JJ_ROW(A, 5), yb, JJ_TRIP(t.q, 2), P);
    jj_sub_store<NL, NW>(JJ_ROW(A, 6), ya, JJ_TRIP(t.p, 3), P);
    jj_sub_store<NL, NW>(JJ_ROW(A, 7), xb, JJ_TRIP(t.q, 3), P);
}

// opened A -> B: xp - p4, yp - q4, nx - p5, rx - q5, ny - p6, ry - q6
template <int NL, int NW>
HB_HD void jj_stage1_elem(uint32_t *B, const uint32_t *A, const JjTrip &t, const uint32_t *rx, const uint32_t *ry, int64_t i, int64_t m, const FpParams<NL> &P) {
    uint32_t xp[NL], yp[NL], a[NL], b[NL], n[NL];
    jj_beaver<NL, NW>(xp, A, A + m * NW, t, 0, i, P);
    jj_beaver<NL, NW>(yp, A + 2 * m * NW, A + 3 * m * NW, t, 1, i, P);
    jj_sub_store<NL, NW>(JJ_ROW(B, 0), xp, JJ_TRIP(t.p, 4), P);
    jj_sub_store<NL, NW>(JJ_ROW(B, 1), yp, JJ_TRIP(t.q, 4), P);
    fp_add<NL>(n, yp, xp, P);
    jj_sub_store<NL, NW>(JJ_ROW(B, 4), n, JJ_TRIP(t.p, 6), P);
    jj_beaver<NL, NW>(a, A + 4 * m * NW, A + 5 * m * NW, t, 2, i, P);
    jj_beaver<NL, NW>(b, A + 6 * m * NW, A + 7 * m * NW, t, 3, i, P);
    fp_add<NL>(n, a, b, P);
    jj_sub_store<NL, NW>(JJ_ROW(B, 2), n, JJ_TRIP(t.p, 5), P);
    load_digits<NL, NW>(a, rx + i * NW);
    jj_sub_store<NL, NW>(JJ_ROW(B, 3), a, JJ_TRIP(t.q, 5), P);
    load_digits<NL, NW>(b, ry + i * NW);
    jj_sub_store<NL, NW>(JJ_ROW(B, 5), b, JJ_TRIP(t.q, 6), P);
}

// opened B -> uv = (u, v) = ([nx rx], [ny ry]) and C: dx - p7, rx - q7, dy - p8, ry - q8 with dx = 1 + d [xp yp], dy = 1 - d [xp yp]
template <int NL, int NW>
HB_HD void jj_stage2_elem(uint32_t *uv, uint32_t *C, const uint32_t *B, const JjTrip &t, const uint32_t *rx, const uint32_t *ry, const uint32_t (&dm)[NL], int64_t i,
                          int64_t m, const FpParams<NL> &P) {
    uint32_t w[NL], s[NL], one[NL];
    jj_beaver<NL, NW>(w, B + 2 * m * NW, B + 3 * m * NW, t, 5, i, P);
    store_digits<NL, NW>(JJ_ROW(uv, 0), w);
    jj_beaver<NL, NW>(w, B + 4 * m * NW, B + 5 * m * NW, t, 6, i, P);
    store_digits<NL, NW>(JJ_ROW(uv, 1), w);
    jj_beaver<NL, NW>(s, B, B + m * NW, t, 4, i, P);
    mont_mul<NL>(w, s, dm, P);                                  // d [xp yp]: a plain residue times d R
#pragma unroll
    for (int q = 0; q < NL; q++) one[q] = q == 0 ? 1u : 0u;
    fp_add<NL>(s, one, w, P);
    jj_sub_store<NL, NW>(JJ_ROW(C, 0), s, JJ_TRIP(t.p, 7), P);
    fp_sub<NL>(s, one, w, P);
    jj_sub_store<NL, NW>(JJ_ROW(C, 2), s, JJ_TRIP(t.p, 8), P);
    load_digits<NL, NW>(w, rx + i * NW);
    jj_sub_store<NL, NW>(JJ_ROW(C, 1), w, JJ_TRIP(t.q, 7), P);
    load_digits<NL, NW>(w, ry + i * NW);
    jj_sub_store<NL, NW>(JJ_ROW(C, 3), w, JJ_TRIP(t.q, 8), P);
}

// opened C -> D = ([dx rx], [dy ry])
template <int NL, int NW> HB_HD void jj_stage3_elem(uint32_t *D, const uint32_t *C, const JjTrip &t, int64_t i, int64_t m, const FpParams<NL> &P) {
    uint32_t s[NL];
    jj_beaver<NL, NW>(s, C, C + m * NW, t, 7, i, P);
    store_digits<NL, NW>(JJ_ROW(D, 0), s);
    jj_beaver<NL, NW>(s, C + 2 * m * NW, C + 3 * m * NW, t, 8, i, P);
    store_digits<NL, NW>(JJ_ROW(D, 1), s);
}

// x3 = u / sig_x, y3 = v / sig_y from the inverted sigs: a product of two plain residues is two Montgomery products (ew_binary_elem)
template <int NL, int NW>
HB_HD void jj_scale_elem(uint32_t *x3, uint32_t *y3, const uint32_t *inv, const uint32_t *uv, int64_t i, int64_t m, const FpParams<NL> &P) {
    uint32_t a[NL], b[NL], r[NL];
    jj_digits_once<NL, NW>(a, JJ_ROW(inv, 0));
    jj_digits_once<NL, NW>(b, JJ_ROW(uv, 0));
    mont_mul<NL>(r, a, b, P);
    mont_mul<NL>(a, P.r2, r, P);
    store_digits<NL, NW>(x3 + i * NW, a);
    jj_digits_once<NL, NW>(a, JJ_ROW(inv, 1));
    jj_digits_once<NL, NW>(b, JJ_ROW(uv, 1));
    mont_mul<NL>(r, a, b, P);
    mont_mul<NL>(a, P.r2, r, P);
    store_digits<NL, NW>(y3 + i * NW, a);
}

// ---------------------------------------------------------------- kernels
template <int NL, int NW>
__global__ void __launch_bounds__(256) k_jj_scalar_mul(const FpParams<NL> P, const uint32_t *n, int n_bcast, const uint32_t *x, const uint32_t *y, int p_bcast,
                                                       const JjConst<NL> am, const JjConst<NL> dm, uint32_t *ox, uint32_t *oy, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    uint32_t nw[NW], xw[NW], yw[NW], rx[NW], ry[NW];
    load_words<NW>(nw, n + (n_bcast ? 0 : i) * NW);
    load_words<NW>(xw, x + (p_bcast ? 0 : i) * NW);
    load_words<NW>(yw, y + (p_bcast ? 0 : i) * NW);
    jj_scalar_mul_elem<NL, NW>(rx, ry, nw, xw, yw, am.d, dm.d, P);
    store_words<NW>(ox + i * NW, rx);
    store_words<NW>(oy + i * NW, ry);
}

template <int NL, int NW>
__global__ void __launch_bounds__(256) k_jj_double_table(const FpParams<NL> P, const uint32_t *x, const uint32_t *y, const JjConst<NL> am, int K, uint32_t *xs,
                                                         uint32_t *ys, uint32_t *zs, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    uint32_t xw[NW], yw[NW];
    load_words<NW>(xw, x + i * NW);
    load_words<NW>(yw, y + i * NW);
    jj_double_table_elem<NL, NW>(xs, ys, zs, xw, yw, am.d, K, i, count, P);
}

template <int NL, int NW>
__global__ void __launch_bounds__(256) k_jj_add_mask(const FpParams<NL> P, const uint32_t *x1, const uint32_t *y1, const uint32_t *x2, const uint32_t *y2,
                                                     const JjTrip t, uint32_t *A, int64_t m) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    jj_mask_elem<NL, NW>(A, x1, y1, x2, y2, t, i, m, P);
}
template <int NL, int NW>
__global__ void __launch_bounds__(256) k_jj_add_stage1(const FpParams<NL> P, const uint32_t *A, const JjTrip t, const uint32_t *rx, const uint32_t *ry, uint32_t *B,
                                                       int64_t m) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    jj_stage1_elem<NL, NW>(B, A, t, rx, ry, i, m, P);
}
template <int NL, int NW>
__global__ void __launch_bounds__(256) k_jj_add_stage2(const FpParams<NL> P, const uint32_t *B, const JjTrip t, const uint32_t *rx, const uint32_t *ry,
                                                       const JjConst<NL> dm, uint32_t *uv, uint32_t *C, int64_t m) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    jj_stage2_elem<NL, NW>(uv, C, B, t, rx, ry, dm.d, i, m, P);
}
template <int NL, int NW>
__global__ void __launch_bounds__(256) k_jj_add_stage3(const FpParams<NL> P, const uint32_t *C, const JjTrip t, uint32_t *D, int64_t m) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    jj_stage3_elem<NL, NW>(D, C, t, i, m, P);
}
template <int NL, int NW>
__global__ void __launch_bounds__(256) k_jj_add_scale(const FpParams<NL> P, const uint32_t *inv, const uint32_t *uv, uint32_t *x3, uint32_t *y3, int64_t m) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    jj_scale_elem<NL, NW>(x3, y3, inv, uv, i, m, P);
}

// ---------------------------------------------------------------- host side
// a curve constant from its packed words -> Montgomery digits; false if it is missing or not below p
template <int NL, int NW> static bool jj_const(JjConst<NL> &c, const FpParams<NL> &P, const uint64_t *host) {
    if (!host) return false;
    uint32_t w[NW], v[NL];
    memcpy(w, host, NW * 4);
    unpack<NL, NW>(v, w);
    bool below = false;
    for (int i = NL - 1; i >= 0; i--)
        if (v[i] != P.p[i]) { below = v[i] < P.p[i]; break; }
    if (!below) return false;
    to_mont<NL>(c.d, v, P);
    return true;
}
struct JjConsts { JjConst<9> aw, dw; JjConst<3> an, dn; };
static bool jj_consts(hb_ctx *ctx, JjConsts &c, const uint64_t *a_host, const uint64_t *d_host) {
    if (ctx->n_limbs == 4) return (!a_host || jj_const<9, 8>(c.aw, ctx->pw, a_host)) && (!d_host || jj_const<9, 8>(c.dw, ctx->pw, d_host));
    return (!a_host || jj_const<3, 2>(c.an, ctx->pn, a_host)) && (!d_host || jj_const<3, 2>(c.dn, ctx->pn, d_host));
}
static JjTrip jj_trip(const uint64_t *p, const uint64_t *q, const uint64_t *pq, int64_t stride) {
    return JjTrip{(const uint32_t *)p, (const uint32_t *)q, (const uint32_t *)pq, stride};
}

// host: the same element functions over `count` elements
template <int NL, int NW>
static int selftest_jj(const uint64_t *p_limbs, int what, const uint64_t *const *ops, const uint64_t *a_host, const uint64_t *d_host, int flags, int64_t arg,
                       uint64_t *out, int64_t count) {
    FpParams<NL> P;
    fp_params_from_limbs(P, p_limbs);
    JjConst<NL> am = {}, dm = {};
    if (a_host && !jj_const<NL, NW>(am, P, a_host)) return HB_ERR_BAD_ARG;
    if (d_host && !jj_const<NL, NW>(dm, P, d_host)) return HB_ERR_BAD_ARG;
    auto U = [](const uint64_t *base) { return reinterpret_cast<const uint32_t *>(base); };
    auto W = [](const uint64_t *base, int64_t i) -> const uint32_t (&)[NW] { return *reinterpret_cast<const uint32_t(*)[NW]>(reinterpret_cast<const uint32_t *>(base) + i * NW); };
    uint32_t *o = reinterpret_cast<uint32_t *>(out);
    const int64_t m = count;
    if (what == HB_JJ_SELFTEST_SCALAR_MUL) {
        const bool nb = (flags & HB_JJ_SCALAR_BROADCAST) != 0, pb = (flags & HB_JJ_POINT_BROADCAST) != 0;
        for (int64_t i = 0; i < count; i++) {
            uint32_t rx[NW], ry[NW];
            jj_scalar_mul_elem<NL, NW>(rx, ry, W(ops[0], nb ? 0 : i), W(ops[1], pb ? 0 : i), W(ops[2], pb ? 0 : i), am.d, dm.d, P);
            memcpy(o + i * NW, rx, NW * 4);
            memcpy(o + (count + i) * NW, ry, NW * 4);
        }
        return HB_OK;
    }
    if (what == HB_JJ_SELFTEST_DOUBLE_TABLE) {
        const int K = (int)arg;
        for (int64_t i = 0; i < count; i++)
            jj_double_table_elem<NL, NW>(o, o + (int64_t)K * count * NW, o + 2 * (int64_t)K * count * NW, W(ops[0], i), W(ops[1], i), am.d, K, i, count, P);
        return HB_OK;
    }
    if (what == HB_JJ_SELFTEST_SCALE) {
        for (int64_t i = 0; i < m; i++) jj_scale_elem<NL, NW>(o, o + m * NW, U(ops[0]), U(ops[1]), i, m, P);
        return HB_OK;
    }
    if (what == HB_JJ_SELFTEST_MASK) {
        const JjTrip t = jj_trip(ops[4], ops[5], nullptr, arg);
        for (int64_t i = 0; i < m; i++) jj_mask_elem<NL, NW>(o, U(ops[0]), U(ops[1]), U(ops[2]), U(ops[3]), t, i, m, P);
        return HB_OK;
    }
    const JjTrip t = jj_trip(ops[1], ops[2], ops[3], arg);
    for (int64_t i = 0; i < m; i++) {
        if (what == HB_JJ_SELFTEST_STAGE1) jj_stage1_elem<NL, NW>(o, U(ops[0]), t, U(ops[4]), U(ops[5]), i, m, P);
        else if (what == HB_JJ_SELFTEST_STAGE2) jj_stage2_elem<NL, NW>(o, o + 2 * m * NW, U(ops[0]), t, U(ops[4]), U(ops[5]), dm.d, i, m, P);
        else jj_stage3_elem<NL, NW>(o, U(ops[0]), t, i, m, P);
    }
    return HB_OK;
}

static bool jj_blocks(int64_t count, unsigned *blocks) {
    const int64_t b = (count + 255) / 256;
    *blocks = (unsigned)b;
    return b <= 0x7fffffffLL;
}

}  // namespace hb

extern "C" {

int hb_jj_scalar_mul(hb_ctx *ctx, const uint64_t *n_dev, int n_broadcast, const uint64_t *x_dev, const uint64_t *y_dev, int point_broadcast, const uint64_t *a_host,
                     const uint64_t *d_host, uint64_t *outx_dev, uint64_t *outy_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0 || !a_host || !d_host || (count > 0 && (!n_dev || !x_dev || !y_dev || !outx_dev || !outy_dev))) return HB_ERR_BAD_ARG;
    if (outx_dev == outy_dev && count > 0) return fail(ctx, HB_ERR_BAD_ARG, "hb_jj_scalar_mul: the two outputs are one array");
    if (count > 1 && ((n_broadcast && (outx_dev == n_dev || outy_dev == n_dev)) ||
                      (point_broadcast && (outx_dev == x_dev || outx_dev == y_dev || outy_dev == x_dev || outy_dev == y_dev))))
        return fail(ctx, HB_ERR_BAD_ARG, "hb_jj_scalar_mul: out aliases a broadcast operand");
    JjConsts c;
    if (!jj_consts(ctx, c, a_host, d_host)) return fail(ctx, HB_ERR_BAD_ARG, "hb_jj_scalar_mul: a curve constant is not below the modulus");
    if (count == 0) return HB_OK;
    unsigned blocks;
    if (!jj_blocks(count, &blocks)) return fail(ctx, HB_ERR_UNSUPPORTED, "hb_jj_scalar_mul: batch too large for one launch");
    hipStream_t s = (hipStream_t)stream;
    const uint32_t *n = (const uint32_t *)n_dev, *x = (const uint32_t *)x_dev, *y = (const uint32_t *)y_dev;
    HB_DISPATCH(ctx, (k_jj_scalar_mul<9, 8><<<blocks, 256, 0, s>>>(ctx->pw, n, n_broadcast != 0, x, y, point_broadcast != 0, c.aw, c.dw, (uint32_t *)outx_dev, (uint32_t *)outy_dev, count)),
                (k_jj_scalar_mul<3, 2><<<blocks, 256, 0, s>>>(ctx->pn, n, n_broadcast != 0, x, y, point_broadcast != 0, c.an, c.dn, (uint32_t *)outx_dev, (uint32_t *)outy_dev, count)));
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_jj_double_table(hb_ctx *ctx, const uint64_t *x_dev, const uint64_t *y_dev, const uint64_t *a_host, int rows, uint64_t *xs_dev, uint64_t *ys_dev, uint64_t *zs_dev,
                       int64_t count, int32_t *zeros_dev, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0 || !a_host || (count > 0 && (!x_dev || !y_dev || !xs_dev || !ys_dev || !zs_dev))) return HB_ERR_BAD_ARG;
    if (rows < 1) return fail(ctx, HB_ERR_BAD_ARG, "hb_jj_double_table: at least one row");
    if (count > 0 && (xs_dev == ys_dev || xs_dev == zs_dev || ys_dev == zs_dev)) return fail(ctx, HB_ERR_BAD_ARG, "hb_jj_double_table: the three arrays must be distinct");
    JjConsts c;
    if (!jj_consts(ctx, c, a_host, nullptr)) return fail(ctx, HB_ERR_BAD_ARG, "hb_jj_double_table: a is not below the modulus");
    if (count == 0) return HB_OK;
    unsigned blocks;
    if (!jj_blocks(count, &blocks) || count > INT64_MAX / rows / 64) return fail(ctx, HB_ERR_UNSUPPORTED, "hb_jj_double_table: batch too large for one launch");
    hipStream_t s = (hipStream_t)stream;
    HB_DISPATCH(ctx, (k_jj_double_table<9, 8><<<blocks, 256, 0, s>>>(ctx->pw, (const uint32_t *)x_dev, (const uint32_t *)y_dev, c.aw, rows, (uint32_t *)xs_dev, (uint32_t *)ys_dev, (uint32_t *)zs_dev, count)),
                (k_jj_double_table<3, 2><<<blocks, 256, 0, s>>>(ctx->pn, (const uint32_t *)x_dev, (const uint32_t *)y_dev, c.an, rows, (uint32_t *)xs_dev, (uint32_t *)ys_dev, (uint32_t *)zs_dev, count)));
    HB_LAUNCH_CHECK(ctx);
    // affine: (X R) / (Z R) = x -- one batched inversion over every row's Z, two element-wise products
    const int64_t all = (int64_t)rows * count;
    int rc = hb_ew_inv(ctx, zs_dev, zs_dev, all, zeros_dev, stream);
    if (rc == HB_OK) rc = hb_ew_op(ctx, HB_EW_MUL, xs_dev, zs_dev, 0, xs_dev, all, stream);
    if (rc == HB_OK) rc = hb_ew_op(ctx, HB_EW_MUL, ys_dev, zs_dev, 0, ys_dev, all, stream);
    return rc;
}

#define JJ_STAGE_GUARD(name, nullcheck)                                                                                           \
    if (!ctx || m < 0 || (m > 0 && (nullcheck))) return HB_ERR_BAD_ARG;                                                           \
    if (trip_stride < m) return fail(ctx, HB_ERR_BAD_ARG, name ": the triples' row stride is below the pair count");              \
    if (m == 0) return HB_OK;                                                                                                     \
    unsigned blocks;                                                                                                              \
    if (!jj_blocks(m, &blocks) || trip_stride > INT64_MAX / 1024) return fail(ctx, HB_ERR_UNSUPPORTED, name ": batch too large for one launch"); \
    hipStream_t s = (hipStream_t)stream

int hb_jj_add_mask(hb_ctx *ctx, const uint64_t *x1_dev, const uint64_t *y1_dev, const uint64_t *x2_dev, const uint64_t *y2_dev, const uint64_t *p_dev,
                   const uint64_t *q_dev, int64_t trip_stride, uint64_t *a_dev, int64_t m, void *stream) { HB_API_GUARD(ctx);
    JJ_STAGE_GUARD("hb_jj_add_mask", !x1_dev || !y1_dev || !x2_dev || !y2_dev || !p_dev || !q_dev || !a_dev);
    const JjTrip t = jj_trip(p_dev, q_dev, nullptr, trip_stride);
    HB_DISPATCH(ctx, (k_jj_add_mask<9, 8><<<blocks, 256, 0, s>>>(ctx->pw, (const uint32_t *)x1_dev, (const uint32_t *)y1_dev, (const uint32_t *)x2_dev, (const uint32_t *)y2_dev, t, (uint32_t *)a_dev, m)),
                (k_jj_add_mask<3, 2><<<blocks, 256, 0, s>>>(ctx->pn, (const uint32_t *)x1_dev, (const uint32_t *)y1_dev, (const uint32_t *)x2_dev, (const uint32_t *)y2_dev, t, (uint32_t *)a_dev, m)));
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_jj_add_stage1(hb_ctx *ctx, const uint64_t *a_open_dev, const uint64_t *p_dev, const uint64_t *q_dev, const uint64_t *pq_dev, int64_t trip_stride,
                     const uint64_t *rx_dev, const uint64_t *ry_dev, uint64_t *b_dev, int64_t m, void *stream) { HB_API_GUARD(ctx);
    JJ_STAGE_GUARD("hb_jj_add_stage1", !a_open_dev || !p_dev || !q_dev || !pq_dev || !rx_dev || !ry_dev || !b_dev);
    const JjTrip t = jj_trip(p_dev, q_dev, pq_dev, trip_stride);
    HB_DISPATCH(ctx, (k_jj_add_stage1<9, 8><<<blocks, 256, 0, s>>>(ctx->pw, (const uint32_t *)a_open_dev, t, (const uint32_t *)rx_dev, (const uint32_t *)ry_dev, (uint32_t *)b_dev, m)),
                (k_jj_add_stage1<3, 2><<<blocks, 256, 0, s>>>(ctx->pn, (const uint32_t *)a_open_dev, t, (const uint32_t *)rx_dev, (const uint32_t *)ry_dev, (uint32_t *)b_dev, m)));
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_jj_add_stage2(hb_ctx *ctx, const uint64_t *b_open_dev, const uint64_t *p_dev, const uint64_t *q_dev, const uint64_t *pq_dev, int64_t trip_stride,
                     const uint64_t *rx_dev, const uint64_t *ry_dev, const uint64_t *d_host, uint64_t *uv_dev, uint64_t *c_dev, int64_t m, void *stream) { HB_API_GUARD(ctx);
    JJ_STAGE_GUARD("hb_jj_add_stage2", !b_open_dev || !p_dev || !q_dev || !pq_dev || !rx_dev || !ry_dev || !uv_dev || !c_dev);
    JjConsts c;
    if (!d_host || !jj_consts(ctx, c, nullptr, d_host)) return fail(ctx, HB_ERR_BAD_ARG, "hb_jj_add_stage2: d is missing or not below the modulus");
    const JjTrip t = jj_trip(p_dev, q_dev, pq_dev, trip_stride);
    HB_DISPATCH(ctx, (k_jj_add_stage2<9, 8><<<blocks, 256, 0, s>>>(ctx->pw, (const uint32_t *)b_open_dev, t, (const uint32_t *)rx_dev, (const uint32_t *)ry_dev, c.dw, (uint32_t *)uv_dev, (uint32_t *)c_dev, m)),
                (k_jj_add_stage2<3, 2><<<blocks, 256, 0, s>>>(ctx->pn, (const uint32_t *)b_open_dev, t, (const uint32_t *)rx_dev, (const uint32_t *)ry_dev, c.dn, (uint32_t *)uv_dev, (uint32_t *)c_dev, m)));
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_jj_add_stage3(hb_ctx *ctx, const uint64_t *c_open_dev, const uint64_t *p_dev, const uint64_t *q_dev, const uint64_t *pq_dev, int64_t trip_stride,
                     uint64_t *d_dev, int64_t m, void *stream) { HB_API_GUARD(ctx);
    JJ_STAGE_GUARD("hb_jj_add_stage3", !c_open_dev || !p_dev || !q_dev || !pq_dev || !d_dev);
    const JjTrip t = jj_trip(p_dev, q_dev, pq_dev, trip_stride);
    HB_DISPATCH(ctx, (k_jj_add_stage3<9, 8><<<blocks, 256, 0, s>>>(ctx->pw, (const uint32_t *)c_open_dev, t, (uint32_t *)d_dev, m)),
                (k_jj_add_stage3<3, 2><<<blocks, 256, 0, s>>>(ctx->pn, (const uint32_t *)c_open_dev, t, (uint32_t *)d_dev, m)));
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_jj_add_finish(hb_ctx *ctx, const uint64_t *d_open_dev, const uint64_t *uv_dev, uint64_t *inv_dev, uint64_t *x3_dev, uint64_t *y3_dev, int64_t m,
                     int32_t *zeros_dev, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || m < 0 || (m > 0 && (!d_open_dev || !uv_dev || !inv_dev || !x3_dev || !y3_dev))) return HB_ERR_BAD_ARG;
    if (m > 0 && (x3_dev == y3_dev || x3_dev == inv_dev || y3_dev == inv_dev || x3_dev == uv_dev || y3_dev == uv_dev))
        return fail(ctx, HB_ERR_BAD_ARG, "hb_jj_add_finish: the outputs must be distinct from each other, from uv and from the inverses");
    if (m == 0) return HB_OK;
    unsigned blocks;
    if (!jj_blocks(m, &blocks)) return fail(ctx, HB_ERR_UNSUPPORTED, "hb_jj_add_finish: batch too large for one launch");
    hipStream_t s = (hipStream_t)stream;
    const int rc = hb_ew_inv(ctx, d_open_dev, inv_dev, 2 * m, zeros_dev, stream);
    if (rc != HB_OK) return rc;
    HB_DISPATCH(ctx, (k_jj_add_scale<9, 8><<<blocks, 256, 0, s>>>(ctx->pw, (const uint32_t *)inv_dev, (const uint32_t *)uv_dev, (uint32_t *)x3_dev, (uint32_t *)y3_dev, m)),
                (k_jj_add_scale<3, 2><<<blocks, 256, 0, s>>>(ctx->pn, (const uint32_t *)inv_dev, (const uint32_t *)uv_dev, (uint32_t *)x3_dev, (uint32_t *)y3_dev, m)));
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_selftest_jj(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *operands, const uint64_t *a, const uint64_t *d, int flags, int64_t arg,
                   uint64_t *out, int64_t count) {
    if (!p_limbs || !operands || count < 0 || (count > 0 && !out) || (n_limbs != 1 && n_limbs != 4)) return HB_ERR_BAD_ARG;
    int n_ops;
    switch (what) {
    case HB_JJ_SELFTEST_SCALAR_MUL:
        if (!a || !d || (flags & ~(HB_JJ_SCALAR_BROADCAST | HB_JJ_POINT_BROADCAST))) return HB_ERR_BAD_ARG;
        n_ops = 3; break;
    case HB_JJ_SELFTEST_DOUBLE_TABLE:
        if (!a || flags || arg < 1 || arg > 0x7fffffffLL) return HB_ERR_BAD_ARG;
        n_ops = 2; break;
    case HB_JJ_SELFTEST_MASK: n_ops = 6; break;
    case HB_JJ_SELFTEST_STAGE1: n_ops = 6; break;
    case HB_JJ_SELFTEST_STAGE2:
        if (!d) return HB_ERR_BAD_ARG;
        n_ops = 6; break;
    case HB_JJ_SELFTEST_STAGE3: n_ops = 4; break;
    case HB_JJ_SELFTEST_SCALE: n_ops = 2; break;
    default: return HB_ERR_BAD_ARG;
    }
    if (what >= HB_JJ_SELFTEST_MASK && what <= HB_JJ_SELFTEST_STAGE3 && (flags || arg < count)) return HB_ERR_BAD_ARG;
    if (what == HB_JJ_SELFTEST_SCALE && flags) return HB_ERR_BAD_ARG;
    for (int k = 0; k < n_ops; k++) if (count > 0 && !operands[k]) return HB_ERR_BAD_ARG;
    if (n_limbs == 4) return selftest_jj<9, 8>(p_limbs, what, operands, a, d, flags, arg, out, count);
    return selftest_jj<3, 2>(p_limbs, what, operands, a, d, flags, arg, out, count);
}

}  // extern "C"

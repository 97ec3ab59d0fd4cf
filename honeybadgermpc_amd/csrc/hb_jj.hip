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
// JjScalarMulRow     out_i = n_i P_i: the accumulator starts at (0 : 1 : 1 : 0) and takes the scalar's bits from the top, one
//                    doubling a bit and one mixed addition a set bit, 32 NW bits in a loop that is not unrolled (the scalar's words are
//                    shifted left a bit a round: no register array is indexed by the loop counter); one fp_inv at the end.  Everything
//                    stays in registers.  n_i = 0 leaves (0, 1).  Scalar and point: one for all (element 0) or one an element.
// JjDoubleTableRow   rows j < K of 2^j P_i, projective: the Montgomery residues X R, Y R, Z R of row j at [j][i] of three arrays.
//                    hb_jj_double_table then makes them affine with ONE hb_ew_inv over the K count values of Z and two hb_ew_op
//                    products ((X R) / (Z R) = x): no inversion an element and row.
//
// Shared addition (curves with a = -1, as the reference's law reads), for m independent pairs, every operand a share array:
//     x3 = (x1 y2 + y1 x2) / (1 + d x1 x2 y1 y2)          y3 = (y1 y2 + x1 x2) / (1 - d x1 x2 y1 y2)
// regrouped so that each numerator rides with the blinding of its denominator, num / den = (num r) / (den r) with den r opened:
// 9 Beaver triples and 2 random shares (rx, ry) a pair.  Triple k multiplies:  0 x1 x2,  1 y1 y2,  2 x1 y2,  3 y1 x2,  4 xp yp,
// 5 nx rx,  6 ny ry,  7 dx rx,  8 dy ry   (xp = x1 x2, yp = y1 y2, nx = x1 y2 + y1 x2, ny = yp + xp, dx = 1 + d xp yp, dy = 1 - d xp yp).
//   JjMaskRow         A [8][m]: rows 2k, 2k + 1 the masked factors (first - p_k, second - q_k) of products 0..3
//   JjStage1Row       opened A -> xp, yp, x1 y2, y1 x2 (four Beaver steps) -> B [6][m]: the masked factors of products 4..6
//   JjStage2Row       opened B -> [xp yp], u = [nx rx], v = [ny ry] (three Beaver steps); u, v kept ([2][m]); C [4][m]: the masked
//                     factors of products 7, 8.  A public 1 and d meet a share alike on every party.
//   JjStage3Row       opened C -> D [2][m]: the shares of sig_x = dx rx, sig_y = dy ry (two Beaver steps)
//   hb_jj_add_finish  opened D -> hb_ew_inv over its 2 m values (batched), then JjScaleRow: x3 = u / sig_x, y3 = v / sig_y
// A zero sig (r = 0, or operands off the curve) is counted by hb_ew_inv's counter.  Six launches and four opens an addition.
// Every Beaver step is ew_beaver_elem of hb_ew_elem.hpp, unchanged; everything between the steps is fp_add / fp_sub / mont_mul on
// canonical residues: there is NO lazy sum in this file beyond ew_beaver_elem's own (bounds stated there), so every digit is below 2^29
// and every value below p between two calls.  p = 2^256 - 189 with every operand p - 1 is the largest case (tests/test_jubjub_host.py).
//
// The steps are rows under the generic kernel k_rows (hb_rows.hpp): a step's row -- which elements it loads, which body it calls,
// where it stores -- is an HB_HD function over a memory policy, so hb_selftest_jj runs on the host the very rows, arithmetic and
// addressing, that k_rows runs on the device.  A row loads what it needs when it needs it -- a stage reads up to 28 elements, more
// than a lane holds at once -- and stores as it goes.  Outputs are distinct arrays.
// Launch shape (all steps): 256-thread workgroups, one element (pair) a thread, grid = ceil(count / 256), no LDS, no grid stride,
// the caller's stream.  What was just opened and the preprocessing are read once: the 32-byte width takes the non-temporal loads.
// Compiler's report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): DESIGN.md section 3l and profiles/jubjub.txt.
#include "hb_common.hpp"
#include "hb_ew_elem.hpp"
#include "hb_rows.hpp"

using namespace hb;

namespace hb {

template <int NL> struct JjPoint { uint32_t X[NL], Y[NL], Z[NL], T[NL]; };
// one party's triples: row k of a component starts k * stride elements behind its base
struct JjTrip { const uint32_t *p, *q, *pq; int64_t stride; };

// ---------------------------------------------------------------- per-element bodies (host and device)
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

// ---------------------------------------------------------------- digits through a memory policy (hb_rows.hpp)
template <int NL, int NW, class Mem> HB_HD void jj_get(uint32_t (&d)[NL], const Mem &mem, const uint32_t *base, int64_t e) {
    uint32_t w[NW];
    mem.load(w, base, e);
    unpack<NL, NW>(d, w);
}
template <int NL, int NW, class Mem> HB_HD void jj_get_once(uint32_t (&d)[NL], const Mem &mem, const uint32_t *base, int64_t e) {
    uint32_t w[NW];
    mem.once(w, base, e);
    unpack<NL, NW>(d, w);
}
template <int NL, int NW, class Mem> HB_HD void jj_put(const Mem &mem, uint32_t *base, int64_t e, const uint32_t (&d)[NL]) {
    uint32_t w[NW];
    pack<NL, NW>(w, d);
    mem.store(base, e, w);
}
// out[e] = v - mask[k]
template <int NL, int NW, class Mem>
HB_HD void jj_put_diff(const Mem &mem, uint32_t *out, int64_t e, const uint32_t (&v)[NL], const uint32_t *mask, int64_t k, const FpParams<NL> &P) {
    uint32_t kd[NL], r[NL];
    jj_get_once<NL, NW>(kd, mem, mask, k);
    fp_sub<NL>(r, v, kd, P);
    jj_put<NL, NW>(mem, out, e, r);
}
// o = the Beaver step of triple k on the opened factors in rows r, r + 1 of `opened` (m elements a row)
template <int NL, int NW, class Mem>
HB_HD void jj_beaver(uint32_t (&o)[NL], const Mem &mem, const uint32_t *opened, int r, const JjTrip &t, int k, int64_t i, int64_t m, const FpParams<NL> &P) {
    uint32_t dw[NW], ew[NW], pw[NW], qw[NW], pqw[NW], ow[NW];
    const int64_t at = (int64_t)k * t.stride + i;
    mem.once(dw, opened, (int64_t)r * m + i);
    mem.once(ew, opened, (int64_t)(r + 1) * m + i);
    mem.once(pw, t.p, at);
    mem.once(qw, t.q, at);
    mem.once(pqw, t.pq, at);
    ew_beaver_elem<NL, NW>(ow, dw, ew, pw, qw, pqw, P);
    unpack<NL, NW>(o, ow);
}

// ---------------------------------------------------------------- the steps' rows (host and device, over a memory policy: hb_rows.hpp)
// One row a step: `count` is the element count of the cleartext steps and the pair count m of the shared addition.  An array of
// several rows of m elements is addressed at row * m + i, the triples at k * t.stride + i: they keep their own row stride.  A stage
// reads up to 28 elements, more than a lane holds at once, so a row loads what it needs when it needs it.
template <int NL> struct JjScalarMulArgs { const uint32_t *n, *x, *y; int n_bcast, p_bcast; uint32_t *ox, *oy; FpConst<NL> am, dm; };

struct JjScalarMulRow {
    template <int NL, int NW, class Mem>
    HB_HD static void run(const JjScalarMulArgs<NL> &A, int, int64_t i, int64_t, const Mem &mem, const FpParams<NL> &P) {
        uint32_t nw[NW], xw[NW], yw[NW], rx[NW], ry[NW];
        mem.load(nw, A.n, A.n_bcast ? 0 : i);
        mem.load(xw, A.x, A.p_bcast ? 0 : i);
        mem.load(yw, A.y, A.p_bcast ? 0 : i);
        jj_scalar_mul_elem<NL, NW>(rx, ry, nw, xw, yw, A.am.d, A.dm.d, P);
        mem.store(A.ox, i, rx);
        mem.store(A.oy, i, ry);
    }
};

// rows j < K of 2^j (x, y), projective, as the Montgomery residues of X, Y, Z: row j of element i at j * count + i.  The rows are
// walked in the thread: each is the double of the one before.
template <int NL> struct JjDoubleTableArgs { const uint32_t *x, *y; uint32_t *xs, *ys, *zs; int K; FpConst<NL> am; };

struct JjDoubleTableRow {
    template <int NL, int NW, class Mem>
    HB_HD static void run(const JjDoubleTableArgs<NL> &A, int, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
        uint32_t t[NL];
        JjPoint<NL> acc;
        jj_get<NL, NW>(t, mem, A.x, i);
        to_mont<NL>(acc.X, t, P);
        jj_get<NL, NW>(t, mem, A.y, i);
        to_mont<NL>(acc.Y, t, P);
        mont_mul<NL>(acc.T, acc.X, acc.Y, P);
        fp_set<NL>(acc.Z, P.one);
#pragma unroll 1
        for (int j = 0; j < A.K; j++) {
            const int64_t at = (int64_t)j * count + i;
            jj_put<NL, NW>(mem, A.xs, at, acc.X);
            jj_put<NL, NW>(mem, A.ys, at, acc.Y);
            jj_put<NL, NW>(mem, A.zs, at, acc.Z);
            if (j + 1 < A.K) jj_double<NL>(acc, acc, A.am.d, P);
        }
    }
};

// A[2k] = first_k - p_k, A[2k + 1] = second_k - q_k for the products 0 x1 x2, 1 y1 y2, 2 x1 y2, 3 y1 x2
struct JjMaskArgs { const uint32_t *x1, *y1, *x2, *y2; JjTrip t; uint32_t *A; };

struct JjMaskRow {
    template <int NL, int NW, class Mem>
    HB_HD static void run(const JjMaskArgs &A, int, int64_t i, int64_t m, const Mem &mem, const FpParams<NL> &P) {
        const auto row = [&](int r) { return (int64_t)r * m + i; };
        const auto trip = [&](int k) { return (int64_t)k * A.t.stride + i; };
        uint32_t xa[NL], ya[NL], xb[NL], yb[NL];
        jj_get<NL, NW>(xa, mem, A.x1, i);
        jj_get<NL, NW>(ya, mem, A.y1, i);
        jj_get<NL, NW>(xb, mem, A.x2, i);
        jj_get<NL, NW>(yb, mem, A.y2, i);
        jj_put_diff<NL, NW>(mem, A.A, row(0), xa, A.t.p, trip(0), P);
        jj_put_diff<NL, NW>(mem, A.A, row(1), xb, A.t.q, trip(0), P);
        jj_put_diff<NL, NW>(mem, A.A, row(2), ya, A.t.p, trip(1), P);
        jj_put_diff<NL, NW>(mem, A.A, row(3), yb, A.t.q, trip(1), P);
        jj_put_diff<NL, NW>(mem, A.A, row(4), xa, A.t.p, trip(2), P);
        jj_put_diff<NL, NW>(mem, A.A, row(5), yb, A.t.q, trip(2), P);
        jj_put_diff<NL, NW>(mem, A.A, row(6), ya, A.t.p, trip(3), P);
        jj_put_diff<NL, NW>(mem, A.A, row(7), xb, A.t.q, trip(3), P);
    }
};

// stages 1 and 3: `in` is the array just opened, `out` the next one (stage 3 takes no rx, ry)
struct JjStageArgs { const uint32_t *in; JjTrip t; const uint32_t *rx, *ry; uint32_t *out; };

// opened A -> B: xp - p4, yp - q4, nx - p5, rx - q5, ny - p6, ry - q6
struct JjStage1Row {
    template <int NL, int NW, class Mem>
    HB_HD static void run(const JjStageArgs &A, int, int64_t i, int64_t m, const Mem &mem, const FpParams<NL> &P) {
        const auto row = [&](int r) { return (int64_t)r * m + i; };
        const auto trip = [&](int k) { return (int64_t)k * A.t.stride + i; };
        uint32_t xp[NL], yp[NL], a[NL], b[NL], n[NL];
        jj_beaver<NL, NW>(xp, mem, A.in, 0, A.t, 0, i, m, P);
        jj_beaver<NL, NW>(yp, mem, A.in, 2, A.t, 1, i, m, P);
        jj_put_diff<NL, NW>(mem, A.out, row(0), xp, A.t.p, trip(4), P);
        jj_put_diff<NL, NW>(mem, A.out, row(1), yp, A.t.q, trip(4), P);
        fp_add<NL>(n, yp, xp, P);
        jj_put_diff<NL, NW>(mem, A.out, row(4), n, A.t.p, trip(6), P);
        jj_beaver<NL, NW>(a, mem, A.in, 4, A.t, 2, i, m, P);
        jj_beaver<NL, NW>(b, mem, A.in, 6, A.t, 3, i, m, P);
        fp_add<NL>(n, a, b, P);
        jj_put_diff<NL, NW>(mem, A.out, row(2), n, A.t.p, trip(5), P);
        jj_get<NL, NW>(a, mem, A.rx, i);
        jj_put_diff<NL, NW>(mem, A.out, row(3), a, A.t.q, trip(5), P);
        jj_get<NL, NW>(b, mem, A.ry, i);
        jj_put_diff<NL, NW>(mem, A.out, row(5), b, A.t.q, trip(6), P);
    }
};

// opened B -> uv = (u, v) = ([nx rx], [ny ry]) and C: dx - p7, rx - q7, dy - p8, ry - q8 with dx = 1 + d [xp yp], dy = 1 - d [xp yp]
template <int NL> struct JjStage2Args { const uint32_t *B; JjTrip t; const uint32_t *rx, *ry; uint32_t *uv, *C; FpConst<NL> dm; };

struct JjStage2Row {
    template <int NL, int NW, class Mem>
    HB_HD static void run(const JjStage2Args<NL> &A, int, int64_t i, int64_t m, const Mem &mem, const FpParams<NL> &P) {
        const auto row = [&](int r) { return (int64_t)r * m + i; };
        const auto trip = [&](int k) { return (int64_t)k * A.t.stride + i; };
        uint32_t w[NL], s[NL], one[NL];
        jj_beaver<NL, NW>(w, mem, A.B, 2, A.t, 5, i, m, P);
        jj_put<NL, NW>(mem, A.uv, row(0), w);
        jj_beaver<NL, NW>(w, mem, A.B, 4, A.t, 6, i, m, P);
        jj_put<NL, NW>(mem, A.uv, row(1), w);
        jj_beaver<NL, NW>(s, mem, A.B, 0, A.t, 4, i, m, P);
        mont_mul<NL>(w, s, A.dm.d, P);                              // d [xp yp]: a plain residue times d R
        small_digits<NL>(one, 1);
        fp_add<NL>(s, one, w, P);
        jj_put_diff<NL, NW>(mem, A.C, row(0), s, A.t.p, trip(7), P);
        fp_sub<NL>(s, one, w, P);
        jj_put_diff<NL, NW>(mem, A.C, row(2), s, A.t.p, trip(8), P);
        jj_get<NL, NW>(w, mem, A.rx, i);
        jj_put_diff<NL, NW>(mem, A.C, row(1), w, A.t.q, trip(7), P);
        jj_get<NL, NW>(w, mem, A.ry, i);
        jj_put_diff<NL, NW>(mem, A.C, row(3), w, A.t.q, trip(8), P);
    }
};

// opened C -> D = ([dx rx], [dy ry])
struct JjStage3Row {
    template <int NL, int NW, class Mem>
    HB_HD static void run(const JjStageArgs &A, int, int64_t i, int64_t m, const Mem &mem, const FpParams<NL> &P) {
        uint32_t s[NL];
        jj_beaver<NL, NW>(s, mem, A.in, 0, A.t, 7, i, m, P);
        jj_put<NL, NW>(mem, A.out, i, s);
        jj_beaver<NL, NW>(s, mem, A.in, 2, A.t, 8, i, m, P);
        jj_put<NL, NW>(mem, A.out, m + i, s);
    }
};

// x3 = u / sig_x, y3 = v / sig_y from the inverted sigs: a product of two plain residues is two Montgomery products (ew_binary_elem)
struct JjScaleArgs { const uint32_t *inv, *uv; uint32_t *x3, *y3; };

struct JjScaleRow {
    template <int NL, int NW, class Mem>
    HB_HD static void run(const JjScaleArgs &A, int, int64_t i, int64_t m, const Mem &mem, const FpParams<NL> &P) {
        uint32_t a[NL], b[NL], r[NL];
        jj_get_once<NL, NW>(a, mem, A.inv, i);
        jj_get_once<NL, NW>(b, mem, A.uv, i);
        mont_mul<NL>(r, a, b, P);
        mont_mul<NL>(a, P.r2, r, P);
        jj_put<NL, NW>(mem, A.x3, i, a);
        jj_get_once<NL, NW>(a, mem, A.inv, m + i);
        jj_get_once<NL, NW>(b, mem, A.uv, m + i);
        mont_mul<NL>(r, a, b, P);
        mont_mul<NL>(a, P.r2, r, P);
        jj_put<NL, NW>(mem, A.y3, i, a);
    }
};

// ---------------------------------------------------------------- host side
static JjTrip jj_trip(const uint64_t *p, const uint64_t *q, const uint64_t *pq, int64_t stride) { return JjTrip{u32(p), u32(q), u32(pq), stride}; }

// a curve constant from its packed words -> Montgomery digits; false if it is missing or not below p
template <int NL> static bool jj_curve_const(FpConst<NL> &c, const FpParams<NL> &P, const uint64_t *host) {
    return host && host_mont<NL, words_of(NL)>(c.d, P, host);
}

// host: the same rows over `count` elements.  `out` is ONE buffer: a step's second and third output start behind the first.
template <int NL, int NW>
static int selftest_jj(const uint64_t *p_limbs, int what, const uint64_t *const *ops, const uint64_t *a_host, const uint64_t *d_host, int flags, int64_t arg,
                       uint64_t *out, int64_t count) {
    FpParams<NL> P;
    fp_params_from_limbs(P, p_limbs);
    FpConst<NL> am = {}, dm = {};
    if ((a_host && !jj_curve_const(am, P, a_host)) || (d_host && !jj_curve_const(dm, P, d_host))) return HB_ERR_BAD_ARG;
    uint32_t *o = u32(out);
    if (what == HB_JJ_SELFTEST_SCALAR_MUL) {
        const JjScalarMulArgs<NL> A = {u32(ops[0]), u32(ops[1]), u32(ops[2]), (flags & HB_JJ_SCALAR_BROADCAST) != 0, (flags & HB_JJ_POINT_BROADCAST) != 0, o, o + count * NW, am, dm};
        host_rows<JjScalarMulRow, NL, NW>(A, 1, count, P);
    } else if (what == HB_JJ_SELFTEST_DOUBLE_TABLE) {
        const int K = (int)arg;
        const JjDoubleTableArgs<NL> A = {u32(ops[0]), u32(ops[1]), o, o + (int64_t)K * count * NW, o + 2 * (int64_t)K * count * NW, K, am};
        host_rows<JjDoubleTableRow, NL, NW>(A, 1, count, P);
    } else if (what == HB_JJ_SELFTEST_SCALE) {
        const JjScaleArgs A = {u32(ops[0]), u32(ops[1]), o, o + count * NW};
        host_rows<JjScaleRow, NL, NW>(A, 1, count, P);
    } else if (what == HB_JJ_SELFTEST_MASK) {
        const JjMaskArgs A = {u32(ops[0]), u32(ops[1]), u32(ops[2]), u32(ops[3]), jj_trip(ops[4], ops[5], nullptr, arg), o};
        host_rows<JjMaskRow, NL, NW>(A, 1, count, P);
    } else if (what == HB_JJ_SELFTEST_STAGE2) {
        const JjStage2Args<NL> A = {u32(ops[0]), jj_trip(ops[1], ops[2], ops[3], arg), u32(ops[4]), u32(ops[5]), o, o + 2 * count * NW, dm};
        host_rows<JjStage2Row, NL, NW>(A, 1, count, P);
    } else {
        const bool first = what == HB_JJ_SELFTEST_STAGE1;
        const JjStageArgs A = {u32(ops[0]), jj_trip(ops[1], ops[2], ops[3], arg), first ? u32(ops[4]) : nullptr, first ? u32(ops[5]) : nullptr, o};
        if (first) host_rows<JjStage1Row, NL, NW>(A, 1, count, P);
        else host_rows<JjStage3Row, NL, NW>(A, 1, count, P);
    }
    return HB_OK;
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
    HB_ROW_BLOCKS(ctx, "hb_jj_scalar_mul");
    const int rc = launch_rows<JjScalarMulRow, JjScalarMulArgs>(ctx, [&](auto &A, const auto &P) {
        A.n = u32(n_dev); A.x = u32(x_dev); A.y = u32(y_dev); A.n_bcast = n_broadcast != 0; A.p_bcast = point_broadcast != 0; A.ox = u32(outx_dev); A.oy = u32(outy_dev);
        return jj_curve_const(A.am, P, a_host) && jj_curve_const(A.dm, P, d_host);
    }, (unsigned)blocks, s, count);
    return rc == HB_ERR_BAD_ARG ? fail(ctx, rc, "hb_jj_scalar_mul: a curve constant is not below the modulus") : rc;
}

int hb_jj_double_table(hb_ctx *ctx, const uint64_t *x_dev, const uint64_t *y_dev, const uint64_t *a_host, int rows, uint64_t *xs_dev, uint64_t *ys_dev, uint64_t *zs_dev,
                       int64_t count, int32_t *zeros_dev, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0 || !a_host || (count > 0 && (!x_dev || !y_dev || !xs_dev || !ys_dev || !zs_dev))) return HB_ERR_BAD_ARG;
    if (rows < 1) return fail(ctx, HB_ERR_BAD_ARG, "hb_jj_double_table: at least one row");
    if (count > 0 && (xs_dev == ys_dev || xs_dev == zs_dev || ys_dev == zs_dev)) return fail(ctx, HB_ERR_BAD_ARG, "hb_jj_double_table: the three arrays must be distinct");
    HB_ROW_BLOCKS(ctx, "hb_jj_double_table");
    if (count > INT64_MAX / rows / 64) return fail(ctx, HB_ERR_UNSUPPORTED, "hb_jj_double_table: batch too large for one launch");
    int rc = launch_rows<JjDoubleTableRow, JjDoubleTableArgs>(ctx, [&](auto &A, const auto &P) {
        A.x = u32(x_dev); A.y = u32(y_dev); A.xs = u32(xs_dev); A.ys = u32(ys_dev); A.zs = u32(zs_dev); A.K = rows;
        return jj_curve_const(A.am, P, a_host);
    }, (unsigned)blocks, s, count);
    if (rc == HB_ERR_BAD_ARG) return fail(ctx, rc, "hb_jj_double_table: a is not below the modulus");
    if (rc != HB_OK || count == 0) return rc;
    // affine: (X R) / (Z R) = x -- one batched inversion over every row's Z, two element-wise products
    const int64_t all = (int64_t)rows * count;
    rc = hb_ew_inv(ctx, zs_dev, zs_dev, all, zeros_dev, stream);
    if (rc == HB_OK) rc = hb_ew_op(ctx, HB_EW_MUL, xs_dev, zs_dev, 0, xs_dev, all, stream);
    if (rc == HB_OK) rc = hb_ew_op(ctx, HB_EW_MUL, ys_dev, zs_dev, 0, ys_dev, all, stream);
    return rc;
}

// what the five stages of the shared addition check alike; count = m for HB_ROW_BLOCKS
#define JJ_STAGE_GUARD(name, nullcheck)                                                                                           \
    if (!ctx || m < 0 || (m > 0 && (nullcheck))) return HB_ERR_BAD_ARG;                                                           \
    if (trip_stride < m) return fail(ctx, HB_ERR_BAD_ARG, name ": the triples' row stride is below the pair count");              \
    if (m == 0) return HB_OK;                                                                                                     \
    const int64_t count = m;                                                                                                      \
    HB_ROW_BLOCKS(ctx, name);                                                                                                     \
    if (trip_stride > INT64_MAX / 1024) return fail(ctx, HB_ERR_UNSUPPORTED, name ": batch too large for one launch")

int hb_jj_add_mask(hb_ctx *ctx, const uint64_t *x1_dev, const uint64_t *y1_dev, const uint64_t *x2_dev, const uint64_t *y2_dev, const uint64_t *p_dev,
                   const uint64_t *q_dev, int64_t trip_stride, uint64_t *a_dev, int64_t m, void *stream) { HB_API_GUARD(ctx);
    JJ_STAGE_GUARD("hb_jj_add_mask", !x1_dev || !y1_dev || !x2_dev || !y2_dev || !p_dev || !q_dev || !a_dev);
    const JjMaskArgs A = {u32(x1_dev), u32(y1_dev), u32(x2_dev), u32(y2_dev), jj_trip(p_dev, q_dev, nullptr, trip_stride), u32(a_dev)};
    return launch_rows<JjMaskRow>(ctx, A, (unsigned)blocks, s, count);
}

int hb_jj_add_stage1(hb_ctx *ctx, const uint64_t *a_open_dev, const uint64_t *p_dev, const uint64_t *q_dev, const uint64_t *pq_dev, int64_t trip_stride,
                     const uint64_t *rx_dev, const uint64_t *ry_dev, uint64_t *b_dev, int64_t m, void *stream) { HB_API_GUARD(ctx);
    JJ_STAGE_GUARD("hb_jj_add_stage1", !a_open_dev || !p_dev || !q_dev || !pq_dev || !rx_dev || !ry_dev || !b_dev);
    const JjStageArgs A = {u32(a_open_dev), jj_trip(p_dev, q_dev, pq_dev, trip_stride), u32(rx_dev), u32(ry_dev), u32(b_dev)};
    return launch_rows<JjStage1Row>(ctx, A, (unsigned)blocks, s, count);
}

int hb_jj_add_stage2(hb_ctx *ctx, const uint64_t *b_open_dev, const uint64_t *p_dev, const uint64_t *q_dev, const uint64_t *pq_dev, int64_t trip_stride,
                     const uint64_t *rx_dev, const uint64_t *ry_dev, const uint64_t *d_host, uint64_t *uv_dev, uint64_t *c_dev, int64_t m, void *stream) { HB_API_GUARD(ctx);
    JJ_STAGE_GUARD("hb_jj_add_stage2", !b_open_dev || !p_dev || !q_dev || !pq_dev || !rx_dev || !ry_dev || !uv_dev || !c_dev);
    const int rc = launch_rows<JjStage2Row, JjStage2Args>(ctx, [&](auto &A, const auto &P) {
        A.B = u32(b_open_dev); A.t = jj_trip(p_dev, q_dev, pq_dev, trip_stride); A.rx = u32(rx_dev); A.ry = u32(ry_dev); A.uv = u32(uv_dev); A.C = u32(c_dev);
        return jj_curve_const(A.dm, P, d_host);
    }, (unsigned)blocks, s, count);
    return rc == HB_ERR_BAD_ARG ? fail(ctx, rc, "hb_jj_add_stage2: d is missing or not below the modulus") : rc;
}

int hb_jj_add_stage3(hb_ctx *ctx, const uint64_t *c_open_dev, const uint64_t *p_dev, const uint64_t *q_dev, const uint64_t *pq_dev, int64_t trip_stride,
                     uint64_t *d_dev, int64_t m, void *stream) { HB_API_GUARD(ctx);
    JJ_STAGE_GUARD("hb_jj_add_stage3", !c_open_dev || !p_dev || !q_dev || !pq_dev || !d_dev);
    const JjStageArgs A = {u32(c_open_dev), jj_trip(p_dev, q_dev, pq_dev, trip_stride), nullptr, nullptr, u32(d_dev)};
    return launch_rows<JjStage3Row>(ctx, A, (unsigned)blocks, s, count);
}

int hb_jj_add_finish(hb_ctx *ctx, const uint64_t *d_open_dev, const uint64_t *uv_dev, uint64_t *inv_dev, uint64_t *x3_dev, uint64_t *y3_dev, int64_t m,
                     int32_t *zeros_dev, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || m < 0 || (m > 0 && (!d_open_dev || !uv_dev || !inv_dev || !x3_dev || !y3_dev))) return HB_ERR_BAD_ARG;
    if (m > 0 && (x3_dev == y3_dev || x3_dev == inv_dev || y3_dev == inv_dev || x3_dev == uv_dev || y3_dev == uv_dev))
        return fail(ctx, HB_ERR_BAD_ARG, "hb_jj_add_finish: the outputs must be distinct from each other, from uv and from the inverses");
    if (m == 0) return HB_OK;
    const int64_t count = m;
    HB_ROW_BLOCKS(ctx, "hb_jj_add_finish");
    const int rc = hb_ew_inv(ctx, d_open_dev, inv_dev, 2 * m, zeros_dev, stream);
    if (rc != HB_OK) return rc;
    const JjScaleArgs A = {u32(inv_dev), u32(uv_dev), u32(x3_dev), u32(y3_dev)};
    return launch_rows<JjScaleRow>(ctx, A, (unsigned)blocks, s, count);
}

#undef JJ_STAGE_GUARD

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

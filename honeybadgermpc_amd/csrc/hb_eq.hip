// hb_eq.hip -- equality of shared values, the reference's Equality mixin (progs/mixins/share_comparison.py:9-80, the probabilistic
// Legendre-symbol test) for arrays of values -- restated on fp29.hpp, not translated.
//
// For every compared pair and each of `rows` test bits the protocol draws a bit share [b] and two random shares [r], [rp], opens
//     c = diff r + _b rp^2,   _b = nr - (nr - 1) b  in {nr, 1},   nr a public quadratic non-residue,
// and turns L = legendre(c) into a factor that is affine in [b]; the product of the factors is the answer.  The three products cost
// three opens: (diff r, rp rp) together, then _b rp^2, then c itself.  Preprocessing arrives as planes: row j of a plane holds test
// bit j's value of every element, so a wave's loads of a row cover consecutive elements.
//
// k_legendre     out[i] = legendre(a_i) in {-1, 0, 1} as int8: a^((p-1)/2) against one and minus one in Montgomery form.  The exponent
//                is the same for every lane: the host derives ONE sliding-window schedule from p (window 3: the odd powers a, a^3, a^5,
//                a^7 stay in registers) and hands it to the kernel by value, so its steps sit in SGPRs and the chain has no divergence.
//                254 squarings and 64 + 4 products for the BLS12-381 scalar field against 254 + ~127 bit by bit.  A zero skips the chain.
// k_eq_mask1     diff = x - y (y may be absent: a test against zero), then the four masked differences of the first two Beaver products
//                of every test bit into ONE array to open, (4, rows, count): diff - pa, r - qa, rp - pb, rp - qb.
// k_eq_mid       that array opened: [diff r] and [rp^2] by ew_beaver_elem, _b = nr - (nr - 1) [b] (one product by a public constant),
//                the next array to open (2, rows, count): _b - pc, [rp^2] - qc, and the plane [diff r].
// k_eq_cshare    [c] = [diff r] + beaver(opened2, triple c): the third array to open.
// k_eq_finish    c opened: the Legendre chain of k_legendre and the affine map of the mode in the same launch,
//                   HB_EQ_BIT        (1 - L) / 2 + L [b]                              a share of exactly 1 or 0
//                   HB_EQ_REFERENCE  L (nr + L) / 2 - (L (nr - 1) / 2) [b]            the reference's expression (nr = 5 there)
//                and zero_rows[row] = 1 where some c of the row is 0 (plain vector stores; every writer stores the same value).
//
// Operands and results are packed canonical residues.  The per-element bodies are HB_HD functions: the __global__ wrappers only
// load, call them and store, and hb_selftest_eq runs the very same functions on the host.
//
// Launch shape (all kernels): 256-thread workgroups, one element a thread in x, the test bit (row) in blockIdx.y.  No LDS, no grid
// stride, one launch a call.  diff is one subtraction and is recomputed by each row's thread from x and y (which stay in L2) rather
// than stored as a plane of its own.  Planes, triples and opened values are read once: the 32-byte width takes the non-temporal
// loads, as k_ew_beaver.
// Compiler's report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): DESIGN.md section 3n.
#include "hb_common.hpp"
#include "hb_ew_elem.hpp"
#include "hb_rows.hpp"

using namespace hb;

namespace hb {

// The exponent (p - 1) / 2 as a left-to-right sliding-window schedule, window EQ_WINDOW: acc starts as table[first]; step s squares
// acc (step >> 8) times and then, if (step & 0xff) != 0, multiplies it by table[(step & 0xff) - 1]; table[k] = a^(2k + 1).
// A multiplying step consumes at least three exponent bits (but for the last), so a 256-bit exponent takes at most 87 steps.
constexpr int EQ_WINDOW = 3;
constexpr int EQ_TABLE = 1 << (EQ_WINDOW - 1);
constexpr int EQ_MAX_STEPS = 96;
struct EqSched { uint32_t first, n; uint32_t step[EQ_MAX_STEPS]; };

// a field element as digits, handed to a kernel by value
template <int NL> struct EqMidConsts { uint32_t nr[NL], nm1m[NL]; };                  // nr canonical, (nr - 1) R
// factor = a + b [bit] with (a, b) chosen by L: a canonical, b in Montgomery form
template <int NL> struct EqFinishConsts { uint32_t a_pos[NL], b_pos[NL], a_neg[NL], b_neg[NL]; };

// ---------------------------------------------------------------- per-element bodies (host and device)
// r = table entry k, a chain of selects on a wave-uniform k: the table stays in registers (an indexed array would go to scratch)
template <int NL>
HB_HD void eq_pick(uint32_t (&r)[NL], const uint32_t (&t1)[NL], const uint32_t (&t3)[NL], const uint32_t (&t5)[NL], const uint32_t (&t7)[NL], uint32_t k) {
#pragma unroll
    for (int q = 0; q < NL; q++) r[q] = k == 0 ? t1[q] : (k == 1 ? t3[q] : (k == 2 ? t5[q] : t7[q]));
}

// legendre(a) for canonical digits a < p: a^((p-1)/2) is one, minus one, or (a = 0) zero
template <int NL> HB_HD int eq_legendre(const uint32_t (&a)[NL], const EqSched &S, const FpParams<NL> &P) {
    if (fp_is_zero<NL>(a)) return 0;
    static_assert(EQ_TABLE == 4, "the table is four named arrays");
    uint32_t t1[NL], t3[NL], t5[NL], t7[NL], sq[NL], acc[NL], b[NL];
    to_mont<NL>(t1, a, P);
    mont_mul<NL>(sq, t1, t1, P);
    mont_mul<NL>(t3, t1, sq, P);
    mont_mul<NL>(t5, t3, sq, P);
    mont_mul<NL>(t7, t5, sq, P);
    eq_pick<NL>(acc, t1, t3, t5, t7, S.first);
#pragma unroll 1
    for (uint32_t s = 0; s < S.n; s++) {
        const uint32_t st = S.step[s], nsq = st >> 8, m = st & 0xffu;
#pragma unroll 1
        for (uint32_t j = 0; j < nsq; j++) mont_mul<NL>(acc, acc, acc, P);
        if (m) {
            eq_pick<NL>(b, t1, t3, t5, t7, m - 1);
            mont_mul<NL>(acc, acc, b, P);
        }
    }
    fp_neg<NL>(b, P.one, P);
    return fp_eq<NL>(acc, P.one) ? 1 : (fp_eq<NL>(acc, b) ? -1 : 0);
}

template <int NL, int NW> HB_HD int eq_legendre_elem(const uint32_t (&aw)[NW], const EqSched &S, const FpParams<NL> &P) {
    uint32_t a[NL];
    unpack<NL, NW>(a, aw);
    return eq_legendre<NL>(a, S, P);
}

// o = v - a on packed words

// the four masked differences of one test bit of one element; HAS_Y = false: diff = x
template <int NL, int NW, bool HAS_Y>
HB_HD void eq_mask1_elem(uint32_t (&o0)[NW], uint32_t (&o1)[NW], uint32_t (&o2)[NW], uint32_t (&o3)[NW], const uint32_t (&xw)[NW], const uint32_t (&yw)[NW],
                         const uint32_t (&rw)[NW], const uint32_t (&rpw)[NW], const uint32_t (&paw)[NW], const uint32_t (&qaw)[NW], const uint32_t (&pbw)[NW],
                         const uint32_t (&qbw)[NW], const FpParams<NL> &P) {
    uint32_t d[NL], a[NL], t[NL];
    unpack<NL, NW>(d, xw);
    if constexpr (HAS_Y) {
        unpack<NL, NW>(a, yw);
        fp_sub<NL>(t, d, a, P);
        fp_set<NL>(d, t);
    }
    unpack<NL, NW>(a, paw);
    fp_sub<NL>(t, d, a, P);
    pack<NL, NW>(o0, t);
    diff_elem<NL, NW>(o1, rw, qaw, P);
    diff_elem<NL, NW>(o2, rpw, pbw, P);
    diff_elem<NL, NW>(o3, rpw, qbw, P);
}

// m0 = _b - pc, m1 = [rp^2] - qc, dr = [diff r];  o0..o3 the first array opened
template <int NL, int NW>
HB_HD void eq_mid_elem(uint32_t (&m0)[NW], uint32_t (&m1)[NW], uint32_t (&dr)[NW], const uint32_t (&o0)[NW], const uint32_t (&o1)[NW], const uint32_t (&o2)[NW],
                       const uint32_t (&o3)[NW], const uint32_t (&paw)[NW], const uint32_t (&qaw)[NW], const uint32_t (&pqaw)[NW], const uint32_t (&pbw)[NW],
                       const uint32_t (&qbw)[NW], const uint32_t (&pqbw)[NW], const uint32_t (&bitw)[NW], const uint32_t (&pcw)[NW], const uint32_t (&qcw)[NW],
                       const EqMidConsts<NL> &K, const FpParams<NL> &P) {
    uint32_t rp2[NW], b[NL], t[NL], u[NL];
    ew_beaver_elem<NL, NW>(dr, o0, o1, paw, qaw, pqaw, P);
    ew_beaver_elem<NL, NW>(rp2, o2, o3, pbw, qbw, pqbw, P);
    unpack<NL, NW>(b, bitw);
    mont_mul<NL>(t, K.nm1m, b, P);                     // (nr - 1) [b], canonical
    fp_sub<NL>(u, K.nr, t, P);                         // _b
    unpack<NL, NW>(b, pcw);
    fp_sub<NL>(t, u, b, P);
    pack<NL, NW>(m0, t);
    diff_elem<NL, NW>(m1, rp2, qcw, P);
}

// [c] = [diff r] + [_b rp^2]
template <int NL, int NW>
HB_HD void eq_cshare_elem(uint32_t (&o)[NW], const uint32_t (&drw)[NW], const uint32_t (&dw)[NW], const uint32_t (&ew)[NW], const uint32_t (&pcw)[NW],
                          const uint32_t (&qcw)[NW], const uint32_t (&pqcw)[NW], const FpParams<NL> &P) {
    uint32_t mw[NW], mm[NL], d[NL], r[NL];
    ew_beaver_elem<NL, NW>(mw, dw, ew, pcw, qcw, pqcw, P);
    unpack<NL, NW>(mm, mw);
    unpack<NL, NW>(d, drw);
    fp_add<NL>(r, d, mm, P);
    pack<NL, NW>(o, r);
}

// the factor of one test bit: -> L; L = 0 (c = 0) writes 0, the row is to be drawn again
template <int NL, int NW>
HB_HD int eq_finish_elem(uint32_t (&o)[NW], const uint32_t (&cw)[NW], const uint32_t (&bitw)[NW], const EqSched &S, const EqFinishConsts<NL> &K, const FpParams<NL> &P) {
    const int L = eq_legendre_elem<NL, NW>(cw, S, P);
    if (L == 0) {
#pragma unroll
        for (int q = 0; q < NW; q++) o[q] = 0;
        return 0;
    }
    uint32_t b[NL], ka[NL], kb[NL], t[NL], r[NL];
    unpack<NL, NW>(b, bitw);
#pragma unroll
    for (int q = 0; q < NL; q++) { ka[q] = L > 0 ? K.a_pos[q] : K.a_neg[q]; kb[q] = L > 0 ? K.b_pos[q] : K.b_neg[q]; }
    mont_mul<NL>(t, kb, b, P);
    fp_add<NL>(r, ka, t, P);
    pack<NL, NW>(o, r);
    return L;
}

// ---------------------------------------------------------------- kernels
// read-once operands (planes, triples, what was just opened)

template <int NL, int NW>
__global__ void __launch_bounds__(256) k_legendre(const FpParams<NL> P, const EqSched S, const uint32_t *__restrict__ a, int8_t *__restrict__ out, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    uint32_t aw[NW];
    load_words<NW>(aw, a + i * NW);
    out[i] = (int8_t)eq_legendre_elem<NL, NW>(aw, S, P);
}

// masked: (4, rows, count), an array of its own
template <int NL, int NW, bool HAS_Y>
__global__ void __launch_bounds__(256) k_eq_mask1(const FpParams<NL> P, const uint32_t *__restrict__ x, const uint32_t *__restrict__ y, const uint32_t *__restrict__ r,
                                                  const uint32_t *__restrict__ rp, const uint32_t *__restrict__ pa, const uint32_t *__restrict__ qa,
                                                  const uint32_t *__restrict__ pb, const uint32_t *__restrict__ qb, uint32_t *__restrict__ masked, int64_t rows,
                                                  int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int64_t e = ((int64_t)blockIdx.y * count + i) * NW, plane = rows * count * NW;
    uint32_t xw[NW], yw[NW], rw[NW], rpw[NW], paw[NW], qaw[NW], pbw[NW], qbw[NW], o0[NW], o1[NW], o2[NW], o3[NW];
    load_words<NW>(xw, x + i * NW);
    if constexpr (HAS_Y) load_words<NW>(yw, y + i * NW);
    else {
#pragma unroll
        for (int q = 0; q < NW; q++) yw[q] = 0;
    }
    load_once<NW>(rw, r + e); load_once<NW>(rpw, rp + e);
    load_once<NW>(paw, pa + e); load_once<NW>(qaw, qa + e); load_once<NW>(pbw, pb + e); load_once<NW>(qbw, qb + e);
    eq_mask1_elem<NL, NW, HAS_Y>(o0, o1, o2, o3, xw, yw, rw, rpw, paw, qaw, pbw, qbw, P);
    store_words<NW>(masked + e, o0);
    store_words<NW>(masked + plane + e, o1);
    store_words<NW>(masked + 2 * plane + e, o2);
    store_words<NW>(masked + 3 * plane + e, o3);
}

template <int NL, int NW>
__global__ void __launch_bounds__(256) k_eq_mid(const FpParams<NL> P, const uint32_t *__restrict__ opened, const uint32_t *__restrict__ pa, const uint32_t *__restrict__ qa,
                                                const uint32_t *__restrict__ pqa, const uint32_t *__restrict__ pb, const uint32_t *__restrict__ qb,
                                                const uint32_t *__restrict__ pqb, const uint32_t *__restrict__ bits, const uint32_t *__restrict__ pc,
                                                const uint32_t *__restrict__ qc, const EqMidConsts<NL> K, uint32_t *__restrict__ masked2, uint32_t *__restrict__ dr,
                                                int64_t rows, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int64_t e = ((int64_t)blockIdx.y * count + i) * NW, plane = rows * count * NW;
    uint32_t o0[NW], o1[NW], o2[NW], o3[NW], paw[NW], qaw[NW], pqaw[NW], pbw[NW], qbw[NW], pqbw[NW], bw[NW], pcw[NW], qcw[NW], m0[NW], m1[NW], drw[NW];
    load_once<NW>(o0, opened + e); load_once<NW>(o1, opened + plane + e); load_once<NW>(o2, opened + 2 * plane + e); load_once<NW>(o3, opened + 3 * plane + e);
    load_once<NW>(paw, pa + e); load_once<NW>(qaw, qa + e); load_once<NW>(pqaw, pqa + e);
    load_once<NW>(pbw, pb + e); load_once<NW>(qbw, qb + e); load_once<NW>(pqbw, pqb + e);
    load_words<NW>(bw, bits + e); load_once<NW>(pcw, pc + e); load_words<NW>(qcw, qc + e);
    eq_mid_elem<NL, NW>(m0, m1, drw, o0, o1, o2, o3, paw, qaw, pqaw, pbw, qbw, pqbw, bw, pcw, qcw, K, P);
    store_words<NW>(masked2 + e, m0);
    store_words<NW>(masked2 + plane + e, m1);
    store_words<NW>(dr + e, drw);
}

// c may be dr (a thread reads its element before it writes it): no __restrict__ on the two
template <int NL, int NW>
__global__ void __launch_bounds__(256) k_eq_cshare(const FpParams<NL> P, const uint32_t *__restrict__ opened2, const uint32_t *dr, const uint32_t *__restrict__ pc,
                                                   const uint32_t *__restrict__ qc, const uint32_t *__restrict__ pqc, uint32_t *c, int64_t rows, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int64_t e = ((int64_t)blockIdx.y * count + i) * NW, plane = rows * count * NW;
    uint32_t dw[NW], ew[NW], drw[NW], pcw[NW], qcw[NW], pqcw[NW], ow[NW];
    load_once<NW>(dw, opened2 + e); load_once<NW>(ew, opened2 + plane + e);
    load_words<NW>(drw, dr + e);
    load_once<NW>(pcw, pc + e); load_once<NW>(qcw, qc + e); load_once<NW>(pqcw, pqc + e);
    eq_cshare_elem<NL, NW>(ow, drw, dw, ew, pcw, qcw, pqcw, P);
    store_words<NW>(c + e, ow);
}

// factor may be c or bits (a thread reads its element before it writes it)
template <int NL, int NW>
__global__ void __launch_bounds__(256) k_eq_finish(const FpParams<NL> P, const EqSched S, const EqFinishConsts<NL> K, const uint32_t *c, const uint32_t *bits,
                                                   uint32_t *factor, int32_t *__restrict__ zero_rows, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int64_t e = ((int64_t)blockIdx.y * count + i) * NW;
    uint32_t cw[NW], bw[NW], ow[NW];
    load_words<NW>(cw, c + e);
    load_words<NW>(bw, bits + e);
    const int L = eq_finish_elem<NL, NW>(ow, cw, bw, S, K, P);
    store_words<NW>(factor + e, ow);
    if (L == 0) zero_rows[blockIdx.y] = 1;
}

// ---------------------------------------------------------------- host side
static bool eq_make_sched(EqSched &S, const uint64_t *p_limbs, int n_limbs) {
    uint64_t e[4] = {0, 0, 0, 0};
    for (int i = 0; i < n_limbs; i++) e[i] = p_limbs[i];
    e[0] -= 1;                                                            // p odd: no borrow
    for (int i = 0; i < 4; i++) e[i] = (e[i] >> 1) | (i < 3 ? e[i + 1] << 63 : 0);
    int top = -1;
    for (int l = 3; l >= 0 && top < 0; l--)
        if (e[l]) top = 64 * l + 63 - __builtin_clzll(e[l]);
    if (top < 0) return false;                                            // p < 3
    auto bit = [&](int i) { return (uint32_t)((e[i >> 6] >> (i & 63)) & 1u); };
    S.first = 0; S.n = 0;
    bool started = false;
    uint32_t pending = 0;
    for (int i = top; i >= 0;) {
        if (!bit(i)) { pending++; i--; continue; }
        int l = i - EQ_WINDOW + 1 > 0 ? i - EQ_WINDOW + 1 : 0;
        while (!bit(l)) l++;
        uint32_t v = 0;
        for (int b = i; b >= l; b--) v = (v << 1) | bit(b);
        if (!started) { S.first = (v - 1) / 2; started = true; }
        else {
            if (S.n >= EQ_MAX_STEPS) return false;
            S.step[S.n++] = ((pending + (uint32_t)(i - l + 1)) << 8) | ((v - 1) / 2 + 1);
        }
        pending = 0;
        i = l - 1;
    }
    if (pending) {
        if (S.n >= EQ_MAX_STEPS) return false;
        S.step[S.n++] = pending << 8;
    }
    for (uint32_t s = S.n; s < EQ_MAX_STEPS; s++) S.step[s] = 0;
    return true;
}

// one canonical element in host memory -> digits; false if it is not below p
template <int NL, int NW> static bool eq_host_digits(uint32_t (&d)[NL], const FpParams<NL> &P, const uint64_t *host) {
    uint32_t w[NW];
    memcpy(w, host, NW * 4);
    unpack<NL, NW>(d, w);
    for (int i = NL - 1; i >= 0; i--)
        if (d[i] != P.p[i]) return d[i] < P.p[i];
    return false;
}
template <int NL> static void eq_small(uint32_t (&r)[NL], uint32_t v) {
    for (int q = 0; q < NL; q++) r[q] = q == 0 ? v : 0u;
}
// nr must be a residue class other than 0 and 1 (that it is a NON-residue is the caller's business: share_comparison.check_nonresidue)
template <int NL, int NW> static bool eq_mid_consts(EqMidConsts<NL> &K, const FpParams<NL> &P, const uint64_t *nr_host) {
    uint32_t one[NL], t[NL];
    if (!eq_host_digits<NL, NW>(K.nr, P, nr_host)) return false;
    eq_small<NL>(one, 1);
    if (fp_is_zero<NL>(K.nr) || fp_eq<NL>(K.nr, one)) return false;
    fp_sub<NL>(t, K.nr, one, P);
    to_mont<NL>(K.nm1m, t, P);
    return true;
}
template <int NL, int NW> static bool eq_finish_consts(EqFinishConsts<NL> &K, const FpParams<NL> &P, const uint64_t *p_limbs, int n_limbs, int mode, const uint64_t *nr_host) {
    uint32_t one[NL], zero[NL];
    eq_small<NL>(one, 1);
    eq_small<NL>(zero, 0);
    if (mode == HB_EQ_BIT) {                                              // L = 1: [b];  L = -1: 1 - [b]
        fp_set<NL>(K.a_pos, zero); fp_set<NL>(K.b_pos, P.one);
        fp_set<NL>(K.a_neg, one); fp_neg<NL>(K.b_neg, P.one, P);
        return true;
    }
    EqMidConsts<NL> M;
    if (!eq_mid_consts<NL, NW>(M, P, nr_host)) return false;
    // 1 / 2 = (p + 1) / 2 on the limbs (p < 2^256 is odd: p + 1 may carry out of the top limb, the shift brings the bit back)
    uint64_t h[4] = {0, 0, 0, 0};
    unsigned __int128 acc = 1;
    for (int i = 0; i < n_limbs; i++) { acc += p_limbs[i]; h[i] = (uint64_t)acc; acc >>= 64; }
    const uint64_t top_carry = (uint64_t)acc;
    for (int i = 0; i < n_limbs; i++) h[i] = (h[i] >> 1) | ((i + 1 < n_limbs ? h[i + 1] : top_carry) << 63);
    uint32_t hw[NW], hd[NL], half_m[NL], g[NL], t[NL];
    memcpy(hw, h, NW * 4);
    unpack<NL, NW>(hd, hw);
    to_mont<NL>(half_m, hd, P);
    fp_sub<NL>(t, M.nr, one, P);
    mont_mul<NL>(g, half_m, t, P);                                        // g = (nr - 1) / 2, canonical
    // L = 1: (nr + 1) / 2 - g [b] = (g + 1) - g [b];  L = -1: -(nr - 1) / 2 + g [b] = -g + g [b]
    fp_add<NL>(K.a_pos, g, one, P);
    fp_neg<NL>(K.a_neg, g, P);
    to_mont<NL>(K.b_neg, g, P);
    fp_neg<NL>(K.b_pos, K.b_neg, P);
    return true;
}

static bool eq_rows_ok(int rows) { return rows >= 1 && rows <= 4096; }

// host: the same element functions over `count` elements
template <int NL, int NW>
static int selftest_eq(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *ops, const int64_t *params, void *const *outs, int64_t count) {
    FpParams<NL> P;
    fp_params_from_limbs(P, p_limbs);
    const int64_t rows = params[0], plane = rows * count;
    const int mode = (int)params[1];
    auto W = [](const uint64_t *base, int64_t i) -> const uint32_t (&)[NW] { return *reinterpret_cast<const uint32_t(*)[NW]>(reinterpret_cast<const uint32_t *>(base) + i * NW); };
    auto O = [](void *base, int64_t i) -> uint32_t * { return reinterpret_cast<uint32_t *>(base) + i * NW; };
    const uint32_t none[NW] = {};
    uint32_t r0[NW], r1[NW], r2[NW], r3[NW];
    EqSched S;
    if (!eq_make_sched(S, p_limbs, n_limbs)) return HB_ERR_BAD_ARG;
    if (what == HB_EQ_SELFTEST_LEGENDRE) {
        for (int64_t i = 0; i < count; i++) reinterpret_cast<int8_t *>(outs[0])[i] = (int8_t)eq_legendre_elem<NL, NW>(W(ops[0], i), S, P);
    } else if (what == HB_EQ_SELFTEST_MASK1) {
        for (int64_t j = 0; j < rows; j++)
            for (int64_t i = 0; i < count; i++) {
                const int64_t e = j * count + i;
                if (ops[1]) eq_mask1_elem<NL, NW, true>(r0, r1, r2, r3, W(ops[0], i), W(ops[1], i), W(ops[2], e), W(ops[3], e), W(ops[4], e), W(ops[5], e), W(ops[6], e), W(ops[7], e), P);
                else eq_mask1_elem<NL, NW, false>(r0, r1, r2, r3, W(ops[0], i), none, W(ops[2], e), W(ops[3], e), W(ops[4], e), W(ops[5], e), W(ops[6], e), W(ops[7], e), P);
                memcpy(O(outs[0], e), r0, NW * 4); memcpy(O(outs[0], plane + e), r1, NW * 4);
                memcpy(O(outs[0], 2 * plane + e), r2, NW * 4); memcpy(O(outs[0], 3 * plane + e), r3, NW * 4);
            }
    } else if (what == HB_EQ_SELFTEST_MID) {
        EqMidConsts<NL> K;
        if (!eq_mid_consts<NL, NW>(K, P, ops[10])) return HB_ERR_BAD_ARG;
        for (int64_t e = 0; e < plane; e++) {
            eq_mid_elem<NL, NW>(r0, r1, r2, W(ops[0], e), W(ops[0], plane + e), W(ops[0], 2 * plane + e), W(ops[0], 3 * plane + e), W(ops[1], e), W(ops[2], e), W(ops[3], e),
                                W(ops[4], e), W(ops[5], e), W(ops[6], e), W(ops[7], e), W(ops[8], e), W(ops[9], e), K, P);
            memcpy(O(outs[0], e), r0, NW * 4); memcpy(O(outs[0], plane + e), r1, NW * 4); memcpy(O(outs[1], e), r2, NW * 4);
        }
    } else if (what == HB_EQ_SELFTEST_CSHARE) {
        for (int64_t e = 0; e < plane; e++) {
            eq_cshare_elem<NL, NW>(r0, W(ops[1], e), W(ops[0], e), W(ops[0], plane + e), W(ops[2], e), W(ops[3], e), W(ops[4], e), P);
            memcpy(O(outs[0], e), r0, NW * 4);
        }
    } else {
        EqFinishConsts<NL> K;
        if (!eq_finish_consts<NL, NW>(K, P, p_limbs, n_limbs, mode, ops[2])) return HB_ERR_BAD_ARG;
        int32_t *zr = reinterpret_cast<int32_t *>(outs[1]);
        for (int64_t j = 0; j < rows; j++)
            for (int64_t i = 0; i < count; i++) {
                const int64_t e = j * count + i;
                const int L = eq_finish_elem<NL, NW>(r0, W(ops[0], e), W(ops[1], e), S, K, P);
                memcpy(O(outs[0], e), r0, NW * 4);
                if (L == 0) zr[j] = 1;
            }
    }
    return HB_OK;
}

template <int NL, int NW>
static bool launch_eq_mid(const FpParams<NL> &P, const uint64_t *opened, const uint64_t *pa, const uint64_t *qa, const uint64_t *pqa, const uint64_t *pb, const uint64_t *qb,
                          const uint64_t *pqb, const uint64_t *bits, const uint64_t *pc, const uint64_t *qc, const uint64_t *nr_host, uint64_t *masked2, uint64_t *dr, int rows,
                          int64_t count, unsigned blocks, hipStream_t s) {
    EqMidConsts<NL> K;
    if (!eq_mid_consts<NL, NW>(K, P, nr_host)) return false;
    if (count)
        k_eq_mid<NL, NW><<<dim3(blocks, (unsigned)rows), 256, 0, s>>>(P, u32(opened), u32(pa), u32(qa), u32(pqa), u32(pb), u32(qb), u32(pqb), u32(bits), u32(pc), u32(qc), K,
                                                                      (uint32_t *)masked2, (uint32_t *)dr, rows, count);
    return true;
}

template <int NL, int NW>
static bool launch_eq_finish(const FpParams<NL> &P, const EqSched &S, const uint64_t *p_limbs, int n_limbs, const uint64_t *c, const uint64_t *bits, int mode,
                             const uint64_t *nr_host, uint64_t *factor, int32_t *zero_rows, int rows, int64_t count, unsigned blocks, hipStream_t s) {
    EqFinishConsts<NL> K;
    if (!eq_finish_consts<NL, NW>(K, P, p_limbs, n_limbs, mode, nr_host)) return false;
    if (count) k_eq_finish<NL, NW><<<dim3(blocks, (unsigned)rows), 256, 0, s>>>(P, S, K, u32(c), u32(bits), (uint32_t *)factor, zero_rows, count);
    return true;
}

}  // namespace hb

extern "C" {


int hb_legendre(hb_ctx *ctx, const uint64_t *a_dev, int8_t *out_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0 || (count > 0 && (!a_dev || !out_dev))) return HB_ERR_BAD_ARG;
    if (count == 0) return HB_OK;
    EqSched S;
    if (!eq_make_sched(S, ctx->p_limbs, ctx->n_limbs)) return fail(ctx, HB_ERR_UNSUPPORTED, "hb_legendre: no schedule for this modulus");
    if (overlap(out_dev, count, a_dev, count * 8 * (int64_t)ctx->n_limbs)) return fail(ctx, HB_ERR_BAD_ARG, "hb_legendre: out overlaps a");
    HB_ROW_BLOCKS(ctx, "hb_legendre");
    HB_DISPATCH(ctx, (k_legendre<9, 8><<<(unsigned)blocks, 256, 0, s>>>(ctx->pw, S, u32(a_dev), out_dev, count)),
                (k_legendre<3, 2><<<(unsigned)blocks, 256, 0, s>>>(ctx->pn, S, u32(a_dev), out_dev, count)));
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_eq_mask1(hb_ctx *ctx, const uint64_t *x_dev, const uint64_t *y_dev, const uint64_t *r_dev, const uint64_t *rp_dev, const uint64_t *pa_dev, const uint64_t *qa_dev,
                const uint64_t *pb_dev, const uint64_t *qb_dev, uint64_t *masked_dev, int rows, int64_t count, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0 || (count > 0 && (!x_dev || !r_dev || !rp_dev || !pa_dev || !qa_dev || !pb_dev || !qb_dev || !masked_dev))) return HB_ERR_BAD_ARG;
    if (!eq_rows_ok(rows)) return fail(ctx, HB_ERR_BAD_ARG, "hb_eq_mask1: needs 1 <= rows <= 4096");
    if (count == 0) return HB_OK;
    const int64_t eb = 8 * (int64_t)ctx->n_limbs, pb_ = rows * count * eb;
    const uint64_t *planes[6] = {r_dev, rp_dev, pa_dev, qa_dev, pb_dev, qb_dev};
    for (const uint64_t *in : planes)
        if (overlap(masked_dev, 4 * pb_, in, pb_)) return fail(ctx, HB_ERR_BAD_ARG, "hb_eq_mask1: masked is an array of its own");
    if (overlap(masked_dev, 4 * pb_, x_dev, count * eb) || overlap(masked_dev, 4 * pb_, y_dev, count * eb))
        return fail(ctx, HB_ERR_BAD_ARG, "hb_eq_mask1: masked is an array of its own");
    HB_ROW_BLOCKS(ctx, "hb_eq_mask1");
    const dim3 grid((unsigned)blocks, (unsigned)rows);
#define EQ_MASK1(NL, NW, HAS_Y, P) \
    k_eq_mask1<NL, NW, HAS_Y><<<grid, 256, 0, s>>>(P, u32(x_dev), u32(y_dev), u32(r_dev), u32(rp_dev), u32(pa_dev), u32(qa_dev), u32(pb_dev), u32(qb_dev), (uint32_t *)masked_dev, rows, count)
    if (y_dev) HB_DISPATCH(ctx, (EQ_MASK1(9, 8, true, ctx->pw)), (EQ_MASK1(3, 2, true, ctx->pn)));
    else HB_DISPATCH(ctx, (EQ_MASK1(9, 8, false, ctx->pw)), (EQ_MASK1(3, 2, false, ctx->pn)));
#undef EQ_MASK1
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_eq_mid(hb_ctx *ctx, const uint64_t *opened_dev, const uint64_t *pa_dev, const uint64_t *qa_dev, const uint64_t *pqa_dev, const uint64_t *pb_dev, const uint64_t *qb_dev,
              const uint64_t *pqb_dev, const uint64_t *bits_dev, const uint64_t *pc_dev, const uint64_t *qc_dev, const uint64_t *nr_host, uint64_t *masked2_dev,
              uint64_t *dr_dev, int rows, int64_t count, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0 || !nr_host) return HB_ERR_BAD_ARG;
    const uint64_t *ins[10] = {opened_dev, pa_dev, qa_dev, pqa_dev, pb_dev, qb_dev, pqb_dev, bits_dev, pc_dev, qc_dev};
    if (count > 0) {
        for (const uint64_t *in : ins) if (!in) return HB_ERR_BAD_ARG;
        if (!masked2_dev || !dr_dev) return HB_ERR_BAD_ARG;
    }
    if (!eq_rows_ok(rows)) return fail(ctx, HB_ERR_BAD_ARG, "hb_eq_mid: needs 1 <= rows <= 4096");
    const int64_t eb = 8 * (int64_t)ctx->n_limbs, pb_ = rows * count * eb;
    if (count > 0) {
        for (int k = 0; k < 10; k++) {
            const int64_t ib = k == 0 ? 4 * pb_ : pb_;
            if (overlap(masked2_dev, 2 * pb_, ins[k], ib) || overlap(dr_dev, pb_, ins[k], ib)) return fail(ctx, HB_ERR_BAD_ARG, "hb_eq_mid: the outputs are arrays of their own");
        }
        if (overlap(masked2_dev, 2 * pb_, dr_dev, pb_)) return fail(ctx, HB_ERR_BAD_ARG, "hb_eq_mid: masked2 overlaps dr");
    }
    HB_ROW_BLOCKS(ctx, "hb_eq_mid");
    bool ok;
    HB_DISPATCH(ctx,
        (ok = launch_eq_mid<9, 8>(ctx->pw, opened_dev, pa_dev, qa_dev, pqa_dev, pb_dev, qb_dev, pqb_dev, bits_dev, pc_dev, qc_dev, nr_host, masked2_dev, dr_dev, rows, count, (unsigned)blocks, s)),
        (ok = launch_eq_mid<3, 2>(ctx->pn, opened_dev, pa_dev, qa_dev, pqa_dev, pb_dev, qb_dev, pqb_dev, bits_dev, pc_dev, qc_dev, nr_host, masked2_dev, dr_dev, rows, count, (unsigned)blocks, s)));
    if (!ok) return fail(ctx, HB_ERR_BAD_ARG, "hb_eq_mid: nr must be a residue class other than 0 and 1");
    if (count) HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_eq_cshare(hb_ctx *ctx, const uint64_t *opened2_dev, const uint64_t *dr_dev, const uint64_t *pc_dev, const uint64_t *qc_dev, const uint64_t *pqc_dev, uint64_t *c_dev,
                 int rows, int64_t count, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0 || (count > 0 && (!opened2_dev || !dr_dev || !pc_dev || !qc_dev || !pqc_dev || !c_dev))) return HB_ERR_BAD_ARG;
    if (!eq_rows_ok(rows)) return fail(ctx, HB_ERR_BAD_ARG, "hb_eq_cshare: needs 1 <= rows <= 4096");
    if (count == 0) return HB_OK;
    const int64_t eb = 8 * (int64_t)ctx->n_limbs, pb_ = rows * count * eb;
    if (overlap(c_dev, pb_, opened2_dev, 2 * pb_) || overlap(c_dev, pb_, pc_dev, pb_) || overlap(c_dev, pb_, qc_dev, pb_) || overlap(c_dev, pb_, pqc_dev, pb_) ||
        (c_dev != dr_dev && overlap(c_dev, pb_, dr_dev, pb_)))
        return fail(ctx, HB_ERR_BAD_ARG, "hb_eq_cshare: c may be dr itself and no other input");
    HB_ROW_BLOCKS(ctx, "hb_eq_cshare");
    const dim3 grid((unsigned)blocks, (unsigned)rows);
    HB_DISPATCH(ctx,
        (k_eq_cshare<9, 8><<<grid, 256, 0, s>>>(ctx->pw, u32(opened2_dev), u32(dr_dev), u32(pc_dev), u32(qc_dev), u32(pqc_dev), (uint32_t *)c_dev, rows, count)),
        (k_eq_cshare<3, 2><<<grid, 256, 0, s>>>(ctx->pn, u32(opened2_dev), u32(dr_dev), u32(pc_dev), u32(qc_dev), u32(pqc_dev), (uint32_t *)c_dev, rows, count)));
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_eq_finish(hb_ctx *ctx, const uint64_t *c_dev, const uint64_t *bits_dev, int mode, const uint64_t *nr_host, uint64_t *factor_dev, int32_t *zero_rows_dev, int rows,
                 int64_t count, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0) return HB_ERR_BAD_ARG;
    if (mode != HB_EQ_BIT && mode != HB_EQ_REFERENCE) return fail(ctx, HB_ERR_BAD_ARG, "hb_eq_finish: unknown mode");
    if ((mode == HB_EQ_REFERENCE && !nr_host) || (count > 0 && (!c_dev || !bits_dev || !factor_dev || !zero_rows_dev))) return HB_ERR_BAD_ARG;
    if (!eq_rows_ok(rows)) return fail(ctx, HB_ERR_BAD_ARG, "hb_eq_finish: needs 1 <= rows <= 4096");
    EqSched S;
    if (!eq_make_sched(S, ctx->p_limbs, ctx->n_limbs)) return fail(ctx, HB_ERR_UNSUPPORTED, "hb_eq_finish: no schedule for this modulus");
    const int64_t eb = 8 * (int64_t)ctx->n_limbs, pb_ = rows * count * eb;
    if (count > 0 && (overlap(zero_rows_dev, 4 * (int64_t)rows, c_dev, pb_) || overlap(zero_rows_dev, 4 * (int64_t)rows, bits_dev, pb_) ||
                      overlap(zero_rows_dev, 4 * (int64_t)rows, factor_dev, pb_) || (factor_dev != c_dev && overlap(factor_dev, pb_, c_dev, pb_)) ||
                      (factor_dev != bits_dev && overlap(factor_dev, pb_, bits_dev, pb_))))
        return fail(ctx, HB_ERR_BAD_ARG, "hb_eq_finish: factor may be c or bits themselves; zero_rows is an array of its own");
    HB_ROW_BLOCKS(ctx, "hb_eq_finish");
    bool ok;
    HB_DISPATCH(ctx,
        (ok = launch_eq_finish<9, 8>(ctx->pw, S, ctx->p_limbs, ctx->n_limbs, c_dev, bits_dev, mode, nr_host, factor_dev, zero_rows_dev, rows, count, (unsigned)blocks, s)),
        (ok = launch_eq_finish<3, 2>(ctx->pn, S, ctx->p_limbs, ctx->n_limbs, c_dev, bits_dev, mode, nr_host, factor_dev, zero_rows_dev, rows, count, (unsigned)blocks, s)));
    if (!ok) return fail(ctx, HB_ERR_BAD_ARG, "hb_eq_finish: nr must be a residue class other than 0 and 1");
    if (count) HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_selftest_eq(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *operands, const int64_t *params, void *const *outs, int64_t count) {
    if (!p_limbs || !operands || !params || !outs || count < 0 || (n_limbs != 1 && n_limbs != 4)) return HB_ERR_BAD_ARG;
    const int64_t rows = params[0], mode = params[1];
    int n_ops = 0, n_outs = 1;
    switch (what) {
    case HB_EQ_SELFTEST_LEGENDRE: n_ops = 1; break;
    case HB_EQ_SELFTEST_MASK1: n_ops = 8; break;
    case HB_EQ_SELFTEST_MID: n_ops = 11; n_outs = 2; break;
    case HB_EQ_SELFTEST_CSHARE: n_ops = 5; break;
    case HB_EQ_SELFTEST_FINISH: n_ops = 2; n_outs = 2; if (mode != HB_EQ_BIT && mode != HB_EQ_REFERENCE) return HB_ERR_BAD_ARG; break;
    default: return HB_ERR_BAD_ARG;
    }
    if (what != HB_EQ_SELFTEST_LEGENDRE && !eq_rows_ok((int)(rows < 0 || rows > 4096 ? 0 : rows))) return HB_ERR_BAD_ARG;
    for (int i = 0; i < n_ops; i++)
        if (count > 0 && !operands[i] && !(what == HB_EQ_SELFTEST_MASK1 && i == 1)) return HB_ERR_BAD_ARG;
    if (what == HB_EQ_SELFTEST_MID && !operands[10]) return HB_ERR_BAD_ARG;
    if (what == HB_EQ_SELFTEST_FINISH && ((mode == HB_EQ_REFERENCE && !operands[2]) || !outs[1])) return HB_ERR_BAD_ARG;
    for (int i = 0; i < n_outs; i++) if (count > 0 && !outs[i]) return HB_ERR_BAD_ARG;
    if (n_limbs == 4) return selftest_eq<9, 8>(p_limbs, n_limbs, what, operands, params, outs, count);
    return selftest_eq<3, 2>(p_limbs, n_limbs, what, operands, params, outs, count);
}

}  // extern "C"

// hb_eq.hip -- equality of shared values, the reference's Equality mixin (progs/mixins/share_comparison.py:9-80, the probabilistic
// Legendre-symbol test) for arrays of values -- restated on fp29.hpp, not translated.
//
// For every compared pair and each of `rows` test bits the protocol draws a bit share [b] and two random shares [r], [rp], opens
//     c = diff r + _b rp^2,   _b = nr - (nr - 1) b  in {nr, 1},   nr a public quadratic non-residue,
// and turns L = legendre(c) into a factor that is affine in [b]; the product of the factors is the answer.  The three products cost
// three opens: (diff r, rp rp) together, then _b rp^2, then c itself.  Preprocessing arrives as planes: row j of a plane holds test
// bit j's value of every element, so a wave's loads of a row cover consecutive elements.
//
// The steps are rows under the generic kernel k_rows (hb_rows.hpp):
// EqLegendreRow  out[i] = legendre(a_i) in {-1, 0, 1} as int8: a^((p-1)/2) against one and minus one in Montgomery form.  The exponent
//                is the same for every lane: the host derives ONE sliding-window schedule from p (window 3: the odd powers a, a^3, a^5,
//                a^7 stay in registers) and hands it to the kernel by value, so its steps sit in SGPRs and the chain has no divergence.
//                254 squarings and 64 + 4 products for the BLS12-381 scalar field against 254 + ~127 bit by bit.  A zero skips the chain.
// EqMask1Row     diff = x - y (y may be absent: a test against zero), then the four masked differences of the first two Beaver products
//                of every test bit into ONE array to open, (4, rows, count): diff - pa, r - qa, rp - pb, rp - qb.
// EqMidRow       that array opened: [diff r] and [rp^2] by ew_beaver_elem, _b = nr - (nr - 1) [b] (one product by a public constant),
//                the next array to open (2, rows, count): _b - pc, [rp^2] - qc, and the plane [diff r].
// EqCshareRow    [c] = [diff r] + beaver(opened2, triple c): the third array to open.
// EqFinishRow    c opened: the Legendre chain of EqLegendreRow and the affine map of the mode in the same launch,
//                   HB_EQ_BIT        (1 - L) / 2 + L [b]                              a share of exactly 1 or 0
//                   HB_EQ_REFERENCE  L (nr + L) / 2 - (L (nr - 1) / 2) [b]            the reference's expression (nr = 5 there)
//                and zero_rows[row] = 1 where some c of the row is 0 (plain vector stores; every writer stores the same value).
//
// Operands and results are packed canonical residues.  The per-element bodies are HB_HD functions; a step's row -- which operands it
// loads, which body it calls, where it stores -- is an HB_HD function over a memory policy, so hb_selftest_eq runs on the host the very
// rows, arithmetic and addressing, that k_rows runs on the device.  The int8 symbols and zero_rows are not packed elements: the rows
// store them directly, which is the same statement on the host and on the device.
//
// Launch shape (all steps): 256-thread workgroups, one element a thread in x, the test bit (row) in blockIdx.y.  No LDS, no grid
// stride, one launch a call.  diff is one subtraction and is recomputed by each row's thread from x and y (which stay in L2) rather
// than stored as a plane of its own.  Planes, triples and opened values are read once: the 32-byte width takes the non-temporal
// loads, as EwBeaverRow.
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

// ---------------------------------------------------------------- the steps' rows (host and device, over a memory policy: hb_rows.hpp)
// Row y is test bit y: element e = y * count + i of a plane of rows * count elements.  Every row issues all its loads ahead of its
// first store, so where the header allows an output to be an input a thread reads its element before it writes it.
struct EqLegendreArgs { EqSched S; const uint32_t *a; int8_t *out; };

struct EqLegendreRow {
    template <int NL, int NW, class Mem>
    HB_HD static void run(const EqLegendreArgs &A, int, int64_t i, int64_t, const Mem &mem, const FpParams<NL> &P) {
        uint32_t aw[NW];
        mem.load(aw, A.a, i);
        A.out[i] = (int8_t)eq_legendre_elem<NL, NW>(aw, A.S, P);              // one byte an element: a plain store, no packed element
    }
};

// masked: (4, rows, count), an array of its own
struct EqMask1Args { const uint32_t *x, *y, *r, *rp, *pa, *qa, *pb, *qb; uint32_t *masked; int64_t rows; };

template <bool HAS_Y> struct EqMask1Row {
    template <int NL, int NW, class Mem>
    HB_HD static void run(const EqMask1Args &A, int y, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
        const int64_t e = (int64_t)y * count + i, plane = A.rows * count;
        uint32_t xw[NW], yw[NW], rw[NW], rpw[NW], paw[NW], qaw[NW], pbw[NW], qbw[NW], o0[NW], o1[NW], o2[NW], o3[NW];
        mem.load(xw, A.x, i);
        if constexpr (HAS_Y) mem.load(yw, A.y, i);
        else {
#pragma unroll
            for (int q = 0; q < NW; q++) yw[q] = 0;
        }
        mem.once(rw, A.r, e); mem.once(rpw, A.rp, e);
        mem.once(paw, A.pa, e); mem.once(qaw, A.qa, e); mem.once(pbw, A.pb, e); mem.once(qbw, A.qb, e);
        eq_mask1_elem<NL, NW, HAS_Y>(o0, o1, o2, o3, xw, yw, rw, rpw, paw, qaw, pbw, qbw, P);
        mem.store(A.masked, e, o0);
        mem.store(A.masked, plane + e, o1);
        mem.store(A.masked, 2 * plane + e, o2);
        mem.store(A.masked, 3 * plane + e, o3);
    }
};

// opened: (4, rows, count); masked2: (2, rows, count)
template <int NL> struct EqMidArgs { const uint32_t *opened, *pa, *qa, *pqa, *pb, *qb, *pqb, *bits, *pc, *qc; uint32_t *masked2, *dr; int64_t rows; EqMidConsts<NL> K; };

struct EqMidRow {
    template <int NL, int NW, class Mem>
    HB_HD static void run(const EqMidArgs<NL> &A, int y, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
        const int64_t e = (int64_t)y * count + i, plane = A.rows * count;
        uint32_t o0[NW], o1[NW], o2[NW], o3[NW], paw[NW], qaw[NW], pqaw[NW], pbw[NW], qbw[NW], pqbw[NW], bw[NW], pcw[NW], qcw[NW], m0[NW], m1[NW], drw[NW];
        mem.once(o0, A.opened, e); mem.once(o1, A.opened, plane + e); mem.once(o2, A.opened, 2 * plane + e); mem.once(o3, A.opened, 3 * plane + e);
        mem.once(paw, A.pa, e); mem.once(qaw, A.qa, e); mem.once(pqaw, A.pqa, e);
        mem.once(pbw, A.pb, e); mem.once(qbw, A.qb, e); mem.once(pqbw, A.pqb, e);
        mem.load(bw, A.bits, e); mem.once(pcw, A.pc, e); mem.load(qcw, A.qc, e);
        eq_mid_elem<NL, NW>(m0, m1, drw, o0, o1, o2, o3, paw, qaw, pqaw, pbw, qbw, pqbw, bw, pcw, qcw, A.K, P);
        mem.store(A.masked2, e, m0);
        mem.store(A.masked2, plane + e, m1);
        mem.store(A.dr, e, drw);
    }
};

// opened2: (2, rows, count); c may be dr
struct EqCshareArgs { const uint32_t *opened2, *dr, *pc, *qc, *pqc; uint32_t *c; int64_t rows; };

struct EqCshareRow {
    template <int NL, int NW, class Mem>
    HB_HD static void run(const EqCshareArgs &A, int y, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
        const int64_t e = (int64_t)y * count + i, plane = A.rows * count;
        uint32_t dw[NW], ew[NW], drw[NW], pcw[NW], qcw[NW], pqcw[NW], ow[NW];
        mem.once(dw, A.opened2, e); mem.once(ew, A.opened2, plane + e);
        mem.load(drw, A.dr, e);
        mem.once(pcw, A.pc, e); mem.once(qcw, A.qc, e); mem.once(pqcw, A.pqc, e);
        eq_cshare_elem<NL, NW>(ow, drw, dw, ew, pcw, qcw, pqcw, P);
        mem.store(A.c, e, ow);
    }
};

// factor may be c or bits; zero_rows: one int32 a row
template <int NL> struct EqFinishArgs { EqSched S; const uint32_t *c, *bits; uint32_t *factor; int32_t *zero_rows; EqFinishConsts<NL> K; };

struct EqFinishRow {
    template <int NL, int NW, class Mem>
    HB_HD static void run(const EqFinishArgs<NL> &A, int y, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
        const int64_t e = (int64_t)y * count + i;
        uint32_t cw[NW], bw[NW], ow[NW];
        mem.load(cw, A.c, e);
        mem.load(bw, A.bits, e);
        const int L = eq_finish_elem<NL, NW>(ow, cw, bw, A.S, A.K, P);
        mem.store(A.factor, e, ow);
        if (L == 0) A.zero_rows[y] = 1;                                         // a plain store; every writer stores the same value
    }
};

// ---------------------------------------------------------------- host side
// One step function a step (hb_rows.hpp): its checks, Args fill and row count run under a DeviceRun in the entry point, a HostRun in hb_selftest_eq.
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

// nr must be a residue class other than 0 and 1 (that it is a NON-residue is the caller's business: share_comparison.check_nonresidue)
template <int NL> static bool eq_mid_consts(EqMidConsts<NL> &K, const FpParams<NL> &P, const uint64_t *nr_host) {
    uint32_t one[NL], t[NL];
    if (!host_digits<NL, words_of(NL)>(K.nr, P, nr_host)) return false;
    small_digits<NL>(one, 1);
    if (fp_is_zero<NL>(K.nr) || fp_eq<NL>(K.nr, one)) return false;
    fp_sub<NL>(t, K.nr, one, P);
    to_mont<NL>(K.nm1m, t, P);
    return true;
}
template <int NL> static bool eq_finish_consts(EqFinishConsts<NL> &K, const FpParams<NL> &P, const uint64_t *p_limbs, int n_limbs, int mode, const uint64_t *nr_host) {
    constexpr int NW = words_of(NL);
    uint32_t one[NL], zero[NL];
    small_digits<NL>(one, 1);
    small_digits<NL>(zero, 0);
    if (mode == HB_EQ_BIT) {                                              // L = 1: [b];  L = -1: 1 - [b]
        fp_set<NL>(K.a_pos, zero); fp_set<NL>(K.b_pos, P.one);
        fp_set<NL>(K.a_neg, one); fp_neg<NL>(K.b_neg, P.one, P);
        return true;
    }
    EqMidConsts<NL> M;
    if (!eq_mid_consts(M, P, nr_host)) return false;
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

template <class Run> static int legendre_step(const Run &run, const uint64_t *a, int8_t *out, int64_t count) {
    if (count < 0 || (count > 0 && (!a || !out))) return HB_ERR_BAD_ARG;
    if (count == 0) return HB_OK;
    EqLegendreArgs A = {{}, u32(a), out};
    if (!eq_make_sched(A.S, run.modulus(), run.limbs())) return run.fail(HB_ERR_UNSUPPORTED, "hb_legendre: no schedule for this modulus");
    if (overlap(out, count, a, count * run.elem_bytes())) return run.fail(HB_ERR_BAD_ARG, "hb_legendre: out overlaps a");
    return run.template rows<EqLegendreRow>(A, 1, count);
}

template <class Run> static int eq_mask1_step(const Run &run, const uint64_t *x, const uint64_t *y, const uint64_t *r, const uint64_t *rp, const uint64_t *pa,
                                              const uint64_t *qa, const uint64_t *pb, const uint64_t *qb, uint64_t *masked, int rows, int64_t count) {
    if (count < 0 || (count > 0 && (!x || !r || !rp || !pa || !qa || !pb || !qb || !masked))) return HB_ERR_BAD_ARG;
    if (!eq_rows_ok(rows)) return run.fail(HB_ERR_BAD_ARG, "hb_eq_mask1: needs 1 <= rows <= 4096");
    if (count == 0) return HB_OK;
    const RowSpan outs[1] = {{masked, 4 * rows}},
                 ins[8] = {{x, 1}, {y, 1}, {r, rows}, {rp, rows}, {pa, rows}, {qa, rows}, {pb, rows}, {qb, rows}};
    if (!outputs_apart(outs, 1, ins, 8, run.elem_bytes() * count)) return run.fail(HB_ERR_BAD_ARG, "hb_eq_mask1: masked is an array of its own");
    const EqMask1Args A = {u32(x), u32(y), u32(r), u32(rp), u32(pa), u32(qa), u32(pb), u32(qb), u32(masked), rows};
    if (y) return run.template rows<EqMask1Row<true>>(A, rows, count);
    return run.template rows<EqMask1Row<false>>(A, rows, count);
}

template <class Run> static int eq_mid_step(const Run &run, const uint64_t *opened, const uint64_t *pa, const uint64_t *qa, const uint64_t *pqa, const uint64_t *pb,
                                            const uint64_t *qb, const uint64_t *pqb, const uint64_t *bits, const uint64_t *pc, const uint64_t *qc,
                                            const uint64_t *nr_host, uint64_t *masked2, uint64_t *dr, int rows, int64_t count) {
    if (count < 0 || !nr_host) return HB_ERR_BAD_ARG;
    const uint64_t *planes[9] = {pa, qa, pqa, pb, qb, pqb, bits, pc, qc};
    if (count > 0) {
        for (const uint64_t *in : planes) if (!in) return HB_ERR_BAD_ARG;
        if (!opened || !masked2 || !dr) return HB_ERR_BAD_ARG;
    }
    if (!eq_rows_ok(rows)) return run.fail(HB_ERR_BAD_ARG, "hb_eq_mid: needs 1 <= rows <= 4096");
    const RowSpan outs[2] = {{masked2, 2 * rows}, {dr, rows}};
    RowSpan ins[10] = {{opened, 4 * rows}};
    for (int k = 0; k < 9; k++) ins[1 + k] = {planes[k], rows};
    if (!outputs_apart(outs, 2, ins, 10, run.elem_bytes() * count)) return run.fail(HB_ERR_BAD_ARG, "hb_eq_mid: the outputs are arrays of their own");
    const int rc = run.template rows<EqMidRow, EqMidArgs>([&](auto &A, const auto &P) {
        A.opened = u32(opened); A.pa = u32(pa); A.qa = u32(qa); A.pqa = u32(pqa); A.pb = u32(pb); A.qb = u32(qb); A.pqb = u32(pqb);
        A.bits = u32(bits); A.pc = u32(pc); A.qc = u32(qc); A.masked2 = u32(masked2); A.dr = u32(dr); A.rows = rows;
        return eq_mid_consts(A.K, P, nr_host);
    }, rows, count);
    return rc == HB_ERR_BAD_ARG ? run.fail(rc, "hb_eq_mid: nr must be a residue class other than 0 and 1") : rc;
}

template <class Run> static int eq_cshare_step(const Run &run, const uint64_t *opened2, const uint64_t *dr, const uint64_t *pc, const uint64_t *qc, const uint64_t *pqc,
                                               uint64_t *c, int rows, int64_t count) {
    if (count < 0 || (count > 0 && (!opened2 || !dr || !pc || !qc || !pqc || !c))) return HB_ERR_BAD_ARG;
    if (!eq_rows_ok(rows)) return run.fail(HB_ERR_BAD_ARG, "hb_eq_cshare: needs 1 <= rows <= 4096");
    if (count == 0) return HB_OK;
    // c == dr is the permitted alias: dr is then left out of the inputs c must keep apart from
    const RowSpan outs[1] = {{c, rows}},
                 ins[5] = {{opened2, 2 * rows}, {c == dr ? nullptr : dr, rows}, {pc, rows}, {qc, rows}, {pqc, rows}};
    if (!outputs_apart(outs, 1, ins, 5, run.elem_bytes() * count)) return run.fail(HB_ERR_BAD_ARG, "hb_eq_cshare: c may be dr itself and no other input");
    const EqCshareArgs A = {u32(opened2), u32(dr), u32(pc), u32(qc), u32(pqc), u32(c), rows};
    return run.template rows<EqCshareRow>(A, rows, count);
}

template <class Run> static int eq_finish_step(const Run &run, const uint64_t *c, const uint64_t *bits, int mode, const uint64_t *nr_host, uint64_t *factor,
                                               int32_t *zero_rows, int rows, int64_t count) {
    if (count < 0) return HB_ERR_BAD_ARG;
    if (mode != HB_EQ_BIT && mode != HB_EQ_REFERENCE) return run.fail(HB_ERR_BAD_ARG, "hb_eq_finish: unknown mode");
    if ((mode == HB_EQ_REFERENCE && !nr_host) || (count > 0 && (!c || !bits || !factor || !zero_rows))) return HB_ERR_BAD_ARG;
    if (!eq_rows_ok(rows)) return run.fail(HB_ERR_BAD_ARG, "hb_eq_finish: needs 1 <= rows <= 4096");
    EqSched S;
    if (!eq_make_sched(S, run.modulus(), run.limbs())) return run.fail(HB_ERR_UNSUPPORTED, "hb_eq_finish: no schedule for this modulus");
    // factor == c and factor == bits are the permitted aliases: such an input is left out of those factor must keep apart from;
    // zero_rows is 4 bytes a row, not rows of elements
    const int64_t row_bytes = run.elem_bytes() * count, zb = 4 * (int64_t)rows;
    const RowSpan outs[1] = {{factor, rows}}, ins[2] = {{factor == c ? nullptr : c, rows}, {factor == bits ? nullptr : bits, rows}};
    if (count > 0 && (!outputs_apart(outs, 1, ins, 2, row_bytes) || overlap(zero_rows, zb, c, rows * row_bytes) ||
                      overlap(zero_rows, zb, bits, rows * row_bytes) || overlap(zero_rows, zb, factor, rows * row_bytes)))
        return run.fail(HB_ERR_BAD_ARG, "hb_eq_finish: factor may be c or bits themselves; zero_rows is an array of its own");
    const int rc = run.template rows<EqFinishRow, EqFinishArgs>([&](auto &A, const auto &P) {
        A.S = S; A.c = u32(c); A.bits = u32(bits); A.factor = u32(factor); A.zero_rows = zero_rows;
        return eq_finish_consts(A.K, P, run.modulus(), run.limbs(), mode, nr_host);
    }, rows, count);
    return rc == HB_ERR_BAD_ARG ? run.fail(rc, "hb_eq_finish: nr must be a residue class other than 0 and 1") : rc;
}

}  // namespace hb

extern "C" {

int hb_legendre(hb_ctx *ctx, const uint64_t *a_dev, int8_t *out_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : legendre_step(DeviceRun{ctx, (hipStream_t)stream, "hb_legendre"}, a_dev, out_dev, count);
}

int hb_eq_mask1(hb_ctx *ctx, const uint64_t *x_dev, const uint64_t *y_dev, const uint64_t *r_dev, const uint64_t *rp_dev, const uint64_t *pa_dev, const uint64_t *qa_dev,
                const uint64_t *pb_dev, const uint64_t *qb_dev, uint64_t *masked_dev, int rows, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : eq_mask1_step(DeviceRun{ctx, (hipStream_t)stream, "hb_eq_mask1"}, x_dev, y_dev, r_dev, rp_dev, pa_dev, qa_dev, pb_dev, qb_dev,
                                                 masked_dev, rows, count);
}

int hb_eq_mid(hb_ctx *ctx, const uint64_t *opened_dev, const uint64_t *pa_dev, const uint64_t *qa_dev, const uint64_t *pqa_dev, const uint64_t *pb_dev, const uint64_t *qb_dev,
              const uint64_t *pqb_dev, const uint64_t *bits_dev, const uint64_t *pc_dev, const uint64_t *qc_dev, const uint64_t *nr_host, uint64_t *masked2_dev,
              uint64_t *dr_dev, int rows, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : eq_mid_step(DeviceRun{ctx, (hipStream_t)stream, "hb_eq_mid"}, opened_dev, pa_dev, qa_dev, pqa_dev, pb_dev, qb_dev, pqb_dev, bits_dev,
                                               pc_dev, qc_dev, nr_host, masked2_dev, dr_dev, rows, count);
}

int hb_eq_cshare(hb_ctx *ctx, const uint64_t *opened2_dev, const uint64_t *dr_dev, const uint64_t *pc_dev, const uint64_t *qc_dev, const uint64_t *pqc_dev, uint64_t *c_dev,
                 int rows, int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : eq_cshare_step(DeviceRun{ctx, (hipStream_t)stream, "hb_eq_cshare"}, opened2_dev, dr_dev, pc_dev, qc_dev, pqc_dev, c_dev, rows, count);
}

int hb_eq_finish(hb_ctx *ctx, const uint64_t *c_dev, const uint64_t *bits_dev, int mode, const uint64_t *nr_host, uint64_t *factor_dev, int32_t *zero_rows_dev, int rows,
                 int64_t count, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : eq_finish_step(DeviceRun{ctx, (hipStream_t)stream, "hb_eq_finish"}, c_dev, bits_dev, mode, nr_host, factor_dev, zero_rows_dev, rows,
                                                  count);
}

// params: rows, mode (read by the steps that take them)
int hb_selftest_eq(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *ops, const int64_t *params, void *const *outs, int64_t count) {
    if (!p_limbs || !ops || !params || !outs || (n_limbs != 1 && n_limbs != 4)) return HB_ERR_BAD_ARG;
    if (params[0] != (int)params[0] || params[1] != (int)params[1]) return HB_ERR_BAD_ARG;    // rows, mode: the steps take them as int
    const HostRun run = {p_limbs, n_limbs};
    const int rows = (int)params[0], mode = (int)params[1];
    switch (what) {
    case HB_EQ_SELFTEST_LEGENDRE: return legendre_step(run, ops[0], (int8_t *)outs[0], count);
    case HB_EQ_SELFTEST_MASK1: return eq_mask1_step(run, ops[0], ops[1], ops[2], ops[3], ops[4], ops[5], ops[6], ops[7], (uint64_t *)outs[0], rows, count);
    case HB_EQ_SELFTEST_MID:
        return eq_mid_step(run, ops[0], ops[1], ops[2], ops[3], ops[4], ops[5], ops[6], ops[7], ops[8], ops[9], ops[10], (uint64_t *)outs[0], (uint64_t *)outs[1], rows, count);
    case HB_EQ_SELFTEST_CSHARE: return eq_cshare_step(run, ops[0], ops[1], ops[2], ops[3], ops[4], (uint64_t *)outs[0], rows, count);
    case HB_EQ_SELFTEST_FINISH: return eq_finish_step(run, ops[0], ops[1], mode, ops[2], (uint64_t *)outs[0], (int32_t *)outs[1], rows, count);
    default: return HB_ERR_BAD_ARG;
    }
}

}  // extern "C"

// hb_rf.hip -- root finding over GF(p): from the opened power sums S_1 .. S_k of power mixing to the k messages (the reference's
// apps/asynchromix/solver/solver.py:20 solve() and the FLINT program behind it) -- restated on fp29.hpp, not translated.
//
//   Newton      k_rf_newton   ONE workgroup: 1 / m for m <= k from one batched inversion (runs of integers a thread, as k_pm_fact), then k
//                             dependent steps  m e_m = sum_{i <= m} (-1)^(i-1) e_(m-i) S_i, each a lazily accumulated dot product split over
//                             the threads and a reduction over LDS; e lives in LDS.  Bit-equal to power_mixing.newton_coefficients.
//   Repeated    roots(f) = distinct(f / g) ++ roots(g), g = gcd(f, f') (p > k, so f' != 0): k_rf_gcd (B = A' made while loading), one
//   roots       synchronise for deg g, k_rf_div (exact division by the monic g).  As many rounds as the largest multiplicity.
//   Splitting   level by level over the live nodes (offset, degree) of a segmented array, every node squarefree and monic:
//                 h = (x + a)^((p-1)/2) mod s     a from a counter-based generator on (seed, level, node, draw)
//                 g1 = gcd(s, h - 1), g2 = gcd(s, h + 1), g0 = gcd(s, h)          (k_rf_gcd, grid = 3 x nodes)
//               At a root r of s, h(r) = (r + a)^((p-1)/2) is 1, -1 or 0; modulo an irreducible factor q of degree > 1, h is none of them
//               (h = +-1 would put x + a, hence x, in GF(p); h = 0 would make q = x + a).  So
//                 deg g1 + deg g2 + deg g0 == deg s   <=>   s is a product of distinct linear factors:
//               validity is DECIDED at every node's first draw, by counting degrees -- the case "-a is a root" is g0 = x + a.  An invalid
//               input ends there (n_roots = -1).  A node that does not split draws again (<= 64 draws, then HB_ERR_HIP); a child of
//               degree 1 yields the root -c0.
//   Chain       nodes above HB_RF_SMALL_DEGREE: per node a table R[m] = x^(d+m) mod s, m < d (k_rf_table: d - 1 shift-and-add steps in one
//               workgroup), then per bit of (p-1)/2 two launches:  k_rf_sqr  c = h^2 (2d - 1 coefficients, tiles of 64 outputs paired
//               t / T-1-t so that workgroups are level, the four waves of a workgroup split the sum),  k_rf_red  h = c' mod s as a
//               vector-matrix product  c'[i] + sum_m c'[d+m] R[m][i],  c' = c (x + a) when the bit is set (a shift and an axpy, formed
//               while staging).  nodes at or below it: k_rf_small, one workgroup of 64 threads a node, table, h, c in LDS, the whole chain
//               in one launch.  No workgroup ever waits for another: a dependency between workgroups is a launch boundary.
//   GCD         one workgroup a pair, both remainders in dynamic LDS (2 (d + 1) coefficients: 74 KB at d = 1024), cross-multiplication
//               steps  U <- lc(V) U - lc(U) x^(du-dv) V  as hb_gao.hip: no inversion a step (one costs ~380 products on one lane, a step's
//               useful work is 2 products a coefficient); one inversion at the end makes the result monic.  <= du + dv + 2 steps.
//
// Working form: coefficients are NL Montgomery digits (values below p).  Lazy accumulation (rf_dot) exactly as hb_pm.hip:28-35: GROUP
// products a carry pass, L = 4 GROUP products a REDC (L p <= 2^(29 NL)), one conditional subtraction, one modular addition.
//
// The bodies are HB_HD and written as phases between barriers (Par::each): the kernels run a phase as the threads of a workgroup and a
// __syncthreads(), hb_selftest_rf runs the same phases thread by thread on the host.  A phase never reads what another thread writes in it.
//
// Compiler's report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; scratch = 0 bytes for every kernel): DESIGN.md 3o.
#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "hb_common.hpp"
#include "../../include/hbmpc_hip_debug.h"

using namespace hb;

namespace hb {

constexpr int RF_MAX_K = HB_RF_MAX_K;
constexpr int RF_SMALL = HB_RF_SMALL_DEGREE;
constexpr int RF_MAX_DRAWS = 64;
constexpr int RF_NT = 256;              // threads of a workgroup (Newton, table, GCD, division, the two chain kernels)
constexpr int RF_NT_SMALL = 64;         // ... of k_rf_small: one wave a node, 2 RF_SMALL outputs of a squaring
constexpr int RF_TI = 64;               // outputs of a tile of k_rf_sqr / k_rf_red; RF_NT / RF_TI waves split each sum
constexpr int RF_SPLIT = RF_NT / RF_TI;

static int64_t g_rf_stats[8];           // hb_debug_rf_stats: levels, launches, synchronisations, rounds, us in chains / GCDs / waits, nodes
                                        // (of the last hb_rf_roots, or of the last HB_RF_SELFTEST_ROOTS: levels, rounds and nodes alone)
static int g_rf_profile = 0;

// the threads of a workgroup, phase by phase
struct RfDev {
    int tid, nt;
    template <class F> HB_HD void each(F f) const {
        f(tid, nt);
#ifdef __HIP_DEVICE_COMPILE__
        __syncthreads();
#endif
    }
};
struct RfHost {
    int nt;
    template <class F> void each(F f) const { for (int t = 0; t < nt; t++) f(t, nt); }
};

template <int NL> struct RfNode {      // a live node of a level
    int32_t off, d;                     // s: d + 1 coefficients at `off` of the level's arena, monic
    int32_t hoff, coff;                 // h: d coefficients; c: 2 d coefficients
    int64_t toff;                       // R: d rows of d coefficients
    uint32_t a[NL];                     // the shift, Montgomery digits
};
struct RfJob {                          // a GCD or a division
    int32_t aoff, da;                   // A: da + 1 coefficients
    int32_t boff, db;                   // B: db + 1 coefficients (mode 3: none)
    int32_t mode;                       // 0: B - 1, 1: B + 1, 2: B, 3: B = A' (up to a constant factor)
    int32_t ooff;                       // result at `ooff` of the output arena (room for da + 1)
};
struct RfEmit { int32_t off, pos; };    // monic x + c0 at `off` -> root -c0 at element `pos`

// ---------------------------------------------------------------- bodies (host and device)
template <int NL> HB_HD void rf_ld(uint32_t (&d)[NL], const uint32_t *p) {
#pragma unroll
    for (int q = 0; q < NL; q++) d[q] = p[q];
}
template <int NL> HB_HD void rf_st(uint32_t *p, const uint32_t (&d)[NL]) {
#pragma unroll
    for (int q = 0; q < NL; q++) p[q] = d[q];
}
template <int NL> HB_HD void rf_zero(uint32_t (&d)[NL]) {
#pragma unroll
    for (int q = 0; q < NL; q++) d[q] = 0;
}
template <int NL> HB_HD bool rf_zero_at(const uint32_t *p) {
    uint32_t o = 0;
#pragma unroll
    for (int q = 0; q < NL; q++) o |= p[q];
    return o == 0;
}
// acc += sum_{t < n} a[t sa] b[t sb]   (strides in coefficients, either sign; operands Montgomery and below p, so is the sum)
template <int NL> HB_HD void rf_dot(uint32_t (&acc)[NL], const uint32_t *a, int64_t sa, const uint32_t *b, int64_t sb, int n, const FpParams<NL> &P) {
    constexpr int G = Lazy<NL>::GROUP, L = 4 * G;      // L p <= 2^(29 NL): hb_pm.hip:28-35
    uint64_t c[2 * NL];
    uint32_t r[NL];
    col_zero(c);
    int cnt = 0;
    for (int t = 0; t < n; t++) {
        uint32_t x[NL], y[NL];
        rf_ld<NL>(x, a + (int64_t)t * sa * NL);
        rf_ld<NL>(y, b + (int64_t)t * sb * NL);
        mac<NL>(c, x, y);
        cnt++;
        if (cnt % G == 0) carry(c);
        if (cnt == L) {
            redc(r, c, P);
            cond_sub_p(r, P);
            fp_add(acc, acc, r, P);
            col_zero(c);
            cnt = 0;
        }
    }
    if (cnt) {
        carry(c);
        redc(r, c, P);
        cond_sub_p(r, P);
        fp_add(acc, acc, r, P);
    }
}
// canonical digits of a small integer
template <int NL> HB_HD void rf_int(uint32_t (&d)[NL], uint32_t v) {
    rf_zero<NL>(d);
    d[0] = v & DMASK;
    if (NL > 1) d[1] = v >> LB;
}
// bits of p, and bit b of (p - 1) / 2 = p >> 1
template <int NL> HB_HD int rf_bitlen(const FpParams<NL> &P) {
    int tq = NL - 1;
    while (tq > 0 && P.p[tq] == 0) tq--;
    int tb = 0;
    while ((P.p[tq] >> tb) > 1u) tb++;
    return LB * tq + tb + 1;
}
template <int NL> HB_HD int rf_ebit(const FpParams<NL> &P, int b) { return (P.p[(b + 1) / LB] >> ((b + 1) % LB)) & 1u; }

HB_HD uint64_t rf_mix(uint64_t z) {                     // the finaliser of splitmix64
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// The shift of draw `draw` of node `node` at level `level`: canonical digits.  base(seed, level, node) below 2^(bits of p - 1) <= p, plus
// draw mod p: a node's draws are distinct mod p as long as there are fewer than p of them.
template <int NL> HB_HD void rf_shift(uint32_t (&a)[NL], const FpParams<NL> &P, uint64_t seed, uint32_t level, uint32_t node, uint32_t draw) {
    const uint64_t key = rf_mix(rf_mix(seed) ^ (((uint64_t)level << 32) | node));
    const int top = rf_bitlen<NL>(P) - 1;               // value below 2^top
    uint32_t b[NL], dd[NL];
#pragma unroll
    for (int q = 0; q < NL; q++) {
        const int lo = LB * q;
        uint32_t w = (uint32_t)rf_mix(key + (uint64_t)q) & DMASK;
        if (top <= lo) w = 0;
        else if (top < lo + LB) w &= (1u << (top - lo)) - 1u;
        b[q] = w;
    }
    uint32_t dr = draw;
    if (top < LB) dr = draw % P.p[0];                   // p is one digit: keep the addend below p
    rf_int<NL>(dd, dr);
    fp_add(a, b, dd, P);
}

// ---- Newton's identities: sums (packed) -> coeffs (packed), coefficient of x^i at i.  e: k + 1, part: nt (work memory of the workgroup);
// T, inv: k + 1 each (global).
template <int NL, int NW, class Par>
HB_HD void rf_newton_run(const Par &par, const FpParams<NL> &P, const uint32_t *sums, int k, uint32_t *e, uint32_t *part, uint32_t *T, uint32_t *inv, uint32_t *coeffs) {
    const int chunk = (k + par.nt - 1) / par.nt;
    // 1 / m, m = 1 .. k: thread t owns the integers lo .. hi; (lo-1)! going up, 1 / hi! coming down, one inversion (of k!)
    par.each([&](int t, int nt) {
        const int lo = 1 + t * chunk, hi = lo + chunk - 1 < k ? lo + chunk - 1 : k;
        uint32_t acc[NL], x[NL], xm[NL];
        fp_set(acc, P.one);
        for (int i = lo; i <= hi; i++) { rf_int<NL>(x, (uint32_t)i); to_mont(xm, x, P); mont_mul(acc, acc, xm, P); }
        rf_st<NL>(part + t * NL, acc);
    });
    par.each([&](int t, int nt) {
        const int lo = 1 + t * chunk, hi = lo + chunk - 1 < k ? lo + chunk - 1 : k;
        if (lo > hi) return;
        uint32_t pre[NL], suf[NL], b[NL], x[NL], xm[NL], all[NL], iv[NL];
        fp_set(pre, P.one);
        fp_set(suf, P.one);
        for (int s = 0; s < nt; s++) {
            rf_ld<NL>(b, part + s * NL);
            if (s < t) mont_mul(pre, pre, b, P);
            if (s > t) mont_mul(suf, suf, b, P);
        }
        rf_ld<NL>(b, part + t * NL);
        mont_mul(all, pre, b, P);
        mont_mul(all, all, suf, P);
        fp_inv(iv, all, P);
        mont_mul(suf, suf, iv, P);                       // 1 / hi!
        for (int i = lo; i <= hi; i++) {
            rf_st<NL>(inv + (size_t)i * NL, pre);        // (i - 1)!
            rf_int<NL>(x, (uint32_t)i); to_mont(xm, x, P); mont_mul(pre, pre, xm, P);
        }
        for (int i = hi; i >= lo; i--) {
            rf_ld<NL>(b, inv + (size_t)i * NL);
            mont_mul(b, b, suf, P);                      // (i - 1)! / i!
            rf_st<NL>(inv + (size_t)i * NL, b);
            rf_int<NL>(x, (uint32_t)i); to_mont(xm, x, P); mont_mul(suf, suf, xm, P);
        }
    });
    // T_i = (-1)^(i-1) S_i, Montgomery; e_0 = 1
    par.each([&](int t, int nt) {
        for (int i = 1 + t; i <= k; i += nt) {
            uint32_t s[NL], m[NL];
            load_digits<NL, NW>(s, sums + (size_t)(i - 1) * NW);
            to_mont(m, s, P);
            if (!(i & 1)) fp_neg(m, m, P);
            rf_st<NL>(T + (size_t)i * NL, m);
        }
        if (t == 0) rf_st<NL>(e, P.one);
    });
    for (int m = 1; m <= k; m++) {
        const int ch = (m + par.nt - 1) / par.nt, active = (m + ch - 1) / ch;
        par.each([&](int t, int nt) {
            if (t >= active) return;
            const int i0 = 1 + t * ch, i1 = i0 + ch - 1 < m ? i0 + ch - 1 : m;
            uint32_t acc[NL];
            rf_zero<NL>(acc);
            rf_dot<NL>(acc, e + (size_t)(m - i0) * NL, -1, T + (size_t)i0 * NL, 1, i1 - i0 + 1, P);
            rf_st<NL>(part + t * NL, acc);
        });
        for (int width = active; width > 1;) {
            const int half = (width + 1) / 2;
            par.each([&](int t, int nt) {
                if (t + half >= width) return;
                uint32_t x[NL], y[NL];
                rf_ld<NL>(x, part + t * NL);
                rf_ld<NL>(y, part + (t + half) * NL);
                fp_add(x, x, y, P);
                rf_st<NL>(part + t * NL, x);
            });
            width = half;
        }
        par.each([&](int t, int nt) {
            if (t) return;
            uint32_t x[NL], y[NL];
            rf_ld<NL>(x, part);
            rf_ld<NL>(y, inv + (size_t)m * NL);
            mont_mul(x, x, y, P);
            rf_st<NL>(e + (size_t)m * NL, x);
        });
    }
    // prod (x - a_c) = sum_m (-1)^m e_m x^(k-m)
    par.each([&](int t, int nt) {
        for (int i = t; i <= k; i += nt) {
            uint32_t x[NL], r[NL];
            rf_ld<NL>(x, e + (size_t)(k - i) * NL);
            if ((k - i) & 1) fp_neg(x, x, P);
            from_mont(r, x, P);
            store_digits<NL, NW>(coeffs + (size_t)i * NW, r);
        }
    });
}

// ---- gcd(A, B) by cross-multiplication, A: da + 1 coefficients, B: da + 1 (zero above its degree), both destroyed; lead: 2, meta: 4 ints.
// The monic gcd goes to out, its degree to *deg.
template <int NL, class Par>
HB_HD void rf_gcd_run(const Par &par, const FpParams<NL> &P, uint32_t *A, uint32_t *B, int da, uint32_t *lead, int32_t *meta, uint32_t *out, int32_t *deg) {
    par.each([&](int t, int nt) { if (t == 0) { meta[0] = da; meta[1] = da; meta[2] = 0; meta[3] = 0; } });
    for (int it = 0; it < 2 * da + 4; it++) {
        // thread 0: the degrees, which of the two is the longer, the leading coefficients
        par.each([&](int t, int nt) {
            if (t) return;
            uint32_t *U = meta[2] ? B : A, *V = meta[2] ? A : B;
            int du = meta[0], dv = meta[1];
            while (du >= 0 && rf_zero_at<NL>(U + (size_t)du * NL)) du--;
            while (dv >= 0 && rf_zero_at<NL>(V + (size_t)dv * NL)) dv--;
            if (du < dv) { uint32_t *w = U; U = V; V = w; const int x = du; du = dv; dv = x; meta[2] ^= 1; }
            meta[0] = du; meta[1] = dv; meta[3] = dv < 0;
            if (dv >= 0) {
#pragma unroll
                for (int q = 0; q < NL; q++) { lead[q] = U[(size_t)du * NL + q]; lead[NL + q] = V[(size_t)dv * NL + q]; }
            }
        });
        if (meta[3]) break;
        // U <- lc(V) U - lc(U) x^(du - dv) V: the leading term cancels
        par.each([&](int t, int nt) {
            uint32_t *U = meta[2] ? B : A;
            const uint32_t *V = meta[2] ? A : B;
            const int du = meta[0], sh = meta[0] - meta[1];
            uint32_t lu[NL], lv[NL];
            rf_ld<NL>(lu, lead);
            rf_ld<NL>(lv, lead + NL);
            for (int i = t; i <= du; i += nt) {
                uint32_t x[NL], y[NL];
                rf_ld<NL>(x, U + (size_t)i * NL);
                mont_mul(x, x, lv, P);
                if (i >= sh) {
                    rf_ld<NL>(y, V + (size_t)(i - sh) * NL);
                    mont_mul(y, y, lu, P);
                    fp_sub(x, x, y, P);
                }
                rf_st<NL>(U + (size_t)i * NL, x);
            }
        });
    }
    par.each([&](int t, int nt) {
        if (t) return;
        const uint32_t *U = meta[2] ? B : A;
        uint32_t x[NL], iv[NL];
        rf_ld<NL>(x, U + (size_t)meta[0] * NL);
        fp_inv(iv, x, P);
        rf_st<NL>(lead, iv);
        *deg = meta[0];
    });
    par.each([&](int t, int nt) {
        const uint32_t *U = meta[2] ? B : A;
        uint32_t iv[NL];
        rf_ld<NL>(iv, lead);
        for (int i = t; i <= meta[0]; i += nt) {
            uint32_t x[NL];
            rf_ld<NL>(x, U + (size_t)i * NL);
            mont_mul(x, x, iv, P);
            rf_st<NL>(out + (size_t)i * NL, x);
        }
    });
}
// one job of k_rf_gcd: load A and B (the job's mode), run
template <int NL, class Par>
HB_HD void rf_gcd_block(const Par &par, const FpParams<NL> &P, const RfJob &jb, const uint32_t *src, const uint32_t *bsrc, uint32_t *dst, int32_t *deg, uint32_t *work) {
    uint32_t *A = work, *B = A + (size_t)(jb.da + 1) * NL, *lead = B + (size_t)(jb.da + 1) * NL;
    int32_t *meta = reinterpret_cast<int32_t *>(lead + 2 * NL);
    par.each([&](int t, int nt) {
        for (int i = t; i <= jb.da; i += nt) {
            uint32_t x[NL], y[NL];
            rf_ld<NL>(x, src + (size_t)(jb.aoff + i) * NL);
            rf_st<NL>(A + (size_t)i * NL, x);
            rf_zero<NL>(y);
            if (jb.mode == 3) {
                // (i + 1) A[i + 1] / R: canonical digits of the integer as a Montgomery factor -- the same constant 1 / R on every
                // coefficient, and a gcd does not see a constant factor
                if (i < jb.da) { rf_ld<NL>(x, src + (size_t)(jb.aoff + i + 1) * NL); rf_int<NL>(y, (uint32_t)(i + 1)); mont_mul(y, x, y, P); }
            } else {
                if (i <= jb.db) rf_ld<NL>(y, bsrc + (size_t)(jb.boff + i) * NL);
                if (i == 0 && jb.mode == 0) fp_sub(y, y, P.one, P);
                if (i == 0 && jb.mode == 1) fp_add(y, y, P.one, P);
            }
            rf_st<NL>(B + (size_t)i * NL, y);
        }
    });
    rf_gcd_run<NL>(par, P, A, B, jb.da, lead, meta, dst + (size_t)jb.ooff * NL, deg);
}
// exact division of A (da + 1) by the monic B (db + 1 <= da + 1): the quotient's da - db + 1 coefficients to dst + ooff
template <int NL, class Par>
HB_HD void rf_div_block(const Par &par, const FpParams<NL> &P, const RfJob &jb, const uint32_t *src, const uint32_t *bsrc, uint32_t *dst, uint32_t *work) {
    uint32_t *A = work, *B = A + (size_t)(jb.da + 1) * NL, *lead = B + (size_t)(jb.da + 1) * NL;
    uint32_t *q = dst + (size_t)jb.ooff * NL;
    par.each([&](int t, int nt) {
        for (int i = t; i <= jb.da; i += nt) {
            uint32_t x[NL];
            rf_ld<NL>(x, src + (size_t)(jb.aoff + i) * NL);
            rf_st<NL>(A + (size_t)i * NL, x);
            if (i <= jb.db) { rf_ld<NL>(x, bsrc + (size_t)(jb.boff + i) * NL); rf_st<NL>(B + (size_t)i * NL, x); }
        }
    });
    for (int j = jb.da - jb.db; j >= 0; j--) {
        par.each([&](int t, int nt) {
            if (t) return;
            uint32_t x[NL];
            rf_ld<NL>(x, A + (size_t)(j + jb.db) * NL);
            rf_st<NL>(lead, x);
            rf_st<NL>(q + (size_t)j * NL, x);
        });
        par.each([&](int t, int nt) {
            uint32_t l[NL];
            rf_ld<NL>(l, lead);
            for (int i = t; i < jb.db; i += nt) {
                uint32_t x[NL], y[NL];
                rf_ld<NL>(x, A + (size_t)(j + i) * NL);
                rf_ld<NL>(y, B + (size_t)i * NL);
                mont_mul(y, y, l, P);
                fp_sub(x, x, y, P);
                rf_st<NL>(A + (size_t)(j + i) * NL, x);
            }
        });
    }
}

// ---- the chain.  R[m] = x^(d + m) mod s, m < d; h = x + a
template <int NL, class Par>
HB_HD void rf_table_block(const Par &par, const FpParams<NL> &P, const RfNode<NL> &nd, const uint32_t *arena, uint32_t *R, uint32_t *h) {
    const uint32_t *s = arena + (size_t)nd.off * NL;
    const int d = nd.d;
    par.each([&](int t, int nt) {
        for (int i = t; i < d; i += nt) {
            uint32_t x[NL];
            rf_ld<NL>(x, s + (size_t)i * NL);
            fp_neg(x, x, P);
            rf_st<NL>(R + (size_t)i * NL, x);
            if (i == 0) rf_ld<NL>(x, nd.a); else if (i == 1) fp_set(x, P.one); else rf_zero<NL>(x);
            rf_st<NL>(h + (size_t)i * NL, x);
        }
    });
    for (int m = 0; m + 1 < d; m++) {
        par.each([&](int t, int nt) {
            const uint32_t *row = R + (size_t)m * d * NL;
            uint32_t top[NL];
            rf_ld<NL>(top, row + (size_t)(d - 1) * NL);
            for (int i = t; i < d; i += nt) {
                uint32_t x[NL], y[NL];
                rf_ld<NL>(y, R + (size_t)i * NL);
                mont_mul(y, y, top, P);
                if (i > 0) { rf_ld<NL>(x, row + (size_t)(i - 1) * NL); fp_add(y, y, x, P); }
                rf_st<NL>(R + ((size_t)(m + 1) * d + i) * NL, y);
            }
        });
    }
}
// the part j in [j0, j1) of c[m] = sum_j h[j] h[m - j]
template <int NL> HB_HD void rf_sqr_part(uint32_t (&acc)[NL], const uint32_t *h, int d, int m, int j0, int j1, const FpParams<NL> &P) {
    const int lo = j0 > m - d + 1 ? j0 : m - d + 1, hi = j1 < m + 1 ? (j1 < d ? j1 : d) : (m + 1 < d ? m + 1 : d);
    if (lo < hi) rf_dot<NL>(acc, h + (size_t)lo * NL, 1, h + (size_t)(m - lo) * NL, -1, hi - lo, P);
}
// c'[M] of c' = mul ? c (x + a) : c, c of 2d coefficients (the last one zero)
template <int NL> HB_HD void rf_mulxa(uint32_t (&r)[NL], const uint32_t *c, int M, int mul, const uint32_t (&a)[NL], const FpParams<NL> &P) {
    rf_ld<NL>(r, c + (size_t)M * NL);
    if (!mul) return;
    mont_mul(r, r, a, P);
    if (M > 0) { uint32_t x[NL]; rf_ld<NL>(x, c + (size_t)(M - 1) * NL); fp_add(r, r, x, P); }
}
// a tile pair of k_rf_sqr: bx and T - 1 - bx of the T = ceil(2d / RF_TI) tiles; part: RF_NT coefficients
template <int NL, class Par>
HB_HD void rf_sqr_block(const Par &par, const FpParams<NL> &P, int d, const uint32_t *h, uint32_t *c, int bx, uint32_t *part) {
    const int T = (2 * d + RF_TI - 1) / RF_TI;
    for (int half = 0; half < 2; half++) {
        const int tile = half == 0 ? bx : T - 1 - bx;
        if (half == 1 && tile <= bx) break;
        const int m0 = tile * RF_TI;
        const int jlo = m0 - d + 1 > 0 ? m0 - d + 1 : 0, jhi = m0 + RF_TI < d ? m0 + RF_TI : d;       // [jlo, jhi) covers every output of the tile
        const int len = jhi > jlo ? jhi - jlo : 0, qn = (len + RF_SPLIT - 1) / RF_SPLIT;
        par.each([&](int t, int nt) {
            const int lane = t % RF_TI, w = t / RF_TI, m = m0 + lane;
            uint32_t acc[NL];
            rf_zero<NL>(acc);
            if (m < 2 * d - 1) rf_sqr_part<NL>(acc, h, d, m, jlo + w * qn, jlo + (w + 1) * qn, P);
            rf_st<NL>(part + (size_t)t * NL, acc);
        });
        par.each([&](int t, int nt) {
            if (t >= RF_TI || m0 + t >= 2 * d) return;
            uint32_t acc[NL], x[NL];
            rf_ld<NL>(acc, part + (size_t)t * NL);
            for (int w = 1; w < RF_SPLIT; w++) { rf_ld<NL>(x, part + (size_t)(w * RF_TI + t) * NL); fp_add(acc, acc, x, P); }
            rf_st<NL>(c + (size_t)(m0 + t) * NL, acc);
        });
    }
}
// tile bx of k_rf_red: h[i] = c'[i] + sum_{m < d} c'[d + m] R[m][i], i in the tile; chi: d coefficients, part: RF_NT
template <int NL, class Par>
HB_HD void rf_red_block(const Par &par, const FpParams<NL> &P, const RfNode<NL> &nd, const uint32_t *c, const uint32_t *R, uint32_t *h, int mul, int bx, uint32_t *chi, uint32_t *part) {
    const int d = nd.d, i0 = bx * RF_TI, qn = (d + RF_SPLIT - 1) / RF_SPLIT;
    par.each([&](int t, int nt) {
        for (int m = t; m < d; m += nt) {
            uint32_t x[NL];
            rf_mulxa<NL>(x, c, d + m, mul, nd.a, P);
            rf_st<NL>(chi + (size_t)m * NL, x);
        }
    });
    par.each([&](int t, int nt) {
        const int lane = t % RF_TI, w = t / RF_TI, i = i0 + lane;
        uint32_t acc[NL];
        rf_zero<NL>(acc);
        const int mlo = w * qn, mhi = (w + 1) * qn < d ? (w + 1) * qn : d;
        if (i < d && mlo < mhi) rf_dot<NL>(acc, chi + (size_t)mlo * NL, 1, R + ((size_t)mlo * d + i) * NL, d, mhi - mlo, P);
        rf_st<NL>(part + (size_t)t * NL, acc);
    });
    par.each([&](int t, int nt) {
        if (t >= RF_TI || i0 + t >= d) return;
        uint32_t acc[NL], x[NL];
        rf_mulxa<NL>(acc, c, i0 + t, mul, nd.a, P);
        for (int w = 0; w < RF_SPLIT; w++) { rf_ld<NL>(x, part + (size_t)(w * RF_TI + t) * NL); fp_add(acc, acc, x, P); }
        rf_st<NL>(h + (size_t)(i0 + t) * NL, acc);
    });
}
// one step of a small node (d <= RF_SMALL) by one workgroup: c = h^2, chi, h = c' mod s; h, c, chi: work memory
template <int NL, class Par>
HB_HD void rf_small_step(const Par &par, const FpParams<NL> &P, const RfNode<NL> &nd, const uint32_t *R, uint32_t *h, uint32_t *c, uint32_t *chi, int mul) {
    const int d = nd.d;
    par.each([&](int t, int nt) {
        for (int m = t; m < 2 * d; m += nt) {
            uint32_t acc[NL];
            rf_zero<NL>(acc);
            if (m < 2 * d - 1) rf_sqr_part<NL>(acc, h, d, m, 0, d, P);
            rf_st<NL>(c + (size_t)m * NL, acc);
        }
    });
    par.each([&](int t, int nt) {
        for (int m = t; m < d; m += nt) {
            uint32_t x[NL];
            rf_mulxa<NL>(x, c, d + m, mul, nd.a, P);
            rf_st<NL>(chi + (size_t)m * NL, x);
        }
    });
    par.each([&](int t, int nt) {
        for (int i = t; i < d; i += nt) {
            uint32_t acc[NL];
            rf_mulxa<NL>(acc, c, i, mul, nd.a, P);
            rf_dot<NL>(acc, chi, 1, R + (size_t)i * NL, d, d, P);
            rf_st<NL>(h + (size_t)i * NL, acc);
        }
    });
}
// the whole chain of a small node: table (work memory), h = (x + a)^((p-1)/2) mod s -> hout
template <int NL, class Par>
HB_HD void rf_small_block(const Par &par, const FpParams<NL> &P, const RfNode<NL> &nd, const uint32_t *arena, uint32_t *hout, uint32_t *R, uint32_t *h, uint32_t *c, uint32_t *chi) {
    rf_table_block<NL>(par, P, nd, arena, R, h);
    for (int b = rf_bitlen<NL>(P) - 3; b >= 0; b--) rf_small_step<NL>(par, P, nd, R, h, c, chi, rf_ebit<NL>(P, b));
    par.each([&](int t, int nt) {
        for (int i = t; i < nd.d; i += nt) { uint32_t x[NL]; rf_ld<NL>(x, h + (size_t)i * NL); rf_st<NL>(hout + (size_t)i * NL, x); }
    });
}

// ---------------------------------------------------------------- kernels
template <int NL, int NW>
__global__ void __launch_bounds__(RF_NT) k_rf_newton(const FpParams<NL> P, const uint32_t *__restrict__ sums, int k, uint32_t *T, uint32_t *inv, uint32_t *__restrict__ coeffs) {
    extern __shared__ __attribute__((aligned(16))) uint32_t rf_lds[];
    rf_newton_run<NL, NW>(RfDev{(int)threadIdx.x, RF_NT}, P, sums, k, rf_lds, rf_lds + (size_t)(k + 1) * NL, T, inv, coeffs);
}
// packed canonical coefficients -> Montgomery digits
template <int NL, int NW>
__global__ void __launch_bounds__(256) k_rf_load(const FpParams<NL> P, const uint32_t *__restrict__ coeffs, int n, uint32_t *__restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t x[NL], m[NL];
    load_digits<NL, NW>(x, coeffs + (size_t)i * NW);
    to_mont(m, x, P);
    rf_st<NL>(out + (size_t)i * NL, m);
}
template <int NL>
__global__ void __launch_bounds__(RF_NT) k_rf_gcd(const FpParams<NL> P, const RfJob *__restrict__ jobs, const uint32_t *src, const uint32_t *bsrc, uint32_t *dst, int32_t *degs) {
    extern __shared__ __attribute__((aligned(16))) uint32_t rf_lds[];
    const RfJob jb = jobs[blockIdx.x];
    rf_gcd_block<NL>(RfDev{(int)threadIdx.x, RF_NT}, P, jb, src, bsrc, dst, degs + blockIdx.x, rf_lds);
}
template <int NL>
__global__ void __launch_bounds__(RF_NT) k_rf_div(const FpParams<NL> P, const RfJob *__restrict__ jobs, const uint32_t *src, const uint32_t *bsrc, uint32_t *dst) {
    extern __shared__ __attribute__((aligned(16))) uint32_t rf_lds[];
    const RfJob jb = jobs[blockIdx.x];
    rf_div_block<NL>(RfDev{(int)threadIdx.x, RF_NT}, P, jb, src, bsrc, dst, rf_lds);
}
template <int NL>
__global__ void __launch_bounds__(RF_NT) k_rf_table(const FpParams<NL> P, const RfNode<NL> *__restrict__ nodes, const uint32_t *arena, uint32_t *tab, uint32_t *hbuf) {
    const RfNode<NL> nd = nodes[blockIdx.x];
    rf_table_block<NL>(RfDev{(int)threadIdx.x, RF_NT}, P, nd, arena, tab + (size_t)nd.toff * NL, hbuf + (size_t)nd.hoff * NL);
}
// grid (tile pairs of the largest node, nodes)
template <int NL>
__global__ void __launch_bounds__(RF_NT) k_rf_sqr(const FpParams<NL> P, const RfNode<NL> *__restrict__ nodes, const uint32_t *hbuf, uint32_t *cbuf) {
    __shared__ uint32_t part[RF_NT * NL];
    const int d = nodes[blockIdx.y].d, hoff = nodes[blockIdx.y].hoff, coff = nodes[blockIdx.y].coff;
    const int T = (2 * d + RF_TI - 1) / RF_TI;
    if ((int)blockIdx.x >= (T + 1) / 2) return;
    rf_sqr_block<NL>(RfDev{(int)threadIdx.x, RF_NT}, P, d, hbuf + (size_t)hoff * NL, cbuf + (size_t)coff * NL, (int)blockIdx.x, part);
}
// grid (tiles of the largest node, nodes); dynamic LDS: d coefficients of the largest node
template <int NL>
__global__ void __launch_bounds__(RF_NT) k_rf_red(const FpParams<NL> P, const RfNode<NL> *__restrict__ nodes, const uint32_t *cbuf, const uint32_t *tab, uint32_t *hbuf, int mul) {
    extern __shared__ __attribute__((aligned(16))) uint32_t rf_lds[];
    __shared__ uint32_t part[RF_NT * NL];
    const RfNode<NL> nd = nodes[blockIdx.y];
    if ((int)blockIdx.x * RF_TI >= nd.d) return;
    rf_red_block<NL>(RfDev{(int)threadIdx.x, RF_NT}, P, nd, cbuf + (size_t)nd.coff * NL, tab + (size_t)nd.toff * NL, hbuf + (size_t)nd.hoff * NL, mul, (int)blockIdx.x, rf_lds, part);
}
// one workgroup (one wave) a node of degree <= RF_SMALL: table, h, c, chi in LDS (RF_SMALL^2 + 4 RF_SMALL coefficients)
template <int NL>
__global__ void __launch_bounds__(RF_NT_SMALL) k_rf_small(const FpParams<NL> P, const RfNode<NL> *__restrict__ nodes, const uint32_t *arena, uint32_t *hbuf) {
    __shared__ uint32_t R[RF_SMALL * RF_SMALL * NL];
    __shared__ uint32_t h[RF_SMALL * NL], c[2 * RF_SMALL * NL], chi[RF_SMALL * NL];
    const RfNode<NL> nd = nodes[blockIdx.x];
    rf_small_block<NL>(RfDev{(int)threadIdx.x, RF_NT_SMALL}, P, nd, arena, hbuf + (size_t)nd.hoff * NL, R, h, c, chi);
}
template <int NL, int NW>
__global__ void __launch_bounds__(256) k_rf_emit(const FpParams<NL> P, const RfEmit *__restrict__ list, int n, const uint32_t *__restrict__ arena, uint32_t *__restrict__ roots) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t x[NL], r[NL];
    rf_ld<NL>(x, arena + (size_t)list[i].off * NL);
    fp_neg(x, x, P);
    from_mont(r, x, P);
    store_digits<NL, NW>(roots + (size_t)list[i].pos * NW, r);
}

// ---------------------------------------------------------------- the level loop, on the device (DEV) or over host memory
namespace {

bool rf_k_below_p(const uint64_t *p_limbs, int n_limbs, int k) {
    for (int i = 1; i < n_limbs; i++) if (p_limbs[i]) return true;
    return (uint64_t)k < p_limbs[0];
}
size_t rf_gcd_lds(int da, int nl) { return ((size_t)(2 * (da + 1) + 2) * nl + 4) * 4; }

template <int NL, int NW, bool DEV>
struct RfRun {
    hb_ctx *ctx;                        // DEV only
    hipStream_t s;
    const FpParams<NL> &P;
    int k;
    int cap;                            // coefficients of an arena
    // buffers (device or host memory): F0, F1 (k + 1), arenas A0, A1 (cap), H (k + 2), C (2k + 4), TAB (k^2), nodes, jobs, degs, emits
    uint32_t *F[2], *AR[2], *H, *C, *TAB, *roots;
    RfNode<NL> *nodes;
    RfJob *jobs;
    int32_t *degs;
    RfEmit *emits;
    std::vector<uint8_t> hostmem;
    int64_t launches = 0, syncs = 0, levels = 0, rounds = 0, us_chain = 0, us_gcd = 0, us_sync = 0, n_nodes = 0;
    std::string err;

    RfRun(hb_ctx *c, hipStream_t st, const FpParams<NL> &p, int kk) : ctx(c), s(st), P(p), k(kk), cap(5 * kk + 16) {}

    struct Layout { size_t o_f[2], o_ar[2], o_h, o_c, o_tab, o_nodes, o_jobs, o_degs, o_emits, bytes; };
    Layout layout() const {
        Layout L;
        size_t o = 0;
        auto take = [&](size_t b) { const size_t at = o; o += (b + 255) & ~(size_t)255; return at; };
        const size_t cw = (size_t)NL * 4;
        L.o_f[0] = take((k + 1) * cw); L.o_f[1] = take((k + 1) * cw);
        L.o_ar[0] = take(cap * cw); L.o_ar[1] = take(cap * cw);
        L.o_h = take((k + 2) * cw); L.o_c = take((2 * (size_t)k + 4) * cw);
        L.o_tab = take((size_t)k * k * cw);
        L.o_nodes = take(((size_t)k / 2 + 2) * sizeof(RfNode<NL>));
        L.o_jobs = take((3 * ((size_t)k / 2 + 2)) * sizeof(RfJob));
        L.o_degs = take((3 * ((size_t)k / 2 + 2)) * sizeof(int32_t));
        L.o_emits = take(((size_t)k + 2) * sizeof(RfEmit));
        L.bytes = o;
        return L;
    }
    void bind(uint8_t *base, const Layout &L) {
        F[0] = (uint32_t *)(base + L.o_f[0]); F[1] = (uint32_t *)(base + L.o_f[1]);
        AR[0] = (uint32_t *)(base + L.o_ar[0]); AR[1] = (uint32_t *)(base + L.o_ar[1]);
        H = (uint32_t *)(base + L.o_h); C = (uint32_t *)(base + L.o_c); TAB = (uint32_t *)(base + L.o_tab);
        nodes = (RfNode<NL> *)(base + L.o_nodes); jobs = (RfJob *)(base + L.o_jobs); degs = (int32_t *)(base + L.o_degs); emits = (RfEmit *)(base + L.o_emits);
    }
    int hip_fail(const char *what, hipError_t e) { err = std::string(what) + ": " + hipGetErrorString(e); return HB_ERR_HIP; }
    int64_t now_us() const { return std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    // profile mode (hb_debug_rf_profile): wait after every stage and charge the time to it
    int64_t stage_begin() { if (DEV && g_rf_profile) { (void)hipStreamSynchronize(s); return now_us(); } return 0; }
    void stage_end(int64_t t0, int64_t &acc) { if (DEV && g_rf_profile) { (void)hipStreamSynchronize(s); acc += now_us() - t0; } }

    // descriptors for the device: the host copy stays alive until the stream is next waited for
    std::vector<std::vector<uint8_t>> staged;
    template <class T> int put(T *dst, const std::vector<T> &v) {
        if (v.empty()) return HB_OK;
        if constexpr (DEV) {
            staged.emplace_back((const uint8_t *)v.data(), (const uint8_t *)(v.data() + v.size()));
            const hipError_t e = hipMemcpyAsync(dst, staged.back().data(), staged.back().size(), hipMemcpyHostToDevice, s);
            if (e != hipSuccess) return hip_fail("hipMemcpyAsync", e);
        } else memcpy(dst, v.data(), v.size() * sizeof(T));
        return HB_OK;
    }
    int get_degs(std::vector<int32_t> &v, int n) {
        v.resize(n);
        if constexpr (DEV) {
            const int64_t t0 = now_us();
            hipError_t e = hipMemcpyAsync(v.data(), degs, (size_t)n * 4, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) return hip_fail("reading the degrees", e);
            us_sync += now_us() - t0;
            syncs++;
            staged.clear();
        } else memcpy(v.data(), degs, (size_t)n * 4);
        return HB_OK;
    }
    int launched() {
        if constexpr (DEV) { const hipError_t e = hipGetLastError(); if (e != hipSuccess) return hip_fail("kernel launch", e); }
        return HB_OK;
    }
    int lds_attr(const void *fn, size_t lds) {
        if constexpr (DEV) {
            if (lds > 48 * 1024) { const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); if (e != hipSuccess) return hip_fail("hipFuncSetAttribute", e); }
        }
        return HB_OK;
    }
    // ---- stages
    int st_gcd(const std::vector<RfJob> &jv, const uint32_t *src, const uint32_t *bsrc, uint32_t *dst) {
        int rc = put(jobs, jv); if (rc) return rc;
        int maxda = 0;
        for (auto &j : jv) maxda = std::max(maxda, j.da);
        const size_t lds = rf_gcd_lds(maxda, NL);
        if constexpr (DEV) {
            rc = lds_attr(reinterpret_cast<const void *>(k_rf_gcd<NL>), lds); if (rc) return rc;
            k_rf_gcd<NL><<<(unsigned)jv.size(), RF_NT, lds, s>>>(P, jobs, src, bsrc, dst, degs);
            launches++;
        } else {
            std::vector<uint32_t> work(lds / 4);
            for (size_t b = 0; b < jv.size(); b++) rf_gcd_block<NL>(RfHost{RF_NT}, P, jobs[b], src, bsrc, dst, degs + b, work.data());
        }
        return launched();
    }
    int st_div(const RfJob &jb, const uint32_t *src, const uint32_t *bsrc, uint32_t *dst) {
        int rc = put(jobs, std::vector<RfJob>{jb}); if (rc) return rc;
        const size_t lds = rf_gcd_lds(jb.da, NL);
        if constexpr (DEV) {
            rc = lds_attr(reinterpret_cast<const void *>(k_rf_div<NL>), lds); if (rc) return rc;
            k_rf_div<NL><<<1, RF_NT, lds, s>>>(P, jobs, src, bsrc, dst);
            launches++;
        } else {
            std::vector<uint32_t> work(lds / 4);
            rf_div_block<NL>(RfHost{RF_NT}, P, jobs[0], src, bsrc, dst, work.data());
        }
        return launched();
    }
    // nv: the level's nodes, the n_large ones above RF_SMALL first
    int st_chain(const std::vector<RfNode<NL>> &nv, int n_large, const uint32_t *arena) {
        int rc = put(nodes, nv); if (rc) return rc;
        const int n_small = (int)nv.size() - n_large, nbits = rf_bitlen<NL>(P) - 1;
        int maxd = 0;
        for (int i = 0; i < n_large; i++) maxd = std::max(maxd, nv[i].d);
        if constexpr (DEV) {
            if (n_large) {
                k_rf_table<NL><<<(unsigned)n_large, RF_NT, 0, s>>>(P, nodes, arena, TAB, H);
                launches++;
                const int T = (2 * maxd + RF_TI - 1) / RF_TI;
                const dim3 gs((unsigned)((T + 1) / 2), (unsigned)n_large), gr((unsigned)((maxd + RF_TI - 1) / RF_TI), (unsigned)n_large);
                const size_t lds = (size_t)maxd * NL * 4;
                for (int b = nbits - 2; b >= 0; b--) {
                    k_rf_sqr<NL><<<gs, RF_NT, 0, s>>>(P, nodes, H, C);
                    k_rf_red<NL><<<gr, RF_NT, lds, s>>>(P, nodes, C, TAB, H, rf_ebit<NL>(P, b));
                    launches += 2;
                }
            }
            if (n_small) { k_rf_small<NL><<<(unsigned)n_small, RF_NT_SMALL, 0, s>>>(P, nodes + n_large, arena, H); launches++; }
        } else {
            std::vector<uint32_t> part((size_t)RF_NT * NL), chi((size_t)std::max(maxd, RF_SMALL) * NL), Rs((size_t)RF_SMALL * RF_SMALL * NL), hs((size_t)RF_SMALL * NL), cs((size_t)2 * RF_SMALL * NL);
            for (int n = 0; n < n_large; n++) rf_table_block<NL>(RfHost{RF_NT}, P, nodes[n], arena, TAB + (size_t)nodes[n].toff * NL, H + (size_t)nodes[n].hoff * NL);
            for (int b = nbits - 2; b >= 0 && n_large; b--) {
                for (int n = 0; n < n_large; n++) {
                    const int T = (2 * nodes[n].d + RF_TI - 1) / RF_TI;
                    for (int bx = 0; bx < (T + 1) / 2; bx++) rf_sqr_block<NL>(RfHost{RF_NT}, P, nodes[n].d, H + (size_t)nodes[n].hoff * NL, C + (size_t)nodes[n].coff * NL, bx, part.data());
                }
                for (int n = 0; n < n_large; n++)
                    for (int bx = 0; bx * RF_TI < nodes[n].d; bx++)
                        rf_red_block<NL>(RfHost{RF_NT}, P, nodes[n], C + (size_t)nodes[n].coff * NL, TAB + (size_t)nodes[n].toff * NL, H + (size_t)nodes[n].hoff * NL, rf_ebit<NL>(P, b), bx, chi.data(), part.data());
            }
            for (int n = n_large; n < (int)nv.size(); n++) rf_small_block<NL>(RfHost{RF_NT_SMALL}, P, nodes[n], arena, H + (size_t)nodes[n].hoff * NL, Rs.data(), hs.data(), cs.data(), chi.data());
        }
        return launched();
    }
    int st_emit(const std::vector<RfEmit> &ev, const uint32_t *arena) {
        if (ev.empty()) return HB_OK;
        int rc = put(emits, ev); if (rc) return rc;
        if constexpr (DEV) { k_rf_emit<NL, NW><<<(unsigned)((ev.size() + 255) / 256), 256, 0, s>>>(P, emits, (int)ev.size(), arena, roots); launches++; }
        else
            for (auto &e : ev) {
                uint32_t x[NL], r[NL];
                rf_ld<NL>(x, arena + (size_t)e.off * NL);
                fp_neg(x, x, P);
                from_mont(r, x, P);
                store_digits<NL, NW>(roots + (size_t)e.pos * NW, r);
            }
        return launched();
    }

    struct Live { int off, d, draws; bool fresh; };

    // F[0] holds the monic f (k + 1 Montgomery coefficients).  *n_roots = k and the roots in `roots`, or -1: f is not a product of linear factors
    int run(uint64_t seed, int32_t *n_roots) {
        int rc;
        std::vector<Live> live;
        std::vector<int32_t> dg;
        int cur = 0, n = k, fcur = 0, pos = 0;
        // roots(f) = distinct(f / g) ++ roots(g): the squarefree parts become the first nodes
        int64_t t0 = stage_begin();
        while (n > 0) {
            rounds++;
            rc = st_gcd({RfJob{0, n, 0, 0, 3, 0}}, F[fcur], F[fcur], F[fcur ^ 1]); if (rc) return rc;
            rc = get_degs(dg, 1); if (rc) return rc;
            const int g = dg[0];
            if (g < 0 || g >= n) { err = "hb_rf_roots: gcd(f, f') has an impossible degree"; return HB_ERR_HIP; }
            rc = st_div(RfJob{0, n, 0, g, 2, pos}, F[fcur], F[fcur ^ 1], AR[cur]); if (rc) return rc;
            live.push_back(Live{pos, n - g, 0, true});
            pos += n - g + 1;
            n = g;
            fcur ^= 1;
        }
        stage_end(t0, us_gcd);
        int nr = 0;
        std::vector<RfEmit> ev;
        for (uint32_t level = 0;; level++) {
            // degree 1: a root; the rest is this level's work, nodes above RF_SMALL first
            std::vector<Live> work;
            ev.clear();
            for (auto &l : live) { if (l.d == 1) ev.push_back(RfEmit{l.off, nr++}); else if (l.d > RF_SMALL) work.push_back(l); }
            const int n_large = (int)work.size();
            for (auto &l : live) if (l.d >= 2 && l.d <= RF_SMALL) work.push_back(l);
            if (nr > k) { err = "hb_rf_roots: more roots than the degree"; return HB_ERR_HIP; }
            rc = st_emit(ev, AR[cur]); if (rc) return rc;
            if (work.empty()) break;
            levels++;
            n_nodes += (int64_t)work.size();
            std::vector<RfNode<NL>> nv(work.size());
            std::vector<RfJob> jv(3 * work.size());
            int hoff = 0, coff = 0, ooff = 0;
            int64_t toff = 0;
            for (size_t i = 0; i < work.size(); i++) {
                const Live &l = work[i];
                if (l.draws >= RF_MAX_DRAWS) { err = "hb_rf_roots: a node did not split in 64 draws"; return HB_ERR_HIP; }
                RfNode<NL> &nd = nv[i];
                nd.off = l.off; nd.d = l.d; nd.hoff = hoff; nd.coff = coff; nd.toff = toff;
                uint32_t a[NL];
                rf_shift<NL>(a, P, seed, level, (uint32_t)i, (uint32_t)l.draws);
                to_mont(nd.a, a, P);
                for (int w = 0; w < 3; w++) { jv[3 * i + w] = RfJob{l.off, l.d, hoff, l.d - 1, w, ooff}; ooff += l.d + 1; }
                hoff += l.d; coff += 2 * l.d; toff += (int64_t)l.d * l.d;
            }
            if (ooff > cap || hoff > k || toff > (int64_t)k * k) { err = "hb_rf_roots: a level outgrew its buffers"; return HB_ERR_HIP; }
            t0 = stage_begin();
            rc = st_chain(nv, n_large, AR[cur]); if (rc) return rc;
            stage_end(t0, us_chain);
            t0 = stage_begin();
            rc = st_gcd(jv, AR[cur], H, AR[cur ^ 1]); if (rc) return rc;
            stage_end(t0, us_gcd);
            rc = get_degs(dg, (int)jv.size()); if (rc) return rc;
            live.clear();
            for (size_t i = 0; i < work.size(); i++) {
                const Live &l = work[i];
                const int dd[3] = {dg[3 * i], dg[3 * i + 1], dg[3 * i + 2]};
                if (dd[0] < 0 || dd[1] < 0 || dd[2] < 0 || dd[0] + dd[1] + dd[2] != l.d) {
                    // the degrees of gcd(s, h - 1), gcd(s, h + 1), gcd(s, h) add up to deg s exactly when s splits into distinct linear factors
                    if (l.fresh) { *n_roots = -1; return HB_OK; }
                    err = "hb_rf_roots: the factors of a split node do not add up";
                    return HB_ERR_HIP;
                }
                for (int w = 0; w < 3; w++) {
                    if (dd[w] == 0) continue;
                    const bool same = dd[w] == l.d;
                    live.push_back(Live{jv[3 * i + w].ooff, dd[w], same ? l.draws + 1 : 0, false});
                }
            }
            cur ^= 1;
        }
        if (nr != k) { err = "hb_rf_roots: fewer roots than the degree"; return HB_ERR_HIP; }
        *n_roots = nr;
        return HB_OK;
    }
};

template <int NL, int NW>
int rf_roots_dev(hb_ctx *ctx, const FpParams<NL> &P, const uint32_t *coeffs, int k, uint64_t seed, uint32_t *roots, int32_t *n_roots, hipStream_t s, void *stream) {
    RfRun<NL, NW, true> run(ctx, s, P, k);
    const auto L = run.layout();
    void *base = nullptr;
    const std::string slot = "rf:" + std::to_string((uintptr_t)stream);
    int rc = ctx_scratch(ctx, slot.c_str(), L.bytes, &base); if (rc) return rc;
    run.bind((uint8_t *)base, L);
    run.roots = roots;
    k_rf_load<NL, NW><<<(unsigned)((k + 1 + 255) / 256), 256, 0, s>>>(P, coeffs, k + 1, run.F[0]);
    run.launches++;
    HB_LAUNCH_CHECK(ctx);
    rc = run.run(seed, n_roots);
    const hipError_t e = hipStreamSynchronize(s);
    run.syncs++;
    g_rf_stats[0] = run.levels; g_rf_stats[1] = run.launches; g_rf_stats[2] = run.syncs; g_rf_stats[3] = run.rounds;
    g_rf_stats[4] = run.us_chain; g_rf_stats[5] = run.us_gcd; g_rf_stats[6] = run.us_sync; g_rf_stats[7] = run.n_nodes;
    if (rc) { ctx->err = run.err; return rc; }
    if (e != hipSuccess) { ctx->err = std::string("hb_rf_roots: ") + hipGetErrorString(e); return HB_ERR_HIP; }
    return HB_OK;
}

template <int NL, int NW>
int rf_newton_dev(hb_ctx *ctx, const FpParams<NL> &P, const uint32_t *sums, int k, uint32_t *coeffs, hipStream_t s, void *stream) {
    void *base = nullptr;
    const std::string slot = "rfn:" + std::to_string((uintptr_t)stream);
    const size_t tw = (size_t)(k + 1) * NL;
    int rc = ctx_scratch(ctx, slot.c_str(), 2 * tw * 4, &base); if (rc) return rc;
    const size_t lds = ((size_t)(k + 1) + RF_NT) * NL * 4;
    if (lds > 48 * 1024) HB_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(k_rf_newton<NL, NW>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    k_rf_newton<NL, NW><<<1, RF_NT, lds, s>>>(P, sums, k, (uint32_t *)base, (uint32_t *)base + tw, coeffs);
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

// host: the same bodies over host memory
template <int NL, int NW>
int selftest_rf(const uint64_t *p_limbs, int what, const uint64_t *const *ops, const int64_t *params, uint64_t *out_host) {
    FpParams<NL> P;
    fp_params_from_limbs(P, p_limbs);
    uint32_t *out = reinterpret_cast<uint32_t *>(out_host);
    auto load = [&](const uint64_t *src, int n) {          // packed canonical -> Montgomery digits
        std::vector<uint32_t> v((size_t)std::max(n, 1) * NL);
        for (int i = 0; i < n; i++) {
            uint32_t x[NL], m[NL];
            load_digits<NL, NW>(x, reinterpret_cast<const uint32_t *>(src) + (size_t)i * NW);
            to_mont(m, x, P);
            rf_st<NL>(v.data() + (size_t)i * NL, m);
        }
        return v;
    };
    auto store = [&](uint32_t *dst, const uint32_t *src, int n) {
        for (int i = 0; i < n; i++) {
            uint32_t x[NL], r[NL];
            rf_ld<NL>(x, src + (size_t)i * NL);
            from_mont(r, x, P);
            store_digits<NL, NW>(dst + (size_t)i * NW, r);
        }
    };
    if (what == HB_RF_SELFTEST_NEWTON) {
        const int k = (int)params[0];
        if (k < 1 || !rf_k_below_p(p_limbs, NW / 2, k)) return HB_ERR_BAD_ARG;
        std::vector<uint32_t> e((size_t)(k + 1) * NL), part((size_t)RF_NT * NL), T((size_t)(k + 1) * NL), inv((size_t)(k + 1) * NL);
        rf_newton_run<NL, NW>(RfHost{RF_NT}, P, reinterpret_cast<const uint32_t *>(ops[0]), k, e.data(), part.data(), T.data(), inv.data(), out);
        return HB_OK;
    }
    if (what == HB_RF_SELFTEST_STEP) {
        // ops = s (d + 1, monic), h (d), a (1); params = d, mul: out (d) = h^2 (x + a)^mul mod s, as a node of its size computes it
        const int d = (int)params[0], mul = (int)params[1];
        if (d < 2 || d > RF_MAX_K) return HB_ERR_BAD_ARG;
        std::vector<uint32_t> s = load(ops[0], d + 1), h = load(ops[1], d), a = load(ops[2], 1);
        std::vector<uint32_t> R((size_t)d * d * NL), c((size_t)2 * d * NL), chi((size_t)d * NL), part((size_t)RF_NT * NL), h0((size_t)d * NL);
        RfNode<NL> nd;
        nd.off = 0; nd.d = d; nd.hoff = 0; nd.coff = 0; nd.toff = 0;
        rf_ld<NL>(nd.a, a.data());
        if (d > RF_SMALL) {
            rf_table_block<NL>(RfHost{RF_NT}, P, nd, s.data(), R.data(), h0.data());
            const int T = (2 * d + RF_TI - 1) / RF_TI;
            for (int bx = 0; bx < (T + 1) / 2; bx++) rf_sqr_block<NL>(RfHost{RF_NT}, P, d, h.data(), c.data(), bx, part.data());
            for (int bx = 0; bx * RF_TI < d; bx++) rf_red_block<NL>(RfHost{RF_NT}, P, nd, c.data(), R.data(), h.data(), mul, bx, chi.data(), part.data());
        } else {
            rf_table_block<NL>(RfHost{RF_NT_SMALL}, P, nd, s.data(), R.data(), h0.data());
            rf_small_step<NL>(RfHost{RF_NT_SMALL}, P, nd, R.data(), h.data(), c.data(), chi.data(), mul);
        }
        store(out, h.data(), d);
        return HB_OK;
    }
    if (what == HB_RF_SELFTEST_GCD) {
        // ops = A (da + 1), B (db + 1 <= da + 1); params = da, db: out[0] = the degree, out[1 ..] the monic gcd
        const int da = (int)params[0], db = (int)params[1];
        if (da < 0 || db < 0 || db > da || da > RF_MAX_K) return HB_ERR_BAD_ARG;
        std::vector<uint32_t> A = load(ops[0], da + 1), B = load(ops[1], db + 1), G((size_t)(da + 1) * NL), work(rf_gcd_lds(da, NL) / 4);
        int32_t deg = -1;
        rf_gcd_block<NL>(RfHost{RF_NT}, P, RfJob{0, da, 0, db, 2, 0}, A.data(), B.data(), G.data(), &deg, work.data());
        memset(out, 0, (size_t)(da + 2) * NW * 4);
        out[0] = (uint32_t)deg;
        if (deg >= 0) store(out + NW, G.data(), deg + 1);
        return HB_OK;
    }
    if (what == HB_RF_SELFTEST_SHIFT) {
        uint32_t a[NL];
        rf_shift<NL>(a, P, (uint64_t)params[0], (uint32_t)params[1], (uint32_t)params[2], (uint32_t)params[3]);
        store_digits<NL, NW>(out, a);
        return HB_OK;
    }
    if (what == HB_RF_SELFTEST_ROOTS) {
        // ops = coeffs (k + 1, monic); params = k, seed: out[0] = the number of roots as a 64-bit integer (-1: not a product of linear
        // factors), out[1 ..] the roots in the order found -- the whole level loop over host memory
        const int k = (int)params[0];
        if (k < 1 || k > RF_MAX_K || !rf_k_below_p(p_limbs, NW / 2, k)) return HB_ERR_BAD_ARG;
        RfRun<NL, NW, false> run(nullptr, nullptr, P, k);
        const auto L = run.layout();
        run.hostmem.assign(L.bytes, 0);
        run.bind(run.hostmem.data(), L);
        run.roots = out + NW;
        std::vector<uint32_t> f = load(ops[0], k + 1);
        memcpy(run.F[0], f.data(), f.size() * 4);
        int32_t nr = 0;
        memset(out, 0, (size_t)(k + 1) * NW * 4);
        const int rc = run.run((uint64_t)params[1], &nr);
        // the host walk's counters, for a test that holds them against the device's (no launches, waits or times here)
        memset(g_rf_stats, 0, sizeof(g_rf_stats));
        g_rf_stats[0] = run.levels; g_rf_stats[3] = run.rounds; g_rf_stats[7] = run.n_nodes;
        if (rc) return rc;
        const int64_t v = nr;
        memcpy(out, &v, 8);
        return HB_OK;
    }
    return HB_ERR_BAD_ARG;
}

}  // namespace
}  // namespace hb

extern "C" {

int hb_rf_newton(hb_ctx *ctx, const uint64_t *sums_dev, int k, uint64_t *coeffs_dev, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || k < 1 || !sums_dev || !coeffs_dev) return HB_ERR_BAD_ARG;
    if (!rf_k_below_p(ctx->p_limbs, ctx->n_limbs, k)) return fail(ctx, HB_ERR_BAD_ARG, "hb_rf_newton: k must be below the modulus");
    if (k > RF_MAX_K) return fail(ctx, HB_ERR_UNSUPPORTED, "hb_rf_newton: k above HB_RF_MAX_K");
    cache_trim(ctx);
    if (ctx->n_limbs == 4) return rf_newton_dev<9, 8>(ctx, ctx->pw, (const uint32_t *)sums_dev, k, (uint32_t *)coeffs_dev, (hipStream_t)stream, stream);
    return rf_newton_dev<3, 2>(ctx, ctx->pn, (const uint32_t *)sums_dev, k, (uint32_t *)coeffs_dev, (hipStream_t)stream, stream);
}

int hb_rf_roots(hb_ctx *ctx, const uint64_t *coeffs_dev, int k, uint64_t seed, uint64_t *roots_dev, int32_t *n_roots_host, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || k < 1 || !coeffs_dev || !roots_dev || !n_roots_host) return HB_ERR_BAD_ARG;
    if (!rf_k_below_p(ctx->p_limbs, ctx->n_limbs, k)) return fail(ctx, HB_ERR_BAD_ARG, "hb_rf_roots: k must be below the modulus");
    if (k > RF_MAX_K) return fail(ctx, HB_ERR_UNSUPPORTED, "hb_rf_roots: k above HB_RF_MAX_K");
    cache_trim(ctx);
    *n_roots_host = 0;
    if (ctx->n_limbs == 4) return rf_roots_dev<9, 8>(ctx, ctx->pw, (const uint32_t *)coeffs_dev, k, seed, (uint32_t *)roots_dev, n_roots_host, (hipStream_t)stream, stream);
    return rf_roots_dev<3, 2>(ctx, ctx->pn, (const uint32_t *)coeffs_dev, k, seed, (uint32_t *)roots_dev, n_roots_host, (hipStream_t)stream, stream);
}

int hb_selftest_rf(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *operands, const int64_t *params, uint64_t *out) {
    if (!p_limbs || !params || !out || (n_limbs != 1 && n_limbs != 4)) return HB_ERR_BAD_ARG;
    if (what < HB_RF_SELFTEST_NEWTON || what > HB_RF_SELFTEST_ROOTS) return HB_ERR_BAD_ARG;
    if (what != HB_RF_SELFTEST_SHIFT && (!operands || !operands[0])) return HB_ERR_BAD_ARG;
    if (n_limbs == 4) return selftest_rf<9, 8>(p_limbs, what, operands, params, out);
    return selftest_rf<3, 2>(p_limbs, what, operands, params, out);
}

void hb_debug_rf_stats(int64_t *out) { if (out) memcpy(out, g_rf_stats, sizeof(g_rf_stats)); }
void hb_debug_rf_profile(int on) { g_rf_profile = on ? 1 : 0; }

}  // extern "C"

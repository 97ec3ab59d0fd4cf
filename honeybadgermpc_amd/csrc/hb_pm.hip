// hb_pm.hip -- power mixing: from the opened c = a - b and this party's shares of b, b^2, ..., b^k to its shares of
// a, a^2, ..., a^k and of the power sums S_m = sum over clients of a^m  (reference apps/asynchromix/powermixing.py:12-95 and the
// NTL program it shells out to, apps/asynchromix/cpp/compute-power-sums.cpp computePowers) -- restated on fp29.hpp, not translated.
//
//     [a^m] = sum_{j <= m} C(m, j) c^(m-j) [b^j]      =>      [a^m] / m! = (u * v)[m],   u_j = [b^j] / j!  ([b^0] = 1),   v_i = c^i / i!
//
// a convolution of a share vector with a public one (the reference walks a recurrence of m dependent products per power).
//
// Tables (both paths):
//   k_pm_fact          i! and 1 / i!, i <= k, Montgomery digits, ONE workgroup: each thread multiplies a run of ceil(k / 256) integers, a
//                      prefix (suffix) over the 256 run products in LDS places it, one inversion of k!; kept with the context ("pmf:k")
//   k_pm_scale_shift   u[c][0] = 1, u[c][j] = powers[c][j-1] / j!                        one element a thread
//   k_pm_table         v[c][i] = c_c^i / i!: thread t of a workgroup owns i = i0 + t + 256 r, r < 8: one square-and-multiply to
//                      c^(i0 + t) (<= 2 log2 k products), then steps of c^256 -- no chain along i, stores coalesced
// Direct path:
//   k_pm_direct        out[g][m] = m! sum_{client in group g} sum_{j <= m} u[j] v[m-j], m = 1 .. k.  A workgroup owns a PAIR of m-tiles
//                      (256 outputs each; tile i with tile T-1-i, so every workgroup walks the same number of j: the triangle is
//                      level) and a client group.  Per window of PmAcc::L values of j it stages u[j0 ..] and v[m0-j0-L+1 .. m0-j0+255]
//                      in LDS digit-major (lanes m, m+1, ... read v[m-j] from consecutive dwords: distinct banks; u[j] is a broadcast)
//                      with zeros outside [0, k] -- so no lane branches on j <= m -- and each lane walks the window for its output.
// NTT path (N the power of two above 2k, N | p - 1):
//   the forward transforms of u and v go through hb_fft_batch_evaluate (LDS kernel up to its order, four-step above), a slab of
//   clients at a time;
//   k_pm_mac           part[g][f] = sum_{client in group g} U[c][f] V[c][f], lanes along f, clients split over workgroups
//   k_pm_reduce        dst[f] (+)= sum_g part[g][f]   (both paths: field additions, no float, no atomics)
//   one inverse transform of W (omega^-1), then k_pm_out: S_m = W'[m] m! / N.
//
// Lazy accumulation (k_pm_direct and k_pm_mac).  A 64-bit column takes GROUP = Lazy<NL>::GROUP products of two NL-digit numbers
// (fp29.hpp:8: NL (2^29 - 1)^2 GROUP < 2^64 - 2^58, which also leaves room for the < 2^30 a carried column starts from); a carry
// pass then makes room for the next GROUP.  The VALUE may grow until REDC's precondition T < p R fails: with every operand below p,
// L products give T < L p^2, and REDC returns T / R + (< p) < p (1 + L p / R) -- below 2p, one conditional subtraction, iff
// L p <= R = 2^(29 NL).  p < 2^(32 NW) gives L <= 2^(29 NL - 32 NW): 32 for 32-byte elements, 2^23 for 8-byte ones.  PmAcc::L is
// 4 GROUP = 28 (NL = 9) and 84 (NL = 3); the top column ends below 2^(log2 L + 64 NW - 29 (2 NL - 1)) < 2^25.  Every operand p - 1 at
// that length over 2^256 - 189 is the largest case (tests/test_power_mixing_host.py).  After L products: one REDC, one
// conditional subtraction, one modular addition into the lane's running sum (of values T / R; one product by R^2 at the end).
//
// Working set.  Clients are taken in slabs: u, v (k + 1 elements each a client) and, on the NTT path, U, V (N each) of one slab
// stay below PM_SLAB_BYTES = 256 MiB (hbmpc_hip.h states the whole bound); the buffer lives with the context per stream
// (ctx_scratch "pm:<stream>") and goes with hb_ctx_cache_clear.
//
// Compiler's report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; scratch = 0 bytes for every kernel): DESIGN.md 3i.
#include <algorithm>
#include <string>
#include <vector>

#include "hb_common.hpp"
#include "../../include/hbmpc_hip_debug.h"

using namespace hb;

namespace hb {

template <int NL> struct PmAcc {
    static constexpr int GROUP = Lazy<NL>::GROUP;   // products between two carry passes
    static constexpr int CHUNKS = 4;
    static constexpr int L = GROUP * CHUNKS;        // products between two reductions: L p <= 2^(29 NL) (see above)
};
constexpr int PM_TM = 256;                          // outputs of a tile of k_pm_direct = threads of a workgroup
constexpr int PM_VR = 8;                            // elements a thread of k_pm_table writes
constexpr int PM_FACT_THREADS = 256;
constexpr int PM_MAX_K = 1 << 22;
static size_t g_pm_slab_bytes = (size_t)256 << 20;  // hb_debug_pm_slab_bytes (tests: a slab boundary inside a small M)

// ---------------------------------------------------------------- bodies (host and device)
template <int NL> HB_HD void pm_zero(uint32_t (&d)[NL]) {
#pragma unroll
    for (int q = 0; q < NL; q++) d[q] = 0;
}
// the Montgomery form of a small integer
template <int NL> HB_HD void pm_int_mont(uint32_t (&r)[NL], uint32_t v, const FpParams<NL> &P) {
    uint32_t d[NL];
    pm_zero<NL>(d);
    d[0] = v & DMASK;
    if (NL > 1) d[1] = v >> LB;
    to_mont(r, d, P);
}
// factorial tables, thread t of nt: its run is the integers lo .. hi (empty when lo > hi)
HB_HD void pm_fact_run(int t, int k, int chunk, int &lo, int &hi) {
    lo = 1 + t * chunk;
    hi = lo + chunk - 1 < k ? lo + chunk - 1 : k;
}
// phase 1: blk[t] = product of the run (Montgomery; the empty product is R mod p)
template <int NL> HB_HD void pm_fact_phase1(int t, int k, int chunk, uint32_t *blk, const FpParams<NL> &P) {
    int lo, hi;
    pm_fact_run(t, k, chunk, lo, hi);
    uint32_t acc[NL], x[NL];
    fp_set(acc, P.one);
    for (int i = lo; i <= hi; i++) { pm_int_mont<NL>(x, (uint32_t)i, P); mont_mul(acc, acc, x, P); }
#pragma unroll
    for (int q = 0; q < NL; q++) blk[t * NL + q] = acc[q];
}
// phase 2: fact[i] = (product of the runs before) * lo * ... * i;  ifact[i] = (1 / k!) * (product of the runs after) * hi * ... * (i + 1)
template <int NL> HB_HD void pm_fact_phase2(int t, int nt, int k, int chunk, const uint32_t *blk, uint32_t *fact, uint32_t *ifact, const FpParams<NL> &P) {
    int lo, hi;
    pm_fact_run(t, k, chunk, lo, hi);
    uint32_t pre[NL], suf[NL], x[NL], b[NL];
    fp_set(pre, P.one);
    fp_set(suf, P.one);
    for (int s = 0; s < nt; s++) {
#pragma unroll
        for (int q = 0; q < NL; q++) b[q] = blk[s * NL + q];
        if (s < t) mont_mul(pre, pre, b, P);
        if (s > t) mont_mul(suf, suf, b, P);
    }
    if (t == 0) {
#pragma unroll
        for (int q = 0; q < NL; q++) { fact[q] = P.one[q]; ifact[q] = P.one[q]; }
    }
    if (lo > hi) return;
    // k! = pre * own * suf
#pragma unroll
    for (int q = 0; q < NL; q++) b[q] = blk[t * NL + q];
    uint32_t all[NL], inv[NL];
    mont_mul(all, pre, b, P);
    mont_mul(all, all, suf, P);
    fp_inv(inv, all, P);
    mont_mul(suf, suf, inv, P);                      // 1 / hi!
    for (int i = lo; i <= hi; i++) {
        pm_int_mont<NL>(x, (uint32_t)i, P);
        mont_mul(pre, pre, x, P);
#pragma unroll
        for (int q = 0; q < NL; q++) fact[(size_t)i * NL + q] = pre[q];
    }
    for (int i = hi; i >= lo; i--) {
#pragma unroll
        for (int q = 0; q < NL; q++) ifact[(size_t)i * NL + q] = suf[q];
        pm_int_mont<NL>(x, (uint32_t)i, P);
        mont_mul(suf, suf, x, P);
    }
}
template <int NL> HB_HD void pm_load_tab(uint32_t (&d)[NL], const uint32_t *tab, int64_t i) {
#pragma unroll
    for (int q = 0; q < NL; q++) d[q] = tab[(size_t)i * NL + q];
}
// u[j] of one client: 1 for j = 0, powers[j - 1] / j! above (canonical times a Montgomery-form factor: canonical)
template <int NL, int NW> HB_HD void pm_u_elem(uint32_t *urow, const uint32_t *prow, int j, const uint32_t *ifact, const FpParams<NL> &P) {
    uint32_t x[NL], f[NL], r[NL];
    if (j == 0) {
        pm_zero<NL>(r);
        r[0] = 1;
    } else {
        load_digits<NL, NW>(x, prow + (size_t)(j - 1) * NW);
        pm_load_tab<NL>(f, ifact, j);
        mont_mul(r, x, f, P);
    }
    store_digits<NL, NW>(urow + (size_t)j * NW, r);
}
// v[i] = c^i / i! for i = first, first + step, ... (PM_VR of them, those <= k): x = c^first canonical, advanced by the Montgomery form of c^step
template <int NL, int NW> HB_HD void pm_v_lane(uint32_t *vrow, const uint32_t *cw, int first, int step, int k, const uint32_t *ifact, const FpParams<NL> &P) {
    if (first > k) return;
    uint32_t cd[NL], cm[NL], x[NL], sm[NL], f[NL], r[NL];
    load_digits<NL, NW>(cd, cw);
    to_mont(cm, cd, P);
    fp_pow_u32(r, cm, (uint32_t)first, P);
    from_mont(x, r, P);
    fp_pow_u32(sm, cm, (uint32_t)step, P);
    for (int rr = 0; rr < PM_VR; rr++) {
        const int i = first + rr * step;
        if (i > k) break;
        pm_load_tab<NL>(f, ifact, i);
        mont_mul(r, x, f, P);
        store_digits<NL, NW>(vrow + (size_t)i * NW, r);
        mont_mul(r, x, sm, P);
        fp_set(x, r);
    }
}
// staging of one window of k_pm_direct by thread tid of nt: uw[q][jj] = digit q of u[j0 + jj], vw[q][s] = digit q of
// v[m0 - j0 - (L - 1) + s], s < PM_TM + L - 1; zero outside [0, k]
template <int NL, int NW> HB_HD void pm_stage(uint32_t *uw, uint32_t *vw, const uint32_t *urow, const uint32_t *vrow, int k, int m0, int j0, int tid, int nt) {
    constexpr int L = PmAcc<NL>::L, VS = PM_TM + L - 1;
    for (int idx = tid; idx < L + VS; idx += nt) {
        const bool isu = idx < L;
        const int s = isu ? idx : idx - L;
        const int e = isu ? j0 + s : m0 - j0 - (L - 1) + s;
        uint32_t d[NL];
        if (e >= 0 && e <= k) load_digits<NL, NW>(d, (isu ? urow : vrow) + (size_t)e * NW); else pm_zero<NL>(d);
        uint32_t *dst = isu ? uw + s : vw + s;
        const int stride = isu ? L : VS;
#pragma unroll
        for (int q = 0; q < NL; q++) dst[q * stride] = d[q];
    }
}
// lane t's share of a window: acc += (sum_{jj < L} u[j0 + jj] v[m - j0 - jj]) / R,  m = m0 + t
template <int NL> HB_HD void pm_window(uint32_t (&acc)[NL], const uint32_t *uw, const uint32_t *vw, int t, const FpParams<NL> &P) {
    constexpr int L = PmAcc<NL>::L, G = PmAcc<NL>::GROUP, VS = PM_TM + L - 1;
    uint64_t c[2 * NL];
    col_zero(c);
    for (int ch = 0; ch < PmAcc<NL>::CHUNKS; ch++) {
#pragma unroll
        for (int g = 0; g < G; g++) {
            const int jj = ch * G + g;
            uint32_t a[NL], b[NL];
#pragma unroll
            for (int q = 0; q < NL; q++) { a[q] = uw[q * L + jj]; b[q] = vw[q * VS + t + (L - 1) - jj]; }
            mac<NL>(c, a, b);
        }
        carry(c);
    }
    uint32_t r[NL];
    redc(r, c, P);
    cond_sub_p(r, P);
    fp_add(acc, acc, r, P);
}
// a running sum of values T / R -> the canonical sum times the Montgomery-form factor f (m!)
template <int NL, int NW> HB_HD void pm_finish(uint32_t *out, const uint32_t (&acc)[NL], const uint32_t (&f)[NL], const FpParams<NL> &P) {
    uint32_t s[NL], r[NL];
    mont_mul(s, P.r2, acc, P);
    mont_mul(r, s, f, P);
    store_digits<NL, NW>(out, r);
}
// o = sum_{c in [c_lo, c_hi)} U[c][f] V[c][f]  (rows of n elements), lazily as above
template <int NL, int NW> HB_HD void pm_mac_lane(uint32_t *o, const uint32_t *U, const uint32_t *V, int64_t f, int64_t n, int64_t c_lo, int64_t c_hi, const FpParams<NL> &P) {
    constexpr int L = PmAcc<NL>::L, G = PmAcc<NL>::GROUP;
    uint32_t acc[NL], r[NL];
    uint64_t c[2 * NL];
    pm_zero<NL>(acc);
    col_zero(c);
    int cnt = 0;
    for (int64_t cl = c_lo; cl < c_hi; cl++) {
        uint32_t a[NL], b[NL];
        load_digits<NL, NW>(a, U + (size_t)(cl * n + f) * NW);
        load_digits<NL, NW>(b, V + (size_t)(cl * n + f) * NW);
        mac<NL>(c, a, b);
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
    mont_mul(r, P.r2, acc, P);
    store_digits<NL, NW>(o, r);
}
// dst = (accumulate ? dst : 0) + sum_{g < G} part[g * stride]
template <int NL, int NW> HB_HD void pm_reduce_elem(uint32_t *dst, const uint32_t *part, int64_t stride, int G, int accumulate, const FpParams<NL> &P) {
    uint32_t acc[NL], x[NL];
    if (accumulate) load_digits<NL, NW>(acc, dst); else pm_zero<NL>(acc);
    for (int g = 0; g < G; g++) {
        load_digits<NL, NW>(x, part + (size_t)g * stride * NW);
        fp_add(acc, acc, x, P);
    }
    store_digits<NL, NW>(dst, acc);
}
// S_m = W'[m] m! / N
template <int NL, int NW> HB_HD void pm_out_elem(uint32_t *o, const uint32_t *w, const uint32_t (&f)[NL], const uint32_t (&ninv)[NL], const FpParams<NL> &P) {
    uint32_t x[NL], r[NL];
    load_digits<NL, NW>(x, w);
    mont_mul(r, x, f, P);
    mont_mul(x, r, ninv, P);
    store_digits<NL, NW>(o, x);
}

template <int NL> struct PmDigits { uint32_t d[NL]; };

// ---------------------------------------------------------------- kernels
template <int NL>
__global__ void __launch_bounds__(PM_FACT_THREADS) k_pm_fact(const FpParams<NL> P, int k, int chunk, uint32_t *fact, uint32_t *ifact) {
    __shared__ uint32_t blk[PM_FACT_THREADS * NL];
    pm_fact_phase1<NL>(threadIdx.x, k, chunk, blk, P);
    __syncthreads();
    pm_fact_phase2<NL>(threadIdx.x, PM_FACT_THREADS, k, chunk, blk, fact, ifact, P);
}
template <int NL, int NW>
__global__ void __launch_bounds__(256) k_pm_scale_shift(const FpParams<NL> P, const uint32_t *__restrict__ powers, const uint32_t *__restrict__ ifact, int k, int64_t clients,
                                                        uint32_t *__restrict__ u) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= clients * (k + 1)) return;
    const int64_t c = e / (k + 1);
    const int j = (int)(e - c * (k + 1));
    pm_u_elem<NL, NW>(u + (size_t)c * (k + 1) * NW, powers + (size_t)c * k * NW, j, ifact, P);
}
template <int NL, int NW>
__global__ void __launch_bounds__(256) k_pm_table(const FpParams<NL> P, const uint32_t *__restrict__ cs, const uint32_t *__restrict__ ifact, int k, uint32_t *__restrict__ v) {
    const int64_t c = blockIdx.y;
    const int first = blockIdx.x * (256 * PM_VR) + threadIdx.x;
    pm_v_lane<NL, NW>(v + (size_t)c * (k + 1) * NW, cs + (size_t)c * NW, first, 256, k, ifact, P);
}
// grid (tile pairs, client groups); out row g holds m = 1 .. k at elements 0 .. k - 1
template <int NL, int NW>
__global__ void __launch_bounds__(PM_TM) k_pm_direct(const FpParams<NL> P, const uint32_t *__restrict__ u, const uint32_t *__restrict__ v, const uint32_t *__restrict__ fact,
                                                     int k, int tiles, int64_t clients, int64_t gs, uint32_t *__restrict__ out) {
    constexpr int L = PmAcc<NL>::L, VS = PM_TM + L - 1;
    __shared__ uint32_t uw[NL * L];
    __shared__ uint32_t vw[NL * VS];
    const int t = threadIdx.x;
    const int64_t g = blockIdx.y, c_lo = g * gs, c_hi = min(clients, c_lo + gs);
    for (int half = 0; half < 2; half++) {
        const int tile = half == 0 ? (int)blockIdx.x : tiles - 1 - (int)blockIdx.x;
        if (half == 1 && tile == (int)blockIdx.x) break;
        const int m0 = 1 + tile * PM_TM, m = m0 + t;
        const int jmax = min(m0 + PM_TM - 1, k);
        uint32_t acc[NL];
        pm_zero<NL>(acc);
        for (int64_t c = c_lo; c < c_hi; c++) {
            const uint32_t *urow = u + (size_t)c * (k + 1) * NW, *vrow = v + (size_t)c * (k + 1) * NW;
            for (int j0 = 0; j0 <= jmax; j0 += L) {
                __syncthreads();
                pm_stage<NL, NW>(uw, vw, urow, vrow, k, m0, j0, t, PM_TM);
                __syncthreads();
                pm_window<NL>(acc, uw, vw, t, P);
            }
        }
        if (m <= k) {
            uint32_t f[NL];
            pm_load_tab<NL>(f, fact, m);
            pm_finish<NL, NW>(out + ((size_t)g * k + (m - 1)) * NW, acc, f, P);
        }
    }
}
// grid (ceil(n / 256), client groups)
template <int NL, int NW>
__global__ void __launch_bounds__(256) k_pm_mac(const FpParams<NL> P, const uint32_t *__restrict__ U, const uint32_t *__restrict__ V, int64_t n, int64_t clients, int64_t gs,
                                                uint32_t *__restrict__ part) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= n) return;
    const int64_t g = blockIdx.y, c_lo = g * gs, c_hi = min(clients, c_lo + gs);
    pm_mac_lane<NL, NW>(part + (size_t)(g * n + f) * NW, U, V, f, n, c_lo, c_hi, P);
}
template <int NL, int NW>
__global__ void __launch_bounds__(256) k_pm_reduce(const FpParams<NL> P, const uint32_t *__restrict__ part, int64_t n, int G, int accumulate, uint32_t *dst) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= n) return;
    pm_reduce_elem<NL, NW>(dst + (size_t)f * NW, part + (size_t)f * NW, n, G, accumulate, P);
}
template <int NL, int NW>
__global__ void __launch_bounds__(256) k_pm_out(const FpParams<NL> P, const uint32_t *__restrict__ w, const uint32_t *__restrict__ fact, const PmDigits<NL> ninv, int k,
                                                uint32_t *__restrict__ sums) {
    const int m = 1 + blockIdx.x * 256 + threadIdx.x;
    if (m > k) return;
    uint32_t f[NL];
    pm_load_tab<NL>(f, fact, m);
    pm_out_elem<NL, NW>(sums + (size_t)(m - 1) * NW, w + (size_t)m * NW, f, ninv.d, P);
}

// ---------------------------------------------------------------- host side
namespace {

bool pm_k_below_p(const uint64_t *p_limbs, int n_limbs, int k) {
    for (int i = 1; i < n_limbs; i++) if (p_limbs[i]) return true;
    return (uint64_t)k < p_limbs[0];
}
int pm_order_for(int k) { int n = 1; while (n <= 2 * k) n <<= 1; return n; }       // the power of two above 2k

// i! and 1 / i! (Montgomery digits, i <= k): built once a context and k, an entry of its bounded cache
int pm_fact_tables(hb_ctx *ctx, int k, uint32_t **fact, uint32_t **ifact, hipStream_t s) {
    const std::string key = "pmf:" + std::to_string(k);
    auto it = ctx->dcache.find(key);
    uint32_t *tab = nullptr;
    if (it != ctx->dcache.end()) { tab = (uint32_t *)it->second; cache_touch(ctx, "d|" + key); }
    else {
        const size_t words = (size_t)(k + 1) * ctx->nl();
        HB_HIP(ctx, hipMalloc(&tab, 2 * words * 4));
        const int chunk = (k + PM_FACT_THREADS - 1) / PM_FACT_THREADS;
        HB_DISPATCH(ctx,
            (k_pm_fact<9><<<1, PM_FACT_THREADS, 0, s>>>(ctx->pw, k, chunk, tab, tab + words)),
            (k_pm_fact<3><<<1, PM_FACT_THREADS, 0, s>>>(ctx->pn, k, chunk, tab, tab + words)));
        if (hipGetLastError() != hipSuccess) { (void)hipFree(tab); return fail(ctx, HB_ERR_HIP, "k_pm_fact: launch failed"); }
        // the table may be read by a call on another stream as soon as it is in the cache
        HB_HIP(ctx, hipStreamSynchronize(s));
        ctx->dcache[key] = tab;
        cache_note(ctx, "d|" + key, [ctx, key]() { auto f = ctx->dcache.find(key); if (f != ctx->dcache.end()) { (void)hipFree(f->second); ctx->dcache.erase(f); } });
    }
    *fact = tab;
    *ifact = tab + (size_t)(k + 1) * ctx->nl();
    return HB_OK;
}

struct PmPlan {
    int64_t slab;          // clients a slab
    int64_t groups, gs;    // client groups of a slab's launch and their size
    size_t o_u, o_v, o_U, o_V, o_part, o_w, o_wi, bytes;
};
// slab size and buffer layout; n = 0: direct path (no transforms), part rows of k elements; n > 0: rows of n
PmPlan pm_plan(const hb_ctx *ctx, int64_t M, int k, int n, int wg_x, bool per_client) {
    const size_t eb = (size_t)ctx->n_limbs * 8;
    const size_t per = (2 * (size_t)(k + 1) + 2 * (size_t)n) * eb;
    PmPlan pl;
    pl.slab = (int64_t)std::max<size_t>(1, g_pm_slab_bytes / per);
    pl.slab = std::min<int64_t>(pl.slab, std::min<int64_t>(M, 32768));             // grid.y
    if (per_client) { pl.groups = pl.slab; pl.gs = 1; }
    else {
        // enough workgroups for four a CU whatever the row length
        int64_t want = std::max<int64_t>(1, (1024 + wg_x - 1) / wg_x);
        want = std::min<int64_t>(want, pl.slab);
        pl.gs = (pl.slab + want - 1) / want;
        pl.groups = (pl.slab + pl.gs - 1) / pl.gs;
    }
    const size_t row = (size_t)(n ? n : k) * eb;
    size_t o = 0;
    auto take = [&](size_t b) { const size_t at = o; o += (b + 255) & ~(size_t)255; return at; };
    pl.o_u = take((size_t)pl.slab * (k + 1) * eb);
    pl.o_v = take((size_t)pl.slab * (k + 1) * eb);
    pl.o_U = take((size_t)pl.slab * n * eb);
    pl.o_V = take((size_t)pl.slab * n * eb);
    pl.o_part = per_client ? o : take((size_t)pl.groups * row);
    pl.o_w = take((size_t)n * eb);
    pl.o_wi = take((size_t)n * eb);
    pl.bytes = o;
    return pl;
}

int pm_tables_for_slab(hb_ctx *ctx, const uint32_t *cs, const uint32_t *powers, const uint32_t *ifact, int k, int64_t clients, uint32_t *u, uint32_t *v, hipStream_t s) {
    const int64_t ublocks = (clients * (k + 1) + 255) / 256;
    const unsigned vx = (unsigned)((k + 1 + 256 * PM_VR - 1) / (256 * PM_VR));
    if (ublocks > 0x7fffffffLL) return fail(ctx, HB_ERR_UNSUPPORTED, "hb_pm: slab too large for one launch");
    HB_DISPATCH(ctx,
        (k_pm_scale_shift<9, 8><<<(unsigned)ublocks, 256, 0, s>>>(ctx->pw, powers, ifact, k, clients, u)),
        (k_pm_scale_shift<3, 2><<<(unsigned)ublocks, 256, 0, s>>>(ctx->pn, powers, ifact, k, clients, u)));
    HB_DISPATCH(ctx,
        (k_pm_table<9, 8><<<dim3(vx, (unsigned)clients), 256, 0, s>>>(ctx->pw, cs, ifact, k, v)),
        (k_pm_table<3, 2><<<dim3(vx, (unsigned)clients), 256, 0, s>>>(ctx->pn, cs, ifact, k, v)));
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int pm_scratch(hb_ctx *ctx, void *stream, size_t bytes, uint8_t **base) {
    // per stream: launches of one stream are ordered, and a regrowth frees through hipFree (which waits for the device)
    const std::string slot = "pm:" + std::to_string((uintptr_t)stream);
    void *b = nullptr;
    const int rc = ctx_scratch(ctx, slot.c_str(), bytes, &b);
    *base = (uint8_t *)b;
    return rc;
}

// direct path; per_client: out [M][k] (groups of one client), else out [k] (partials added up)
int pm_direct(hb_ctx *ctx, const uint32_t *cs, const uint32_t *powers, int64_t M, int k, bool per_client, uint32_t *out, hipStream_t s, void *stream) {
    const int NW = ctx->elem_words();
    const int tiles = (k + PM_TM - 1) / PM_TM, pairs = (tiles + 1) / 2;
    uint32_t *fact = nullptr, *ifact = nullptr;
    int rc = pm_fact_tables(ctx, k, &fact, &ifact, s); if (rc) return rc;
    const PmPlan pl = pm_plan(ctx, M, k, 0, pairs, per_client);
    uint8_t *base = nullptr;
    rc = pm_scratch(ctx, stream, pl.bytes, &base); if (rc) return rc;
    uint32_t *u = (uint32_t *)(base + pl.o_u), *v = (uint32_t *)(base + pl.o_v), *part = (uint32_t *)(base + pl.o_part);
    for (int64_t c0 = 0; c0 < M; c0 += pl.slab) {
        const int64_t S = std::min(pl.slab, M - c0);
        rc = pm_tables_for_slab(ctx, cs + (size_t)c0 * NW, powers + (size_t)c0 * k * NW, ifact, k, S, u, v, s); if (rc) return rc;
        const int64_t G = (S + pl.gs - 1) / pl.gs;
        uint32_t *dst = per_client ? out + (size_t)c0 * k * NW : part;
        HB_DISPATCH(ctx,
            (k_pm_direct<9, 8><<<dim3((unsigned)pairs, (unsigned)G), PM_TM, 0, s>>>(ctx->pw, u, v, fact, k, tiles, S, pl.gs, dst)),
            (k_pm_direct<3, 2><<<dim3((unsigned)pairs, (unsigned)G), PM_TM, 0, s>>>(ctx->pn, u, v, fact, k, tiles, S, pl.gs, dst)));
        if (!per_client) {
            HB_DISPATCH(ctx,
                (k_pm_reduce<9, 8><<<(unsigned)((k + 255) / 256), 256, 0, s>>>(ctx->pw, part, k, (int)G, c0 > 0, out)),
                (k_pm_reduce<3, 2><<<(unsigned)((k + 255) / 256), 256, 0, s>>>(ctx->pn, part, k, (int)G, c0 > 0, out)));
        }
        HB_LAUNCH_CHECK(ctx);
    }
    return HB_OK;
}

template <int NL, int NW>
void pm_host_consts(const FpParams<NL> &P, const uint64_t *omega, int n, uint64_t *omega_inv, PmDigits<NL> *ninv) {
    uint32_t ww[NW], d[NL], m[NL], r[NL];
    for (int i = 0; i < NW; i++) ww[i] = (uint32_t)(omega[i / 2] >> (32 * (i & 1)));
    unpack<NL, NW>(d, ww);
    to_mont(m, d, P);
    fp_pow_u32(r, m, (uint32_t)(n - 1), P);           // omega^(n-1) = 1 / omega
    from_mont(d, r, P);
    pack<NL, NW>(ww, d);
    for (int i = 0; i < NW / 2; i++) omega_inv[i] = (uint64_t)ww[2 * i] | ((uint64_t)ww[2 * i + 1] << 32);
    pm_int_mont<NL>(m, (uint32_t)n, P);
    fp_inv(ninv->d, m, P);
}

struct PmHostConsts { uint64_t winv[4]; PmDigits<9> w; PmDigits<3> n; };

int pm_ntt(hb_ctx *ctx, const uint32_t *cs, const uint32_t *powers, int64_t M, int k, const uint64_t *omega, int n, uint32_t *sums, hipStream_t s, void *stream) {
    const int NW = ctx->elem_words();
    uint32_t *fact = nullptr, *ifact = nullptr;
    int rc = pm_fact_tables(ctx, k, &fact, &ifact, s); if (rc) return rc;
    const int fx = (n + 255) / 256;
    const PmPlan pl = pm_plan(ctx, M, k, n, fx, false);
    uint8_t *base = nullptr;
    rc = pm_scratch(ctx, stream, pl.bytes, &base); if (rc) return rc;
    uint32_t *u = (uint32_t *)(base + pl.o_u), *v = (uint32_t *)(base + pl.o_v), *U = (uint32_t *)(base + pl.o_U), *V = (uint32_t *)(base + pl.o_V);
    uint32_t *part = (uint32_t *)(base + pl.o_part), *W = (uint32_t *)(base + pl.o_w), *Wi = (uint32_t *)(base + pl.o_wi);
    // 1 / omega and 1 / N: a host inversion (some hundred microseconds), kept per (modulus, N, omega)
    uint64_t winv[4] = {0, 0, 0, 0};
    PmDigits<9> ninv_w;
    PmDigits<3> ninv_n;
    {
        static std::mutex mu;
        static std::map<std::string, PmHostConsts> cache;
        std::string key((const char *)ctx->p_limbs, sizeof(ctx->p_limbs));
        key.append((const char *)&ctx->n_limbs, sizeof(int)).append((const char *)&n, sizeof(int)).append((const char *)omega, (size_t)ctx->n_limbs * 8);
        std::lock_guard<std::mutex> lock(mu);
        auto it = cache.find(key);
        if (it == cache.end()) {
            PmHostConsts hc;
            memset(&hc, 0, sizeof(hc));
            if (ctx->n_limbs == 4) pm_host_consts<9, 8>(ctx->pw, omega, n, hc.winv, &hc.w); else pm_host_consts<3, 2>(ctx->pn, omega, n, hc.winv, &hc.n);
            if (cache.size() >= 64) cache.clear();
            it = cache.emplace(key, hc).first;
        }
        memcpy(winv, it->second.winv, sizeof(winv));
        ninv_w = it->second.w;
        ninv_n = it->second.n;
    }
    for (int64_t c0 = 0; c0 < M; c0 += pl.slab) {
        const int64_t S = std::min(pl.slab, M - c0);
        rc = pm_tables_for_slab(ctx, cs + (size_t)c0 * NW, powers + (size_t)c0 * k * NW, ifact, k, S, u, v, s); if (rc) return rc;
        rc = hb_fft_batch_evaluate(ctx, omega, n, (const uint64_t *)u, S, k + 1, n, (uint64_t *)U, stream); if (rc) return rc;
        rc = hb_fft_batch_evaluate(ctx, omega, n, (const uint64_t *)v, S, k + 1, n, (uint64_t *)V, stream); if (rc) return rc;
        const int64_t G = (S + pl.gs - 1) / pl.gs;
        HB_DISPATCH(ctx,
            (k_pm_mac<9, 8><<<dim3((unsigned)fx, (unsigned)G), 256, 0, s>>>(ctx->pw, U, V, n, S, pl.gs, part)),
            (k_pm_mac<3, 2><<<dim3((unsigned)fx, (unsigned)G), 256, 0, s>>>(ctx->pn, U, V, n, S, pl.gs, part)));
        HB_DISPATCH(ctx,
            (k_pm_reduce<9, 8><<<(unsigned)fx, 256, 0, s>>>(ctx->pw, part, n, (int)G, c0 > 0, W)),
            (k_pm_reduce<3, 2><<<(unsigned)fx, 256, 0, s>>>(ctx->pn, part, n, (int)G, c0 > 0, W)));
        HB_LAUNCH_CHECK(ctx);
    }
    rc = hb_fft_batch_evaluate(ctx, winv, n, (const uint64_t *)W, 1, n, n, (uint64_t *)Wi, stream); if (rc) return rc;
    HB_DISPATCH(ctx,
        (k_pm_out<9, 8><<<(unsigned)((k + 255) / 256), 256, 0, s>>>(ctx->pw, Wi, fact, ninv_w, k, sums)),
        (k_pm_out<3, 2><<<(unsigned)((k + 255) / 256), 256, 0, s>>>(ctx->pn, Wi, fact, ninv_n, k, sums)));
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

// host: the kernels' bodies, walked as their workgroups and lanes walk them
template <int NL, int NW>
int selftest_pm(const uint64_t *p_limbs, int what, const uint64_t *c_host, const uint64_t *powers_host, int64_t M, int k, int64_t group, uint64_t *out_host) {
    FpParams<NL> P;
    fp_params_from_limbs(P, p_limbs);
    constexpr int L = PmAcc<NL>::L, VS = PM_TM + L - 1;
    const uint32_t *cs = reinterpret_cast<const uint32_t *>(c_host), *pw = reinterpret_cast<const uint32_t *>(powers_host);
    uint32_t *out = reinterpret_cast<uint32_t *>(out_host);
    if (group < 1) group = 1;
    if (what == HB_PM_SELFTEST_MAC) {
        // c_host = U, powers_host = V, rows of k elements: partials of `group` clients, then their sum
        const int64_t G = (M + group - 1) / group;
        std::vector<uint32_t> part((size_t)std::max<int64_t>(G, 1) * k * NW);
        for (int64_t g = 0; g < G; g++)
            for (int64_t f = 0; f < k; f++) pm_mac_lane<NL, NW>(part.data() + (size_t)(g * k + f) * NW, cs, pw, f, k, g * group, std::min(M, (g + 1) * group), P);
        for (int64_t f = 0; f < k; f++) pm_reduce_elem<NL, NW>(out + (size_t)f * NW, part.data() + (size_t)f * NW, k, (int)G, 0, P);
        return HB_OK;
    }
    // HB_PM_SELFTEST_CONV: c_host = u, powers_host = v as given, rows of k + 1 elements, no factorials: the windows alone
    const bool conv = what == HB_PM_SELFTEST_CONV;
    std::vector<uint32_t> fact((size_t)(k + 1) * NL), ifact((size_t)(k + 1) * NL), blk((size_t)PM_FACT_THREADS * NL);
    std::vector<uint32_t> u((size_t)std::max<int64_t>(M, 1) * (k + 1) * NW), v(u.size());
    if (conv) {
        memcpy(u.data(), cs, (size_t)M * (k + 1) * NW * 4);
        memcpy(v.data(), pw, (size_t)M * (k + 1) * NW * 4);
    } else {
        const int chunk = (k + PM_FACT_THREADS - 1) / PM_FACT_THREADS;
        for (int t = 0; t < PM_FACT_THREADS; t++) pm_fact_phase1<NL>(t, k, chunk, blk.data(), P);
        for (int t = 0; t < PM_FACT_THREADS; t++) pm_fact_phase2<NL>(t, PM_FACT_THREADS, k, chunk, blk.data(), fact.data(), ifact.data(), P);
        for (int64_t c = 0; c < M; c++) {
            for (int j = 0; j <= k; j++) pm_u_elem<NL, NW>(u.data() + (size_t)c * (k + 1) * NW, pw + (size_t)c * k * NW, j, ifact.data(), P);
            for (int b = 0; b * (256 * PM_VR) <= k; b++)
                for (int t = 0; t < 256; t++) pm_v_lane<NL, NW>(v.data() + (size_t)c * (k + 1) * NW, cs + (size_t)c * NW, b * (256 * PM_VR) + t, 256, k, ifact.data(), P);
        }
    }
    if (what == HB_PM_SELFTEST_TABLES) {
        memcpy(out, u.data(), (size_t)M * (k + 1) * NW * 4);
        memcpy(out + (size_t)M * (k + 1) * NW, v.data(), (size_t)M * (k + 1) * NW * 4);
        return HB_OK;
    }
    const bool per_client = what == HB_PM_SELFTEST_POWERS;
    if (per_client) group = 1;
    const int64_t G = (M + group - 1) / group;
    const int tiles = (k + PM_TM - 1) / PM_TM;
    std::vector<uint32_t> part((size_t)std::max<int64_t>(G, 1) * k * NW), uw((size_t)NL * L), vw((size_t)NL * VS);
    uint32_t *dst = per_client ? out : part.data();
    for (int64_t g = 0; g < G; g++)
        for (int tile = 0; tile < tiles; tile++) {
            const int m0 = 1 + tile * PM_TM, jmax = std::min(m0 + PM_TM - 1, k);
            std::vector<PmDigits<NL>> acc(PM_TM);
            for (auto &a : acc) pm_zero<NL>(a.d);
            for (int64_t c = g * group; c < std::min(M, (g + 1) * group); c++)
                for (int j0 = 0; j0 <= jmax; j0 += L) {
                    pm_stage<NL, NW>(uw.data(), vw.data(), u.data() + (size_t)c * (k + 1) * NW, v.data() + (size_t)c * (k + 1) * NW, k, m0, j0, 0, 1);
                    for (int t = 0; t < PM_TM && m0 + t <= k; t++) pm_window<NL>(acc[t].d, uw.data(), vw.data(), t, P);
                }
            for (int t = 0; t < PM_TM && m0 + t <= k; t++) {
                uint32_t f[NL];
                if (conv) fp_set(f, P.one); else pm_load_tab<NL>(f, fact.data(), m0 + t);
                pm_finish<NL, NW>(dst + ((size_t)g * k + (m0 + t - 1)) * NW, acc[t].d, f, P);
            }
        }
    if (!per_client) {
        if (M == 0) memset(out, 0, (size_t)k * NW * 4);
        else for (int64_t f = 0; f < k; f++) pm_reduce_elem<NL, NW>(out + (size_t)f * NW, part.data() + (size_t)f * NW, k, (int)G, 0, P);
    }
    return HB_OK;
}

}  // namespace
}  // namespace hb

extern "C" {

int hb_pm_power_sums(hb_ctx *ctx, const uint64_t *c_dev, const uint64_t *powers_dev, int64_t M, int k, int method, const uint64_t *omega_host, int order,
                     uint64_t *sums_dev, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || M < 0 || k <= 0 || !sums_dev || (M > 0 && (!c_dev || !powers_dev))) return HB_ERR_BAD_ARG;
    if (method != HB_PM_AUTO && method != HB_PM_DIRECT && method != HB_PM_NTT) return fail(ctx, HB_ERR_BAD_ARG, "hb_pm_power_sums: unknown method");
    if (!pm_k_below_p(ctx->p_limbs, ctx->n_limbs, k)) return fail(ctx, HB_ERR_BAD_ARG, "hb_pm_power_sums: k must be below the modulus");
    if (k > PM_MAX_K) return fail(ctx, HB_ERR_UNSUPPORTED, "hb_pm_power_sums: k too large");
    const bool omega_ok = omega_host && order == pm_order_for(k) && order <= (1 << 22);
    if (method == HB_PM_NTT && !omega_ok) return fail(ctx, HB_ERR_UNSUPPORTED, "hb_pm_power_sums: the NTT path needs a root of unity of order the power of two above 2k");
    hipStream_t s = (hipStream_t)stream;
    if (M == 0) { HB_HIP(ctx, hipMemsetAsync(sums_dev, 0, (size_t)k * ctx->n_limbs * 8, s)); return HB_OK; }
    cache_trim(ctx);
    // HB_PM_AUTO: above the crossover, and only while the transforms fit the batched LDS kernel (data + twiddles in 160 KiB) -- beyond
    // it hb_fft_batch_evaluate's four-step takes one polynomial at a time, three launches a client, and the direct path wins by far
    const bool batched = ((size_t)order + order / 2) * ctx->nl() * 4 <= 160 * 1024;
    const bool ntt = method == HB_PM_NTT || (method == HB_PM_AUTO && omega_ok && batched && k > HB_PM_CROSSOVER);
    if (ntt) return pm_ntt(ctx, (const uint32_t *)c_dev, (const uint32_t *)powers_dev, M, k, omega_host, order, (uint32_t *)sums_dev, s, stream);
    return pm_direct(ctx, (const uint32_t *)c_dev, (const uint32_t *)powers_dev, M, k, false, (uint32_t *)sums_dev, s, stream);
}

int hb_pm_powers(hb_ctx *ctx, const uint64_t *c_dev, const uint64_t *powers_dev, int64_t M, int k, uint64_t *out_dev, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || M < 0 || k <= 0 || (M > 0 && (!c_dev || !powers_dev || !out_dev))) return HB_ERR_BAD_ARG;
    if (!pm_k_below_p(ctx->p_limbs, ctx->n_limbs, k)) return fail(ctx, HB_ERR_BAD_ARG, "hb_pm_powers: k must be below the modulus");
    if (k > PM_MAX_K) return fail(ctx, HB_ERR_UNSUPPORTED, "hb_pm_powers: k too large");
    if (M == 0) return HB_OK;
    cache_trim(ctx);
    return pm_direct(ctx, (const uint32_t *)c_dev, (const uint32_t *)powers_dev, M, k, true, (uint32_t *)out_dev, (hipStream_t)stream, stream);
}

int hb_selftest_pm(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *c_host, const uint64_t *powers_host, int64_t M, int k, int64_t group,
                   uint64_t *out) {
    if (!p_limbs || M < 0 || k <= 0 || !out || (M > 0 && (!c_host || !powers_host))) return HB_ERR_BAD_ARG;
    if (what < HB_PM_SELFTEST_SUMS || what > HB_PM_SELFTEST_CONV) return HB_ERR_BAD_ARG;
    if (n_limbs != 1 && n_limbs != 4) return HB_ERR_BAD_ARG;
    if (what < HB_PM_SELFTEST_MAC && !pm_k_below_p(p_limbs, n_limbs, k)) return HB_ERR_BAD_ARG;
    if (n_limbs == 4) return selftest_pm<9, 8>(p_limbs, what, c_host, powers_host, M, k, group, out);
    return selftest_pm<3, 2>(p_limbs, what, c_host, powers_host, M, k, group, out);
}

void hb_debug_pm_slab_bytes(int64_t bytes) { g_pm_slab_bytes = bytes > 0 ? (size_t)bytes : (size_t)256 << 20; }

}  // extern "C"

// hb_off.hip -- the local arithmetic of the offline phase (reference honeybadgermpc/offline_randousha.py:34-232: randousha,
// generate_triples, generate_bits) -- restated on fp29.hpp, not translated.  The protocol is honeybadgermpc_amd/offline.py; the three
// places where composing the library's existing entry points is wasteful are kernels here.
//
// OffMulAddRow         out = a b + c: the masked local product of both generators (a b + r_2t for triples, :179; u u + r_2t for bits,
//                      :218).  Three reads and one write an element instead of hb_ew_op(MUL) + hb_ew_op(ADD)'s five and two.
// k_off_invsqrt_scale  the finish of generate_bits (:223, u / sqrt(u^2)): x the opened u^2, w = x^(-1/2) computed directly and
//                      out = u w (HB_OFF_PM1), (u w + 1) / 2 (HB_OFF_01) or w itself (no u).  With p - 1 = q 2^s and c = z^q for the
//                      smallest non-residue z >= 2 (the constant of hb_sqrt.hip), w = x^((q-1)/2) c^e for the unique e in [0, 2^(s-1))
//                      with x^q c^(2e) = 1: ONE exponentiation ((q - 1) / 2, a wave-uniform exponent) and the Tonelli-Shanks
//                      correction applied to the pair (w, t = x w^2): w^2 x = t throughout, so at t = 1 the root hb_sqrt_mod returns
//                      is x w and w is its inverse.  No inversion, no Legendre exponentiation: after the s - 1 bits of e a non-residue
//                      is the element whose t is still not 1 (its x^q has order 2^s, which no even power of c cancels).
//                      The correction is wave-uniform: the bits of e are found lowest first in windows of OFF_WIN = 4 over the table
//                      g_i = c^(2^i), i < s, kept with the context.  With i bits known, T = x^q c^(2 e_low) has order dividing
//                      2^(s-1-i); U = T^(2^(s-1-i-nb)) has order dividing 2^nb, and bit j of the window is [U^(2^(nb-1-j)) != 1],
//                      after which U, T and w take g_(s-nb+j), g_(i+j+1) and g_(i+j) by select.  For s = 32: 105 + 45 squarings and
//                      93 selected products a lane, every lane the same; the lane-divergent loop of hb_sqrt.hip costs a wave the
//                      longest lane of every round (about 560 products at s = 32), a bit-at-a-time uniform loop s^2 / 2 + 2 s.
//                      
// k_off_degree_check   the checkers' verdict (:95-123) over the coefficient-major [n][2k] block one inverse-Vandermonde mat-vec
//                      writes: per column j < k, is the t-sharing of exact degree t, the 2t-sharing of exact degree 2t, and are the
//                      two constant terms equal.  Words are compared, nothing is multiplied.
//
// Operands and results are packed canonical residues.  The per-element bodies are HB_HD functions.  The masked product is a row
// (hb_rows.hpp): k_rows runs it on the device and hb_selftest_off runs the very same row, addressing included, on the host.  The
// other two keep kernels of their own (wave sums: no lane may leave early); those only load, call the bodies and store, and the
// self test runs the same bodies.
//
// Launch shapes (all kernels: 256-thread workgroups, no LDS, no grid stride, one launch a call):
//   k_rows<OffMulAddRow> one element a thread; grid = ceil(count / 256)
//   k_off_invsqrt_scale  one element a thread; grid = ceil(count / 256); no lane leaves early: a lane past `count` works on x = 1 and
//                        stores nothing; the two status counts are summed over the wave and added by one lane
//   k_off_degree_check   one column pair (j, k + j) a thread, walking the n coefficient rows (every load of a wave covers 64
//                        consecutive elements); grid = ceil(k / 256); the three counts are summed over the wave and added by one lane
// Compiler's report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; scratch = 0 bytes for every kernel):
//   k_rows<OffMulAddRow, 9, 8> 62 VGPRs: 8 waves a SIMD       k_rows<OffMulAddRow, 3, 2> 21 VGPRs: 8 waves
//   k_off_invsqrt_scale<9, 8>  98 VGPRs: 4 waves              k_off_invsqrt_scale<3, 2>  31 VGPRs: 8 waves
//   k_off_degree_check<8>      44 VGPRs: 8 waves              k_off_degree_check<2>      20 VGPRs: 8 waves
// (the constants and the table of the inverse root are read through wave-uniform addresses: scalar loads, scalar branches)
#include "hb_common.hpp"
#include "hb_ew_elem.hpp"
#include "hb_rows.hpp"

using namespace hb;

namespace hb {

constexpr int OFF_WIN = 4;

// what the inverse root needs beside the modulus: (q - 1) / 2 and its bit length, s, (p + 1) / 2 as a Montgomery factor
struct OffConsts {
    uint64_t e[4];
    int ebits;
    int s;
    uint32_t half_m[9];
};

// ---------------------------------------------------------------- per-element bodies (host and device)
// The masked product o = a b + c is ew_mul_add_elem of hb_ew_elem.hpp (hb_offpow.hip multiplies its powers with the same body).

HB_HD uint32_t off_exp_bit(const OffConsts &K, int b) {
    const uint64_t w = b < 64 ? K.e[0] : (b < 128 ? K.e[1] : (b < 192 ? K.e[2] : K.e[3]));
    return (uint32_t)(w >> (b & 63)) & 1u;
}
template <int NL> HB_HD void off_tab_load(uint32_t (&g)[NL], const uint32_t *tab, int i) {
#pragma unroll
    for (int q = 0; q < NL; q++) g[q] = tab[i * NL + q];
}
// r = take ? r g : r (the product is formed either way: every lane of a wave does the same work)
template <int NL> HB_HD void off_mul_if(uint32_t (&r)[NL], bool take, const uint32_t (&g)[NL], const FpParams<NL> &P) {
    uint32_t m[NL];
    mont_mul<NL>(m, r, g, P);
#pragma unroll
    for (int q = 0; q < NL; q++) r[q] = take ? m[q] : r[q];
}

// wm = the Montgomery form of x^(-1/2) as the header defines it, xd the digits of the plain residue x; tab = g_i = c^(2^i), i < s,
// Montgomery digits.  Returns 0, 1 for x = 0, 2 for a non-residue (wm is then of no use).
template <int NL>
HB_HD int off_invsqrt_core(uint32_t (&wm)[NL], const uint32_t (&xd)[NL], const OffConsts &K, const uint32_t *tab, const FpParams<NL> &P) {
    uint32_t xm[NL], T[NL], U[NL], V[NL], g[NL];
    to_mont<NL>(xm, xd, P);
    fp_set<NL>(wm, P.one);
    for (int b = K.ebits - 1; b >= 0; b--) {                   // the exponent is the same for every lane
        mont_mul<NL>(wm, wm, wm, P);
        if (off_exp_bit(K, b)) mont_mul<NL>(wm, wm, xm, P);
    }
    mont_mul<NL>(T, wm, wm, P);
    mont_mul<NL>(T, T, xm, P);                                 // x^q
    const int s = K.s;
    for (int i = 0; i < s - 1; i += OFF_WIN) {
        const int nb = (s - 1 - i) < OFF_WIN ? (s - 1 - i) : OFF_WIN;
        fp_set<NL>(U, T);
        for (int r = 0; r < s - 1 - i - nb; r++) mont_mul<NL>(U, U, U, P);
        for (int j = 0; j < nb; j++) {
            fp_set<NL>(V, U);
            for (int r = 0; r < nb - 1 - j; r++) mont_mul<NL>(V, V, V, P);
            const bool bit = !fp_eq<NL>(V, P.one);
            if (j + 1 < nb) { off_tab_load<NL>(g, tab, s - nb + j); off_mul_if<NL>(U, bit, g, P); }
            off_tab_load<NL>(g, tab, i + j + 1);
            off_mul_if<NL>(T, bit, g, P);
            off_tab_load<NL>(g, tab, i + j);
            off_mul_if<NL>(wm, bit, g, P);
        }
    }
    if (fp_is_zero<NL>(xd)) return 1;
    return fp_eq<NL>(T, P.one) ? 0 : 2;
}

// o = u w (HB_OFF_PM1), (u w + 1) / 2 (HB_OFF_01) or, without u, w; 0 for a zero and for a non-residue.  Returns the core's code.
template <int NL, int NW>
HB_HD int off_invsqrt_elem(uint32_t (&o)[NW], const uint32_t (&xw)[NW], const uint32_t (&uw)[NW], bool has_u, int mode, const OffConsts &K,
                           const uint32_t *tab, const FpParams<NL> &P) {
    uint32_t xd[NL], wm[NL], r[NL], t[NL];
    unpack<NL, NW>(xd, xw);
    const int code = off_invsqrt_core<NL>(wm, xd, K, tab, P);
    if (has_u) {
        uint32_t ud[NL];
        unpack<NL, NW>(ud, uw);
        mont_mul<NL>(r, ud, wm, P);                            // plain u times Montgomery w: the plain product
        if (mode == HB_OFF_01) {
            uint32_t one[NL], hm[NL];
#pragma unroll
            for (int q = 0; q < NL; q++) { one[q] = q == 0 ? 1u : 0u; hm[q] = K.half_m[q]; }
            fp_add<NL>(t, r, one, P);
            mont_mul<NL>(r, t, hm, P);
        }
    } else {
        from_mont<NL>(r, wm, P);
    }
#pragma unroll
    for (int q = 0; q < NL; q++) r[q] = code ? 0u : r[q];
    pack<NL, NW>(o, r);
    return code;
}

// column pair j of the coefficient-major block: bit 0 = the t-sharing is not of exact degree t, bit 1 = the 2t-sharing not of exact
// degree 2t, bit 2 = the constant terms differ.  Canonical residues: a coefficient is zero when its words are.
template <int NW> HB_HD uint32_t off_words_or(const uint32_t (&w)[NW]) {
    uint32_t o = 0;
#pragma unroll
    for (int q = 0; q < NW; q++) o |= w[q];
    return o;
}
template <int NW> HB_HD int off_degree_check_column(const uint32_t *coeffs, int n, int64_t k, int t, int64_t j) {
    uint32_t a[NW], b[NW];
    uint32_t lead_a = 0, lead_b = 0, above_a = 0, above_b = 0, diff = 0;
    for (int e = 0; e < n; e++) {
        load_words<NW>(a, coeffs + ((int64_t)e * 2 * k + j) * NW);
        load_words<NW>(b, coeffs + ((int64_t)e * 2 * k + k + j) * NW);
        const uint32_t oa = off_words_or<NW>(a), ob = off_words_or<NW>(b);
        if (e == 0) {
#pragma unroll
            for (int q = 0; q < NW; q++) diff |= a[q] ^ b[q];
        }
        lead_a = e == t ? oa : lead_a;
        lead_b = e == 2 * t ? ob : lead_b;
        above_a |= e > t ? oa : 0u;
        above_b |= e > 2 * t ? ob : 0u;
    }
    return ((lead_a == 0 || above_a != 0) ? 1 : 0) | ((lead_b == 0 || above_b != 0) ? 2 : 0) | (diff ? 4 : 0);
}

// ---------------------------------------------------------------- the row of the masked product (host and device: hb_rows.hpp)
// out may be a, b or c, and b may be a: the row reads its three operands before it stores.
struct OffMulAddArgs { const uint32_t *a, *b, *c; uint32_t *out; };

struct OffMulAddRow {
    template <int NL, int NW, class Mem> HB_HD static void run(const OffMulAddArgs &A, int, int64_t i, int64_t, const Mem &mem, const FpParams<NL> &P) {
        uint32_t aw[NW], bw[NW], cw[NW], ow[NW];
        mem.load(aw, A.a, i);
        mem.load(bw, A.b, i);
        mem.load(cw, A.c, i);
        ew_mul_add_elem<NL, NW>(ow, aw, bw, cw, P);
        mem.store(A.out, i, ow);
    }
};

// ---------------------------------------------------------------- kernels of a shape of their own (wave sums: no lane leaves early)
__device__ __forceinline__ int off_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int NL, int NW>
__global__ void __launch_bounds__(256) k_off_invsqrt_scale(const FpParams<NL> P, const OffConsts *__restrict__ Kp, const uint32_t *__restrict__ tab, const uint32_t *x,
                                                           const uint32_t *u, int mode, uint32_t *out, int64_t count, int32_t *status) {
    // the constants are read through a uniform address: scalar loads, so the exponent's bits and the loop bounds branch the whole wave
    const OffConsts &K = *Kp;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < count;
    uint32_t xw[NW], uw[NW], ow[NW];
#pragma unroll
    for (int q = 0; q < NW; q++) { xw[q] = q == 0 ? 1u : 0u; uw[q] = 0; }
    if (live) {
        load_words<NW>(xw, x + i * NW);
        if (u) load_words<NW>(uw, u + i * NW);
    }
    const int code = off_invsqrt_elem<NL, NW>(ow, xw, uw, u != nullptr, mode, K, tab, P);
    if (live) store_words<NW>(out + i * NW, ow);
    const int zeros = off_wave_sum(live && code == 1 ? 1 : 0), nonres = off_wave_sum(live && code == 2 ? 1 : 0);
    if ((threadIdx.x & 63) == 0) {
        if (zeros) atomicAdd(status, zeros);
        if (nonres) atomicAdd(status + 1, nonres);
    }
}

template <int NW>
__global__ void __launch_bounds__(256) k_off_degree_check(const uint32_t *__restrict__ coeffs, int n, int64_t k, int t, int32_t *__restrict__ counters) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int bad = j < k ? off_degree_check_column<NW>(coeffs, n, k, t, j) : 0;
    const int c0 = off_wave_sum(bad & 1), c1 = off_wave_sum((bad >> 1) & 1), c2 = off_wave_sum((bad >> 2) & 1);
    if ((threadIdx.x & 63) == 0) {
        if (c0) atomicAdd(counters, c0);
        if (c1) atomicAdd(counters + 1, c1);
        if (c2) atomicAdd(counters + 2, c2);
    }
}

// ---------------------------------------------------------------- host side
// the constants and the table g_i = c^(2^i) from the modulus alone, with the same field functions the kernels use
template <int NL> static void off_pow_limbs(uint32_t (&r)[NL], const uint32_t (&a)[NL], const uint64_t (&e)[4], const FpParams<NL> &P) {
    uint32_t acc[NL];
    fp_set<NL>(acc, P.one);
    for (int b = 255; b >= 0; b--) {
        mont_mul<NL>(acc, acc, acc, P);
        if ((e[b >> 6] >> (b & 63)) & 1) mont_mul<NL>(acc, acc, a, P);
    }
    fp_set<NL>(r, acc);
}
static void off_shr1(uint64_t (&v)[4]) {
    for (int i = 0; i < 4; i++) v[i] = (v[i] >> 1) | (i < 3 ? v[i + 1] << 63 : 0);
}
template <int NL>
static void off_make_consts(OffConsts &K, std::vector<uint32_t> &tab, const uint64_t *p_limbs, int n_limbs, const FpParams<NL> &P) {
    uint64_t pm1[4] = {0, 0, 0, 0}, half[4], q[4], h[4];
    for (int i = 0; i < n_limbs; i++) pm1[i] = p_limbs[i];
    pm1[0] -= 1;                                               // p odd: no borrow
    memcpy(half, pm1, 32); off_shr1(half);                     // (p - 1) / 2
    memcpy(q, pm1, 32);
    int s = 0;
    while ((q[0] & 1) == 0) { off_shr1(q); s++; }
    memcpy(K.e, q, 32); off_shr1(K.e);                         // (q - 1) / 2
    K.ebits = 0;
    for (int b = 255; b >= 0; b--) if ((K.e[b >> 6] >> (b & 63)) & 1) { K.ebits = b + 1; break; }
    K.s = s;
    // (p + 1) / 2 = (p - 1) / 2 + 1 as a Montgomery factor
    memcpy(h, half, 32);
    for (int i = 0; i < 4; i++) { if (++h[i]) break; }
    uint32_t hd[NL], hm[NL];
    for (int i = 0; i < NL; i++) {
        const int bit = LB * i, j = bit >> 6, sh = bit & 63;
        uint64_t lo = j < 4 ? h[j] >> sh : 0;
        if (sh > 64 - LB && j + 1 < 4) lo |= h[j + 1] << (64 - sh);
        hd[i] = (uint32_t)lo & DMASK;
    }
    to_mont<NL>(hm, hd, P);
    for (int i = 0; i < 9; i++) K.half_m[i] = i < NL ? hm[i] : 0u;
    // c = z^q for the smallest non-residue z >= 2 (k_sqrt_setup's choice)
    uint32_t minus1[NL], zd[NL], zm[NL], l[NL], c[NL];
    fp_neg<NL>(minus1, P.one, P);
    for (uint32_t z = 2;; z++) {
        for (int i = 0; i < NL; i++) zd[i] = 0;
        zd[0] = z;
        to_mont<NL>(zm, zd, P);
        if (fp_is_zero<NL>(zm)) continue;
        off_pow_limbs<NL>(l, zm, half, P);
        if (fp_eq<NL>(l, minus1)) { off_pow_limbs<NL>(c, zm, q, P); break; }
    }
    tab.assign((size_t)s * NL, 0u);
    for (int i = 0; i < s; i++) {
        for (int d = 0; d < NL; d++) tab[(size_t)i * NL + d] = c[d];
        mont_mul<NL>(c, c, c, P);
    }
}

// The context's blob, made on first use and kept with the context as the square root's constant is: OffConsts at byte 0, the table
// at byte OFF_TAB_AT.
constexpr size_t OFF_TAB_AT = 128;
static_assert(sizeof(OffConsts) <= OFF_TAB_AT, "the constants come first");
static int off_blob(hb_ctx *ctx, const uint8_t **out, hipStream_t s) {
    auto it = ctx->dcache.find("off_tab");
    if (it != ctx->dcache.end()) { *out = (const uint8_t *)it->second; return HB_OK; }
    OffConsts K;
    std::vector<uint32_t> tab;
    if (ctx->n_limbs == 4) off_make_consts<9>(K, tab, ctx->p_limbs, 4, ctx->pw);
    else off_make_consts<3>(K, tab, ctx->p_limbs, 1, ctx->pn);
    std::vector<uint8_t> host(OFF_TAB_AT + tab.size() * 4, 0);
    memcpy(host.data(), &K, sizeof(K));
    if (!tab.empty()) memcpy(host.data() + OFF_TAB_AT, tab.data(), tab.size() * 4);
    void *dev = nullptr;
    HB_HIP(ctx, hipMalloc(&dev, host.size()));
    const int rc = upload_table(ctx, dev, host.data(), host.size(), s);
    if (rc != HB_OK) { (void)hipFree(dev); return rc; }
    ctx->dcache["off_tab"] = dev;
    *out = (const uint8_t *)dev;
    return HB_OK;
}

// host: the masked product as the row the device runs, the other two as the same element functions over `count` elements
template <int NL, int NW>
static int selftest_off(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *ops, uint64_t *out, int64_t count) {
    FpParams<NL> P;
    fp_params_from_limbs(P, p_limbs);
    const int op = what & 0xff, mode = (what >> 8) & 0xff;
    auto W = [](const uint64_t *base, int64_t i) -> const uint32_t (&)[NW] { return *reinterpret_cast<const uint32_t(*)[NW]>(reinterpret_cast<const uint32_t *>(base) + i * NW); };
    uint32_t *o = reinterpret_cast<uint32_t *>(out);
    uint32_t r[NW];
    if (op == HB_OFF_SELFTEST_MUL_ADD) {
        const OffMulAddArgs A = {u32(ops[0]), u32(ops[1]), u32(ops[2]), o};
        host_rows<OffMulAddRow, NL, NW>(A, 1, count, P);
        return HB_OK;
    }
    if (op == HB_OFF_SELFTEST_INVSQRT) {
        OffConsts K;
        std::vector<uint32_t> tab;
        off_make_consts<NL>(K, tab, p_limbs, n_limbs, P);
        const uint32_t none[NW] = {};
        uint64_t status[2] = {0, 0};
        for (int64_t i = 0; i < count; i++) {
            const int code = off_invsqrt_elem<NL, NW>(r, W(ops[0], i), ops[1] ? W(ops[1], i) : none, ops[1] != nullptr, mode, K, tab.data(), P);
            if (code) status[code - 1]++;
            memcpy(o + i * NW, r, NW * 4);
        }
        if (ops[2]) { uint64_t *st = const_cast<uint64_t *>(ops[2]); st[0] = status[0]; st[1] = status[1]; }
        return HB_OK;
    }
    // HB_OFF_SELFTEST_DEGREE_CHECK: count = k, operands[1] = {n, t}
    const int64_t n = (int64_t)ops[1][0], t = (int64_t)ops[1][1];
    if (n < 1 || n > 0x7fffffff || t < 0 || 2 * t >= n) return HB_ERR_BAD_ARG;
    uint64_t c[3] = {0, 0, 0};
    for (int64_t j = 0; j < count; j++) {
        const int bad = off_degree_check_column<NW>(reinterpret_cast<const uint32_t *>(ops[0]), (int)n, count, (int)t, j);
        c[0] += bad & 1; c[1] += (bad >> 1) & 1; c[2] += (bad >> 2) & 1;
    }
    out[0] = c[0]; out[1] = c[1]; out[2] = c[2];
    return HB_OK;
}

}  // namespace hb

extern "C" {

int hb_off_mul_add(hb_ctx *ctx, const uint64_t *a_dev, const uint64_t *b_dev, const uint64_t *c_dev, uint64_t *out_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0 || (count > 0 && (!a_dev || !b_dev || !c_dev || !out_dev))) return HB_ERR_BAD_ARG;
    if (count == 0) return HB_OK;
    HB_ROW_BLOCKS(ctx, "hb_off_mul_add");
    const OffMulAddArgs A = {u32(a_dev), u32(b_dev), u32(c_dev), u32(out_dev)};
    return launch_rows<OffMulAddRow>(ctx, A, (unsigned)blocks, s, count);
}

int hb_off_invsqrt_scale(hb_ctx *ctx, const uint64_t *x_dev, const uint64_t *u_dev, int mode, uint64_t *out_dev, int64_t count, int32_t *status_dev, void *stream) {
    HB_API_GUARD(ctx);
    if (!ctx || count < 0 || (count > 0 && (!x_dev || !out_dev || !status_dev))) return HB_ERR_BAD_ARG;
    if (mode != HB_OFF_PM1 && mode != HB_OFF_01) return fail(ctx, HB_ERR_BAD_ARG, "hb_off_invsqrt_scale: unknown mode");
    if (count == 0) return HB_OK;
    const int64_t blocks = (count + 255) / 256;
    if (blocks > 0x7fffffffLL) return fail(ctx, HB_ERR_UNSUPPORTED, "hb_off_invsqrt_scale: batch too large for one launch");
    hipStream_t s = (hipStream_t)stream;
    const uint8_t *blob = nullptr;
    const int rc = off_blob(ctx, &blob, s);
    if (rc != HB_OK) return rc;
    const OffConsts *K = (const OffConsts *)blob;
    const uint32_t *tab = (const uint32_t *)(blob + OFF_TAB_AT);
    HB_DISPATCH(ctx,
        (k_off_invsqrt_scale<9, 8><<<(unsigned)blocks, 256, 0, s>>>(ctx->pw, K, tab, u32(x_dev), u32(u_dev), mode, (uint32_t *)out_dev, count, status_dev)),
        (k_off_invsqrt_scale<3, 2><<<(unsigned)blocks, 256, 0, s>>>(ctx->pn, K, tab, u32(x_dev), u32(u_dev), mode, (uint32_t *)out_dev, count, status_dev)));
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_off_degree_check(hb_ctx *ctx, const uint64_t *coeffs_dev, int n, int64_t k, int t, int32_t *counters_dev, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || k < 0 || n < 1 || t < 0 || 2 * (int64_t)t >= n) return HB_ERR_BAD_ARG;
    if (k > 0 && (!coeffs_dev || !counters_dev)) return HB_ERR_BAD_ARG;
    if (k == 0) return HB_OK;
    const int64_t blocks = (k + 255) / 256;
    if (blocks > 0x7fffffffLL) return fail(ctx, HB_ERR_UNSUPPORTED, "hb_off_degree_check: batch too large for one launch");
    hipStream_t s = (hipStream_t)stream;
    HB_DISPATCH(ctx,
        (k_off_degree_check<8><<<(unsigned)blocks, 256, 0, s>>>(u32(coeffs_dev), n, k, t, counters_dev)),
        (k_off_degree_check<2><<<(unsigned)blocks, 256, 0, s>>>(u32(coeffs_dev), n, k, t, counters_dev)));
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_selftest_off(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *operands, uint64_t *out, int64_t count) {
    if (!p_limbs || !operands || count < 0 || (n_limbs != 1 && n_limbs != 4)) return HB_ERR_BAD_ARG;
    const int op = what & 0xff, mode = (what >> 8) & 0xff;
    if (op > HB_OFF_SELFTEST_DEGREE_CHECK || (what & ~0xffff) || (op != HB_OFF_SELFTEST_INVSQRT && mode) || (mode != HB_OFF_PM1 && mode != HB_OFF_01)) return HB_ERR_BAD_ARG;
    if (op == HB_OFF_SELFTEST_DEGREE_CHECK) {
        if (!out || !operands[1] || (count > 0 && !operands[0])) return HB_ERR_BAD_ARG;
    } else {
        if (count > 0 && !out) return HB_ERR_BAD_ARG;
        const int n_ops = op == HB_OFF_SELFTEST_MUL_ADD ? 3 : 1;
        for (int k = 0; k < n_ops; k++) if (count > 0 && !operands[k]) return HB_ERR_BAD_ARG;
    }
    if (n_limbs == 4) return selftest_off<9, 8>(p_limbs, n_limbs, what, operands, out, count);
    return selftest_off<3, 2>(p_limbs, n_limbs, what, operands, out, count);
}

}  // extern "C"

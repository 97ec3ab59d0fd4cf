// hb_bf.hip -- one layer of the iterated butterfly (switching) network, the mixer of the reference's AsynchroMix server
// (apps/asynchromix/butterfly_network.py:9-53: batch_switch and the loops of iterated_butterfly_network that deal the inputs
// to it) -- restated on fp29.hpp, not translated.
//
// A layer with stride s = 2^a over k inputs has k / 2 switches.  Switch j takes x = in[xi], y = in[yi],
//     xi = ((j >> a) << (a + 1)) | (j & (s - 1)),   yi = xi | s
// (blocks of s inputs go alternately to the x side and the y side), a shared sign b_j in {1, -1} and one Beaver triple:
//     m = b_j (x - y),   out[2j] = (x + y + m) / 2,   out[2j + 1] = (x + y - m) / 2        (interleaved, not in place).
// The multiplication opens b_j - p_j and (x - y) - q_j, so a layer is two local passes around one open:
//   k_bf_mask    gather + both masked differences, written to ONE buffer [b - p (k/2) | (x - y) - q (k/2)] -- the layer's open
//                is one array; with the signs' half opened in advance (bits == nullptr) only the second half (k/2 elements)
//   k_bf_switch  gather again + the Beaver step (ew_beaver_elem, the body of k_ew_beaver) + both sums halved + the interleave
// 16 element reads and writes a switch (mask 5 + 2, switch 7 + 2) against 36 for the same layer composed from hb_ew_op /
// hb_ew_beaver launches and gathers.
//
// Halving needs no product: v / 2 = (v + (v odd ? p : 0)) >> 1, taken on the digits, where v + p < 2p has headroom (nine
// 29-bit digits hold 261 bits, three hold 87) -- bf_halve.
//
// Operands and results are packed canonical residues.  The per-element bodies are HB_HD functions: the __global__ wrappers
// only compute the two indices, load, call them and store, and hb_selftest_bf runs the very same functions on the host.
//
// Launch shape (both kernels): 256-thread workgroups, one switch a thread, grid = ceil(k / 2 / 256), no LDS, no grid stride,
// one launch a call.  The index arithmetic is shifts and masks on the kernel argument `a`.  8-byte elements at stride 1
// (a == 0): x and y are neighbours and one 16-byte load serves both -- an instantiation of its own (ADJ), picked by the host
// when the stride is 1 and `in` is 16-byte aligned: as a wave-uniform branch inside one kernel the compiler if-converted it
// back into 8- and 4-byte loads.  The two outputs of a switch are always neighbours: the compiler merges their two 8-byte
// stores into one dwordx4 by itself (32-byte elements: two dwordx4 each).  The triple, the sign and the opened values are read once and take
// the non-temporal loads in the 32-byte width, as in k_ew_beaver; `in` is read by both kernels of a layer and loaded plainly.
// Compiler's report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): DESIGN.md section 3j.
#include "hb_common.hpp"
#include "hb_ew_elem.hpp"
#include "hb_rows.hpp"

using namespace hb;

namespace hb {

// ---------------------------------------------------------------- per-element bodies (host and device)
// index of switch j's x input in a layer of stride 2^a; its y input is bf_xi | (1 << a)
HB_HD int64_t bf_xi(int64_t j, int a) { return ((j >> a) << (a + 1)) | (j & (((int64_t)1 << a) - 1)); }

// r = v / 2 mod p for a canonical v: p is odd, so v or v + p is even.  v + p < 2p < 2^(32 NW + 1): the top digit takes the excess.
template <int NL> HB_HD void bf_halve(uint32_t (&r)[NL], const uint32_t (&v)[NL], const FpParams<NL> &P) {
    const uint32_t odd = 0u - (v[0] & 1u);
    uint32_t w[NL], carry_ = 0;
#pragma unroll
    for (int i = 0; i < NL; i++) {
        const uint32_t t = v[i] + (P.p[i] & odd) + carry_;
        if (i < NL - 1) { carry_ = t >> LB; w[i] = t & DMASK; } else w[i] = t;
    }
#pragma unroll
    for (int i = 0; i < NL - 1; i++) r[i] = (w[i] >> 1) | ((w[i + 1] & 1u) << (LB - 1));
    r[NL - 1] = w[NL - 1] >> 1;
}

// o = a - b
template <int NL, int NW> HB_HD void bf_mask_bit(uint32_t (&o)[NW], const uint32_t (&bw)[NW], const uint32_t (&pw)[NW], const FpParams<NL> &P) {
    uint32_t b[NL], p[NL], r[NL];
    unpack<NL, NW>(b, bw);
    unpack<NL, NW>(p, pw);
    fp_sub<NL>(r, b, p, P);
    pack<NL, NW>(o, r);
}
// o = (x - y) - q
template <int NL, int NW>
HB_HD void bf_mask_diff(uint32_t (&o)[NW], const uint32_t (&xw)[NW], const uint32_t (&yw)[NW], const uint32_t (&qw)[NW], const FpParams<NL> &P) {
    uint32_t x[NL], y[NL], t[NL], r[NL];
    unpack<NL, NW>(x, xw);
    unpack<NL, NW>(y, yw);
    fp_sub<NL>(t, x, y, P);
    unpack<NL, NW>(y, qw);
    fp_sub<NL>(r, t, y, P);
    pack<NL, NW>(o, r);
}
// m = d e + d q + e p + pq (this party's share of b (x - y));  o0 = (x + y + m) / 2,  o1 = (x + y - m) / 2
template <int NL, int NW>
HB_HD void bf_switch_elem(uint32_t (&o0)[NW], uint32_t (&o1)[NW], const uint32_t (&xw)[NW], const uint32_t (&yw)[NW], const uint32_t (&dw)[NW],
                          const uint32_t (&ew)[NW], const uint32_t (&pw)[NW], const uint32_t (&qw)[NW], const uint32_t (&pqw)[NW], const FpParams<NL> &P) {
    uint32_t mw[NW], m[NL], x[NL], y[NL], t[NL], u[NL], r[NL];
    ew_beaver_elem<NL, NW>(mw, dw, ew, pw, qw, pqw, P);
    unpack<NL, NW>(m, mw);
    unpack<NL, NW>(x, xw);
    unpack<NL, NW>(y, yw);
    fp_add<NL>(t, x, y, P);
    fp_add<NL>(u, t, m, P);
    bf_halve<NL>(r, u, P);
    pack<NL, NW>(o0, r);
    fp_sub<NL>(u, t, m, P);
    bf_halve<NL>(r, u, P);
    pack<NL, NW>(o1, r);
}

// ---------------------------------------------------------------- kernels
// the two inputs of switch j.  ADJ (8-byte elements, a == 0, `in` 16-byte aligned): they sit side by side, one dwordx4.
template <int NW, bool ADJ>
__device__ __forceinline__ void bf_load_pair(uint32_t (&x)[NW], uint32_t (&y)[NW], const uint32_t *__restrict__ in, int64_t j, int a) {
    if constexpr (ADJ) {
        static_assert(NW == 2, "two 8-byte elements in one 16-byte access");
        const uint4 v = *reinterpret_cast<const uint4 *>(in + 4 * j);
        x[0] = v.x; x[1] = v.y; y[0] = v.z; y[1] = v.w;
    } else {
        const int64_t xi = bf_xi(j, a);
        load_words<NW>(x, in + xi * NW);
        load_words<NW>(y, in + (xi | ((int64_t)1 << a)) * NW);
    }
}
// out[2j], out[2j + 1]: 2 NW adjacent words
template <int NW> __device__ __forceinline__ void bf_store_pair(uint32_t *__restrict__ out, int64_t j, const uint32_t (&o0)[NW], const uint32_t (&o1)[NW]) {
    uint32_t *dst = out + 2 * j * NW;
    store_words<NW>(dst, o0);
    store_words<NW>(dst + NW, o1);
}
static bool bf_aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
// read-once operands (the triple, the sign, the opened values)

// masked[(BITS ? half : 0) + j] = in[xi] - in[yi] - q[j];  BITS: masked[j] = bits[j] - p[j].  `masked` does not overlap `in`.
template <int NL, int NW, bool BITS, bool ADJ>
__global__ void __launch_bounds__(256) k_bf_mask(const FpParams<NL> P, const uint32_t *in, const uint32_t *bits, const uint32_t *p, const uint32_t *q,
                                                 int64_t half, int a, uint32_t *masked) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= half) return;
    uint32_t xw[NW], yw[NW], qw[NW], ow[NW];
    bf_load_pair<NW, ADJ>(xw, yw, in, j, a);
    load_once<NW>(qw, q + j * NW);
    if constexpr (BITS) {
        uint32_t bw[NW], pw[NW], mw[NW];
        load_once<NW>(bw, bits + j * NW);
        load_once<NW>(pw, p + j * NW);
        bf_mask_bit<NL, NW>(mw, bw, pw, P);
        store_words<NW>(masked + j * NW, mw);
    }
    bf_mask_diff<NL, NW>(ow, xw, yw, qw, P);
    store_words<NW>(masked + ((BITS ? half : 0) + j) * NW, ow);
}

// out[2j], out[2j + 1] from in[xi], in[yi], the opened d[j], e[j] and the triple.  `out` does not overlap `in`: switch j writes
// positions other switches read.
template <int NL, int NW, bool ADJ>
__global__ void __launch_bounds__(256) k_bf_switch(const FpParams<NL> P, const uint32_t *in, const uint32_t *d, const uint32_t *e, const uint32_t *p,
                                                   const uint32_t *q, const uint32_t *pq, int64_t half, int a, uint32_t *out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= half) return;
    uint32_t xw[NW], yw[NW], dw[NW], ew[NW], pw[NW], qw[NW], pqw[NW], o0[NW], o1[NW];
    bf_load_pair<NW, ADJ>(xw, yw, in, j, a);
    load_once<NW>(dw, d + j * NW); load_once<NW>(ew, e + j * NW); load_once<NW>(qw, q + j * NW);
    load_once<NW>(pw, p + j * NW); load_once<NW>(pqw, pq + j * NW);
    bf_switch_elem<NL, NW>(o0, o1, xw, yw, dw, ew, pw, qw, pqw, P);
    bf_store_pair<NW>(out, j, o0, o1);
}

// k a power of two >= 2 and 0 <= a < log2(k)
static bool bf_shape_ok(int64_t k, int a) { return k >= 2 && (k & (k - 1)) == 0 && a >= 0 && a < 62 && ((int64_t)1 << a) < k; }

template <int NL, int NW, bool BITS>
static void launch_mask(const FpParams<NL> &P, const uint32_t *in, const uint32_t *b, const uint32_t *p, const uint32_t *q, int64_t half, int a, uint32_t *o,
                        unsigned blocks, hipStream_t s) {
    if constexpr (NW == 2) {
        if (a == 0 && bf_aligned16(in)) { k_bf_mask<NL, NW, BITS, true><<<blocks, 256, 0, s>>>(P, in, b, p, q, half, a, o); return; }
    }
    k_bf_mask<NL, NW, BITS, false><<<blocks, 256, 0, s>>>(P, in, b, p, q, half, a, o);
}
template <int NL, int NW>
static void launch_switch(const FpParams<NL> &P, const uint32_t *in, const uint32_t *d, const uint32_t *e, const uint32_t *p, const uint32_t *q, const uint32_t *pq,
                          int64_t half, int a, uint32_t *o, unsigned blocks, hipStream_t s) {
    if constexpr (NW == 2) {
        if (a == 0 && bf_aligned16(in)) { k_bf_switch<NL, NW, true><<<blocks, 256, 0, s>>>(P, in, d, e, p, q, pq, half, a, o); return; }
    }
    k_bf_switch<NL, NW, false><<<blocks, 256, 0, s>>>(P, in, d, e, p, q, pq, half, a, o);
}

// host: the same element functions, switch by switch
template <int NL, int NW>
static int selftest_bf(const uint64_t *p_limbs, int what, const uint64_t *const *ops, int64_t k, int a, uint64_t *out) {
    FpParams<NL> P;
    fp_params_from_limbs(P, p_limbs);
    auto W = [](const uint64_t *base, int64_t i) -> const uint32_t (&)[NW] { return *reinterpret_cast<const uint32_t(*)[NW]>(reinterpret_cast<const uint32_t *>(base) + i * NW); };
    uint32_t *o = reinterpret_cast<uint32_t *>(out);
    if (what == HB_BF_SELFTEST_HALVE) {
        for (int64_t i = 0; i < k; i++) {
            uint32_t v[NL], r[NL], w[NW];
            unpack<NL, NW>(v, W(ops[0], i));
            bf_halve<NL>(r, v, P);
            pack<NL, NW>(w, r);
            memcpy(o + i * NW, w, NW * 4);
        }
        return HB_OK;
    }
    const int64_t half = k / 2;
    for (int64_t j = 0; j < half; j++) {
        const int64_t xi = bf_xi(j, a), yi = xi | ((int64_t)1 << a);
        if (what == HB_BF_SELFTEST_MASK) {
            uint32_t r[NW];
            if (ops[1]) { bf_mask_bit<NL, NW>(r, W(ops[1], j), W(ops[2], j), P); memcpy(o + j * NW, r, NW * 4); }
            bf_mask_diff<NL, NW>(r, W(ops[0], xi), W(ops[0], yi), W(ops[3], j), P);
            memcpy(o + ((ops[1] ? half : 0) + j) * NW, r, NW * 4);
        } else {
            uint32_t r0[NW], r1[NW];
            bf_switch_elem<NL, NW>(r0, r1, W(ops[0], xi), W(ops[0], yi), W(ops[1], j), W(ops[2], j), W(ops[3], j), W(ops[4], j), W(ops[5], j), P);
            memcpy(o + 2 * j * NW, r0, NW * 4);
            memcpy(o + (2 * j + 1) * NW, r1, NW * 4);
        }
    }
    return HB_OK;
}

}  // namespace hb

extern "C" {

int hb_bf_mask(hb_ctx *ctx, const uint64_t *in_dev, const uint64_t *bits_dev, const uint64_t *p_dev, const uint64_t *q_dev, int64_t k, int log2_stride,
               uint64_t *masked_dev, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || !in_dev || !q_dev || !masked_dev || (bits_dev && !p_dev)) return HB_ERR_BAD_ARG;
    if (!bf_shape_ok(k, log2_stride)) return fail(ctx, HB_ERR_BAD_ARG, "hb_bf_mask: k must be a power of two >= 2 and 0 <= log2_stride < log2(k)");
    const int64_t eb = 8 * (int64_t)ctx->n_limbs, half = k / 2;
    if (overlap(masked_dev, (bits_dev ? k : half) * eb, in_dev, k * eb)) return fail(ctx, HB_ERR_BAD_ARG, "hb_bf_mask: masked overlaps in");
    const int64_t blocks = (half + 255) / 256;
    if (blocks > 0x7fffffffLL) return fail(ctx, HB_ERR_UNSUPPORTED, "hb_bf_mask: layer too large for one launch");
    hipStream_t s = (hipStream_t)stream;
    const uint32_t *in = (const uint32_t *)in_dev, *b = (const uint32_t *)bits_dev, *p = (const uint32_t *)p_dev, *q = (const uint32_t *)q_dev;
    uint32_t *o = (uint32_t *)masked_dev;
    if (bits_dev)
        HB_DISPATCH(ctx, (launch_mask<9, 8, true>(ctx->pw, in, b, p, q, half, log2_stride, o, (unsigned)blocks, s)),
                    (launch_mask<3, 2, true>(ctx->pn, in, b, p, q, half, log2_stride, o, (unsigned)blocks, s)));
    else
        HB_DISPATCH(ctx, (launch_mask<9, 8, false>(ctx->pw, in, nullptr, nullptr, q, half, log2_stride, o, (unsigned)blocks, s)),
                    (launch_mask<3, 2, false>(ctx->pn, in, nullptr, nullptr, q, half, log2_stride, o, (unsigned)blocks, s)));
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_bf_switch(hb_ctx *ctx, const uint64_t *in_dev, const uint64_t *d_dev, const uint64_t *e_dev, const uint64_t *p_dev, const uint64_t *q_dev,
                 const uint64_t *pq_dev, int64_t k, int log2_stride, uint64_t *out_dev, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || !in_dev || !d_dev || !e_dev || !p_dev || !q_dev || !pq_dev || !out_dev) return HB_ERR_BAD_ARG;
    if (!bf_shape_ok(k, log2_stride)) return fail(ctx, HB_ERR_BAD_ARG, "hb_bf_switch: k must be a power of two >= 2 and 0 <= log2_stride < log2(k)");
    const int64_t eb = 8 * (int64_t)ctx->n_limbs, half = k / 2;
    if (overlap(out_dev, k * eb, in_dev, k * eb)) return fail(ctx, HB_ERR_BAD_ARG, "hb_bf_switch: out overlaps in (a layer is not in place)");
    const int64_t blocks = (half + 255) / 256;
    if (blocks > 0x7fffffffLL) return fail(ctx, HB_ERR_UNSUPPORTED, "hb_bf_switch: layer too large for one launch");
    hipStream_t s = (hipStream_t)stream;
    HB_DISPATCH(ctx,
        (launch_switch<9, 8>(ctx->pw, (const uint32_t *)in_dev, (const uint32_t *)d_dev, (const uint32_t *)e_dev, (const uint32_t *)p_dev, (const uint32_t *)q_dev,
                             (const uint32_t *)pq_dev, half, log2_stride, (uint32_t *)out_dev, (unsigned)blocks, s)),
        (launch_switch<3, 2>(ctx->pn, (const uint32_t *)in_dev, (const uint32_t *)d_dev, (const uint32_t *)e_dev, (const uint32_t *)p_dev, (const uint32_t *)q_dev,
                             (const uint32_t *)pq_dev, half, log2_stride, (uint32_t *)out_dev, (unsigned)blocks, s)));
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_selftest_bf(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *operands, int64_t k, int log2_stride, uint64_t *out) {
    if (!p_limbs || !out || (n_limbs != 1 && n_limbs != 4)) return HB_ERR_BAD_ARG;
    if (what == HB_BF_SELFTEST_HALVE) {
        if (k < 0 || !operands || (k > 0 && !operands[0])) return HB_ERR_BAD_ARG;
    } else {
        if (!bf_shape_ok(k, log2_stride)) return HB_ERR_BAD_ARG;
        if (what == HB_BF_SELFTEST_INDEX) {
            for (int64_t j = 0; j < k / 2; j++) { out[2 * j] = (uint64_t)bf_xi(j, log2_stride); out[2 * j + 1] = out[2 * j] | ((uint64_t)1 << log2_stride); }
            return HB_OK;
        }
        if ((what != HB_BF_SELFTEST_MASK && what != HB_BF_SELFTEST_SWITCH) || !operands) return HB_ERR_BAD_ARG;
        const int n_ops = what == HB_BF_SELFTEST_MASK ? 4 : 6;
        for (int i = 0; i < n_ops; i++)
            if (!operands[i] && !(what == HB_BF_SELFTEST_MASK && (i == 1 || (i == 2 && !operands[1])))) return HB_ERR_BAD_ARG;   // mask: the signs (and then p) may be NULL
        if (operands[0] == out) return HB_ERR_BAD_ARG;
    }
    if (n_limbs == 4) return selftest_bf<9, 8>(p_limbs, what, operands, k, log2_stride, out);
    return selftest_bf<3, 2>(p_limbs, what, operands, k, log2_stride, out);
}

}  // extern "C"

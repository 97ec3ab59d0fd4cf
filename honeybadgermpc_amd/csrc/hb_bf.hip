// hb_bf.hip -- one layer of the iterated butterfly (switching) network, the mixer of the reference's AsynchroMix server
// (apps/asynchromix/butterfly_network.py:9-53: batch_switch and the loops of iterated_butterfly_network that deal the inputs
// to it) -- restated on fp29.hpp, not translated.
//
// A layer with stride s = 2^a over k inputs has k / 2 switches.  Switch j takes x = in[xi], y = in[yi],
//     xi = ((j >> a) << (a + 1)) | (j & (s - 1)),   yi = xi | s
// (blocks of s inputs go alternately to the x side and the y side), a shared sign b_j in {1, -1} and one Beaver triple:
//     m = b_j (x - y),   out[2j] = (x + y + m) / 2,   out[2j + 1] = (x + y - m) / 2        (interleaved, not in place).
// The multiplication opens b_j - p_j and (x - y) - q_j, so a layer is two local passes around one open:
//   BfMaskRow    gather + both masked differences, written to ONE buffer [b - p (k/2) | (x - y) - q (k/2)] -- the layer's open
//                is one array; with the signs' half opened in advance (bits == nullptr) only the second half (k/2 elements)
//   BfSwitchRow  gather again + the Beaver step (ew_beaver_elem, the body of EwBeaverRow) + both sums halved + the interleave
// 16 element reads and writes a switch (mask 5 + 2, switch 7 + 2) against 36 for the same layer composed from hb_ew_op /
// hb_ew_beaver launches and gathers.
//
// Halving needs no product: v / 2 = (v + (v odd ? p : 0)) >> 1, taken on the digits, where v + p < 2p has headroom (nine
// 29-bit digits hold 261 bits, three hold 87) -- bf_halve.
//
// Operands and results are packed canonical residues.  The per-element bodies are HB_HD functions; both steps are rows
// (hb_rows.hpp): the two indices, the loads, the body and the stores are an HB_HD function over a memory policy, so hb_selftest_bf
// runs on the host the very rows, arithmetic and addressing, that k_rows runs on the device.
//
// Launch shape (both steps): k_rows -- 256-thread workgroups, one switch a thread, grid = ceil(k / 2 / 256), no LDS, no grid stride,
// one launch a call.  The index arithmetic is shifts and masks on the argument `a`.  8-byte elements at stride 1
// (a == 0): x and y are neighbours and one 16-byte load serves both (the policy's pair) -- a row of its own (ADJ), picked by the
// host when the stride is 1 and `in` is 16-byte aligned: as a wave-uniform branch inside one kernel the compiler if-converted it
// back into 8- and 4-byte loads.  The two outputs of a switch are always neighbours: the compiler merges their two 8-byte
// stores into one dwordx4 by itself (32-byte elements: two dwordx4 each).  The triple, the sign and the opened values are read once and take
// the non-temporal loads in the 32-byte width, as in EwBeaverRow; `in` is read by both kernels of a layer and loaded plainly.
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

// ---------------------------------------------------------------- the steps' rows (host and device, over a memory policy: hb_rows.hpp)
// Element j of a row is switch j, `count` = k / 2.  The two inputs of switch j; ADJ (stride 1): the neighbours 2j and 2j + 1, mem.pair's.
template <bool ADJ, int NW, class Mem> HB_HD void bf_inputs(uint32_t (&x)[NW], uint32_t (&y)[NW], const uint32_t *in, int64_t j, int a, const Mem &mem) {
    if constexpr (ADJ) {
        mem.pair(x, y, in, 2 * j);
    } else {
        const int64_t xi = bf_xi(j, a);
        mem.load(x, in, xi);
        mem.load(y, in, xi | ((int64_t)1 << a));
    }
}

// masked[(BITS ? half : 0) + j] = in[xi] - in[yi] - q[j];  BITS: masked[j] = bits[j] - p[j].  `masked` does not overlap `in`.
struct BfMaskArgs { const uint32_t *in, *bits, *p, *q; uint32_t *masked; int a; };

template <bool BITS, bool ADJ> struct BfMaskRow {
    template <int NL, int NW, class Mem> HB_HD static void run(const BfMaskArgs &A, int, int64_t j, int64_t half, const Mem &mem, const FpParams<NL> &P) {
        uint32_t xw[NW], yw[NW], qw[NW], ow[NW];
        bf_inputs<ADJ>(xw, yw, A.in, j, A.a, mem);
        mem.once(qw, A.q, j);
        if constexpr (BITS) {
            uint32_t bw[NW], pw[NW], mw[NW];
            mem.once(bw, A.bits, j);
            mem.once(pw, A.p, j);
            bf_mask_bit<NL, NW>(mw, bw, pw, P);
            mem.store(A.masked, j, mw);
        }
        bf_mask_diff<NL, NW>(ow, xw, yw, qw, P);
        mem.store(A.masked, (BITS ? half : 0) + j, ow);
    }
};

// out[2j], out[2j + 1] from in[xi], in[yi], the opened d[j], e[j] and the triple.  `out` does not overlap `in`: switch j writes
// positions other switches read.
struct BfSwitchArgs { const uint32_t *in, *d, *e, *p, *q, *pq; uint32_t *out; int a; };

template <bool ADJ> struct BfSwitchRow {
    template <int NL, int NW, class Mem> HB_HD static void run(const BfSwitchArgs &A, int, int64_t j, int64_t, const Mem &mem, const FpParams<NL> &P) {
        uint32_t xw[NW], yw[NW], dw[NW], ew[NW], pw[NW], qw[NW], pqw[NW], o0[NW], o1[NW];
        bf_inputs<ADJ>(xw, yw, A.in, j, A.a, mem);
        mem.once(dw, A.d, j); mem.once(ew, A.e, j); mem.once(qw, A.q, j);
        mem.once(pw, A.p, j); mem.once(pqw, A.pq, j);
        bf_switch_elem<NL, NW>(o0, o1, xw, yw, dw, ew, pw, qw, pqw, P);
        mem.store(A.out, 2 * j, o0);
        mem.store(A.out, 2 * j + 1, o1);
    }
};

// k a power of two >= 2 and 0 <= a < log2(k)
static bool bf_shape_ok(int64_t k, int a) { return k >= 2 && (k & (k - 1)) == 0 && a >= 0 && a < 62 && ((int64_t)1 << a) < k; }

// AdjRow exactly when the elements are 8 bytes, the stride is 1 and `in` is 16-byte aligned (the narrow width alone has that row), else Row
template <class AdjRow, class Row, class Args> static int bf_launch(hb_ctx *ctx, const Args &A, unsigned blocks, hipStream_t s, int64_t half) {
    if (ctx->n_limbs != 4 && A.a == 0 && ((uintptr_t)A.in & 15) == 0) {
        k_rows<AdjRow, 3, 2><<<blocks, 256, 0, s>>>(ctx->pn, A, half);
        HB_LAUNCH_CHECK(ctx);
        return HB_OK;
    }
    return launch_rows<Row>(ctx, A, blocks, s, half);
}

// host: the same rows, switch by switch.  MASK and SWITCH run the general row (two loads at bf_xi); at stride 1 in the 8-byte width
// the ADJ row then runs too and writes the same outputs over them, so the host walks mem.pair as well.
template <int NL, int NW>
static int selftest_bf(const uint64_t *p_limbs, int what, const uint64_t *const *ops, int64_t k, int a, uint64_t *out) {
    FpParams<NL> P;
    fp_params_from_limbs(P, p_limbs);
    uint32_t *o = u32(out);
    if (what == HB_BF_SELFTEST_HALVE) {
        for (int64_t i = 0; i < k; i++) {
            uint32_t v[NL], r[NL], w[NW];
            memcpy(w, u32(ops[0]) + i * NW, NW * 4);
            unpack<NL, NW>(v, w);
            bf_halve<NL>(r, v, P);
            pack<NL, NW>(w, r);
            memcpy(o + i * NW, w, NW * 4);
        }
        return HB_OK;
    }
    const int64_t half = k / 2;
    const bool adj = NW == 2 && a == 0;
    if (what == HB_BF_SELFTEST_MASK) {
        const BfMaskArgs A = {u32(ops[0]), u32(ops[1]), u32(ops[2]), u32(ops[3]), o, a};
        if (A.bits) {
            host_rows<BfMaskRow<true, false>, NL, NW>(A, 1, half, P);
            if (adj) host_rows<BfMaskRow<true, true>, NL, NW>(A, 1, half, P);
        } else {
            host_rows<BfMaskRow<false, false>, NL, NW>(A, 1, half, P);
            if (adj) host_rows<BfMaskRow<false, true>, NL, NW>(A, 1, half, P);
        }
    } else {
        const BfSwitchArgs A = {u32(ops[0]), u32(ops[1]), u32(ops[2]), u32(ops[3]), u32(ops[4]), u32(ops[5]), o, a};
        host_rows<BfSwitchRow<false>, NL, NW>(A, 1, half, P);
        if (adj) host_rows<BfSwitchRow<true>, NL, NW>(A, 1, half, P);
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
    const BfMaskArgs A = {u32(in_dev), u32(bits_dev), u32(p_dev), u32(q_dev), u32(masked_dev), log2_stride};
    if (bits_dev) return bf_launch<BfMaskRow<true, true>, BfMaskRow<true, false>>(ctx, A, (unsigned)blocks, s, half);
    return bf_launch<BfMaskRow<false, true>, BfMaskRow<false, false>>(ctx, A, (unsigned)blocks, s, half);
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
    const BfSwitchArgs A = {u32(in_dev), u32(d_dev), u32(e_dev), u32(p_dev), u32(q_dev), u32(pq_dev), u32(out_dev), log2_stride};
    return bf_launch<BfSwitchRow<true>, BfSwitchRow<false>>(ctx, A, (unsigned)blocks, s, half);
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

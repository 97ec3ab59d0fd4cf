// hb_ew.hip -- element-wise GF(p) arithmetic on packed share arrays: the `modarith` device library of SURVEY section 2
// (add / sub / mul / neg / inv) and the fused Beaver step, for the MPC programs the opens exist to feed
// (reference honeybadgermpc/progs/mixins/share_arithmetic.py:24-45, 71-103, 120-135, 151-161; the local operators of
// progs/mixins/dataflow.py ShareArray.__add__ / __sub__ / __mul__) -- restated on fp29.hpp, not translated.
//
// Operands and results are packed canonical residues (what every other entry point of the library writes).  The per-element
// bodies are HB_HD functions.  The binary ops and the Beaver step are rows (hb_rows.hpp): which operands a step loads, which body it
// calls and where it stores is an HB_HD function over a memory policy, so hb_selftest_ew runs on the host the very rows, arithmetic
// and addressing, that k_rows runs on the device.  The inversion keeps a kernel of its own (a wave sums its zeros: no lane may leave
// early); its self test walks the kernel's lane function tile by tile.
//
// Launch shapes (all kernels: 256-thread workgroups, no LDS, no grid stride, one launch per call):
//   k_rows<EwBinaryRow<OP, BCAST>>, k_rows<EwBeaverRow>   one element a thread; grid = ceil(count / 256)
//   k_ew_inv      one tile of 64 E elements a wave, four tiles a workgroup; lane l owns elements l, l + 64, ... of its tile
//                 (E = 8 for 32-byte elements, 16 for 8-byte ones)
// Compiler's report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; scratch = 0 bytes for every kernel):
//   k_rows<EwBinaryRow, 9, 8>  MUL 52 VGPRs (broadcast 46), ADD / SUB / NEG 20-22: 8 waves a SIMD     k_rows<EwBinaryRow, 3, 2>  8-18 VGPRs: 8 waves
//   k_rows<EwBeaverRow, 9, 8>  70 VGPRs: 7 waves a SIMD                                              k_rows<EwBeaverRow, 3, 2>  25 VGPRs: 8 waves
//   k_ew_inv<9, 8, 8>  255 VGPRs + 72 accumulation registers: 1 wave a SIMD                  k_ew_inv<3, 2, 16> 234 VGPRs: 2 waves
// (asked for two waves a SIMD the wide inversion spills 292 bytes a lane; DESIGN.md section 3h has the findings and the timings)
#include <type_traits>

#include "hb_common.hpp"
#include "hb_ew_elem.hpp"
#include "hb_rows.hpp"

using namespace hb;

namespace hb {

enum { EW_ADD = HB_EW_ADD, EW_SUB = HB_EW_SUB, EW_MUL = HB_EW_MUL, EW_NEG = HB_EW_NEG };

template <int NL> struct EwTile { static constexpr int E = (NL >= 9) ? 8 : 16; };

// ---------------------------------------------------------------- per-element bodies (host and device)
// o = a OP b on packed words.  MUL of two plain residues: one product gives ab / R (below 2p, one conditional subtraction),
// a second one by R^2 brings ab back -- 2 mac + 2 redc, the same count as converting an operand first, and its multiplier
// (P.r2) is a kernel argument, so the second product's left operand sits in SGPRs whatever b is.
template <int NL, int NW, int OP>
HB_HD void ew_binary_elem(uint32_t (&o)[NW], const uint32_t (&a)[NW], const uint32_t (&b)[NW], const FpParams<NL> &P) {
    uint32_t ad[NL], bd[NL], r[NL];
    unpack<NL, NW>(ad, a);
    if constexpr (OP == EW_NEG) {
        fp_neg<NL>(r, ad, P);
    } else {
        unpack<NL, NW>(bd, b);
        if constexpr (OP == EW_ADD) fp_add<NL>(r, ad, bd, P);
        else if constexpr (OP == EW_SUB) fp_sub<NL>(r, ad, bd, P);
        else {
            uint32_t t[NL];
            mont_mul<NL>(t, bd, ad, P);
            mont_mul<NL>(r, P.r2, t, P);
        }
    }
    pack<NL, NW>(o, r);
}

// The fused Beaver step d e + d q + e p + pq: ew_beaver_elem of hb_ew_elem.hpp (hb_bf.hip computes its switches with the same body).

// One lane's share of an inversion tile: the E elements in[first + k * step], k < E, that lie below `count` (Montgomery's trick:
// prefix products, one inversion, back-substitution; 3 (E - 1) products and one fp_inv).  Returns the number of zeros it met.
// The plain residues are used as they are (as the Montgomery forms of a_k / R): with M(x, y) = x y / R the prefixes are
// c_k = M(c_(k-1), a_k); fp_inv(c_(E-1)) = R^2 / c_(E-1), two bare REDCs make it u = 1 / c_(E-1) (plain); then
// out_k = M(u, c_(k-1)) = 1 / a_k and u <- M(u, a_k) = 1 / c_(k-1): nothing is converted on the way in or out.
// A zero (and a slot past `count`) stands in the chain as R mod p, which M leaves a value unchanged by; its output is 0.
// (The two passes are unrolled by template recursion: the arrays must be indexed by constants to stay in registers, and the
// unroller declines a pragma on bodies of this size.)
template <int K, int N, class F> HB_HD void ew_static_for(F &&f) {
    if constexpr (K < N) { f(std::integral_constant<int, K>{}); ew_static_for<K + 1, N>(f); }
}
template <int NL, int NW, int E>
HB_HD int ew_inv_lane(const uint32_t *in, uint32_t *out, int64_t first, int64_t step, int64_t count, const FpParams<NL> &P) {
    uint32_t a[E][NL], c[E][NL], u[NL], t[NL];
    uint32_t zero_mask = 0;
    int zeros = 0;
    ew_static_for<0, E>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        const int64_t i = first + k * step;
        bool z = true;
        if (i < count) {
            load_digits<NL, NW>(a[k], in + i * NW);
            z = fp_is_zero<NL>(a[k]);
            zeros += z ? 1 : 0;
        }
        if (z) { fp_set<NL>(a[k], P.one); zero_mask |= 1u << k; }
        if constexpr (k == 0) fp_set<NL>(c[0], a[0]);
        else mont_mul<NL>(c[k], c[k - 1], a[k], P);
    });
    fp_inv<NL>(t, c[E - 1], P);
    from_mont<NL>(u, t, P);
    from_mont<NL>(t, u, P);
    fp_set<NL>(u, t);
    ew_static_for<0, E>([&](auto kc) {
        constexpr int k = E - 1 - decltype(kc)::value;
        const int64_t i = first + k * step;
        if constexpr (k > 0) mont_mul<NL>(t, u, c[k - 1], P); else fp_set<NL>(t, u);
        if ((zero_mask >> k) & 1u) {
#pragma unroll
            for (int q = 0; q < NL; q++) t[q] = 0;
        }
        if (i < count) store_digits<NL, NW>(out + i * NW, t);
        if constexpr (k > 0) { mont_mul<NL>(t, u, a[k], P); fp_set<NL>(u, t); }
    });
    return zeros;
}

// ---------------------------------------------------------------- the steps' rows (host and device, over a memory policy: hb_rows.hpp)
// out[i] = a[i] OP b[BCAST ? 0 : i].  out may be a or b: a row reads its operands before it stores.  The broadcast element is
// mem.same's: on the device its digits live in SGPRs (the `a` operand of mac, fp29.hpp:72) and its unpack is scalar work.
struct EwBinaryArgs { const uint32_t *a, *b; uint32_t *out; };

template <int OP, bool BCAST> struct EwBinaryRow {
    template <int NL, int NW, class Mem> HB_HD static void run(const EwBinaryArgs &A, int, int64_t i, int64_t, const Mem &mem, const FpParams<NL> &P) {
        uint32_t aw[NW], bw[NW], ow[NW];
        mem.load(aw, A.a, i);
        if constexpr (OP == EW_NEG) {
#pragma unroll
            for (int q = 0; q < NW; q++) bw[q] = 0;
        } else if constexpr (BCAST) {
            mem.same(bw, A.b);
        } else {
            mem.load(bw, A.b, i);
        }
        ew_binary_elem<NL, NW, OP>(ow, aw, bw, P);
        mem.store(A.out, i, ow);
    }
};

// The fused Beaver step: five reads and one write an element, nothing in between goes to memory.  d and e are values just
// opened and the triple is consumed: every byte is read once (mem.once), so the 32-byte elements take the non-temporal loads
// (load_words_nt: they pass the CU's vector L1, where no line of this launch is ever asked for twice, and are served by L2 as
// plain loads are).  The result is stored plainly: a plain or non-temporal store leaves the line in L2 alike, and the next
// launch of the program reads it.  8-byte elements use the plain dwordx2 forms (the _nt helpers move whole dwordx4).
struct EwBeaverArgs { const uint32_t *d, *e, *p, *q, *pq; uint32_t *out; };

struct EwBeaverRow {
    template <int NL, int NW, class Mem> HB_HD static void run(const EwBeaverArgs &A, int, int64_t i, int64_t, const Mem &mem, const FpParams<NL> &P) {
        uint32_t dw[NW], ew[NW], pw[NW], qw[NW], pqw[NW], ow[NW];
        mem.once(dw, A.d, i); mem.once(ew, A.e, i); mem.once(qw, A.q, i);
        mem.once(pw, A.p, i); mem.once(pqw, A.pq, i);
        ew_beaver_elem<NL, NW>(ow, dw, ew, pw, qw, pqw, P);
        mem.store(A.out, i, ow);
    }
};

// f(the row of (op, broadcast)): the one switch of the launch and of the self test
template <class F> static int with_binary_row(int op, bool bcast, F &&f) {
    switch (op) {
    case EW_ADD: return bcast ? f(EwBinaryRow<EW_ADD, true>{}) : f(EwBinaryRow<EW_ADD, false>{});
    case EW_SUB: return bcast ? f(EwBinaryRow<EW_SUB, true>{}) : f(EwBinaryRow<EW_SUB, false>{});
    case EW_MUL: return bcast ? f(EwBinaryRow<EW_MUL, true>{}) : f(EwBinaryRow<EW_MUL, false>{});
    default: return f(EwBinaryRow<EW_NEG, false>{});
    }
}

// ---------------------------------------------------------------- the inversion's kernel
// Batched inversion: wave w of the launch owns the tile [w 64 E, (w + 1) 64 E); lane l its elements l, l + 64, ... so that every
// load and store of the wave covers 64 consecutive elements.  No lane leaves early (the ragged last tile is predicated inside
// ew_inv_lane): the zero count is summed over the wave and added to *zeros by one lane, one atomic a wave that met a zero.
template <int NL, int NW, int E>
__global__ void __launch_bounds__(256) k_ew_inv(const FpParams<NL> P, const uint32_t *in, uint32_t *out, int64_t count, int32_t *zeros) {
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    int z = ew_inv_lane<NL, NW, E>(in, out, wave * (64 * E) + lane, 64, count, P);
    if (zeros) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) z += __shfl_xor(z, o, 64);
        if (lane == 0 && z) atomicAdd(zeros, z);
    }
}

// host: the same rows (the inversion: the same lane function, tile by tile) over `count` elements
template <int NL, int NW>
static int selftest_ew(const uint64_t *p_limbs, int what, const uint64_t *const *ops, uint64_t *out, int64_t count) {
    FpParams<NL> P;
    fp_params_from_limbs(P, p_limbs);
    const int op = what & 0xff;
    const bool bcast = (what & HB_EW_SELFTEST_BROADCAST) != 0;
    uint32_t *o = u32(out);
    if (op == HB_EW_SELFTEST_INV) {
        constexpr int E = EwTile<NL>::E;
        uint64_t zeros = 0;
        for (int64_t tile = 0; tile * (64 * E) < count; tile++)
            for (int lane = 0; lane < 64; lane++)
                zeros += (uint64_t)ew_inv_lane<NL, NW, E>(reinterpret_cast<const uint32_t *>(ops[0]), o, tile * (64 * E) + lane, 64, count, P);
        if (ops[1]) *const_cast<uint64_t *>(ops[1]) = zeros;
        return HB_OK;
    }
    if (op == HB_EW_SELFTEST_BEAVER) {
        const EwBeaverArgs A = {u32(ops[0]), u32(ops[1]), u32(ops[2]), u32(ops[3]), u32(ops[4]), o};
        host_rows<EwBeaverRow, NL, NW>(A, 1, count, P);
        return HB_OK;
    }
    const EwBinaryArgs A = {u32(ops[0]), u32(ops[1]), o};
    return with_binary_row(op, bcast, [&](auto row) { host_rows<decltype(row), NL, NW>(A, 1, count, P); return (int)HB_OK; });
}

}  // namespace hb

extern "C" {

int hb_ew_op(hb_ctx *ctx, int op, const uint64_t *a_dev, const uint64_t *b_dev, int b_broadcast, uint64_t *out_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0) return HB_ERR_BAD_ARG;
    if (op != HB_EW_ADD && op != HB_EW_SUB && op != HB_EW_MUL && op != HB_EW_NEG) return fail(ctx, HB_ERR_BAD_ARG, "hb_ew_op: unknown op");
    if (count > 0 && (!a_dev || !out_dev || (op != HB_EW_NEG && !b_dev))) return HB_ERR_BAD_ARG;
    // a broadcast operand is read by every wave of the launch: it cannot also be the output of more than its own element
    if (op != HB_EW_NEG && b_broadcast && count > 1 && out_dev == b_dev) return fail(ctx, HB_ERR_BAD_ARG, "hb_ew_op: out aliases the broadcast operand");
    if (count == 0) return HB_OK;
    HB_ROW_BLOCKS(ctx, "hb_ew_op");
    const EwBinaryArgs A = {u32(a_dev), u32(b_dev), u32(out_dev)};
    return with_binary_row(op, b_broadcast != 0, [&](auto row) { return launch_rows<decltype(row)>(ctx, A, (unsigned)blocks, s, count); });
}

int hb_ew_beaver(hb_ctx *ctx, const uint64_t *d_dev, const uint64_t *e_dev, const uint64_t *p_dev, const uint64_t *q_dev, const uint64_t *pq_dev,
                 uint64_t *out_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0) return HB_ERR_BAD_ARG;
    if (count > 0 && (!d_dev || !e_dev || !p_dev || !q_dev || !pq_dev || !out_dev)) return HB_ERR_BAD_ARG;
    if (count == 0) return HB_OK;
    HB_ROW_BLOCKS(ctx, "hb_ew_beaver");
    const EwBeaverArgs A = {u32(d_dev), u32(e_dev), u32(p_dev), u32(q_dev), u32(pq_dev), u32(out_dev)};
    return launch_rows<EwBeaverRow>(ctx, A, (unsigned)blocks, s, count);
}

int hb_ew_inv(hb_ctx *ctx, const uint64_t *in_dev, uint64_t *out_dev, int64_t count, int32_t *zeros_dev, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0) return HB_ERR_BAD_ARG;
    if (count > 0 && (!in_dev || !out_dev)) return HB_ERR_BAD_ARG;
    if (count == 0) return HB_OK;
    const int E = ctx->n_limbs == 4 ? EwTile<9>::E : EwTile<3>::E;
    const int64_t tiles = (count + 64 * E - 1) / (64 * E);
    const int64_t blocks = (tiles + 3) / 4;
    if (blocks > 0x7fffffffLL) return fail(ctx, HB_ERR_UNSUPPORTED, "hb_ew_inv: batch too large for one launch");
    hipStream_t s = (hipStream_t)stream;
    HB_DISPATCH(ctx,
        (k_ew_inv<9, 8, EwTile<9>::E><<<(unsigned)blocks, 256, 0, s>>>(ctx->pw, (const uint32_t *)in_dev, (uint32_t *)out_dev, count, zeros_dev)),
        (k_ew_inv<3, 2, EwTile<3>::E><<<(unsigned)blocks, 256, 0, s>>>(ctx->pn, (const uint32_t *)in_dev, (uint32_t *)out_dev, count, zeros_dev)));
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_selftest_ew(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *operands, uint64_t *out, int64_t count) {
    if (!p_limbs || !operands || count < 0 || (count > 0 && !out)) return HB_ERR_BAD_ARG;
    const int op = what & 0xff;
    if (op > HB_EW_SELFTEST_INV || (what & ~(0xff | HB_EW_SELFTEST_BROADCAST))) return HB_ERR_BAD_ARG;
    const int n_ops = op == HB_EW_SELFTEST_BEAVER ? 5 : (op == HB_EW_NEG || op == HB_EW_SELFTEST_INV) ? 1 : 2;
    for (int k = 0; k < n_ops; k++) if (count > 0 && !operands[k]) return HB_ERR_BAD_ARG;
    if (n_limbs == 4) return selftest_ew<9, 8>(p_limbs, what, operands, out, count);
    if (n_limbs == 1) return selftest_ew<3, 2>(p_limbs, what, operands, out, count);
    return HB_ERR_BAD_ARG;
}

}  // extern "C"

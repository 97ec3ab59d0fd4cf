// hb_offsb.hip -- the local arithmetic of the share bits of the offline phase (honeybadgermpc_amd/offline.py: share_bits_round,
// generate_share_bits): a random residue r shared together with its bit planes, what share_comparison.less_than
// consumes.  The reference has no generator for them (its preprocessing.py deals them, get_share_bits); the protocol is rejection
// sampling of a bitwise-shared value: L = bit_length(p) shared random bits are a candidate r = sum_i 2^i b_i < 2^L, kept when r < p.
// The test [r > p - 1] is the comparison of hb_lt.hip against a PUBLIC value that is the same for every candidate, so its leaves take
// their public bit from a bound held by value; the tree over them is hb_fxp.hip's, unchanged, and its root is opened.
//
// The steps are rows under the generic kernel k_rows (hb_rows.hpp):
//   SbLeavesRow   (g, p), L planes each, most significant bit first: plane y of candidate i is the DIRECT leaf (lt_leaf_elem,
//                 hb_lt_elem.hpp) of bit L - 1 - y of the bound against bits[L - 1 - y][i]: bound bit 0 -> (b, 1 - b), 1 -> (0, b).  The
//                 bound's bit is word_bit on the packed words in the argument struct: no array of c is read or made.
//   SbFinishRow   after the verdicts are open: output slot j takes candidate index[j].  The L planes are walked from the most
//                 significant down: r_bits[q][j] = bits[q][index[j]] and r <- 2 r + b_q, r[j] stored at the end -- the gather of the kept
//                 planes and the composition of r in ONE pass over them; nothing is computed for a rejected candidate.  The loads of
//                 SB_UNROLL planes are issued together, ahead of the additions that consume them.  An index outside [0, candidates)
//                 is never used as an address: its slot gets zeros in r and in every plane.
// Operands and results are packed canonical residues; every array of elements is read once (mem.once).  host_rows runs the very same
// functions -- index arithmetic included -- on host memory for hb_selftest_off_share_bits.
//
// Launch shape: k_rows (256-thread workgroups, one element a thread in x, no LDS, no grid stride), one launch a call.  SbLeavesRow takes
// the plane in blockIdx.y: grid = (ceil(count / 256), L); SbFinishRow: grid = ceil(count / 256), a thread walks the L planes of its slot.
// Compiler's report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; scratch = 0 bytes for every kernel):
//   k_rows<SbLeavesRow, 9, 8>   33 VGPRs: 8 waves a SIMD       k_rows<SbLeavesRow, 3, 2>   12 VGPRs: 8 waves
//   k_rows<SbFinishRow, 9, 8>   79 VGPRs: 6 waves              k_rows<SbFinishRow, 3, 2>   46 VGPRs: 8 waves
// SbFinishRow<9, 8> holds SB_UNROLL = 4 planes of 8 words in flight beside the 9 digits of r: that is where its registers go.
#include "hb_common.hpp"
#include "hb_lt_elem.hpp"
#include "hb_rows.hpp"

using namespace hb;

namespace hb {

constexpr int SB_UNROLL = 4;                       // planes whose loads are in flight together in the finish

// g, p: L planes each; plane y holds bit L - 1 - y.  bound: the public value as packed words, by value (the narrow width reads two)
struct SbLeavesArgs { const uint32_t *bits; uint32_t *g, *p; uint32_t bound[8]; int L; };

struct SbLeavesRow {
    template <int NL, int NW, class Mem>
    HB_HD static void run(const SbLeavesArgs &A, int y, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
        const int bit = A.L - 1 - y;
        uint32_t cw[NW], bw[NW], gw[NW], pw[NW];
#pragma unroll
        for (int q = 0; q < NW; q++) cw[q] = A.bound[q];
        mem.once(bw, A.bits, (int64_t)bit * count + i);
        lt_leaf_elem<NL, NW>(gw, pw, word_bit<NW>(cw, bit), bw, HB_LT_DIRECT, P);
        mem.store(A.g, (int64_t)y * count + i, gw);
        mem.store(A.p, (int64_t)y * count + i, pw);
    }
};

// bits: (L, candidates); index: count slots; r: count; r_bits: (L, count)
struct SbFinishArgs { const uint32_t *bits; const int64_t *index; uint32_t *r, *r_bits; int64_t candidates; int L; };

// acc <- 2 acc + the packed bit share bw
template <int NL, int NW> HB_HD void sb_double_add(uint32_t (&acc)[NL], const uint32_t (&bw)[NW], const FpParams<NL> &P) {
    uint32_t b[NL], t[NL];
    unpack<NL, NW>(b, bw);
    fp_add<NL>(t, acc, acc, P);
    fp_add<NL>(acc, t, b, P);
}

struct SbFinishRow {
    template <int NL, int NW, class Mem>
    HB_HD static void run(const SbFinishArgs &A, int, int64_t j, int64_t count, const Mem &mem, const FpParams<NL> &P) {
        const int64_t c = A.index[j];
        uint32_t acc[NL], ow[NW];
        small_digits<NL>(acc, 0);
        if (c < 0 || c >= A.candidates) {                          // never an address: the slot is zeros
            pack<NL, NW>(ow, acc);
            for (int q = 0; q < A.L; q++) mem.store(A.r_bits, (int64_t)q * count + j, ow);
            mem.store(A.r, j, ow);
            return;
        }
        int q = A.L - 1;
        for (; (q + 1) % SB_UNROLL; q--) {                         // the planes above a multiple of SB_UNROLL, one by one
            uint32_t bw[NW];
            mem.once(bw, A.bits, (int64_t)q * A.candidates + c);
            mem.store(A.r_bits, (int64_t)q * count + j, bw);
            sb_double_add<NL, NW>(acc, bw, P);
        }
        for (; q >= 0; q -= SB_UNROLL) {                           // q + 1 is a multiple of SB_UNROLL: planes q .. q - SB_UNROLL + 1
            uint32_t bw[SB_UNROLL][NW];
#pragma unroll
            for (int u = 0; u < SB_UNROLL; u++) mem.once(bw[u], A.bits, (int64_t)(q - u) * A.candidates + c);
#pragma unroll
            for (int u = 0; u < SB_UNROLL; u++) mem.store(A.r_bits, (int64_t)(q - u) * count + j, bw[u]);
#pragma unroll
            for (int u = 0; u < SB_UNROLL; u++) sb_double_add<NL, NW>(acc, bw[u], P);
        }
        pack<NL, NW>(ow, acc);
        mem.store(A.r, j, ow);
    }
};

// ---------------------------------------------------------------- host side: what the entry points and the self test refuse
// The public bound as packed words: bound_limbs (n_limbs limbs on the host), or p - 1 where it is null.  False: not below 2^L.
static bool sb_bound(uint32_t (&words)[8], const uint64_t *bound_limbs, const uint64_t *p_limbs, int n_limbs, int L) {
    uint64_t b[4] = {0, 0, 0, 0};
    if (bound_limbs) {
        for (int l = 0; l < n_limbs; l++) b[l] = bound_limbs[l];
    } else {
        uint64_t borrow = 1;                                       // p - 1
        for (int l = 0; l < n_limbs; l++) {
            b[l] = p_limbs[l] - borrow;
            borrow = (borrow && p_limbs[l] == 0) ? 1 : 0;
        }
    }
    for (int i = L; i < 64 * n_limbs; i++)
        if ((b[i >> 6] >> (i & 63)) & 1u) return false;
    for (int q = 0; q < 8; q++) words[q] = (uint32_t)(b[q >> 1] >> (32 * (q & 1)));
    return true;
}

// leaves: bits, g, p are (L, count) of elements of elem_bytes
static bool sb_leaves_ok(const void *bits, const void *g, const void *p, int L, int p_bits, int64_t count, int64_t elem_bytes) {
    if (count < 0 || L != p_bits || L < 1) return false;
    if (count == 0) return true;
    if (!bits || !g || !p) return false;
    int64_t row;
    if (__builtin_mul_overflow(count, elem_bytes, &row) || row > INT64_MAX / L) return false;
    const RowSpan outs[2] = {{g, L}, {p, L}}, ins[1] = {{bits, L}};
    return outputs_apart(outs, 2, ins, 1, row);
}

// finish: bits (L, candidates), index int64[count], r count, r_bits (L, count)
static bool sb_finish_ok(const void *bits, const void *index, const void *r, const void *r_bits, int L, int p_bits, int64_t candidates, int64_t count,
                         int64_t elem_bytes) {
    if (count < 0 || candidates < 0 || L != p_bits || L < 1) return false;
    if (count == 0) return true;
    if (!index || !r || !r_bits || (candidates > 0 && !bits)) return false;
    int64_t in_row, out_row;
    if (__builtin_mul_overflow(candidates, elem_bytes, &in_row) || in_row > INT64_MAX / L) return false;
    if (__builtin_mul_overflow(count, elem_bytes, &out_row) || out_row > INT64_MAX / L) return false;
    const int64_t in_bytes = in_row * L, planes_bytes = out_row * L, index_bytes = count * 8;
    return !overlap(r, out_row, r_bits, planes_bytes) && !overlap(r, out_row, bits, in_bytes) && !overlap(r, out_row, index, index_bytes) &&
           !overlap(r_bits, planes_bytes, bits, in_bytes) && !overlap(r_bits, planes_bytes, index, index_bytes);
}

}  // namespace hb

extern "C" {

int hb_off_sb_leaves(hb_ctx *ctx, const uint64_t *bits_dev, int L, const uint64_t *bound_limbs, uint64_t *g_dev, uint64_t *p_dev, int64_t count, void *stream) {
    HB_API_GUARD(ctx);
    if (!ctx) return HB_ERR_BAD_ARG;
    if (!sb_leaves_ok(bits_dev, g_dev, p_dev, L, modulus_bits(ctx->p_limbs, ctx->n_limbs), count, 8 * ctx->n_limbs))
        return fail(ctx, HB_ERR_BAD_ARG, "hb_off_sb_leaves: null operand, count < 0, L not the bit length of the modulus, or g, p not arrays of their own");
    SbLeavesArgs A{u32(bits_dev), u32(g_dev), u32(p_dev), {}, L};
    if (!sb_bound(A.bound, bound_limbs, ctx->p_limbs, ctx->n_limbs, L)) return fail(ctx, HB_ERR_BAD_ARG, "hb_off_sb_leaves: the bound must be below 2^L");
    if (count == 0) return HB_OK;
    HB_ROW_BLOCKS(ctx, "hb_off_sb_leaves");
    return launch_rows<SbLeavesRow>(ctx, A, dim3((unsigned)blocks, (unsigned)L), s, count);
}

int hb_off_sb_finish(hb_ctx *ctx, const uint64_t *bits_dev, int L, int64_t candidates, const int64_t *index_dev, uint64_t *r_dev, uint64_t *r_bits_dev, int64_t count,
                     void *stream) {
    HB_API_GUARD(ctx);
    if (!ctx) return HB_ERR_BAD_ARG;
    if (!sb_finish_ok(bits_dev, index_dev, r_dev, r_bits_dev, L, modulus_bits(ctx->p_limbs, ctx->n_limbs), candidates, count, 8 * ctx->n_limbs))
        return fail(ctx, HB_ERR_BAD_ARG, "hb_off_sb_finish: null operand, negative size, L not the bit length of the modulus, or r, r_bits not arrays of their own");
    if (count == 0) return HB_OK;
    HB_ROW_BLOCKS(ctx, "hb_off_sb_finish");
    const SbFinishArgs A{u32(bits_dev), index_dev, u32(r_dev), u32(r_bits_dev), candidates, L};
    return launch_rows<SbFinishRow>(ctx, A, dim3((unsigned)blocks), s, count);
}

int hb_selftest_off_share_bits(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *bits, int L, const uint64_t *bound_limbs, int64_t candidates,
                               const int64_t *index, uint64_t *out0, uint64_t *out1, int64_t count) {
    if (!p_limbs || (n_limbs != 1 && n_limbs != 4) || (what != HB_OFF_SB_SELFTEST_LEAVES && what != HB_OFF_SB_SELFTEST_FINISH)) return HB_ERR_BAD_ARG;
    const int p_bits = modulus_bits(p_limbs, n_limbs);
    SbLeavesArgs LA{u32(bits), u32(out0), u32(out1), {}, L};
    if (what == HB_OFF_SB_SELFTEST_LEAVES) {
        if (!sb_leaves_ok(bits, out0, out1, L, p_bits, count, 8 * n_limbs) || !sb_bound(LA.bound, bound_limbs, p_limbs, n_limbs, L)) return HB_ERR_BAD_ARG;
    } else if (!sb_finish_ok(bits, index, out0, out1, L, p_bits, candidates, count, 8 * n_limbs)) {
        return HB_ERR_BAD_ARG;
    }
    if (count == 0) return HB_OK;
    const SbFinishArgs FA{u32(bits), index, u32(out0), u32(out1), candidates, L};
    if (n_limbs == 4) {
        FpParams<9> P;
        fp_params_from_limbs(P, p_limbs);
        if (what == HB_OFF_SB_SELFTEST_LEAVES) host_rows<SbLeavesRow, 9, 8>(LA, L, count, P);
        else host_rows<SbFinishRow, 9, 8>(FA, 1, count, P);
    } else {
        FpParams<3> P;
        fp_params_from_limbs(P, p_limbs);
        if (what == HB_OFF_SB_SELFTEST_LEAVES) host_rows<SbLeavesRow, 3, 2>(LA, L, count, P);
        else host_rows<SbFinishRow, 3, 2>(FA, 1, count, P);
    }
    return HB_OK;
}

}  // extern "C"

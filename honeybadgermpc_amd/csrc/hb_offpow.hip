// hb_offpow.hip -- the local arithmetic of the shared powers and cubes of the offline phase (honeybadgermpc_amd/offline.py:
// generate_powers, generate_cubes).  The reference has no generator for either (its preprocessing.py deals them);
// the protocol grows b^1 .. b^k by doubling: with b^1 .. b^m held, level (m, w), w <= m, makes b^(m+1+j) = b^m b^(j+1) for j < w by
// degree reduction -- mask, one open at degree 2t, finish.  The two launches of a level are the kernels here.
//
// The powers of `count` items live in one array: power e (1-based) of item c is element c item_stride + (e - 1) power_stride (strides
// in elements; (k, 1) is item-major, (1, count) power-major).  The flat index e in [0, count w) is item c = e / w and product j = e % w,
// so what a level sends to the open and gets back from it is contiguous:
//   PowMaskRow    out[c w + j] = P[c][m] P[c][j+1] + r2t[c w + j]: the factor P[c][m] is shared by the w lanes of an item (one address, one
//                 cache line), P[c][j+1] and r2t are one element a lane, r2t read once.  j + 1 = m is the square: the element is loaded
//                 once and multiplied by itself.
//   PowFinishRow  P[c][m+1+j] = opened[c w + j] - rt[c w + j]: both read once; columns m .. m + w - 1 (0-based) alone are written.
// Operands and results are packed canonical residues.  The rows are hb_rows.hpp's: k_rows runs them on the device, host_rows runs the
// very same functions -- index arithmetic included -- on host memory for hb_selftest_off_powers.
//
// Launch shape: k_rows (256-thread workgroups, one element a thread, grid = ceil(count w / 256), no LDS, no grid stride), one launch
// a call.  c = e / w is a 32-bit division where count w < 2^32 (a wave-uniform choice).
// Compiler's report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; scratch = 0 bytes for every kernel):
//   k_rows<PowMaskRow, 9, 8>    63 VGPRs: 8 waves a SIMD       k_rows<PowMaskRow, 3, 2>    20 VGPRs: 8 waves
//   k_rows<PowFinishRow, 9, 8>  28 VGPRs: 8 waves              k_rows<PowFinishRow, 3, 2>  13 VGPRs: 8 waves
#include "hb_common.hpp"
#include "hb_ew_elem.hpp"
#include "hb_rows.hpp"

using namespace hb;

namespace hb {

struct PowArgs {
    const uint32_t *powers;        // read by the mask
    uint32_t *powers_out;          // written by the finish
    const uint32_t *x, *r;         // mask: r = r2t; finish: x = opened, r = rt
    uint32_t *out;                 // mask: the masked products
    int64_t item_stride, power_stride;
    int m, w;
};

// flat index e -> (item, product); the cell of power q (0-based) of item c
HB_HD void pow_split(int64_t e, int64_t total, int w, int64_t &c, int &j) {
    c = total <= 0xffffffffLL ? (int64_t)((uint32_t)e / (uint32_t)w) : e / w;
    j = (int)(e - c * w);
}
HB_HD int64_t pow_cell(const PowArgs &A, int64_t c, int q) { return c * A.item_stride + (int64_t)q * A.power_stride; }

// The masked product a b + c is ew_mul_add_elem of hb_ew_elem.hpp (hb_off.hip's OffMulAddRow computes the same).
struct PowMaskRow {
    template <int NL, int NW, class Mem> HB_HD static void run(const PowArgs &A, int, int64_t e, int64_t total, const Mem &mem, const FpParams<NL> &P) {
        int64_t c;
        int j;
        pow_split(e, total, A.w, c, j);
        uint32_t a[NW], b[NW], r[NW], o[NW];
        mem.load(a, A.powers, pow_cell(A, c, A.m - 1));
        if (j + 1 == A.m) {                                        // the square: the one element, loaded once
#pragma unroll
            for (int q = 0; q < NW; q++) b[q] = a[q];
        } else {
            mem.load(b, A.powers, pow_cell(A, c, j));
        }
        mem.once(r, A.r, e);
        ew_mul_add_elem<NL, NW>(o, a, b, r, P);
        mem.store(A.out, e, o);
    }
};

struct PowFinishRow {
    template <int NL, int NW, class Mem> HB_HD static void run(const PowArgs &A, int, int64_t e, int64_t total, const Mem &mem, const FpParams<NL> &P) {
        int64_t c;
        int j;
        pow_split(e, total, A.w, c, j);
        uint32_t v[NW], r[NW], o[NW];
        mem.once(v, A.x, e);
        mem.once(r, A.r, e);
        diff_elem<NL, NW>(o, v, r, P);
        mem.store(A.powers_out, pow_cell(A, c, A.m + j), o);
    }
};

// ---------------------------------------------------------------- host side: what both entry points and the self test refuse
static int64_t pow_gcd(int64_t a, int64_t b) {
    while (b) { const int64_t t = a % b; a = b; b = t; }
    return a;
}

// The arguments of one level over elements of elem_bytes; *total = count w.  False: HB_ERR_BAD_ARG.
// Strides are positive.  Two cells (c, q), (c', q') of the count x (m + w) block share an element iff dc item_stride = dq power_stride
// has a solution with 0 < dc < count, 0 < dq < m + w, and the smallest one is (power_stride, item_stride) / gcd.
static bool pow_args_ok(int what, const void *powers, int64_t item_stride, int64_t power_stride, const void *x, const void *r, const void *out, int m, int w,
                        int64_t count, int64_t elem_bytes, int64_t *total) {
    if (count < 0 || m < 1 || w < 1 || w > m) return false;
    if (__builtin_mul_overflow(count, (int64_t)w, total)) return false;
    if (count == 0) return true;                                   // (no cell: the power-major stride of no item is 0)
    if (item_stride < 1 || power_stride < 1) return false;
    const int64_t cols = (int64_t)m + w, g = pow_gcd(item_stride, power_stride);
    if (power_stride / g < count && item_stride / g < cols) return false;
    if (!powers || !r || (what == 0 ? !out : !x)) return false;
    // the block's extent in bytes, and the extent of the columns the finish writes
    int64_t last_item, last_col, first_written, span, bytes, written_at, all_bytes;
    if (__builtin_mul_overflow(count - 1, item_stride, &last_item) || __builtin_mul_overflow(cols - 1, power_stride, &last_col) ||
        __builtin_mul_overflow((int64_t)m, power_stride, &first_written) || __builtin_add_overflow(last_item, last_col, &span) ||
        __builtin_add_overflow(span, (int64_t)1, &span) || __builtin_mul_overflow(span, elem_bytes, &bytes) ||
        __builtin_mul_overflow(first_written, elem_bytes, &written_at) || __builtin_mul_overflow(*total, elem_bytes, &all_bytes))
        return false;
    if (what == 0) return !overlap(out, all_bytes, powers, bytes) && !overlap(out, all_bytes, r, all_bytes);
    const char *wr = (const char *)powers + written_at;
    return !overlap(x, all_bytes, wr, bytes - written_at) && !overlap(r, all_bytes, wr, bytes - written_at);
}

template <class Row> static int pow_launch(hb_ctx *ctx, const PowArgs &A, int64_t count, void *stream) {
    HB_ROW_BLOCKS(ctx, "hb_off_pow");
    return launch_rows<Row>(ctx, A, dim3((unsigned)blocks), s, count);
}

}  // namespace hb

extern "C" {

int hb_off_pow_mask(hb_ctx *ctx, const uint64_t *powers_dev, int64_t item_stride, int64_t power_stride, const uint64_t *r2t_dev, int m, int w, uint64_t *out_dev,
                    int64_t count, void *stream) { HB_API_GUARD(ctx);
    int64_t total = 0;
    if (!ctx || !pow_args_ok(0, powers_dev, item_stride, power_stride, nullptr, r2t_dev, out_dev, m, w, count, 8 * ctx->n_limbs, &total))
        return fail(ctx, HB_ERR_BAD_ARG, "hb_off_pow_mask: null operand, count < 0, not 1 <= w <= m, aliasing strides or overlapping output");
    if (total == 0) return HB_OK;
    PowArgs A{u32(powers_dev), nullptr, nullptr, u32(r2t_dev), u32(out_dev), item_stride, power_stride, m, w};
    return pow_launch<PowMaskRow>(ctx, A, total, stream);
}

int hb_off_pow_finish(hb_ctx *ctx, const uint64_t *opened_dev, const uint64_t *rt_dev, uint64_t *powers_dev, int64_t item_stride, int64_t power_stride, int m, int w,
                      int64_t count, void *stream) { HB_API_GUARD(ctx);
    int64_t total = 0;
    if (!ctx || !pow_args_ok(1, powers_dev, item_stride, power_stride, opened_dev, rt_dev, nullptr, m, w, count, 8 * ctx->n_limbs, &total))
        return fail(ctx, HB_ERR_BAD_ARG, "hb_off_pow_finish: null operand, count < 0, not 1 <= w <= m, aliasing strides or overlapping input");
    if (total == 0) return HB_OK;
    PowArgs A{nullptr, u32(powers_dev), u32(opened_dev), u32(rt_dev), nullptr, item_stride, power_stride, m, w};
    return pow_launch<PowFinishRow>(ctx, A, total, stream);
}

int hb_selftest_off_powers(const uint64_t *p_limbs, int n_limbs, int what, uint64_t *powers, int64_t item_stride, int64_t power_stride, const uint64_t *x,
                           const uint64_t *r, int m, int w, uint64_t *out, int64_t count) {
    int64_t total = 0;
    if (!p_limbs || (n_limbs != 1 && n_limbs != 4) || (what != HB_OFF_POWERS_SELFTEST_MASK && what != HB_OFF_POWERS_SELFTEST_FINISH)) return HB_ERR_BAD_ARG;
    if (!pow_args_ok(what, powers, item_stride, power_stride, x, r, out, m, w, count, 8 * n_limbs, &total)) return HB_ERR_BAD_ARG;
    if (total == 0) return HB_OK;
    PowArgs A{u32(powers), u32(powers), u32(x), u32(r), u32(out), item_stride, power_stride, m, w};
    if (n_limbs == 4) {
        FpParams<9> P;
        fp_params_from_limbs(P, p_limbs);
        if (what == HB_OFF_POWERS_SELFTEST_MASK) host_rows<PowMaskRow, 9, 8>(A, 1, total, P);
        else host_rows<PowFinishRow, 9, 8>(A, 1, total, P);
    } else {
        FpParams<3> P;
        fp_params_from_limbs(P, p_limbs);
        if (what == HB_OFF_POWERS_SELFTEST_MASK) host_rows<PowMaskRow, 3, 2>(A, 1, total, P);
        else host_rows<PowFinishRow, 3, 2>(A, 1, total, P);
    }
    return HB_OK;
}

}  // extern "C"

// hb_sort.hip -- oblivious sort of shared values: the three fused steps between the opens of one layer of Batcher's merge exchange
// (Knuth 5.2.2, Algorithm M; progs/sorting.py has the network).  A table is `width` columns of `batch` arrays of n rows, column-major:
// table[w][b n + i], column 0 the key.  A layer (a, r, d, cnt) compares, in every array, rows lo(e) and lo(e) + d for e < cnt with
// lo(e) = ((e >> a) << (a + 1)) | (e & (2^a - 1)) | r: a closed form, so the kernels read no index list.  Slot s of the layer is array
// s / cnt, comparator s % cnt; every array a step reads or writes beside the table has `slots` = batch cnt elements a row, no holes.
//
// The comparison is FixedPoint.lt on the difference of the keys (hb_fxp.hip): open c = d + 2^(k-1) + r1 + 2^(k-1) r2, take the carry
// of (c mod 2^(k-1)) against r1 out of the tree (hb_fxp_ltl_leaves, hb_fxp_carry_mask / hb_fxp_carry_combine: unchanged), and
// [d < 0] = ((c mod 2^(k-1)) - r1 + 2^(k-1) (1 - carry) - d) 2^(-(k-1)).  The steps are rows under k_rows (hb_rows.hpp):
// SortCmpMaskRow     d = key[lo] - key[hi], then fxp_mask_elem over the slot's k + kappa bit planes: writes c's share and r1.  Two key
//                    reads, k + kappa plane reads, two writes a slot -- what two gathers, a subtraction and hb_fxp_mask did in four launches.
// SortSwapMaskRow    after the tree's root: u = 1 - [d < 0] = [key_lo >= key_hi] ONCE a slot (fxp_finish_elem, HB_FXP_NEG_TRUNC, and the
//                    affine map; the bit is never stored), then for every column w rows 2w, 2w + 1 = u - p_w, (T[w][lo] - T[w][hi]) - q_w of
//                    the array to open.  Column 0's difference is d: the keys are read once.
// SortSwapFinishRow  for every column: m = de + dq + ep + pq = [u (T[w][lo] - T[w][hi])] (ew_beaver_elem), T[w][lo] -= m, T[w][hi] += m,
//                    IN PLACE.  That is safe because a layer is a matching: bit a of lo + d differs from bit a of lo (d is an odd
//                    multiple of 2^a: sort_layer_ok), so no row is written by one slot and read or written by another, and a thread
//                    loads its two rows before it stores them.  Rows no comparator touches are never written.
//
// Launch shape: 256-thread workgroups, one slot a thread in x, nothing in blockIdx.y (batch is folded into the slot index: it may
// exceed 65535).  No LDS, no grid stride, no waiting between workgroups, one launch a call.  Planes, triples and opened values are
// read once: the 32-byte width takes the non-temporal loads (mem.once), the table the plain ones.
// Compiler's report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; scratch = 0 bytes for every kernel):
//   SortCmpMaskRow<9, 8>      88 VGPRs: 5 waves a SIMD        SortCmpMaskRow<3, 2>      34 VGPRs: 8 waves
//   SortSwapMaskRow<9, 8>     64 VGPRs: 8 waves               SortSwapMaskRow<3, 2>     30 VGPRs: 8 waves
//   SortSwapFinishRow<9, 8>   88 VGPRs: 5 waves               SortSwapFinishRow<3, 2>   38 VGPRs: 8 waves
// (DESIGN.md section 3z has the network, the layout and the counts.)
#include "hb_common.hpp"
#include "hb_sort_elem.hpp"

using namespace hb;

namespace hb {

// ---------------------------------------------------------------- the steps' rows (host and device, over a memory policy: hb_rows.hpp)
// i = the slot, count = the slots; the table's column w begins at element w * plane
template <int NL> struct SortCmpMaskArgs { const uint32_t *table, *bits; uint32_t *masked, *r1; SortLayer L; int nbits, m; FpConst<NL> half; };

struct SortCmpMaskRow {
    template <int NL, int NW, class Mem>
    HB_HD static void run(const SortCmpMaskArgs<NL> &A, int, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
        int64_t lo, hi;
        sort_slot_rows(A.L, i, lo, hi);
        uint32_t xw[NW], yw[NW], dw[NW], o0[NW], o1[NW];
        mem.load(xw, A.table, lo); mem.load(yw, A.table, hi);
        diff_elem<NL, NW>(dw, xw, yw, P);
        fxp_mask_elem<NL, NW, true>(o0, o1, dw, [&](uint32_t (&w)[NW], int row) { mem.once(w, A.bits, (int64_t)row * count + i); }, A.nbits, A.m, A.half.d, P);
        mem.store(A.masked, i, o0);
        mem.store(A.r1, i, o1);
    }
};

template <int NL> struct SortSwapMaskArgs { const uint32_t *table, *c, *r1, *carry, *p, *q; uint32_t *out; SortLayer L; int width, m; FxpFinishConsts<NL> K; };

struct SortSwapMaskRow {
    template <int NL, int NW, class Mem>
    HB_HD static void run(const SortSwapMaskArgs<NL> &A, int, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
        int64_t lo, hi;
        sort_slot_rows(A.L, i, lo, hi);
        uint32_t xw[NW], yw[NW], dw[NW], cw[NW], rw[NW], kw[NW], uw[NW], o0[NW], o1[NW];
        mem.load(xw, A.table, lo); mem.load(yw, A.table, hi);
        diff_elem<NL, NW>(dw, xw, yw, P);
        mem.once(cw, A.c, i); mem.once(rw, A.r1, i); mem.once(kw, A.carry, i);
        sort_swap_bit_elem<NL, NW>(uw, dw, cw, rw, kw, A.m, A.K, P);
        for (int w = 0; w < A.width; w++) {
            if (w) {
                mem.load(xw, A.table, (int64_t)w * A.L.plane + lo); mem.load(yw, A.table, (int64_t)w * A.L.plane + hi);
                diff_elem<NL, NW>(dw, xw, yw, P);
            }
            mem.once(xw, A.p, (int64_t)w * count + i); mem.once(yw, A.q, (int64_t)w * count + i);
            diff_elem<NL, NW>(o0, uw, xw, P);
            diff_elem<NL, NW>(o1, dw, yw, P);
            mem.store(A.out, (int64_t)(2 * w) * count + i, o0);
            mem.store(A.out, (int64_t)(2 * w + 1) * count + i, o1);
        }
    }
};

struct SortSwapFinishArgs { uint32_t *table; const uint32_t *opened, *p, *q, *pq; SortLayer L; int width; };

struct SortSwapFinishRow {
    template <int NL, int NW, class Mem>
    HB_HD static void run(const SortSwapFinishArgs &A, int, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P) {
        int64_t lo, hi;
        sort_slot_rows(A.L, i, lo, hi);
        uint32_t dw[NW], ew[NW], pw[NW], qw[NW], pqw[NW], mw[NW], xw[NW], yw[NW];
        for (int w = 0; w < A.width; w++) {
            const int64_t t = (int64_t)w * count + i, col = (int64_t)w * A.L.plane;
            mem.once(dw, A.opened, (int64_t)(2 * w) * count + i); mem.once(ew, A.opened, (int64_t)(2 * w + 1) * count + i);
            mem.once(pw, A.p, t); mem.once(qw, A.q, t); mem.once(pqw, A.pq, t);
            ew_beaver_elem<NL, NW>(mw, dw, ew, pw, qw, pqw, P);
            mem.load(xw, A.table, col + lo); mem.load(yw, A.table, col + hi);                // both loads ahead of the stores
            sort_exchange_elem<NL, NW>(xw, yw, mw, P);
            mem.store(A.table, col + lo, xw);
            mem.store(A.table, col + hi, yw);
        }
    }
};

// ---------------------------------------------------------------- host side
// One step function a step (hb_rows.hpp): its checks, Args fill and row count run under a DeviceRun in the entry point, a HostRun in hb_selftest_sort.
static bool sort_width_ok(int width) { return width >= 1 && width <= 256; }

// k and kappa as hb_fxp_mask checks them with m = k - 1
static bool sort_params_ok(int bits, int k, int kappa) { return k >= 2 && fxp_params_ok(bits, k, k - 1, kappa); }

template <int NL> static bool sort_cmp_consts(SortCmpMaskArgs<NL> &A, const FpParams<NL> &P, int k, int kappa) {
    A.nbits = k + kappa; A.m = k - 1;
    fxp_pow2<NL>(A.half.d, k - 1, false, P);
    return true;
}
template <int NL> static bool sort_swap_consts(SortSwapMaskArgs<NL> &A, const FpParams<NL> &P, int k, const uint64_t *inv2m_host) {
    A.m = k - 1;
    return fxp_finish_fill<NL>(A.K, P, k - 1, HB_FXP_NEG_TRUNC, inv2m_host);
}

template <class Run> static int sort_cmp_mask_step(const Run &run, const uint64_t *table, int64_t n, int64_t batch, int a, int64_t r, int64_t d, int64_t cnt,
                                                   const uint64_t *bits, int k, int kappa, uint64_t *masked, uint64_t *r1) {
    SortLayer L;
    if (!sort_layer_ok(L, n, batch, a, r, d, cnt)) return run.fail(HB_ERR_BAD_ARG, "hb_sort_cmp_mask: not a layer of comparators inside n rows");
    if (!sort_params_ok(run.bits(), k, kappa))
        return run.fail(HB_ERR_BAD_ARG, "hb_sort_cmp_mask: needs k >= 2, kappa >= 0 and k + kappa + 1 <= bits(p) - 1");
    const int64_t count = batch * cnt, eb = run.elem_bytes();
    if (count > 0 && (!table || !bits || !masked || !r1)) return HB_ERR_BAD_ARG;
    if (count == 0) return HB_OK;
    if (overlap(masked, eb * count, r1, eb * count) || overlap(masked, eb * count, table, eb * L.plane) || overlap(r1, eb * count, table, eb * L.plane) ||
        overlap(masked, eb * count, bits, eb * count * (k + kappa)) || overlap(r1, eb * count, bits, eb * count * (k + kappa)))
        return run.fail(HB_ERR_BAD_ARG, "hb_sort_cmp_mask: masked and r1 are arrays of their own");
    return run.template rows<SortCmpMaskRow, SortCmpMaskArgs>([&](auto &A, const auto &P) {
        A.table = u32(table); A.bits = u32(bits); A.masked = u32(masked); A.r1 = u32(r1); A.L = L;
        return sort_cmp_consts(A, P, k, kappa);
    }, 1, count);
}

template <class Run> static int sort_swap_mask_step(const Run &run, const uint64_t *table, int width, int64_t n, int64_t batch, int a, int64_t r, int64_t d, int64_t cnt,
                                                    const uint64_t *c, const uint64_t *r1, const uint64_t *carry, const uint64_t *p, const uint64_t *q, int k,
                                                    const uint64_t *inv2m_host, uint64_t *out) {
    if (!inv2m_host) return HB_ERR_BAD_ARG;
    SortLayer L;
    if (!sort_layer_ok(L, n, batch, a, r, d, cnt)) return run.fail(HB_ERR_BAD_ARG, "hb_sort_swap_mask: not a layer of comparators inside n rows");
    if (!sort_width_ok(width)) return run.fail(HB_ERR_BAD_ARG, "hb_sort_swap_mask: needs 1 <= width <= 256");
    if (k < 2 || !fxp_m_ok(run.bits(), k - 1)) return run.fail(HB_ERR_BAD_ARG, "hb_sort_swap_mask: needs 2 <= k <= bits(p) - 1");
    const int64_t count = batch * cnt, eb = run.elem_bytes();
    if (count > 0 && (!table || !c || !r1 || !carry || !p || !q || !out)) return HB_ERR_BAD_ARG;
    const int64_t ob = eb * count * 2 * width;
    if (count > 0 && (overlap(out, ob, table, eb * L.plane * width) || overlap(out, ob, c, eb * count) || overlap(out, ob, r1, eb * count) ||
                      overlap(out, ob, carry, eb * count) || overlap(out, ob, p, eb * count * width) || overlap(out, ob, q, eb * count * width)))
        return run.fail(HB_ERR_BAD_ARG, "hb_sort_swap_mask: out is an array of its own");
    const int rc = run.template rows<SortSwapMaskRow, SortSwapMaskArgs>([&](auto &A, const auto &P) {
        A.table = u32(table); A.c = u32(c); A.r1 = u32(r1); A.carry = u32(carry); A.p = u32(p); A.q = u32(q); A.out = u32(out);
        A.L = L; A.width = width;
        return sort_swap_consts(A, P, k, inv2m_host);
    }, 1, count);
    return rc == HB_ERR_BAD_ARG ? run.fail(rc, "hb_sort_swap_mask: inv2m is not below the modulus") : rc;
}

template <class Run> static int sort_swap_finish_step(const Run &run, uint64_t *table, int width, int64_t n, int64_t batch, int a, int64_t r, int64_t d, int64_t cnt,
                                                      const uint64_t *opened, const uint64_t *p, const uint64_t *q, const uint64_t *pq) {
    SortLayer L;
    if (!sort_layer_ok(L, n, batch, a, r, d, cnt)) return run.fail(HB_ERR_BAD_ARG, "hb_sort_swap_finish: not a layer of comparators inside n rows");
    if (!sort_width_ok(width)) return run.fail(HB_ERR_BAD_ARG, "hb_sort_swap_finish: needs 1 <= width <= 256");
    const int64_t count = batch * cnt, eb = run.elem_bytes();
    if (count > 0 && (!table || !opened || !p || !q || !pq)) return HB_ERR_BAD_ARG;
    if (count == 0) return HB_OK;
    const int64_t tb = eb * L.plane * width;
    if (overlap(table, tb, opened, eb * count * 2 * width) || overlap(table, tb, p, eb * count * width) || overlap(table, tb, q, eb * count * width) ||
        overlap(table, tb, pq, eb * count * width))
        return run.fail(HB_ERR_BAD_ARG, "hb_sort_swap_finish: the table is an array of its own");
    const SortSwapFinishArgs A = {u32(table), u32(opened), u32(p), u32(q), u32(pq), L, width};
    return run.template rows<SortSwapFinishRow>(A, 1, count);
}

}  // namespace hb

extern "C" {

int hb_sort_cmp_mask(hb_ctx *ctx, const uint64_t *table_dev, int64_t n, int64_t batch, int a, int64_t r, int64_t d, int64_t cnt, const uint64_t *bits_dev, int k,
                     int kappa, uint64_t *masked_dev, uint64_t *r1_dev, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : sort_cmp_mask_step(DeviceRun{ctx, (hipStream_t)stream, "hb_sort_cmp_mask"}, table_dev, n, batch, a, r, d, cnt, bits_dev, k, kappa,
                                                      masked_dev, r1_dev);
}

int hb_sort_swap_mask(hb_ctx *ctx, const uint64_t *table_dev, int width, int64_t n, int64_t batch, int a, int64_t r, int64_t d, int64_t cnt, const uint64_t *c_dev,
                      const uint64_t *r1_dev, const uint64_t *carry_dev, const uint64_t *p_dev, const uint64_t *q_dev, int k, const uint64_t *inv2m_host,
                      uint64_t *out_dev, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : sort_swap_mask_step(DeviceRun{ctx, (hipStream_t)stream, "hb_sort_swap_mask"}, table_dev, width, n, batch, a, r, d, cnt, c_dev, r1_dev,
                                                       carry_dev, p_dev, q_dev, k, inv2m_host, out_dev);
}

int hb_sort_swap_finish(hb_ctx *ctx, uint64_t *table_dev, int width, int64_t n, int64_t batch, int a, int64_t r, int64_t d, int64_t cnt, const uint64_t *opened_dev,
                        const uint64_t *p_dev, const uint64_t *q_dev, const uint64_t *pq_dev, void *stream) { HB_API_GUARD(ctx);
    return !ctx ? HB_ERR_BAD_ARG : sort_swap_finish_step(DeviceRun{ctx, (hipStream_t)stream, "hb_sort_swap_finish"}, table_dev, width, n, batch, a, r, d, cnt,
                                                         opened_dev, p_dev, q_dev, pq_dev);
}

// params = {n, batch, width, a, r, d, cnt, k, kappa}
int hb_selftest_sort(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *ops, const int64_t *params, uint64_t *const *outs) {
    if (!p_limbs || !ops || !params || !outs || (n_limbs != 1 && n_limbs != 4)) return HB_ERR_BAD_ARG;
    for (int i = 0; i < 9; i++) if (params[i] < -((int64_t)1 << 41) || params[i] > ((int64_t)1 << 41)) return HB_ERR_BAD_ARG;
    const HostRun run = {p_limbs, n_limbs};
    const int64_t n = params[0], batch = params[1], r = params[4], d = params[5], cnt = params[6];
    const int width = (int)params[2], a = (int)params[3], k = (int)params[7], kappa = (int)params[8];
    switch (what) {
    case HB_SORT_SELFTEST_CMP_MASK: return sort_cmp_mask_step(run, ops[0], n, batch, a, r, d, cnt, ops[1], k, kappa, outs[0], outs[1]);
    case HB_SORT_SELFTEST_SWAP_MASK: return sort_swap_mask_step(run, ops[0], width, n, batch, a, r, d, cnt, ops[1], ops[2], ops[3], ops[4], ops[5], k, ops[6], outs[0]);
    case HB_SORT_SELFTEST_SWAP_FINISH: return sort_swap_finish_step(run, outs[0], width, n, batch, a, r, d, cnt, ops[0], ops[1], ops[2], ops[3]);
    default: return HB_ERR_BAD_ARG;
    }
}

}  // extern "C"

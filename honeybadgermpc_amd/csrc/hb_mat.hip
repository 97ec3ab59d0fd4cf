// hb_mat.hip -- products of share matrices: out[b] = A[b] B[b] (op) C[b] over GF(p) for `batch` independent products, A m x k, B k x n,
// C and out m x n, all row-major packed canonical residues in HBM, every operand used once.  The local step of both degree-reduction
// routes to a shared matrix product (honeybadgermpc_amd/linalg.py): X Y - r_2t is what the double-sharing route opens, and
// D (E + Q) + (P E + PQ) is what the matrix Beaver triple combines.  Arithmetic restated on fp29.hpp, not translated from anywhere.
//
// k_mat_mul     A workgroup of MAT_THREADS = 256 lanes owns one MAT_TM x MAT_TN = 16 x 32 tile of one product's output and (split path)
//               one slice of the inner dimension.  Per step of MAT_TK = 16 it stages a 16 x 16 tile of A and a 16 x 32 tile of B in LDS
//               as 29-bit digits -- unpacked once a tile, not once a product -- with zeros outside the matrices and outside the slice,
//               so no lane branches on an edge inside the inner loop.  Lane (ty, tx) = (tid / 16, tid % 16) keeps a 1 x MAT_RN = 1 x 2
//               register block: outputs (m0 + ty, n0 + tx) and (m0 + ty, n0 + tx + 16), each a 2 NL column accumulator; A's digits are
//               read once for both.
// k_mat_reduce  split path only: out = (sum over slices of the partial products) (op) C, one element a thread, field additions in
//               slice order (no float, no atomics, nothing waits for another workgroup).
//
// LDS layout.  Bs[q][kk][col], col < 32 (dword index (q MAT_TK + kk) 32 + col): the 16 lanes tx of a row read consecutive dwords, the
// four rows ty of a wave read the same ones -- 16 distinct banks of 64, the rest a broadcast -- and the second output reads the
// other 16.  As[q][kk][row] with a row stride of MAT_AS = 17 dwords: the four rows of a wave read four consecutive dwords, every tx the
// same (broadcast).  Staging writes: lane idx of the A tile is (row, kk) = (idx / 16, idx % 16), dword kk 17 + row; over a wave
// (kk < 16, four rows) these are 64 distinct values mod 64 (17 kk mod 64 = 0, 17, 34, 51, 4, 21, ...: sixteen runs of four that do
// not meet) -- the padding is there for the writes.  B's writes are 32 consecutive dwords per kk.  Global reads of a tile are runs
// of 16 (A) and 32 (B) consecutive elements.
//
// Lazy accumulation, as k_pm_direct (hb_pm.hip, whose derivation this restates and whose L is taken over unchanged).
//   Columns: a product of two NL-digit numbers adds at most NL terms below 2^58 to a column; GROUP = Lazy<NL>::GROUP products from a
//   carried state (columns < 2^29, the top one aside) stay below GROUP NL 2^58 + 2^30 < 2^64 (7 x 9 = 63 and 21 x 3 = 63 < 64).  The top
//   column receives carries only and ends below 2^(log2 L + 64 NW - 29 (2 NL - 1)) < 2^25.  A carry pass every GROUP products.
//   Value: with every operand below p, L products give T < L p^2, and REDC returns T / R + (< p) < p (1 + L p / R): below 2 p, one
//   conditional subtraction, iff L p <= R = 2^(29 NL).  p < 2^(32 NW) gives L <= 2^(29 NL - 32 NW) = 32 (NL = 9) and 2^23 (NL = 3); L is
//   4 GROUP = 28 and 84.  A REDC, one conditional subtraction and one modular addition into the lane's running sum every L products
//   (zero products of the padding count: they add nothing and keep the count wave-uniform).  The running sum is a sum of values T / R:
//   ONE product by R^2 at the end, then the epilogue on canonical digits (fp_add / fp_sub), then pack.
//   Every operand p - 1 with C = p - 1 at inner = L, L + 1, 4 L over 2^256 - 189 and 2^64 - 59 is the tight case (tests/test_linalg_host.py).
//
// Split over the inner dimension.  With W = batch * tiles workgroups of output: when W <= MAT_SPLIT_MAX_WGS = 64 and
// k >= MAT_SPLIT_MIN_K = 2048, the inner dimension is cut into S = min(MAT_SPLIT_TARGET_WGS / W, k / MAT_SPLIT_SLICE_K) slices
// (512, 1024; S >= 2 by the two conditions) of ceil(k / S) rounded up to whole MAT_TK steps.  Launch one (grid.y = S) writes
// canonical partial products to the per-stream scratch slot "mat:<stream>"; launch two adds them and applies the epilogue; both on the
// caller's stream with nothing in between.  Results are canonical residues either way: the same bits as the unsplit path.
// Scratch bound: S W <= 512 tiles of 16 x 32 elements = 8 MiB (32-byte elements), 2 MiB (8-byte).
//
// The per-tile bodies are HB_HD functions: the __global__ wrappers only load, call them and store, and hb_selftest_mat walks the same
// bodies over host memory workgroup by workgroup, lane by lane, split path included.
//
// Compiler's report (VGPRs, LDS bytes, scratch = 0 bytes for every instantiation) and the choice of the register block: below the kernels.
#include <algorithm>
#include <string>
#include <vector>

#include "hb_common.hpp"
#include "hb_rows.hpp"
#include "../../include/hbmpc_hip_debug.h"

using namespace hb;

namespace hb {

constexpr int MAT_THREADS = 256;
constexpr int MAT_TM = 16, MAT_TN = 32, MAT_TK = 16;
constexpr int MAT_RN = 2;                           // outputs a lane: columns tx and tx + 16 of its row
constexpr int MAT_TX = MAT_TN / MAT_RN;             // 16 lanes along a row
constexpr int MAT_AS = MAT_TM + 1;                  // row stride of the staged A tile (see the header: conflict-free staging writes)
constexpr int MAT_SPLIT_MAX_WGS = 64;               // split only when the output gives at most this many workgroups ...
constexpr int MAT_SPLIT_MIN_K = 2048;               // ... and the inner dimension is at least this long
constexpr int MAT_SPLIT_SLICE_K = 1024;             // shortest slice the automatic rule makes
constexpr int MAT_SPLIT_TARGET_WGS = 512;           // two workgroups a CU
static_assert(MAT_TM * MAT_TX == MAT_THREADS && MAT_TM * MAT_TK == MAT_THREADS, "one output row block and one A element a lane");
static int g_mat_split_mode = 0;                    // hb_debug_mat_split: 0 the rule above, 1 slices of one MAT_TK step, -1 never

template <int NL> struct MatAcc {
    static constexpr int GROUP = Lazy<NL>::GROUP;   // products between two carry passes
    static constexpr int L = 4 * GROUP;             // products between two reductions: PmAcc<NL>::L of hb_pm.hip
    static constexpr int NW = NL == 9 ? 8 : 2;
    static_assert(29 * NL - 32 * NW < 31 && L <= (1 << (29 * NL - 32 * NW)), "L p <= R for every p below 2^(32 NW)");
    static_assert((uint64_t)GROUP * NL < 64, "GROUP products fit a 64-bit column");
};

// what a lane carries through the inner dimension
template <int NL> struct MatLane {
    uint64_t c[MAT_RN][2 * NL];
    uint32_t acc[MAT_RN][NL];
};

// ---------------------------------------------------------------- bodies (host and device)
template <int NL> HB_HD void mat_lane_init(MatLane<NL> &s) {
#pragma unroll
    for (int r = 0; r < MAT_RN; r++) {
        col_zero(s.c[r]);
#pragma unroll
        for (int q = 0; q < NL; q++) s.acc[r][q] = 0;
    }
}
// carried columns -> acc += T / R, columns cleared
template <int NL> HB_HD void mat_lane_reduce(MatLane<NL> &s, const FpParams<NL> &P) {
#pragma unroll
    for (int r = 0; r < MAT_RN; r++) {
        uint32_t t[NL];
        redc(t, s.c[r], P);
        cond_sub_p(t, P);
        fp_add(s.acc[r], s.acc[r], t, P);
        col_zero(s.c[r]);
    }
}
// staging of one step by thread tid of nt: rows m0 .. of A and columns n0 .. of B at inner indices k0 .. k0 + MAT_TK - 1, zero at and
// beyond k_hi (the end of the slice) and outside the matrices.  A, B: this product's matrices.
template <int NL, int NW>
HB_HD void mat_stage(uint32_t *As, uint32_t *Bs, const uint32_t *A, const uint32_t *B, int m, int k, int n, int m0, int n0, int k0, int k_hi, int tid, int nt) {
    for (int idx = tid; idx < MAT_TM * MAT_TK + MAT_TK * MAT_TN; idx += nt) {
        const bool is_a = idx < MAT_TM * MAT_TK;                  // the same for every lane of a pass: MAT_TM * MAT_TK = the workgroup's size
        const int j = is_a ? idx : idx - MAT_TM * MAT_TK;
        const int row = is_a ? m0 + j / MAT_TK : 0, kk = is_a ? j % MAT_TK : j / MAT_TN, col = is_a ? 0 : n0 + j % MAT_TN;
        const bool in = k0 + kk < k_hi && (is_a ? row < m : col < n);
        uint32_t d[NL];
#pragma unroll
        for (int q = 0; q < NL; q++) d[q] = 0;
        if (in) load_digits<NL, NW>(d, is_a ? A + ((size_t)row * k + (k0 + kk)) * NW : B + ((size_t)(k0 + kk) * n + col) * NW);
        uint32_t *dst = is_a ? As + kk * MAT_AS + j / MAT_TK : Bs + kk * MAT_TN + j % MAT_TN;
        const int stride = is_a ? MAT_TK * MAT_AS : MAT_TK * MAT_TN;
#pragma unroll
        for (int q = 0; q < NL; q++) dst[q * stride] = d[q];
    }
}
// lane (ty, tx)'s share of one staged step: MAT_TK products into each of its outputs.  cnt: products since the last reduction, the same
// in every lane of the launch, so the carry and reduction tests are scalar branches.
template <int NL>
HB_HD void mat_step(MatLane<NL> &s, int &cnt, const uint32_t *As, const uint32_t *Bs, int ty, int tx, const FpParams<NL> &P) {
    constexpr int G = MatAcc<NL>::GROUP, L = MatAcc<NL>::L, UN = NL >= 9 ? 1 : 4;
#pragma unroll UN
    for (int kk = 0; kk < MAT_TK; kk++) {
        uint32_t a[NL], b[NL];
#pragma unroll
        for (int q = 0; q < NL; q++) a[q] = As[(q * MAT_TK + kk) * MAT_AS + ty];
#pragma unroll
        for (int r = 0; r < MAT_RN; r++) {
#pragma unroll
            for (int q = 0; q < NL; q++) b[q] = Bs[(q * MAT_TK + kk) * MAT_TN + tx + r * MAT_TX];
            mac<NL>(s.c[r], a, b);
        }
        cnt++;
        if (cnt % G == 0) {
#pragma unroll
            for (int r = 0; r < MAT_RN; r++) carry(s.c[r]);
        }
        if (cnt == L) { mat_lane_reduce<NL>(s, P); cnt = 0; }
    }
}
// after the last step: what is left in the columns
template <int NL> HB_HD void mat_lane_flush(MatLane<NL> &s, int cnt, const FpParams<NL> &P) {
    if (cnt == 0) return;
#pragma unroll
    for (int r = 0; r < MAT_RN; r++) carry(s.c[r]);
    mat_lane_reduce<NL>(s, P);
}
// (x) (op) c on canonical digits -> packed; cw is read before o is written (o may be cw)
template <int NL, int NW> HB_HD void mat_epilogue(uint32_t *o, const uint32_t (&x)[NL], const uint32_t *cw, int op, const FpParams<NL> &P) {
    uint32_t r[NL], cd[NL];
    fp_set(r, x);
    if (op != HB_MAT_NONE) {
        load_digits<NL, NW>(cd, cw);
        if (op == HB_MAT_ADD) fp_add(r, x, cd, P); else fp_sub(r, x, cd, P);
    }
    store_digits<NL, NW>(o, r);
}
// a running sum of values T / R -> the canonical sum, the epilogue, the store
template <int NL, int NW> HB_HD void mat_finish(uint32_t *o, const uint32_t (&acc)[NL], const uint32_t *cw, int op, const FpParams<NL> &P) {
    uint32_t x[NL];
    mont_mul(x, P.r2, acc, P);
    mat_epilogue<NL, NW>(o, x, cw, op, P);
}
// split path, one element: o = (sum_{s < S} part[s * stride]) (op) c
template <int NL, int NW> HB_HD void mat_reduce_elem(uint32_t *o, const uint32_t *part, int64_t stride, int S, const uint32_t *cw, int op, const FpParams<NL> &P) {
    uint32_t acc[NL], x[NL];
#pragma unroll
    for (int q = 0; q < NL; q++) acc[q] = 0;
    for (int s = 0; s < S; s++) {
        load_digits<NL, NW>(x, part + (size_t)s * stride * NW);
        fp_add(acc, acc, x, P);
    }
    mat_epilogue<NL, NW>(o, acc, cw, op, P);
}

// slices and their length for W workgroups of output and inner dimension k (mode: g_mat_split_mode)
struct MatPlan { int slices, kslice; };
inline MatPlan mat_plan(int64_t W, int k, int mode) {
    MatPlan pl{1, std::max(k, 1)};
    if (mode < 0 || W > MAT_SPLIT_MAX_WGS || W < 1) return pl;
    int64_t S;
    if (mode > 0) S = std::min<int64_t>((k + MAT_TK - 1) / MAT_TK, MAT_SPLIT_TARGET_WGS / W);
    else if (k >= MAT_SPLIT_MIN_K) S = std::min<int64_t>(k / MAT_SPLIT_SLICE_K, MAT_SPLIT_TARGET_WGS / W);
    else S = 1;
    if (S < 2) return pl;
    const int len = (int)(((k + S - 1) / S + MAT_TK - 1) / MAT_TK) * MAT_TK;
    pl.kslice = len;
    pl.slices = (k + len - 1) / len;                              // rounding the length up may leave fewer slices
    if (pl.slices < 2) { pl.slices = 1; pl.kslice = std::max(k, 1); }
    return pl;
}

// ---------------------------------------------------------------- kernels
// grid (batch * tiles_m * tiles_n, slices).  No __restrict__ on C and out: out may be C (a lane reads its element before it writes it).
// gridDim.y > 1: out is the partials buffer, `slice_elems` elements a slice, and the host passes op = HB_MAT_NONE.
template <int NL, int NW>
__global__ void __launch_bounds__(MAT_THREADS) k_mat_mul(const FpParams<NL> P, const uint32_t *A, const uint32_t *B, const uint32_t *C, int op, uint32_t *out, int m,
                                                         int k, int n, int tiles_m, int tiles_n, int kslice, int64_t slice_elems) {
    __shared__ uint32_t As[NL * MAT_TK * MAT_AS];
    __shared__ uint32_t Bs[NL * MAT_TK * MAT_TN];
    const int tid = threadIdx.x, ty = tid / MAT_TX, tx = tid % MAT_TX;
    const int per = tiles_m * tiles_n;
    const int64_t b = blockIdx.x / per;
    const int tile = (int)(blockIdx.x % per);
    const int m0 = (tile / tiles_n) * MAT_TM, n0 = (tile % tiles_n) * MAT_TN;
    const int k_lo = (int)blockIdx.y * kslice, k_hi = min(k, k_lo + kslice);
    const uint32_t *Ab = A + (size_t)b * m * k * NW, *Bb = B + (size_t)b * k * n * NW;
    MatLane<NL> s;
    mat_lane_init<NL>(s);
    int cnt = 0;
    for (int k0 = k_lo; k0 < k_hi; k0 += MAT_TK) {
        __syncthreads();
        mat_stage<NL, NW>(As, Bs, Ab, Bb, m, k, n, m0, n0, k0, k_hi, tid, MAT_THREADS);
        __syncthreads();
        mat_step<NL>(s, cnt, As, Bs, ty, tx, P);
    }
    mat_lane_flush<NL>(s, cnt, P);
    const int row = m0 + ty;
#pragma unroll
    for (int r = 0; r < MAT_RN; r++) {
        const int col = n0 + tx + r * MAT_TX;
        if (row < m && col < n) {
            const size_t e = ((size_t)b * m + row) * n + col;
            mat_finish<NL, NW>(out + ((size_t)blockIdx.y * slice_elems + e) * NW, s.acc[r], C ? C + e * NW : nullptr, op, P);
        }
    }
}
template <int NL, int NW>
__global__ void __launch_bounds__(256) k_mat_reduce(const FpParams<NL> P, const uint32_t *__restrict__ part, int64_t elems, int S, const uint32_t *C, int op, uint32_t *out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= elems) return;
    mat_reduce_elem<NL, NW>(out + (size_t)e * NW, part + (size_t)e * NW, elems, S, C ? C + (size_t)e * NW : nullptr, op, P);
}
// Compiler's report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; scratch = 0 bytes for every instantiation):
//   k_mat_mul<9, 8>     151 VGPRs: 3 waves a SIMD, LDS 28224 bytes (five workgroups a CU by LDS: the registers bound first)
//   k_mat_mul<3, 2>     72 VGPRs: 7 waves a SIMD, LDS 9408 bytes
//   k_mat_reduce<9, 8>  39 VGPRs: 8 waves, no LDS          k_mat_reduce<3, 2>  15 VGPRs: 8 waves, no LDS
// The 1 x 2 block: two outputs cost 72 VGPRs of columns and 18 of running sums at NL = 9; A's nine digits are read once for both, so a
// step reads 27 dwords of LDS for 162 multiply-adds.  A 2 x 2 block (144 + 36 VGPRs before operands) would leave two waves a SIMD for
// 36 dwords per 324 -- LDS is not what limits this loop (k_pm_direct runs the unblocked 18 per 81), occupancy hides its latency.

// ---------------------------------------------------------------- host side
namespace {

// the argument table of hb_mat_mul, shared with the host run
int mat_check_args(const void *a, const void *b, const void *c, int c_op, const void *out, int64_t batch, int64_t m, int64_t k, int64_t n) {
    if (batch < 0 || m < 0 || k < 0 || n < 0) return HB_ERR_BAD_ARG;
    if (m > 0x7fffffff || k > 0x7fffffff || n > 0x7fffffff) return HB_ERR_BAD_ARG;
    if (c_op != HB_MAT_NONE && c_op != HB_MAT_ADD && c_op != HB_MAT_SUB) return HB_ERR_BAD_ARG;
    if (c_op != HB_MAT_NONE && !c) return HB_ERR_BAD_ARG;
    if (out && (out == a || out == b)) return HB_ERR_BAD_ARG;
    if (batch > 0 && m > 0 && n > 0) {
        if (!out) return HB_ERR_BAD_ARG;
        if (k > 0 && (!a || !b)) return HB_ERR_BAD_ARG;
    }
    return HB_OK;
}

// host: the kernels' bodies, walked as their workgroups and lanes walk them; S slices of kslice (S = 1: the unsplit launch)
template <int NL, int NW>
int selftest_mat(const uint64_t *p_limbs, const uint64_t *a_host, const uint64_t *b_host, const uint64_t *c_host, int op, int64_t batch, int m, int k, int n, MatPlan pl,
                 uint64_t *out_host) {
    FpParams<NL> P;
    fp_params_from_limbs(P, p_limbs);
    const uint32_t *A = reinterpret_cast<const uint32_t *>(a_host), *B = reinterpret_cast<const uint32_t *>(b_host), *C = reinterpret_cast<const uint32_t *>(c_host);
    uint32_t *out = reinterpret_cast<uint32_t *>(out_host);
    const int tiles_m = (m + MAT_TM - 1) / MAT_TM, tiles_n = (n + MAT_TN - 1) / MAT_TN, S = pl.slices;
    const int64_t elems = batch * m * n;
    std::vector<uint32_t> part(S > 1 ? (size_t)S * elems * NW : 0), As((size_t)NL * MAT_TK * MAT_AS), Bs((size_t)NL * MAT_TK * MAT_TN);
    std::vector<MatLane<NL>> lanes(MAT_THREADS);
    std::vector<int> cnt(MAT_THREADS);
    for (int64_t b = 0; b < batch; b++)
        for (int tile = 0; tile < tiles_m * tiles_n; tile++)
            for (int sl = 0; sl < S; sl++) {
                const int m0 = (tile / tiles_n) * MAT_TM, n0 = (tile % tiles_n) * MAT_TN;
                const int k_lo = sl * pl.kslice, k_hi = std::min(k, k_lo + pl.kslice);
                const uint32_t *Ab = A + (size_t)b * m * k * NW, *Bb = B + (size_t)b * k * n * NW;
                for (int t = 0; t < MAT_THREADS; t++) { mat_lane_init<NL>(lanes[t]); cnt[t] = 0; }
                for (int k0 = k_lo; k0 < k_hi; k0 += MAT_TK) {
                    mat_stage<NL, NW>(As.data(), Bs.data(), Ab, Bb, m, k, n, m0, n0, k0, k_hi, 0, 1);
                    for (int t = 0; t < MAT_THREADS; t++) mat_step<NL>(lanes[t], cnt[t], As.data(), Bs.data(), t / MAT_TX, t % MAT_TX, P);
                }
                for (int t = 0; t < MAT_THREADS; t++) {
                    mat_lane_flush<NL>(lanes[t], cnt[t], P);
                    const int row = m0 + t / MAT_TX;
                    for (int r = 0; r < MAT_RN; r++) {
                        const int col = n0 + t % MAT_TX + r * MAT_TX;
                        if (row >= m || col >= n) continue;
                        const size_t e = ((size_t)b * m + row) * n + col;
                        if (S > 1) mat_finish<NL, NW>(part.data() + ((size_t)sl * elems + e) * NW, lanes[t].acc[r], nullptr, HB_MAT_NONE, P);
                        else mat_finish<NL, NW>(out + e * NW, lanes[t].acc[r], C ? C + e * NW : nullptr, op, P);
                    }
                }
            }
    if (S > 1)
        for (int64_t e = 0; e < elems; e++) mat_reduce_elem<NL, NW>(out + (size_t)e * NW, part.data() + (size_t)e * NW, elems, S, C ? C + (size_t)e * NW : nullptr, op, P);
    return HB_OK;
}

}  // namespace
}  // namespace hb

extern "C" {


int hb_mat_mul(hb_ctx *ctx, const uint64_t *a_dev, const uint64_t *b_dev, const uint64_t *c_dev, int c_op, uint64_t *out_dev, int64_t batch, int m, int k, int n,
               void *stream) { HB_API_GUARD(ctx);
    if (!ctx) return HB_ERR_BAD_ARG;
    if (mat_check_args(a_dev, b_dev, c_dev, c_op, out_dev, batch, m, k, n) != HB_OK) return fail(ctx, HB_ERR_BAD_ARG, "hb_mat_mul: bad argument");
    if (batch == 0 || m == 0 || n == 0) return HB_OK;
    const int tiles_m = (m + MAT_TM - 1) / MAT_TM, tiles_n = (n + MAT_TN - 1) / MAT_TN;
    const int64_t W = batch * tiles_m * tiles_n, elems = batch * m * n;
    if ((int64_t)tiles_m * tiles_n > 0x7fffffffLL || W > 0x7fffffffLL) return fail(ctx, HB_ERR_UNSUPPORTED, "hb_mat_mul: too many output tiles for one launch");
    hipStream_t s = (hipStream_t)stream;
    const uint32_t *C = c_op == HB_MAT_NONE ? nullptr : u32(c_dev);
    const MatPlan pl = mat_plan(W, k, g_mat_split_mode);
    if (pl.slices == 1) {
        HB_DISPATCH(ctx,
            (k_mat_mul<9, 8><<<dim3((unsigned)W, 1), MAT_THREADS, 0, s>>>(ctx->pw, u32(a_dev), u32(b_dev), C, c_op, (uint32_t *)out_dev, m, k, n, tiles_m, tiles_n, pl.kslice, 0)),
            (k_mat_mul<3, 2><<<dim3((unsigned)W, 1), MAT_THREADS, 0, s>>>(ctx->pn, u32(a_dev), u32(b_dev), C, c_op, (uint32_t *)out_dev, m, k, n, tiles_m, tiles_n, pl.kslice, 0)));
        HB_LAUNCH_CHECK(ctx);
        return HB_OK;
    }
    // per stream: launches of one stream are ordered, and a regrowth frees through hipFree (which waits for the device)
    const std::string slot = "mat:" + std::to_string((uintptr_t)stream);
    void *base = nullptr;
    const int rc = ctx_scratch(ctx, slot.c_str(), (size_t)pl.slices * elems * ctx->n_limbs * 8, &base);
    if (rc != HB_OK) return rc;
    uint32_t *part = (uint32_t *)base;
    const unsigned rblocks = (unsigned)((elems + 255) / 256);
    HB_DISPATCH(ctx,
        (k_mat_mul<9, 8><<<dim3((unsigned)W, (unsigned)pl.slices), MAT_THREADS, 0, s>>>(ctx->pw, u32(a_dev), u32(b_dev), nullptr, HB_MAT_NONE, part, m, k, n, tiles_m, tiles_n,
                                                                                      pl.kslice, elems)),
        (k_mat_mul<3, 2><<<dim3((unsigned)W, (unsigned)pl.slices), MAT_THREADS, 0, s>>>(ctx->pn, u32(a_dev), u32(b_dev), nullptr, HB_MAT_NONE, part, m, k, n, tiles_m, tiles_n,
                                                                                      pl.kslice, elems)));
    HB_DISPATCH(ctx,
        (k_mat_reduce<9, 8><<<rblocks, 256, 0, s>>>(ctx->pw, part, elems, pl.slices, C, c_op, (uint32_t *)out_dev)),
        (k_mat_reduce<3, 2><<<rblocks, 256, 0, s>>>(ctx->pn, part, elems, pl.slices, C, c_op, (uint32_t *)out_dev)));
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_mat_constants(int n_limbs, int32_t *out) {
    if (!out || (n_limbs != 1 && n_limbs != 4)) return HB_ERR_BAD_ARG;
    const int32_t v[HB_MAT_CONSTANTS] = {MAT_TM, MAT_TN, MAT_TK, n_limbs == 4 ? MatAcc<9>::GROUP : MatAcc<3>::GROUP, n_limbs == 4 ? MatAcc<9>::L : MatAcc<3>::L,
                                         MAT_SPLIT_MIN_K, MAT_SPLIT_MAX_WGS, MAT_SPLIT_TARGET_WGS};
    memcpy(out, v, sizeof(v));
    return HB_OK;
}

int hb_selftest_mat(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *operands, const int64_t *params, uint64_t *out) {
    if (!p_limbs || !operands || !params || (n_limbs != 1 && n_limbs != 4)) return HB_ERR_BAD_ARG;
    const int op = what & 0xff, mode = what & ~0xff;
    if (mode != 0 && mode != HB_MAT_SELFTEST_SPLIT && mode != HB_MAT_SELFTEST_AUTO) return HB_ERR_BAD_ARG;
    const int64_t batch = params[0], m = params[1], k = params[2], n = params[3], slices = params[4];
    if (mat_check_args(operands[0], operands[1], operands[2], op, out, batch, m, k, n) != HB_OK) return HB_ERR_BAD_ARG;
    if (batch == 0 || m == 0 || n == 0) return HB_OK;
    if (batch * m * n > (int64_t)1 << 26) return HB_ERR_UNSUPPORTED;
    MatPlan pl{1, (int)std::max<int64_t>(k, 1)};
    if (mode == HB_MAT_SELFTEST_AUTO) pl = mat_plan(batch * ((m + MAT_TM - 1) / MAT_TM) * ((n + MAT_TN - 1) / MAT_TN), (int)k, 0);
    if (mode == HB_MAT_SELFTEST_SPLIT) {
        // `slices` slices as the device cuts them: whole MAT_TK steps
        if (slices < 1 || slices > 1024) return HB_ERR_BAD_ARG;
        const int len = (int)(((std::max<int64_t>(k, 1) + slices - 1) / slices + MAT_TK - 1) / MAT_TK) * MAT_TK;
        pl.kslice = len;
        pl.slices = (int)std::max<int64_t>(1, (k + len - 1) / len);
    }
    const uint64_t *c = op == HB_MAT_NONE ? nullptr : operands[2];
    if (n_limbs == 4) return selftest_mat<9, 8>(p_limbs, operands[0], operands[1], c, op, batch, (int)m, (int)k, (int)n, pl, out);
    return selftest_mat<3, 2>(p_limbs, operands[0], operands[1], c, op, batch, (int)m, (int)k, (int)n, pl, out);
}

void hb_debug_mat_split(int mode) { g_mat_split_mode = mode > 0 ? 1 : (mode < 0 ? -1 : 0); }

}  // extern "C"

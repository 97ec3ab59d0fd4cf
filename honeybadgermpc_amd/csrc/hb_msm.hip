// hb_msm.hip -- multi-scalar multiplication in BLS12-381 G1: out[m] = sum_k s[m][k] P[m or 0][k], m < M rows of K terms each, the sum the
// reference's interpolate_g1_at_x (betterpairing.py:800) and every other "product of powers" is.  Built from the bodies of hb_g1_elem.hpp.
// Scalars: plain 256-bit integers, read as they are.  Points: affine, 12 words, the identity all zeros; one set of K bases for all rows or
// one a row.  Out: affine canonical, one inversion a row.
//
// Two paths fill a workspace with Jacobian partials (48 words each: X, Y, Z as 14 Montgomery digits + 2 words of padding), one fold ends both.
//   k_msm_direct   K small.  A workgroup takes 256 consecutive terms of one row: lane t computes s_t P_t (g1_mul_affine, the 255 doublings
//                  of scalar_mul), the TREE adds the 256 results, lane 0 writes the partial.  W = 1 "window", ceil(K / 256) partials a row.
//   k_msm_bucket   window c = 8: digit w of a scalar is its byte w, W = 32 windows.  A workgroup takes one (row, window, chunk of at most
//                  `chunk` <= 4096 terms):
//                    count    the chunk's digits into 256 LDS counters (digit 0 is skipped: it contributes nothing)
//                    scan     start[b] = the counters before b
//                    scatter  term indices into `list`, sorted by digit (counting sort; the order inside a bucket is the order the LDS
//                             atomics were served in: partials differ in representation from run to run, the affine output cannot)
//                    walk     lane b adds bucket b's points with g1_add_mixed (complete: a repeated base doubles, P then -P is the identity)
//                    heavy    a bucket longer than thr = max(16, 4 chunk / 256) is NOT walked by its lane: the whole workgroup takes it,
//                             lane t the entries t, t + 256, ..., the TREE adds the 256 partial sums; the sum is parked in LDS for lane b.  Equal
//                             scalars (all ones, small weights) put a whole chunk into one bucket a window: 16 additions a lane and a
//                             tree instead of 4096 in one lane.
//                    scale    lane b: b B_b by an 8-bit double-and-add on its own bucket -- no serial running sum over the buckets
//                    TREE     adds the 255 results; lane 0 writes the partial
//   TREE           256 nodes in LDS, a node a Jacobian point of 3 x 14 digits at a stride of 43 words (odd: lanes of a step hit distinct
//                  banks), 43 KB; 8 steps, step h: lane t < h adds node t + h to node t (g1_add, complete).
//   k_msm_fold     one workgroup a (row, window): lane t adds the chunk partials t, t + 256, ..., the TREE ends it: S_w.  (M = 1 with many
//                  chunks is no serial chain either.)
//   k_msm_finish   one lane a row: acc = S_(W-1); acc = 2^8 acc + S_w down to w = 0; to affine.  W = 1: no doubling.  This is 248 dependent
//                  doublings and 31 additions: a call on the bucket path is never faster than about one scalar_mul chain.
// LDS of k_msm_bucket: 43 KB of nodes, 11 KB of parked heavy sums, 8 KB of list (16-bit indices into the chunk), 4 KB of counters: 66 KB, two workgroups a CU at the
// two waves a SIMD these kernels run at.  Products a term: direct 255 x 7 + 11 a set bit + 2 (the load) ~ 3 200; bucket 32 x (11 + 2) = 416,
// and a workgroup 7 x 7 + 7 x 16 (scale) + 8 x 16 (tree) ~ 300 a lane on top, whatever its chunk holds.
// 256-thread workgroups, every load bounded by K, nothing waits for another workgroup, the caller's stream, nothing allocated.
// The per-lane steps (msm_digit, msm_walk, msm_scale, msm_tree_step, msm_fold_lane, msm_finish_row) are HB_HD: hb_selftest_g1_msm drives
// the very same functions lane by lane over host arrays in place of LDS.  Compiler's report: profiles/g1_msm.txt.
// (MSM_NODE, msm_node_store, msm_node_load and msm_tree_step live in hb_g1_elem.hpp: hb_crs.hip's split rows end in the same tree.)
#include "hb_g1_elem.hpp"

using namespace hb;

namespace hb {

constexpr int MSM_WG = 256;                              // lanes a workgroup = buckets a window = tree nodes
constexpr int MSM_W = 32;                                // windows of 8 bits
constexpr int MSM_PART = 48;                             // words a partial in the workspace
constexpr int MSM_HEAVY = 64;                             // heavy buckets a chunk can hold: fewer than chunk / thr <= 64
constexpr int MSM_CHUNK = 4096;                          // terms a workgroup of the bucket path takes at most (16-bit list entries)
constexpr int MSM_AUTO_TERMS = 22;                       // method 0: bucket from this K on (g1.py: MSM_CROSSOVER, profiles/g1_msm.txt)
constexpr int MSM_DIRECT = 1, MSM_BUCKET = 2, MSM_BUCKET_HEAVY = 3;   // 3: the self test's, every non-empty bucket by the whole workgroup

HB_HD int msm_threshold(int chunk) { return 4 * chunk / MSM_WG > 16 ? 4 * chunk / MSM_WG : 16; }
// window digit w of the scalar at s: its byte w
HB_HD uint32_t msm_digit(const uint32_t *s, int w) { return (s[w >> 2] >> (8 * (w & 3))) & 255u; }

HB_HD void msm_part_store(uint32_t *p, const G1Jac &j) {
    g1_store16(p, j.X);
    g1_store16(p + 16, j.Y);
    g1_store16(p + 32, j.Z);
}
HB_HD void msm_part_load(G1Jac &j, const uint32_t *p) {
    g1_load16(j.X, p);
    g1_load16(j.Y, p + 16);
    g1_load16(j.Z, p + 32);
}
// acc = the sum of the points list[from], list[from + step], ... (indices below `to`) of the chunk whose points start at pts
HB_HD void msm_walk(G1Jac &acc, const uint16_t *list, int from, int to, int step, const uint32_t *pts, const FpParams<QL> &P) {
    g1_set_identity(acc, P);
#pragma unroll 1
    for (int i = from; i < to; i += step) {
        G1Aff a;
        g1_load(a, pts + (int64_t)list[i] * G1_PT, P);
        g1_add_mixed(acc, a, P);
    }
}
// r = b B, b < 256
HB_HD void msm_scale(G1Jac &r, const G1Jac &B, uint32_t b, const FpParams<QL> &P) {
    g1_set_identity(r, P);
    if (fp_is_zero<QL>(B.Z)) return;
    bool started = false;
#pragma unroll 1
    for (int bit = 7; bit >= 0; bit--) {
        if (started) g1_double(r, r, P);
        if ((b >> bit) & 1u) { g1_add(r, B, P); started = true; }
    }
}
// the direct path's lane: acc = s P
HB_HD void msm_direct_lane(G1Jac &acc, const uint32_t *s, const uint32_t *p, const FpParams<QL> &P) {
    uint32_t kw[SW];
    G1Aff a;
    g1_load_scalar(kw, s);
    g1_load(a, p, P);
    g1_mul_affine(acc, kw, a, P);
}
// the fold's lane: acc = partials lane, lane + 256, ... of n
HB_HD void msm_fold_lane(G1Jac &acc, const uint32_t *parts, int64_t n, int lane, const FpParams<QL> &P) {
    g1_set_identity(acc, P);
#pragma unroll 1
    for (int64_t c = lane; c < n; c += MSM_WG) {
        G1Jac t;
        msm_part_load(t, parts + c * MSM_PART);
        g1_add(acc, t, P);
    }
}
// one row's end: Horner over its W window sums from the top, then to affine
HB_HD void msm_finish_row(uint32_t *out, const uint32_t *S, int W, const FpParams<QL> &P) {
    G1Jac acc, t;
    msm_part_load(acc, S + (int64_t)(W - 1) * MSM_PART);
#pragma unroll 1
    for (int w = W - 2; w >= 0; w--) {
#pragma unroll 1
        for (int d = 0; d < 8; d++) g1_double(acc, acc, P);
        msm_part_load(t, S + (int64_t)w * MSM_PART);
        g1_add(acc, t, P);
    }
    g1_store(out, acc, P);
}

// ---------------------------------------------------------------- kernels
// the tree over the workgroup's nodes (every lane has stored its node; no barrier yet); the sum is node 0 for every lane afterwards
__device__ __forceinline__ void msm_tree(uint32_t *nodes, int tid, const FpParams<QL> &P) {
    __syncthreads();
#pragma unroll 1
    for (int half = MSM_WG / 2; half >= 1; half >>= 1) {
        msm_tree_step(nodes, tid, half, P);
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) k_msm_direct(const uint32_t *s, const uint32_t *p, int p_rows, int64_t K, int64_t nch, uint32_t *parts) {
    __shared__ uint32_t nodes[MSM_WG * MSM_NODE];
    const int tid = threadIdx.x;
    const int64_t bid = blockIdx.x, m = bid / nch, k = (bid % nch) * MSM_WG + tid;
    const FpParams<QL> P = fq_params();
    G1Jac v;
    if (k < K) msm_direct_lane(v, s + (m * K + k) * SW, p + ((p_rows ? m * K : 0) + k) * G1_PT, P);
    else g1_set_identity(v, P);
    msm_node_store(nodes, tid, v);
    msm_tree(nodes, tid, P);
    if (tid == 0) {
        msm_node_load(v, nodes, 0);
        msm_part_store(parts + bid * MSM_PART, v);
    }
}

__global__ void __launch_bounds__(256) k_msm_bucket(const uint32_t *s, const uint32_t *p, int p_rows, int64_t K, int chunk, int64_t nch, uint32_t *parts) {
    __shared__ uint32_t nodes[MSM_WG * MSM_NODE], heavy[MSM_HEAVY * MSM_NODE];
    __shared__ uint16_t list[MSM_CHUNK];
    __shared__ int cnt[MSM_WG], cur[MSM_WG], start[MSM_WG + 1], slot[MSM_WG];
    const int tid = threadIdx.x;
    const int64_t bid = blockIdx.x, m = bid / (nch * MSM_W), k0 = (bid % nch) * chunk;
    const int w = (int)((bid / nch) % MSM_W);
    const int len = (int)(K - k0 < chunk ? K - k0 : chunk);
    const uint32_t *sc = s + (m * K + k0) * SW, *pc = p + ((p_rows ? m * K : 0) + k0) * G1_PT;
    const FpParams<QL> P = fq_params();
    const int thr = msm_threshold(chunk);
    cnt[tid] = 0;
    slot[tid] = -1;
    __syncthreads();
    for (int i = tid; i < len; i += MSM_WG) {
        const uint32_t d = msm_digit(sc + (int64_t)i * SW, w);
        if (d) atomicAdd(&cnt[d], 1);
    }
    __syncthreads();
    int before = 0;
    for (int b = 0; b < tid; b++) before += cnt[b];
    start[tid] = before;
    cur[tid] = before;
    if (tid == MSM_WG - 1) start[MSM_WG] = before + cnt[tid];
    __syncthreads();
    for (int i = tid; i < len; i += MSM_WG) {
        const uint32_t d = msm_digit(sc + (int64_t)i * SW, w);
        if (d) list[atomicAdd(&cur[d], 1)] = (uint16_t)i;
    }
    __syncthreads();
    // rounds 1 .. 255: heavy bucket b by the whole workgroup, its sum parked in `heavy` (fewer than chunk / thr <= 64 of them: thr >=
    // chunk / 64); round 256: every lane its own bucket (walked, or fetched from `heavy`), scaled, and the tree over all of them.
    // One loop, so that the walk and the tree stand once in the code; no bucket sum is live in registers across a tree.
    int n_heavy = 0;
#pragma unroll 1
    for (int b = 1; b <= MSM_WG; b++) {
        const bool fin = b == MSM_WG;
        if (!fin && (start[b + 1] - start[b] <= thr || n_heavy == MSM_HEAVY)) continue;   // the same for every lane
        int from, to, step = MSM_WG;
        if (!fin) {
            from = start[b] + tid;
            to = start[b + 1];
        } else {
            from = start[tid];
            to = slot[tid] >= 0 ? from : start[tid + 1];
            step = 1;
        }
        G1Jac v;
        msm_walk(v, list, from, to, step, pc, P);
        if (fin) {
            G1Jac mine = v;
            if (slot[tid] >= 0) msm_node_load(mine, heavy, slot[tid]);
            msm_scale(v, mine, (uint32_t)tid, P);
        }
        msm_node_store(nodes, tid, v);
        msm_tree(nodes, tid, P);
        if (!fin) {
            if (tid < MSM_NODE) heavy[n_heavy * MSM_NODE + tid] = nodes[tid];
            if (tid == 0) slot[b] = n_heavy;
            n_heavy++;
            __syncthreads();
        } else if (tid == 0) {
            msm_node_load(v, nodes, 0);
            msm_part_store(parts + bid * MSM_PART, v);
        }
    }
}

__global__ void __launch_bounds__(256) k_msm_fold(const uint32_t *parts, int64_t nch, uint32_t *sums) {
    __shared__ uint32_t nodes[MSM_WG * MSM_NODE];
    const int tid = threadIdx.x;
    const int64_t bid = blockIdx.x;
    const FpParams<QL> P = fq_params();
    G1Jac v;
    msm_fold_lane(v, parts + bid * nch * MSM_PART, nch, tid, P);
    msm_node_store(nodes, tid, v);
    msm_tree(nodes, tid, P);
    if (tid == 0) {
        msm_node_load(v, nodes, 0);
        msm_part_store(sums + bid * MSM_PART, v);
    }
}

__global__ void __launch_bounds__(256) k_msm_finish(const uint32_t *sums, int W, uint32_t *out, int64_t rows) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= rows) return;
    const FpParams<QL> P = fq_params();
    msm_finish_row(out + m * G1_PT, sums + m * W * MSM_PART, W, P);
}

// ---------------------------------------------------------------- host side
struct MsmPlan { int path, W, chunk; int64_t nch, parts; };                    // parts: partials of the first stage, rows * W * nch
// false: bad arguments (or a shape beyond one launch)
static bool msm_plan(int64_t rows, int64_t terms, int method, int chunk, bool selftest, MsmPlan *pl) {
    if (rows < 0 || terms < 0 || method < 0 || method > (selftest ? MSM_BUCKET_HEAVY : MSM_BUCKET)) return false;
    if (chunk == 0) chunk = MSM_CHUNK;
    if (chunk < 64 || chunk > MSM_CHUNK || chunk % 64) return false;
    if (terms > (1LL << 32) || (terms > 0 && rows > (1LL << 36) / terms)) return false;
    pl->path = method ? method : (terms < MSM_AUTO_TERMS ? MSM_DIRECT : MSM_BUCKET);
    pl->W = pl->path == MSM_DIRECT ? 1 : MSM_W;
    pl->chunk = chunk;
    const int64_t per = pl->path == MSM_DIRECT ? MSM_WG : chunk;
    pl->nch = terms ? (terms + per - 1) / per : 1;
    pl->parts = (rows ? rows : 1) * pl->W * pl->nch;
    return pl->parts <= 0x7fffffffLL;
}
static int64_t msm_workspace_words(const MsmPlan &pl, int64_t rows) { return (pl.parts + (rows ? rows : 1) * pl.W) * MSM_PART; }

// the workgroup of k_msm_bucket on the host: arrays in place of LDS, lanes one after another between what are barriers on the device
// (`heavy` has a slot a bucket here: thr = 0, the self test's forced mode, makes every non-empty bucket heavy)
static void msm_host_bucket(const uint32_t *sc, const uint32_t *pc, int len, int w, int thr, uint32_t *part, const FpParams<QL> &P) {
    std::vector<uint32_t> nodes(MSM_WG * MSM_NODE), heavy(MSM_WG * MSM_NODE);
    std::vector<uint16_t> list(len ? len : 1);
    int cur[MSM_WG], start[MSM_WG + 1] = {0}, slot[MSM_WG], n_heavy = 0;
    for (int i = 0; i < len; i++) {
        const uint32_t d = msm_digit(sc + (int64_t)i * SW, w);
        if (d) start[d + 1]++;
    }
    for (int b = 0; b < MSM_WG; b++) { start[b + 1] += start[b]; cur[b] = start[b]; slot[b] = -1; }
    for (int i = 0; i < len; i++) {
        const uint32_t d = msm_digit(sc + (int64_t)i * SW, w);
        if (d) list[cur[d]++] = (uint16_t)i;
    }
    for (int b = 1; b <= MSM_WG; b++) {
        const bool fin = b == MSM_WG;
        if (!fin && start[b + 1] - start[b] <= thr) continue;
        for (int tid = 0; tid < MSM_WG; tid++) {
            int from, to, step = MSM_WG;
            if (!fin) {
                from = start[b] + tid;
                to = start[b + 1];
            } else {
                from = start[tid];
                to = slot[tid] >= 0 ? from : start[tid + 1];
                step = 1;
            }
            G1Jac v;
            msm_walk(v, list.data(), from, to, step, pc, P);
            if (fin) {
                G1Jac mine = v;
                if (slot[tid] >= 0) msm_node_load(mine, heavy.data(), slot[tid]);
                msm_scale(v, mine, (uint32_t)tid, P);
            }
            msm_node_store(nodes.data(), tid, v);
        }
        for (int half = MSM_WG / 2; half >= 1; half >>= 1)
            for (int tid = 0; tid < MSM_WG; tid++) msm_tree_step(nodes.data(), tid, half, P);
        G1Jac v;
        msm_node_load(v, nodes.data(), 0);
        if (!fin) {
            msm_node_store(heavy.data(), n_heavy, v);
            slot[b] = n_heavy++;
        } else msm_part_store(part, v);
    }
}
// k_msm_direct's and k_msm_fold's workgroups: `lane` fills node t, the tree, node 0 to `part`
template <typename Lane> static void msm_host_tree(Lane lane, uint32_t *part, const FpParams<QL> &P) {
    std::vector<uint32_t> nodes(MSM_WG * MSM_NODE);
    G1Jac v;
    for (int tid = 0; tid < MSM_WG; tid++) {
        lane(v, tid);
        msm_node_store(nodes.data(), tid, v);
    }
    for (int half = MSM_WG / 2; half >= 1; half >>= 1)
        for (int tid = 0; tid < MSM_WG; tid++) msm_tree_step(nodes.data(), tid, half, P);
    msm_node_load(v, nodes.data(), 0);
    msm_part_store(part, v);
}

}  // namespace hb

extern "C" {

int64_t hb_g1_msm_workspace_bytes(int64_t rows, int64_t terms, int method, int chunk) {
    MsmPlan pl;
    return msm_plan(rows, terms, method, chunk, false, &pl) ? msm_workspace_words(pl, rows) * 4 : 0;
}

int hb_g1_msm(hb_ctx *ctx, const uint64_t *s_dev, const uint64_t *p_dev, int points_per_row, uint64_t *out_dev, int64_t rows, int64_t terms, int method, int chunk,
              void *workspace_dev, int64_t workspace_bytes, void *stream) {
    G1_ENTER("hb_g1_msm", rows, !out_dev || !workspace_dev || (terms > 0 && (!s_dev || !p_dev)));
    MsmPlan pl;
    if (!msm_plan(rows, terms, method, chunk, false, &pl))
        return fail(ctx, HB_ERR_BAD_ARG, "hb_g1_msm: terms >= 0, method 0 (auto), 1 (direct) or 2 (bucket), chunk 0 or a multiple of 64 in [64, 4096], a shape within one launch");
    if (workspace_bytes < msm_workspace_words(pl, rows) * 4) return fail(ctx, HB_ERR_BAD_ARG, "hb_g1_msm: the workspace is smaller than hb_g1_msm_workspace_bytes says");
    const int p_rows = points_per_row != 0;
    auto overlaps = [&](const void *q, int64_t bytes) {
        const char *a = (const char *)out_dev, *b = (const char *)q;
        return q && a < b + bytes && b < a + rows * G1_PT * 4;
    };
    if (rows > 0 && (overlaps(s_dev, rows * terms * SW * 4) || overlaps(p_dev, (p_rows ? rows : 1) * terms * G1_PT * 4) || overlaps(workspace_dev, workspace_bytes)))
        return fail(ctx, HB_ERR_BAD_ARG, "hb_g1_msm: out aliases an input or the workspace");
    if (rows == 0) return HB_OK;
    if (terms == 0) {
        HB_HIP(ctx, hipMemsetAsync(out_dev, 0, rows * G1_PT * 4, s));
        return HB_OK;
    }
    uint32_t *parts = (uint32_t *)workspace_dev, *sums = parts + pl.parts * MSM_PART;
    if (pl.path == MSM_DIRECT) k_msm_direct<<<(unsigned)pl.parts, 256, 0, s>>>((const uint32_t *)s_dev, (const uint32_t *)p_dev, p_rows, terms, pl.nch, parts);
    else k_msm_bucket<<<(unsigned)pl.parts, 256, 0, s>>>((const uint32_t *)s_dev, (const uint32_t *)p_dev, p_rows, terms, pl.chunk, pl.nch, parts);
    HB_LAUNCH_CHECK(ctx);
    k_msm_fold<<<(unsigned)(rows * pl.W), 256, 0, s>>>(parts, pl.nch, sums);
    HB_LAUNCH_CHECK(ctx);
    k_msm_finish<<<blocks, 256, 0, s>>>(sums, pl.W, (uint32_t *)out_dev, rows);
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_selftest_g1_msm(const uint64_t *s, const uint64_t *p, int points_per_row, uint64_t *out, int64_t rows, int64_t terms, int method, int chunk) {
    MsmPlan pl;
    if (!out || !g1_consts_ok() || !msm_plan(rows, terms, method, chunk, true, &pl) || (terms > 0 && rows > 0 && (!s || !p))) return HB_ERR_BAD_ARG;
    const FpParams<QL> P = fq_params();
    uint32_t *o = reinterpret_cast<uint32_t *>(out);
    if (terms == 0) {
        memset(o, 0, rows * G1_PT * 4);
        return HB_OK;
    }
    const uint32_t *sw = reinterpret_cast<const uint32_t *>(s), *pw = reinterpret_cast<const uint32_t *>(p);
    const bool p_rows = points_per_row != 0;
    const int thr = pl.path == MSM_BUCKET_HEAVY ? 0 : msm_threshold(pl.chunk);
    // (16-byte aligned, as the device's workspace: partials go through dwordx4 accesses)
    std::vector<uint4> ws((size_t)msm_workspace_words(pl, rows) / 4);
    uint32_t *parts = reinterpret_cast<uint32_t *>(ws.data()), *sums = parts + pl.parts * MSM_PART;
    for (int64_t bid = 0; bid < rows * pl.W * pl.nch; bid++) {
        if (pl.path == MSM_DIRECT) {
            const int64_t m = bid / pl.nch, c = bid % pl.nch;
            msm_host_tree([&](G1Jac &v, int tid) {
                const int64_t k = c * MSM_WG + tid;
                if (k < terms) msm_direct_lane(v, sw + (m * terms + k) * SW, pw + ((p_rows ? m * terms : 0) + k) * G1_PT, P);
                else g1_set_identity(v, P);
            }, parts + bid * MSM_PART, P);
        } else {
            const int64_t m = bid / (pl.nch * MSM_W), k0 = (bid % pl.nch) * pl.chunk;
            const int w = (int)((bid / pl.nch) % MSM_W);
            const int len = (int)(terms - k0 < pl.chunk ? terms - k0 : pl.chunk);
            msm_host_bucket(sw + (m * terms + k0) * SW, pw + ((p_rows ? m * terms : 0) + k0) * G1_PT, len, w, thr, parts + bid * MSM_PART, P);
        }
    }
    for (int64_t bid = 0; bid < rows * pl.W; bid++)
        msm_host_tree([&](G1Jac &v, int tid) { msm_fold_lane(v, parts + bid * pl.nch * MSM_PART, pl.nch, tid, P); }, sums + bid * MSM_PART, P);
    for (int64_t m = 0; m < rows; m++) msm_finish_row(o + m * G1_PT, sums + m * pl.W * MSM_PART, pl.W, P);
    return HB_OK;
}

}  // extern "C"

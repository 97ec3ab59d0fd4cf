// hb_mfma_fused.hip -- decode + validate at small-integer points as ONE launch of the small-entry matrix-core kernel.
//
// Reference: IncrementalDecoder's optimistic step (honeybadgermpc/reed_solomon.py:305-326): decoder.decode_batch over the first
// d arrivals z (vandermonde_batch_interpolate, hbmpc_ntl_helpers.pyx:139-197: V(z)^-1 rebuilt per call, then a mat-mul),
// encoder.encode_batch of the guess, and the compare loop over the later arrivals zc.
//
// Round 2 fused the three into one launch of the FULL-SIZE kernel (hb_mfma_wide.hip) over [V^-1 ; V[zc] V^-1], whose entries are
// arbitrary residues: 32 digits an entry, 63 columns an output.  At the production points x_i = i + 1 that throws a structure
// away.  With A_j(X) = prod_{q != j} (X - x_zq) and den_j = A_j(x_zj),
//
//     V^-1[m][j]        = coeff_m(A_j) / den_j           coeff_m(A_j): an INTEGER, |.| <= prod (1 + x_zq) < 2^122 at n = 64, t = 21
//     (V[zc] V^-1)[i][j] = A_j(x_zci) / den_j            A_j(x_i) = prod_{q != j} (x_i - x_zq): an INTEGER, |.| < 2^124
//
// so  [V^-1 ; V[zc] V^-1] y  =  [N ; P] (y ./ den)  with a matrix of SMALL integers (16 balanced base-256 digits: half the MFMAs
// of the full-size kernel, 47 columns instead of 63 per output) applied to the received columns divided by den_j -- one modular
// multiplication per INPUT element instead of per matrix entry.  Round 1's pipeline already knew this factorisation for the
// decode alone (k_prescale_tab + k_mm8 over N, hb_fast.hip / hb_mfma.hip), as three launches with the scaled columns making a
// round trip through HBM.  Here:
//
//   * k_mm8f: the k_mm8 pass (gen_mm8.py's MFMA phases, the same epilogue) in workgroups of EIGHT waves over units of 64 chunks.
//     The input elements do not arrive by LDS-DMA: the waves that have a pass less than the others (43 rows = 3 row tiles: 12
//     passes for 8 waves) read the next unit's elements, multiply them by 1 / den_l (x / den = sum_q x_q T_q over the 29-bit
//     digits of x with T_q = 2^(29 q) / den_l tabulated -- wave-uniform, scalar loads -- and a two-digit Barrett quotient: the
//     arithmetic of k_prescale_tab) and write them to LDS in MFMA operand order.  The GEMM takes ANY 256-bit representative, so
//     the scaled element is not even made canonical.  Per row a mode: store the canonical sum (a coefficient row) or compare it
//     with the received row of a later arrival (flag, first disagreeing chunk, bitmap of disagreeing chunks).
//   * k_fs_build: [N ; P], the per-row constants, the T tables and the row modes ON THE DEVICE, in plain 128-bit integer
//     arithmetic (the entries are small integers, so A(X), the synthetic divisions and the products are a microsecond of shifts
//     and multiplies); the only field arithmetic is 1 / den_j = prod_q 1 / (x_zj - x_zq) from the point set's table of inverse
//     differences (hb_quick.hip) and one multiplication per row constant.  Two halves that can be launched apart: everything
//     that depends on z alone (N, T: known when the d-th column arrives) and the rows of the compared senders (P: known when the
//     last column arrives).
//
// Applies to wide contexts with 2^254 <= p < 2^256, points that are distinct integers below 2^16, 4 <= d <= 22, and bounds
// (checked on the host from the point set) that keep every entry below 2^125; everything else stays on the full-size kernel.
#include <math.h>

#include <algorithm>
#include <atomic>
#include <type_traits>

#include "hb_mm8.hpp"

namespace hb {

#include "hb_mm8_body.inc"

constexpr int FS_WAVES = 8, FS_TPW = 4;
#ifdef HB_MM8_TIMING
// per wave, ticks of s_memtime summed over its units.  Slot 0: kernel entry to the end of the wave's share of the first unit's scaling (the
// prologue included; once per workgroup); 7: the wait for its LDS writes ahead of a unit's barrier; 1: the barrier; 2: scaling the next
// unit; 3 / 5: the MFMA halves; 4: parking half 0; 6: words, reduction, store / compare
__device__ unsigned long long g_fs_t[256 * 8 * 8];
#define FS_T(k) do { const unsigned long long tn_ = __builtin_amdgcn_s_memtime(); tacc[k] += tn_ - tlast; tlast = tn_; } while (0)
#else
#define FS_T(k) do { } while (0)
#endif
constexpr int FS_MAXD = 24, FS_MAXC = 104;      // terms (three K-blocks), compared rows
constexpr size_t FS_LDS_LIMIT = 156 * 1024;

struct FsIdx { uint16_t z[FS_MAXD], xz[FS_MAXD], zc[FS_MAXC], xzc[FS_MAXC]; };
// the compared senders of a launch whose rows come from the per-party candidate store (k_fs_cand): rows n_coef .. n_coef + nc - 1 of the
// matrix are the candidates of parties zc[0 .. nc)
struct FsPick { const uint4 *cand; const uint32_t *cand_crow; int n_coef, nc; uint16_t zc[FS_MAXC]; };
// which waves scale which terms of the NEXT unit while a unit's passes run (bit l of terms[w]: wave w takes term l): dealt on the host so
// that the two waves of a SIMD (w and w + 4) reach the unit's barrier together -- a wave that waits leaves its SIMD to ONE wave, and one
// wave issues at 0.7 of the rate two reach (fs_split)
struct FsSplit { uint32_t terms[FS_WAVES]; };
// A narrow last row tile PACKED: the two digit groups of an output on M rows m and m + 8 of one sixteen-byte piece per K-block, so the
// pass over it issues 39 NKB MFMAs instead of 78 NKB (Mm8PhasePacked).  Output `reg` of lane (n, g) is M row 4 reg + g, so the two partial
// sums of a merged output are regs r and r + 2 of ONE lane: no lane of the tile ever needs another's.  nm merged outputs take M rows
// 0 .. nm - 1 (and 8 .. 8 + nm - 1); ns rows whose digit group 1 is empty take one M row each, 4 .. 7 and 12 .. 15 (regs 1 and 3: only
// with nm <= 4, so that every reg of the tile is of one kind in all its lanes).  Either nm <= 8 and ns = 0, or nm <= 4 and 5 <= ns <= 8
// (the two forms k_mm8f is compiled for); nm = ns = 0: no packed tile.
struct FsPack { int nm, ns; uint8_t single[8]; };
// the image slot (16 row tile + M row) of matrix row i; kind 0: both digit groups in the slot's own two pieces, 1: merged, 2: single-group.
// The single-group rows leave their places, the rows behind them move up, the last nm of the rest are the merged ones.
__host__ __device__ inline int fs_slot(const FsPack &pk, int i, int n_out, int &kind) {
    kind = 0;
    if (!(pk.nm | pk.ns)) return i;
    const int base = 16 * ((n_out + 15) / 16 - 1);
    int before = 0;
    for (int k = 0; k < pk.ns; k++) {
        if (pk.single[k] == i) { kind = 2; return base + 4 + (k & 3) + 8 * (k >> 2); }
        before += pk.single[k] < i;
    }
    const int pos = i - before;
    if (pos >= base) kind = 1;
    return pos;
}
// Does the last row tile pack?  rem = the rows of the ragged last tile, small[i]: coefficient row i has no digit above the eighth.  Up to
// eight rows merge where they stand; more need single-group rows to trade places with (the LAST small coefficient rows, eight at most).
static bool fs_pack_decide(int d, int n_coef, int nc, const uint8_t *small, FsPack *pk) {
    memset(pk, 0, sizeof *pk);
    const int n_out = n_coef + nc, rem = n_out - 16 * ((n_out + 15) / 16 - 1);
    if ((int64_t)d * 8 * 128 * 128 > MM8_BIAS_PACK) return false;
    if (rem <= 8) { pk->nm = rem; return true; }
    if (rem == 16) return false;
    int ns = 0;
    for (int i = n_coef - 1; i >= 0 && ns < 8; i--)
        if (small[i]) pk->single[ns++] = (uint8_t)i;
    std::reverse(pk->single, pk->single + ns);
    if (rem - ns > 4) { memset(pk, 0, sizeof *pk); return false; }      // (rem > 8: where this holds ns >= 5, and regs 1 and 3 both hold rows)
    pk->nm = rem - ns; pk->ns = ns;
    return true;
}
constexpr int FS_CAND_MAXN = 128;               // parties a candidate store is built for (n d 128-bit entries in the builder's LDS)

// ---------------------------------------------------------------------------------------------------------------------
// the kernel
// ---------------------------------------------------------------------------------------------------------------------
// LDS: row constants [n_rt * 16][16] | matrix digits [n_rt][NKB][2][64] x 16 B | two element buffers [4 tiles][NKB][2][2][64] x 16 B |
// rowl[32] | maskl[16 n_rt] | fold table
// | (ms_d > 0: the launch divides by den on the matrix cores) the tables of fs_ms_q(ms_d)
__host__ __device__ inline int fs_ms_q(int d) { return d * 64 + d * 8; }      // in uint4: per term a 1 KB row of digits, then per term 128 B of constants
__host__ __device__ inline size_t fs_lds_bytes(int n_rt, int nkb, int ms_d = 0) {
    return ((size_t)n_rt * 64 + (size_t)n_rt * nkb * 2 * 64 + (size_t)2 * FS_TPW * nkb * 4 * 64 + MM8_FOLD_Q + (ms_d ? fs_ms_q(ms_d) : 0)) * 16 +
           (size_t)(32 + 16 * n_rt) * 4;
}

// The reduction of one output of lane (n, g) in k_mm8f, as TEXT (a lambda with this body costs the kernel registers it does not have: the
// instance without a packed tile must stay the code it was).  I_: the image slot (its mode and constant); F_(k), k < 12: the output's columns
// (4k+1, 4k+2) as lo + 256 hi; E_(k), k < 11: columns (4k+3, 4k+4) likewise; C0_: column 0.  A packed pass hands it the same 47 columns,
// summed from its two digit groups.  Uses the kernel's locals (chunk, n, lane, the opaque constants, the tables in LDS).  Notes on the body:
//   * the compared row is loaded unconditionally (from the buffer's first element when there is nothing to compare): a load under `cmp`
//     makes hipcc wrap the whole reduction in that divergent branch, and the register copies at its join spill
//   * glo / ghi are G_7 .. G_11; `top` is bit 256 of the remainder (r < 2p < 2^257)
//   * the empty asm keeps the reduction outside the exec masks of the compare and the store (same reason as the load)
//   * disagreements are reported once per wave and output (an adversary that corrupts everything would otherwise queue a million atomics
//     on one word: 430 us instead of 55 for config 3's launch): lane (n, g) holds chunk tile_base + n, so the sixteen chunk bits of the
//     wave are the OR of its four lane groups
#define FS_REDUCE(I_, F_, E_, C0_) \
    do { \
        const int i = (I_); \
        const int md = maskl[i]; \
        const bool live = chunk < n_chunks; \
        const bool cmp = live && md > 0, st = live && md < 0; \
        uint32_t ew[8]; \
        load_words<8>(ew, in_pk + (cmp ? (chunk * in_sc + (int64_t)(md - 1) * in_sl) * 8 : 0)); \
        uint64_t pw[8]; \
        { \
            const uint4 *cr = reinterpret_cast<const uint4 *>(crl + (size_t)i * 16); \
        _Pragma("unroll") \
            for (int k = 0; k < 4; k++) { \
                const uint4 c = cr[k]; \
                pw[2 * k] = (uint64_t)c.x | ((uint64_t)c.y << 32); \
                pw[2 * k + 1] = (uint64_t)c.z | ((uint64_t)c.w << 32); \
            } \
        } \
        uint32_t glo[5], ghi[5]; \
        _Pragma("unroll") \
        for (int k = 0; k < 12; k++) { \
            uint64_t gk = (uint64_t)F_(k) * k256 + (k < 7 ? pw[k] : 0ull); \
            if (k < 11) gk += (uint64_t)E_(k) * k16m; \
            if (k < 7) pw[k] = gk; \
            else { glo[k - 7] = (uint32_t)gk; ghi[k - 7] = (uint32_t)(gk >> 32); } \
        } \
        pw[0] += (uint64_t)(C0_) * u1; \
        pw[7] += (uint64_t)glo[0] * u1; \
        uint32_t hw[5]; \
        { \
            unsigned cyw = 0; \
        _Pragma("unroll") \
            for (int k = 0; k < 4; k++) hw[k] = __builtin_addc(glo[k + 1], ghi[k], cyw, &cyw); \
            hw[4] = ghi[4] + cyw; \
        } \
        v4i hb; \
        _Pragma("unroll") \
        for (int k = 0; k < 4; k++) hb[k] = (int)(hw[k] ^ 0x80808080u); \
        v4i dcol[8]; \
        _Pragma("unroll") \
        for (int eb = 0; eb < 8; eb++) \
            dcol[eb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fold_lane[eb * (MM8_FOLD_ROW / 16)], hb, v4i{0, 0, 0, 0}, 0, 0, 0); \
        _Pragma("unroll") \
        for (int k = 0; k < 8; k++) pw[k] += (uint64_t)hw[4] * bp.c384[k]; \
        _Pragma("unroll") \
        for (int k = 0; k < 8; k++) { \
            int64_t tt = (int64_t)pw[k] + (int64_t)dcol[k][0] * s1; \
            tt += (int64_t)dcol[k][1] * s256; \
            tt += (int64_t)dcol[k][2] * s64k; \
            tt += (int64_t)dcol[k][3] * s16m; \
            pw[k] = (uint64_t)tt; \
        } \
        const uint64_t tq = pw[7] + (pw[6] >> 32); \
        const uint32_t qh = (uint32_t)(((uint64_t)(uint32_t)(tq >> 16) * bp.mu) >> 46); \
        _Pragma("unroll") \
        for (int k = 0; k < 8; k++) pw[k] += (uint64_t)qh * bp.pneg[k]; \
        uint32_t ow[8]; \
        uint32_t top; \
        { \
            unsigned cy = 0; \
            ow[0] = (uint32_t)pw[0]; \
        _Pragma("unroll") \
            for (int k = 1; k < 8; k++) ow[k] = __builtin_addc((uint32_t)pw[k], (uint32_t)(pw[k - 1] >> 32), cy, &cy); \
            top = (uint32_t)(pw[7] >> 32) + cy - qh; \
        } \
        if (__builtin_amdgcn_ballot_w64(top != 0 || ow[7] >= ~bp.pneg[7]) != 0) { \
            uint32_t u[8]; \
            unsigned cy2 = 0; \
        _Pragma("unroll") \
            for (int k = 0; k < 8; k++) u[k] = __builtin_addc(ow[k], bp.pneg[k], cy2, &cy2); \
            const bool take = cy2 || top; \
        _Pragma("unroll") \
            for (int k = 0; k < 8; k++) ow[k] = take ? u[k] : ow[k]; \
        } \
        uint32_t diff = 0; \
        _Pragma("unroll") \
        for (int k = 0; k < 8; k++) diff |= ew[k] ^ ow[k]; \
        asm volatile("" : "+v"(diff), "+v"(ow[0]), "+v"(ow[1]), "+v"(ow[2]), "+v"(ow[3]), "+v"(ow[4]), "+v"(ow[5]), "+v"(ow[6]), "+v"(ow[7])); \
        const unsigned long long bad_lanes = __builtin_amdgcn_ballot_w64(cmp && diff); \
        if (bad_lanes) { \
            const uint32_t bits16 = (uint32_t)((bad_lanes | (bad_lanes >> 16) | (bad_lanes >> 32) | (bad_lanes >> 48)) & 0xffffull); \
            if (lane == 0) { \
                const int64_t tile_base = chunk - n; \
                const int32_t cmin = (int32_t)tile_base + __builtin_ctz(bits16); \
                if (*reinterpret_cast<volatile int32_t *>(mismatch) == 0) atomicOr(mismatch, 1); \
                if (first_bad && *reinterpret_cast<volatile int32_t *>(first_bad) > cmin) atomicMin(first_bad, cmin); \
                if (bad_map) atomicOr(bad_map + (tile_base >> 5), bits16 << (tile_base & 31)); \
            } \
        } \
        const int64_t oidx = chunk * out_sc + (int64_t)(-md - 1) * out_sl; \
        if (st && oidx < out_count) store_words<8>(out_pk + oidx * 8, ow); \
    } while (0)

// rowmode[i]: 0 = nothing, v > 0: compare the sum with row v - 1 of the input buffer, v < 0: store it as output row -v - 1
// PK: the last row tile is a packed one (FsPack) -- 1: merged outputs alone (regs 0 and 1, each with its partner two regs up), 2: up to four
// merged outputs (reg 0) and five to eight single-group rows (regs 1 and 3); the image's rows are then its 16 n_rt slots, and no row is
// picked.  PK = 0 is the kernel as it was: what a decoder launches, and every image whose last tile does not pack.
// MSC: the received columns are divided by den on the matrix cores (the tables MS; fs_mscale) instead of by the T_q multiplication (KT)
template <int NKB, int PK, bool MSC>
__global__ __launch_bounds__(64 * FS_WAVES, 2) void k_mm8f(const int4 *__restrict__ a8, const uint32_t *__restrict__ crowd, const v4i *__restrict__ foldg,
                                                          const uint32_t *__restrict__ KT, const PrescaleParams PP,
                                                          const uint32_t *__restrict__ in_pk, int64_t in_sc, int64_t in_sl, const int32_t *__restrict__ in_rows,
                                                          int64_t in_count, int d, const int32_t *__restrict__ rowmode,
                                                          uint32_t *__restrict__ out_pk, int64_t out_sc, int64_t out_sl, int64_t out_count,
                                                          int32_t *__restrict__ mismatch, int32_t *__restrict__ first_bad, uint32_t *__restrict__ bad_map,
                                                          int n_out, int n_rt, int64_t n_chunks, int64_t n_units, BarrettParams bp, const FsDone done, const FsPick pick,
                                                          const FsSplit split, const v4i *__restrict__ MS) {
    constexpr bool PACKED = PK != 0;
    const int n_slots = PACKED ? 16 * n_rt : n_out;      // rows of the image (PACKED: n_out goes unused)
    constexpr int NT = 64 * FS_WAVES, NL = 9, NW = 8;
    extern __shared__ uint4 fs_lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = lane & 15, g = lane >> 4;
    uint32_t *crl = reinterpret_cast<uint32_t *>(fs_lds);
    int4 *abuf = reinterpret_cast<int4 *>(fs_lds + n_rt * 64);
    uint4 *xbuf = fs_lds + n_rt * 64 + n_rt * NKB * 2 * 64;
    constexpr int bufsz = FS_TPW * NKB * 4 * 64;
    int32_t *rowl = reinterpret_cast<int32_t *>(xbuf + 2 * bufsz);
    int32_t *maskl = rowl + 32;
    v4i *foldl = reinterpret_cast<v4i *>(maskl + 16 * n_rt);
    v4i *msl = foldl + MM8_FOLD_Q;                  // (MS: the tables of the division by den on the matrix cores, fs_ms_q(d) pieces)

#ifdef HB_MM8_TIMING
    unsigned long long tacc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tlast = __builtin_amdgcn_s_memtime();
#endif
    // one scaling task = term l of a unit's 64 chunks: lane = chunk (tile lane >> 4, column lane & 15).  The first unit's tasks run in the
    // prologue, before any table is in LDS: they take the row of a term from in_rows itself (wave-uniform: a scalar load)
    auto unit_chunk = [&](int64_t unit) {
        const int64_t chunk = unit * 64 + lane;
        return chunk >= n_chunks ? n_chunks - 1 : chunk;          // (results of padding chunks are never stored or compared)
    };
    // MSC: a task is two dense 32x32x32 products (32 columns x 32 chunks x 32 bytes), so lane (r, h) = (lane & 31, lane >> 5) loads bytes
    // 16 h .. 16 h + 15 of chunk r of the unit (w[0 .. 3]) and of chunk 32 + r (w[4 .. 7]): the row, the clamp and the bound as fetch_row
    // has them, per source chunk.  okk is the test of the lane's OWN chunk (chunk = lane, as everywhere behind the half swap)
    auto fetch_halves = [&](int64_t unit, int row, uint32_t (&w)[NW], bool &okk) {
        const int r = lane & 31, h = lane >> 5;
        bool oks[2];
#pragma unroll
        for (int s = 0; s < 2; s++) {
            int64_t chunk = unit * 64 + 32 * s + r;
            chunk = chunk >= n_chunks ? n_chunks - 1 : chunk;
            const int64_t idx = chunk * in_sc + (int64_t)row * in_sl;
            oks[s] = idx < in_count;
            const uint4 v = *reinterpret_cast<const uint4 *>(in_pk + (oks[s] ? idx : 0) * NW + 4 * h);
            w[4 * s] = v.x; w[4 * s + 1] = v.y; w[4 * s + 2] = v.z; w[4 * s + 3] = v.w;
        }
        okk = h ? oks[1] : oks[0];
    };
    auto fetch_row = [&](int64_t chunk, int row, uint32_t (&w)[NW], bool &okk) {
        const int64_t idx = chunk * in_sc + (int64_t)row * in_sl;
        okk = idx < in_count;
        load_words<NW>(w, in_pk + (okk ? idx : 0) * NW);
    };
    // ---- prologue: the first unit's first loads, tables, zeros for the terms d .. 8 NKB - 1 (never written again) ---------
    // every wave takes its share of the first unit (terms wave, wave + 8, wave + 16): the loads of its first term are issued ahead of the
    // tables' copy and return under it (the T_q multiplication; MSC: below)
    const uint32_t first_terms = (0x01010101u << wave) & (d < 32 ? (1u << d) - 1u : ~0u);
    uint32_t x_first[NW] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool ok_first = false;
    // MSC: the words of ALL of the wave's terms (NKB at most: d <= 8 NKB), loaded BEHIND the tables' loads below (the copy then waits for the
    // tables alone, not for HBM).  A term the wave does not have (l >= d) loads term d - 1's words and is masked: a load under a branch is
    // waited for where the branch joins
    uint32_t xf[MSC ? NKB : 1][NW];
    bool okf[MSC ? NKB : 1];
    if (!MSC && first_terms) {
        const int l0 = __builtin_ctz(first_terms);
        fetch_row(unit_chunk(blockIdx.x), in_rows ? in_rows[l0] : l0, x_first, ok_first);
    }
    // the rows of the compared senders were built per PARTY when the first d arrivals were known (k_fs_cand); which of them this launch
    // compares, and in which row, is only known now: their digit pieces and row constants are FETCHED here, ahead of the tables' copy (two
    // dependent loads, the sender's number and then its row: they ride under the copy), and written over the image's empty rows behind it
    uint4 pk_piece = make_uint4(0, 0, 0, 0), pk_crow = make_uint4(0, 0, 0, 0);
    const int pk_e = threadIdx.x;
    const bool pk_has_piece = !PACKED && pick.cand && pk_e < pick.nc * NKB * 8, pk_has_crow = !PACKED && pick.cand && pk_e < pick.nc * 4;
    // (one piece a thread ahead of the copy: config 3's 21 compared rows are 504 pieces for the 512 threads; what a larger launch has beyond
    // that is fetched behind the copy, below -- five pieces a thread in registers went to scratch memory)
    if (pk_has_piece) {
        const int j = pk_e / (NKB * 8), pc = pk_e - j * (NKB * 8);
        pk_piece = pick.cand[(size_t)pick.zc[j] * (NKB * 8) + pc];
    }
    if (pk_has_crow) pk_crow = reinterpret_cast<const uint4 *>(pick.cand_crow)[(size_t)pick.zc[pk_e >> 2] * 4 + (pk_e & 3)];
    // the tables.  Every load of a thread is in flight before its first word is written to LDS (addresses clamped, so that no load stands
    // under a branch; the image three pieces a thread at a time: config 3's 1152 pieces are one round) -- a copy loop of load, wait, write
    // pays the loads' latency once per trip, and one table after the other
    {
        const int tid = threadIdx.x, n_mask = n_rt * 16, n_crow = n_rt * 64, n_img = n_rt * NKB * 2 * 64;
        const int lc = tid < d ? tid : d - 1;
        int32_t rw = in_rows ? in_rows[lc] : lc;
        int32_t mk = rowmode[tid < n_slots ? tid : 0];
        v4i cr = reinterpret_cast<const v4i *>(crowd)[tid < n_crow ? tid : 0];
        v4i fo = foldg[tid < MM8_FOLD_Q ? tid : 0];
        v4i img[3];
#pragma unroll
        for (int k = 0; k < 3; k++) img[k] = reinterpret_cast<const v4i *>(a8)[tid + k * NT < n_img ? tid + k * NT : 0];
        // MSC: the division's tables go to LDS by OWNER -- a wave copies the rows of its own terms wave, wave + 8, ... (64 pieces a row: one
        // piece a lane) and their constants (8 pieces a term: lanes 0 .. 8 NKB - 1).  So the first
        // unit's tasks read their operands from LDS that their own wave wrote: no barrier, and no second fetch of the same rows from
        // global memory.  A term the wave does not have (l >= d) copies row d - 1 again (the same words as its owner writes).
        const int ms_lj = wave + 8 * (lane >> 3), ms_cq = d * 64 + (ms_lj < d ? ms_lj : d - 1) * 8 + (lane & 7);
        v4i msv[MSC ? NKB + 1 : 1];
        if constexpr (MSC) {
#pragma unroll
            for (int j = 0; j < NKB; j++) {
                const int l = wave + 8 * j, lc = l < d ? l : d - 1;
                msv[j] = MS[lc * 64 + lane];
            }
            msv[NKB] = MS[ms_cq];
#pragma unroll
            for (int j = 0; j < NKB; j++) {
                const int l = wave + 8 * j, lc = l < d ? l : d - 1;
                fetch_halves(blockIdx.x, in_rows ? in_rows[lc] : lc, xf[j], okf[j]);
                okf[j] = okf[j] && l < d;
            }
        }
        // (the words are wanted HERE: hipcc otherwise sinks each load into the branch of its write, one wait per load again)
        asm volatile("" : "+v"(rw), "+v"(mk), "+v"(cr), "+v"(fo), "+v"(img[0]), "+v"(img[1]), "+v"(img[2]));
        if constexpr (MSC) {
#pragma unroll
            for (int j = 0; j <= NKB; j++) asm volatile("" : "+v"(msv[j]));
        }
        if (tid < 32) rowl[tid] = rw;
        if (tid < n_mask) maskl[tid] = tid < n_slots ? mk : 0;
        if (tid < n_crow) reinterpret_cast<v4i *>(fs_lds)[tid] = cr;
        if (tid < MM8_FOLD_Q) foldl[tid] = fo;
#pragma unroll
        for (int k = 0; k < 3; k++)
            if (tid + k * NT < n_img) reinterpret_cast<v4i *>(abuf)[tid + k * NT] = img[k];
        if constexpr (MSC) {
#pragma unroll
            for (int j = 0; j < NKB; j++) {
                const int l = wave + 8 * j, lc = l < d ? l : d - 1;
                msl[lc * 64 + lane] = msv[j];
            }
            if (lane < 8 * NKB) msl[ms_cq] = msv[NKB];
        }
        // (what a larger launch has beyond one round)
        for (int i = tid + NT; i < n_mask; i += NT) maskl[i] = i < n_slots ? rowmode[i] : 0;
        for (int i = tid + NT; i < n_crow; i += NT) fs_lds[i] = reinterpret_cast<const uint4 *>(crowd)[i];
        for (int i = tid + 3 * NT; i < n_img; i += NT) abuf[i] = a8[i];
    }
    // the slots [buffer][tile][half][column] of a padding term, 256 in all: no scaling task ever writes them, and they are all that is
    // zeroed -- every other slot is written by the unit's scaling tasks before a pass reads it
    // (MSC: the buffers hold biased bytes in the interleaved granules of put_biased below -- a padding term's dwords are the same 256 bytes
    // a buffer and tile, positions e and 2 + e of its lane's four granules; its matrix digits are zero, so zeros serve there too)
    for (int i = threadIdx.x; i < (8 * NKB - d) * 256; i += NT) {
        const int l = d + (i >> 8), b = (i >> 7) & 1, t = (i >> 5) & 3, h = (i >> 4) & 1, c = i & 15;
        const int kb = l >> 3, gg = (l & 7) >> 1, e = l & 1;
        if constexpr (MSC) {
            uint32_t *gr = reinterpret_cast<uint32_t *>(xbuf + (size_t)b * bufsz + (size_t)(((t * NKB + kb) * 4 + 2 * h) * 64) + (c + 16 * gg)) + e;
            gr[0] = 0; gr[2] = 0; gr[256] = 0; gr[258] = 0;
        } else
            xbuf[(size_t)b * bufsz + (size_t)((((t * NKB + kb) * 2 + e) * 2 + h) * 64) + (c + 16 * gg)] = make_uint4(0, 0, 0, 0);
    }
    // MSC: a scaled element enters LDS as the passes' B operand wants it (gen_mm8.py, the pre-biased phases): every byte XOR 0x80, and
    // granule j of lane (n, gg) of K-block kb holds {e0[2j], e1[2j], e0[2j+1], e1[2j+1]} -- element e's words 2 j and 2 j + 1 at dwords e
    // and 2 + e.  The lane and its four granules (slots 4 (t NKB + kb) + j) are the ones the raw layout gives the pair of elements
    auto put_biased = [&](uint4 *dst, int t, int kb, int gg, int e, const uint32_t (&w)[NW]) __attribute__((always_inline)) {
        uint32_t *gr = reinterpret_cast<uint32_t *>(dst + (size_t)((t * NKB + kb) * 4) * 64 + (n + 16 * gg)) + e;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            gr[256 * j] = w[2 * j] ^ 0x80808080u;
            gr[256 * j + 2] = w[2 * j + 1] ^ 0x80808080u;
        }
    };
    // (tile, row tile) pairs of a unit: wave w takes w, w + 8, ...; which terms of the next unit a wave scales beside its passes: split.terms
    const int n_pairs = FS_TPW * n_rt;
    const uint32_t my_terms = (uint32_t)__builtin_amdgcn_readfirstlane((int)split.terms[wave]);

    uint32_t ms64k = 1u << 16;                   // opaque: a word of the matrix-core division is one v_mad_u64_u32 over two shifted adds
    if constexpr (MSC) asm volatile("" : "+s"(ms64k));
    // ---- the division by den on the matrix cores: x / den_l = sum_b x_b U_l[b] over the element's 32 bytes, U_l[b] = 256^b / den_l as 32
    // balanced digits.  U_l is the same for every chunk, so a task is the dense product [32 columns] x [32 bytes] x [64 chunks]: two
    // independent v_mfma_i32_32x32x32_i8, chunks 0 .. 31 and 32 .. 63 of the unit.  Lane (r, h):
    //   B  its 16 bytes 16 h .. 16 h + 15 of chunk r (and of chunk 32 + r), XOR 0x80 (fetch_halves)
    //   A  byte j = digit r of U_l[16 h + j]: piece l * 64 + lane of the tables, the same for both products (whatever order the hardware
    //      gives the 32 values of K, element j of A's lane (m, h) meets element j of B's lane (n, h): the sum over K is all that counts)
    //   C  2^20 + byte c of the term's constant (128 sum_b U_l[b] - the biases, mod p), c = (i & 3) + 8 (i >> 2) + 4 h for register i
    //      (the 32x32 accumulator map: column = lane & 31, row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5)): pieces d * 64 + l * 8 + 4 h ..
    // Every column arrives positive and below 2^21 (tests/fs_mscale_model.py has the bounds; tests/fs_mscale32_model.py these maps).
    typedef int v16i __attribute__((ext_vector_type(16)));
    const v4i *ms_al = msl + lane, *ms_cl = msl + d * 64 + 4 * (lane >> 5);
    auto ms_products = [&](int l, const uint32_t (&x)[NW], v16i &acc0, v16i &acc1) __attribute__((always_inline)) {
        const v4i a = ms_al[l * 64];
        const v4i *cl = ms_cl + l * 8;
        v16i c;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const v4i cq = cl[q];
#pragma unroll
            for (int k = 0; k < 4; k++) c[4 * q + k] = cq[k];
        }
        const v4i b0 = v4i{(int)(x[0] ^ 0x80808080u), (int)(x[1] ^ 0x80808080u), (int)(x[2] ^ 0x80808080u), (int)(x[3] ^ 0x80808080u)};
        const v4i b1 = v4i{(int)(x[4] ^ 0x80808080u), (int)(x[5] ^ 0x80808080u), (int)(x[6] ^ 0x80808080u), (int)(x[7] ^ 0x80808080u)};
        acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b0, c, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b1, c, 0, 0, 0);
    };
    // The words: lane (r, h) holds the columns of the 32-bit-word addends 2 q + h, q < 4, of chunk r in acc0 and of chunk 32 + r in acc1
    // (an addend is two shifted adds and one multiply-add, below 2^46).  The half swap (lanes 32 .. 63 of the destination against lanes
    // 0 .. 31 of the source) with acc0's addends as destination and acc1's as source leaves the even addends of chunk = lane in the
    // destination and the odd ones in the source, in every lane: from there on lane = chunk again
    auto ms_words = [&](const v16i &acc0, const v16i &acc1, uint64_t (&mw)[8]) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            uint64_t ad[2];
#pragma unroll
            for (int s = 0; s < 2; s++) {
                const v16i &m = s ? acc1 : acc0;
                const uint32_t lo = (uint32_t)m[4 * q] + ((uint32_t)m[4 * q + 1] << 8), hi = (uint32_t)m[4 * q + 2] + ((uint32_t)m[4 * q + 3] << 8);
                ad[s] = (uint64_t)hi * ms64k + lo;
            }
            const auto slo = __builtin_amdgcn_permlane32_swap((uint32_t)ad[0], (uint32_t)ad[1], false, false);
            const auto shi = __builtin_amdgcn_permlane32_swap((uint32_t)(ad[0] >> 32), (uint32_t)(ad[1] >> 32), false, false);
            mw[2 * q] = (uint64_t)slo[0] | ((uint64_t)shi[0] << 32);
            mw[2 * q + 1] = (uint64_t)slo[1] | ((uint64_t)shi[1] << 32);
        }
    };
    // T_q of a task's term is wave-uniform (scalar loads).  first: the prologue's call -- its first term's words are already in registers
    // (x_first), and rowl is not in LDS yet
    auto scale_unit = [&](auto first, int64_t unit, uint4 *dst, uint32_t terms) {
        constexpr bool FIRST = decltype(first)::value;
        const int64_t chunk = unit_chunk(unit);
        const int t = lane >> 4;
        uint32_t xw[NW];
        bool ok = false;
        auto fetch = [&](int l, uint32_t (&w)[NW], bool &okk) {
            if constexpr (MSC) fetch_halves(unit, rowl[l], w, okk);
            else fetch_row(chunk, FIRST ? (in_rows ? in_rows[l] : l) : rowl[l], w, okk);
        };
        terms &= d < 32 ? (1u << d) - 1u : ~0u;
        int l = terms ? __builtin_ctz(terms) : d;
        if constexpr (FIRST) {
#pragma unroll
            for (int k = 0; k < NW; k++) xw[k] = x_first[k];
            ok = ok_first;
        } else if (l < d) fetch(l, xw, ok);
        while (l < d) {
            terms &= terms - 1u;
            const int ln = terms ? __builtin_ctz(terms) : d;
            // the next term's words, in flight under this term's arithmetic.  Unconditional: hipcc waits for a load issued under a branch
            // where the branch joins -- here, ahead of this term's arithmetic, with the whole latency exposed once per task -- so the last
            // task loads its own words again (a cache hit that nobody reads)
            uint32_t xn[NW];
            bool okn = false;
            fetch(ln < d ? ln : l, xn, okn);
            uint32_t w[NW];
            bool over;                  // bit 256 of the representative r < 2p that w holds the low 256 bits of
            if constexpr (MSC) {
                // ---- on the matrix cores (ms_products, ms_words above): two independent 32x32x32 products of the term's digits with the
                // halves this lane loaded, the words' addends, the half swap -- and the quotient is FS_REDUCE's, with lane = chunk.
                //
                // The first unit's tasks are a block of their own, below, where this lambda's `first` call stands for the T_q multiplication.
                static_assert(!FIRST, "the first unit's matrix-core tasks are the block at the call site");
                v16i acc0, acc1;
                ms_products(l, xw, acc0, acc1);
                uint64_t mw[8];
                ms_words(acc0, acc1, mw);
                const uint64_t tq = mw[7] + (mw[6] >> 32);
                const uint32_t mq = (uint32_t)(((uint64_t)(uint32_t)(tq >> 16) * bp.mu) >> 46);
#pragma unroll
                for (int k = 0; k < 8; k++) mw[k] += (uint64_t)mq * bp.pneg[k];
                unsigned cyw = 0;
                w[0] = (uint32_t)mw[0];
#pragma unroll
                for (int k = 1; k < 8; k++) w[k] = __builtin_addc((uint32_t)mw[k], (uint32_t)(mw[k - 1] >> 32), cyw, &cyw);
                over = (uint32_t)(mw[7] >> 32) + cyw != mq;
            } else {
                const uint32_t *__restrict__ T = KT + (size_t)l * (NL * NL);
                uint32_t xd[NL];
                unpack<NL, NW>(xd, xw);
                uint64_t col[NL + 1];
#pragma unroll
                for (int j = 0; j <= NL; j++) col[j] = 0;
#pragma unroll
                for (int q = 0; q < NL; q++)
#pragma unroll
                    for (int j = 0; j < NL; j++) col[j] += (uint64_t)xd[q] * T[q * NL + j];
                uint32_t v[NL + 1];
#pragma unroll
                for (int k = 0; k < NL; k++) { v[k] = (uint32_t)col[k] & DMASK; col[k + 1] += col[k] >> LB; }
                v[NL] = (uint32_t)col[NL];
                const uint64_t mid = (uint64_t)v[9] * PP.m0 + (uint64_t)v[8] * PP.m1 + (((uint64_t)v[8] * PP.m0) >> LB);
                const uint64_t qh = (uint64_t)v[9] * PP.m1 + (mid >> LB);
                const uint32_t q0 = (uint32_t)qh & DMASK, q1 = (uint32_t)(qh >> LB);
                uint64_t dc[NL];
#pragma unroll
                for (int k = 0; k < NL; k++) {
                    dc[k] = v[k] + (uint64_t)q0 * PP.pbar[k];
                    if (k > 0) dc[k] += (uint64_t)q1 * PP.pbar[k - 1];
                }
                uint32_t r[NL];
#pragma unroll
                for (int k = 0; k < NL; k++) {
                    r[k] = (uint32_t)dc[k] & DMASK;
                    if (k < NL - 1) dc[k + 1] += dc[k] >> LB;
                }
                pack<NL, NW>(w, r);
                over = (r[NL - 1] >> 24) != 0;
            }
            const uint32_t *pneg = MSC ? bp.pneg : PP.pneg;       // (the same words: whichever the instance holds already)
            if (pneg[NW - 1] >> 31) {
                // p < 2^255: r < 2p < 2^256 is a 256-bit representative as it is, and the GEMM takes any
#pragma unroll
                for (int k = 0; k < NW; k++) w[k] = ok ? w[k] : 0u;
            } else {
                // r < 2p may pass 2^256, where the packed words would drop bit 256: made canonical
                uint32_t u[NW];
                unsigned cy = 0;
#pragma unroll
                for (int k = 0; k < NW; k++) u[k] = __builtin_addc(w[k], pneg[k], cy, &cy);
                const bool take = cy || over;
#pragma unroll
                for (int k = 0; k < NW; k++) w[k] = ok ? (take ? u[k] : w[k]) : 0u;
            }
            const int kb = l >> 3, gg = (l & 7) >> 1, e = l & 1;
            if constexpr (MSC) put_biased(dst, t, kb, gg, e, w);
            else {
                uint4 *slot = dst + (size_t)(((t * NKB + kb) * 2 + e) * 2) * 64 + (n + 16 * gg);
                slot[0] = make_uint4(w[0], w[1], w[2], w[3]);
                slot[64] = make_uint4(w[4], w[5], w[6], w[7]);
            }
#pragma unroll
            for (int k = 0; k < NW; k++) xw[k] = xn[k];
            ok = okn;
            l = ln;
        }
    };

    // the first unit: every wave scales its share into buffer 0.  Nothing it touches depends on the tables (the padding slots are other
    // slots), so no barrier stands between the copy and this: the loop's first barrier covers both
    if constexpr (MSC) {
        // All eight waves only scale here: the wave's terms wave, wave + 8, ... as ONE straight-line block (scale_unit's arithmetic term by
        // term).  What the head waits for is the first unit's words from HBM, every workgroup's at once, and vector loads return in order:
        // so the words' loads are the LAST vector loads of the prologue, the operands are LDS reads (the rows this wave copied itself,
        // above), and term j's MFMAs wait for term j's words alone -- its words, quotient and carries then run in one block with the
        // MFMAs of term j + 1, under the arrival of the later words.  (Operands from the tables in global memory: their loads queue
        // behind every word load that was issued ahead of them, and the whole block waits for the last word.)
        const int t = lane >> 4;
        auto first_block = [&](auto canon_c) __attribute__((always_inline)) {
            constexpr bool CANON = decltype(canon_c)::value;      // p >= 2^255: r < 2p may pass 2^256, made canonical (scale_unit)
            v16i mc[NKB][2];
#pragma unroll
            for (int s = 0; s <= NKB; s++) {
                if (s < NKB) {
                    // the two products of term s: they wait for ITS words alone (the loads return in order), the operands are LDS reads
                    const int j = s, l = wave + 8 * j, lc = l < d ? l : d - 1;
                    ms_products(lc, xf[j], mc[j][0], mc[j][1]);
                }
                if (s > 0) {
                    // the words, the half swap, the quotient and the carries of term s - 1, in one block with the next term's MFMAs
                    const int j = s - 1, l = wave + 8 * j;
                    uint64_t mw[8];
                    ms_words(mc[j][0], mc[j][1], mw);
                    const uint64_t tq = mw[7] + (mw[6] >> 32);
                    const uint32_t mq = (uint32_t)(((uint64_t)(uint32_t)(tq >> 16) * bp.mu) >> 46);
#pragma unroll
                    for (int k = 0; k < 8; k++) mw[k] += (uint64_t)mq * bp.pneg[k];
                    uint32_t w[NW];
                    unsigned cyw = 0;
                    w[0] = (uint32_t)mw[0];
#pragma unroll
                    for (int k = 1; k < 8; k++) w[k] = __builtin_addc((uint32_t)mw[k], (uint32_t)(mw[k - 1] >> 32), cyw, &cyw);
                    if constexpr (CANON) {
                        const bool over = (uint32_t)(mw[7] >> 32) + cyw != mq;
                        uint32_t u[NW];
                        unsigned cy = 0;
#pragma unroll
                        for (int k = 0; k < NW; k++) u[k] = __builtin_addc(w[k], bp.pneg[k], cy, &cy);
                        const bool take = cy || over;
#pragma unroll
                        for (int k = 0; k < NW; k++) w[k] = okf[j] ? (take ? u[k] : w[k]) : 0u;
                    } else {
#pragma unroll
                        for (int k = 0; k < NW; k++) w[k] = okf[j] ? w[k] : 0u;
                    }
                    // (a term the wave does not have is a padding term of K-block j: its digits are zero, whatever its dwords hold)
                    put_biased(xbuf, t, j, (l & 7) >> 1, l & 1, w);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        if (bp.pneg[NW - 1] >> 31) first_block(std::false_type{});
        else first_block(std::true_type{});
    } else
        scale_unit(std::true_type{}, blockIdx.x, xbuf, first_terms);
    if (!PACKED && pick.cand) {
        __syncthreads();      // (the image's copy is in LDS: the picked rows go over its empty rows)
        auto put = [&](int e, const uint4 &v) {
            const int j = e / (NKB * 8), pc = e - j * (NKB * 8);
            const int ri = pick.n_coef + j, rt = ri >> 4, r16 = ri & 15, r = 4 * (r16 & 3) + (r16 >> 2);
            const int kb = pc >> 3, grp = (pc >> 2) & 1, gg = pc & 3;
            reinterpret_cast<uint4 *>(abuf)[((rt * NKB + kb) * 2 + grp) * 64 + r + 16 * gg] = v;
        };
        if (pk_has_piece) put(pk_e, pk_piece);
        for (int e = pk_e + NT; e < pick.nc * NKB * 8; e += NT) {
            const int j = e / (NKB * 8), pc = e - j * (NKB * 8);
            put(e, pick.cand[(size_t)pick.zc[j] * (NKB * 8) + pc]);
        }
        if (pk_has_crow) fs_lds[(pick.n_coef + (pk_e >> 2)) * 4 + (pk_e & 3)] = pk_crow;
        for (int j = threadIdx.x; j < pick.nc; j += NT) maskl[pick.n_coef + j] = (int32_t)pick.zc[j] + 1;
    }

    const v4i biasv = v4i{MM8_BIAS, MM8_BIAS, MM8_BIAS, MM8_BIAS};
    uint32_t k256 = 256u, k16m = 1u << 24;      // opaque, so that the word assembly stays two v_mad_u64_u32 per word
    int32_t s1 = 1, s256 = 256, s64k = 1 << 16, s16m = 1 << 24;   // and the gathering of the fold's columns one v_mad_i64_i32 each
    uint32_t u1 = 1u;
    asm volatile("" : "+s"(k256), "+s"(k16m), "+s"(s1), "+s"(s256), "+s"(s64k), "+s"(s16m), "+s"(u1));
    // the fold's A operand: lane (m, g') of the diagonal block g' = m / 4 reads its 16 digits, every other lane the row's zero bytes
    const v4i *fold_lane = reinterpret_cast<const v4i *>(reinterpret_cast<const char *>(foldl) + (g == (n >> 2) ? 16 * n : 256));

    int buf = 0;
    int64_t unit = blockIdx.x;
    FS_T(0);
    for (; unit < n_units; unit += gridDim.x, buf ^= 1) {
        // every wave's share of this unit's elements is in LDS, and nobody reads the other buffer any more
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        FS_T(7);
        __builtin_amdgcn_s_barrier();
        FS_T(1);
        if (my_terms && unit + gridDim.x < n_units) scale_unit(std::false_type{}, unit + gridDim.x, xbuf + (size_t)(buf ^ 1) * bufsz, my_terms);
        FS_T(2);
        for (int pidx = wave; pidx < n_pairs; pidx += FS_WAVES) {
            // two row tiles: the waves of one SIMD (w and w + 4) get one of each, so the ragged second tile's shorter passes spread evenly
            const int tl = n_rt == 2 ? (pidx >> 1) : pidx / n_rt;
            const int rt = n_rt == 2 ? ((pidx ^ (pidx >> 2)) & 1) : pidx - tl * n_rt;
            const int64_t chunk = (unit * FS_TPW + tl) * 16 + n;
            const uint4 *xs = xbuf + (size_t)buf * bufsz + (size_t)tl * NKB * 4 * 64 + lane;
            const int4 *as = abuf + (size_t)rt * NKB * 2 * 64 + lane;
            uint32_t eap[4][11], c0p[4];     // half 0's column pairs, parked across the second MFMA block
            // output `reg` of lane (n, g) is row 16 rt + 4 reg + g: a ragged last tile fills its outputs from the top
            const int rows_here = n_out - 16 * rt < 16 ? n_out - 16 * rt : 16;
            const int nreg = PACKED ? 4 : (rows_here + 3) >> 2;      // (PACKED: the only tile that is not full takes the branch below)
            const uint32_t xs_addr = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void *)xs;
            const uint32_t as_addr = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void *)as;
            if (PACKED && rt == n_rt - 1) {
                // ---- the packed tile (FsPack): one MFMA a window.  Accumulator c' of reg r < 2 is column c' of the output on M row 4 r + g,
                // of reg r + 2 column c' + 8 of the same output (merged), or both are columns c' of two single-group rows.  Reg 0 is always
                // merged; reg 1 is merged with reg 3 (PK = 1), or regs 1 and 3 hold single-group rows (PK = 2).  The columns of a merged
                // output are summed HERE, pair by pair, and go through the reduction of every other pass.
                const v4i biaspv = v4i{MM8_BIAS_PACK, MM8_BIAS_PACK, MM8_BIAS_PACK, MM8_BIAS_PACK};
                // half 0 holds c' = 0 in acc[0] and the pairs (4j+3, 4j+4), j < 9, in acc[1 + 2j], acc[2 + 2j]; half 1 the pairs (4k+1, 4k+2),
                // k < 10, in acc[2k], acc[2k + 1]
                auto park_merged = [&](auto rc, const v4i (&acc)[20]) __attribute__((always_inline)) {
                    constexpr int r = decltype(rc)::value;
                    c0p[r] = (uint32_t)acc[0][r];
#pragma unroll
                    for (int j = 0; j < 11; j++) {
                        uint32_t lo = 0, hi = 0;
                        if (j < 9) { lo = (uint32_t)acc[1 + 2 * j][r]; hi = (uint32_t)acc[2 + 2 * j][r]; }
                        if (j >= 2) { lo += (uint32_t)acc[2 * j - 3][r + 2]; hi += (uint32_t)acc[2 * j - 2][r + 2]; }
                        if (j == 1) hi += (uint32_t)acc[0][r + 2];
                        eap[r][j] = lo + (hi << 8);
                    }
                };
                auto park_single = [&](auto rc, const v4i (&acc)[20]) __attribute__((always_inline)) {
                    constexpr int r = decltype(rc)::value;
                    c0p[r] = (uint32_t)acc[0][r];
#pragma unroll
                    for (int j = 0; j < 11; j++) eap[r][j] = j < 9 ? (uint32_t)acc[1 + 2 * j][r] + ((uint32_t)acc[2 + 2 * j][r] << 8) : 0u;
                };
                auto keep = [&](auto rc) __attribute__((always_inline)) {
                    constexpr int r = decltype(rc)::value;
                    asm volatile("" ::"v"(c0p[r]), "v"(eap[r][0]), "v"(eap[r][1]), "v"(eap[r][2]), "v"(eap[r][3]), "v"(eap[r][4]), "v"(eap[r][5]),
                                 "v"(eap[r][6]), "v"(eap[r][7]), "v"(eap[r][8]), "v"(eap[r][9]), "v"(eap[r][10]));
                    __builtin_amdgcn_sched_barrier(0);
                };
                {
                    v4i acc[20];
                    asm volatile("" ::: "memory");
                    __builtin_amdgcn_sched_barrier(0);
                    __builtin_amdgcn_s_setprio(0);
                    if constexpr (MSC) Mm8PhasePackedB<NKB, 0>::run(acc, xs_addr, as_addr, biaspv);
                    else Mm8PhasePacked<NKB, 0>::run(acc, xs_addr, as_addr, biaspv);
                    __builtin_amdgcn_s_setprio(2);
                    __builtin_amdgcn_sched_barrier(0);
                    FS_T(3);
                    park_merged(std::integral_constant<int, 0>{}, acc);
                    keep(std::integral_constant<int, 0>{});
                    if constexpr (PK == 1) park_merged(std::integral_constant<int, 1>{}, acc);
                    else park_single(std::integral_constant<int, 1>{}, acc);
                    keep(std::integral_constant<int, 1>{});
                    if constexpr (PK == 2) {
                        park_single(std::integral_constant<int, 3>{}, acc);
                        keep(std::integral_constant<int, 3>{});
                    }
                }
                {
                    v4i acc[20];
                    asm volatile("" ::: "memory");
                    __builtin_amdgcn_sched_barrier(0);
                    FS_T(4);
                    __builtin_amdgcn_s_setprio(0);
                    if constexpr (MSC) Mm8PhasePackedB<NKB, 1>::run(acc, xs_addr, as_addr, biaspv);
                    else Mm8PhasePacked<NKB, 1>::run(acc, xs_addr, as_addr, biaspv);
                    __builtin_amdgcn_s_setprio(2);
                    __builtin_amdgcn_sched_barrier(0);
                    FS_T(5);
                    // pair k of a merged output on regs r, r + 2 / of a single-group row on reg r
                    auto pair_merged = [&](auto rc, int k) __attribute__((always_inline)) {
                        constexpr int r = decltype(rc)::value;
                        uint32_t lo = 0, hi = 0;
                        if (k < 10) { lo = (uint32_t)acc[2 * k][r]; hi = (uint32_t)acc[2 * k + 1][r]; }
                        if (k >= 2) { lo += (uint32_t)acc[2 * k - 4][r + 2]; hi += (uint32_t)acc[2 * k - 3][r + 2]; }
                        return lo + (hi << 8);
                    };
                    auto pair_single = [&](auto rc, int k) __attribute__((always_inline)) {
                        constexpr int r = decltype(rc)::value;
                        return k < 10 ? (uint32_t)acc[2 * k][r] + ((uint32_t)acc[2 * k + 1][r] << 8) : 0u;
                    };
#define FS_FM0(k) pair_merged(std::integral_constant<int, 0>{}, k)
#define FS_FM1(k) pair_merged(std::integral_constant<int, 1>{}, k)
#define FS_FS1(k) pair_single(std::integral_constant<int, 1>{}, k)
#define FS_FS3(k) pair_single(std::integral_constant<int, 3>{}, k)
#define FS_E0(k) eap[0][k]
#define FS_E1(k) eap[1][k]
#define FS_E3(k) eap[3][k]
                    // (reg 3 first: with its accumulators and parked pairs out of the way the other two fit the register file)
                    if constexpr (PK == 2) { FS_REDUCE(16 * rt + 12 + g, FS_FS3, FS_E3, c0p[3]); __builtin_amdgcn_sched_barrier(0); }
                    FS_REDUCE(16 * rt + g, FS_FM0, FS_E0, c0p[0]);
                    if constexpr (PK == 1) FS_REDUCE(16 * rt + 4 + g, FS_FM1, FS_E1, c0p[1]);
                    else FS_REDUCE(16 * rt + 4 + g, FS_FS1, FS_E1, c0p[1]);
#undef FS_FM0
#undef FS_FM1
#undef FS_FS1
#undef FS_FS3
#undef FS_E0
#undef FS_E1
#undef FS_E3
                }
                FS_T(6);
                continue;
            }
            {   // ---- half 0: c = 0 and the pairs (4j+3, 4j+4)
                v4i acc[24];
                asm volatile("" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_setprio(0);        // (the phases yield to reductions and scaling: hb_mfma.hip, k_mm8)
                if constexpr (MSC) Mm8PhaseB<NKB, 0, false>::run(acc, xs_addr, as_addr, biasv);
                else Mm8Phase<NKB, 0, false>::run(acc, xs_addr, as_addr, biasv);
                __builtin_amdgcn_s_setprio(2);
                __builtin_amdgcn_sched_barrier(0);
                FS_T(3);
#pragma unroll
                for (int reg = 0; reg < 4; reg++) {
                    if (reg >= 2 && reg >= nreg) break;
                    c0p[reg] = (uint32_t)acc[0][reg];
#pragma unroll
                    for (int j = 0; j < 11; j++) eap[reg][j] = (uint32_t)acc[1 + 2 * j][reg] + ((uint32_t)acc[2 + 2 * j][reg] << 8);
                    asm volatile("" ::"v"(c0p[reg]), "v"(eap[reg][0]), "v"(eap[reg][1]), "v"(eap[reg][2]), "v"(eap[reg][3]), "v"(eap[reg][4]),
                                 "v"(eap[reg][5]), "v"(eap[reg][6]), "v"(eap[reg][7]), "v"(eap[reg][8]), "v"(eap[reg][9]), "v"(eap[reg][10]));
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            {   // ---- half 1: the pairs (4k+1, 4k+2)
                v4i acc[24];
                asm volatile("" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
                FS_T(4);
                __builtin_amdgcn_s_setprio(0);
                if constexpr (MSC) Mm8PhaseB<NKB, 1, false>::run(acc, xs_addr, as_addr, biasv);
                else Mm8Phase<NKB, 1, false>::run(acc, xs_addr, as_addr, biasv);
                __builtin_amdgcn_s_setprio(2);
                __builtin_amdgcn_sched_barrier(0);
                FS_T(5);
#pragma unroll
                for (int reg = 0; reg < 4; reg++) {
                    if (reg >= 2 && reg >= nreg) break;
#define FS_F(k) ((uint32_t)acc[2 * (k)][reg] + ((uint32_t)acc[2 * (k) + 1][reg] << 8))
#define FS_E(k) eap[reg][k]
                    FS_REDUCE(16 * rt + 4 * reg + g, FS_F, FS_E, c0p[reg]);
#undef FS_F
#undef FS_E
                    if (reg & 1) __builtin_amdgcn_sched_barrier(0);   // two reductions at a time: ILP for the carry chains
                }
            }
            FS_T(6);
        }
    }
#ifdef HB_MM8_TIMING
    if (lane == 0 && blockIdx.x < 256) for (int k = 0; k < 8; k++) g_fs_t[(blockIdx.x * 8 + wave) * 8 + k] = tacc[k];
#endif
    // a caller that waits for the verdict: the last workgroup to finish hands the status words to pinned host memory (and resets
    // them for the next launch), the sequence number last -- the host polls that word instead of synchronising the stream
    fs_workgroup_done(done, mismatch, first_bad);
}

// ---------------------------------------------------------------------------------------------------------------------
// the builder: [N ; P] as int8 digits, row constants, T tables, row modes
// ---------------------------------------------------------------------------------------------------------------------
typedef __int128 i128;

struct FsConsts {
    uint32_t c80r[9], biasmod[9], biasmod_pm[9], biasmod_ps[9];     // (biasmod_p*: the rows of a packed tile, hb_mm8.hpp)
    uint32_t ms_c80[9], ms_bias[9], pneg[8];                        // (the division by den on the matrix cores: fs_build_mscale)
};
constexpr int FS_MS_BIAS = 1 << 20;               // what a column of the division by den starts from: above 32 * 128 * 128, its largest sum
constexpr int32_t FS_OVERFLOW = 0x40000000;       // OR-ed into the status word if an entry does not fit (the host's bound rules it out)

// byte address of digit b (< 16) of entry (row i, term l) in the image (the layout of mm8_from_fast, hb_mfma.hip)
__device__ __forceinline__ size_t fs_digit_addr(int i, int l, int b, int nkb) {
    const int lane_ = (4 * ((i % 16) % 4) + (i % 16) / 4) + 16 * ((l % 8) / 2), el = l & 1;
    const int grp = b >> 3, r7 = 7 - (b & 7), hi = r7 >> 2, bi = r7 & 3;
    return ((((size_t)(i / 16) * nkb + l / 8) * 2 + grp) * 64 + (size_t)lane_) * 16 + 4 * (2 * hi + el) + bi;
}

// the constant of one matrix row from its d entries: (0x80..80 * sum - bias sum) mod p as eight pairs [bias of the fold's columns + word].
// kind (fs_slot): the bias sum is over the columns the row's accumulators cover -- 47, or the 39 + 39 of a merged row, or 39
__device__ __forceinline__ void fs_row_constant(const FpParams<9> &P, const FsConsts &cs, const i128 *row, int d, uint32_t *dst16, int kind = 0) {
    constexpr int NL = 9, NW = 8;
    uint32_t s5[5] = {0, 0, 0, 0, 0};                   // the row sum in 160 bits two's complement
    for (int l = 0; l < d; l++) {
        const i128 v = row[l];
        const uint32_t vw[5] = {(uint32_t)v, (uint32_t)(v >> 32), (uint32_t)(v >> 64), (uint32_t)(v >> 96), (uint32_t)(v >> 127 >> 1)};
        unsigned cy = 0;
#pragma unroll
        for (int k = 0; k < 5; k++) s5[k] = __builtin_addc(s5[k], vw[k], cy, &cy);
    }
    const bool negs = (s5[4] >> 31) != 0;
    if (negs) {
        unsigned cy = 1;
#pragma unroll
        for (int k = 0; k < 5; k++) s5[k] = __builtin_addc(~s5[k], 0u, cy, &cy);
    }
    uint32_t w8[NW] = {s5[0], s5[1], s5[2], s5[3], s5[4], 0, 0, 0}, fe[NL], prod[NL], corr[NL], k80[NL], bm[NL];
    unpack<NL, NW>(fe, w8);
    if (negs) fp_neg(fe, fe, P);
#pragma unroll
    for (int k = 0; k < NL; k++) { k80[k] = cs.c80r[k]; bm[k] = kind == 0 ? cs.biasmod[k] : kind == 1 ? cs.biasmod_pm[k] : cs.biasmod_ps[k]; }
    mont_mul(prod, fe, k80, P);
    fp_sub(corr, prod, bm, P);
    uint32_t cw[NW];
    pack<NL, NW>(cw, corr);
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint64_t pair = (uint64_t)cw[k] + ((0x1010ull << 32) | 0x10100000ull);
        dst16[2 * k] = (uint32_t)pair;
        dst16[2 * k + 1] = (uint32_t)(pair >> 32);
    }
}

// One workgroup of 1024.  Roles of the first phase:
//   wave 0        A(X) = prod_q (X - x_zq) over the integers (coefficient t on lane t), then per arrival j the coefficients of
//                 A_j = A / (X - x_zj) by synthetic division                                                    [Z]
//   waves 1, 2    1 / den_j = prod_{q != j} 1 / (x_zj - x_zq): four lanes per arrival, a quarter of the factors each      [Z]
//   waves 3 ..    P[i][j] = prod_{q != j} (x_zci - x_zq), one thread per entry                                         [ZC]
// Second phase: a thread per entry writes its 16 balanced digits; a thread per row its constant; 9 d threads the T tables.
__device__ __forceinline__ void fs_build_body(uint8_t *fb_lds, const FpParams<9> &P, const uint32_t *__restrict__ inv, int n, const FsIdx &ix, int d, int nc, int n_coef,
                                              int flags, const FsConsts &cs, uint8_t *__restrict__ a8, uint32_t *__restrict__ crow, uint32_t *__restrict__ KT,
                                              int32_t *__restrict__ rowmode, int32_t *__restrict__ z_dev, int32_t *__restrict__ status, const FsPack &pk,
                                              uint8_t *__restrict__ ms = nullptr) {
    constexpr int NL = 9, NW = 8;
    const int n_out = n_coef + nc, nkb = (d + 7) / 8, n_rt = (n_out + 15) / 16;
    i128 *ent = reinterpret_cast<i128 *>(fb_lds);                       // [n_out][d]
    i128 *Ac = ent + (size_t)n_out * d;                                 // [d + 1]
    uint32_t *wj = reinterpret_cast<uint32_t *>(Ac + (d + 1));          // [d][NL] Montgomery
    uint32_t *part = wj + (size_t)d * NL;                               // [d][4][NL]
    const int tid = threadIdx.x;
    const bool do_z = flags & FS_BUILD_Z, do_zc = flags & FS_BUILD_ZC;
    if (do_z) {
        // the image and the row constants of ALL row tiles start from "no row": zero digits, the bias pairs alone
        const size_t img = (size_t)n_rt * nkb * 2 * 64 * 16;
        for (size_t i = tid; i < img / 16; i += 1024) reinterpret_cast<uint4 *>(a8)[i] = make_uint4(0, 0, 0, 0);
        for (int i = tid; i < n_rt * 16 * 8; i += 1024) { crow[2 * i] = 0x10100000u; crow[2 * i + 1] = 0x1010u; }
        for (int i = tid; i < n_rt * 16; i += 1024) rowmode[i] = 0;      // (the coefficient rows' modes: behind the barriers, by slot)
        if (tid < d) z_dev[tid] = ix.z[tid];
    }
    if (do_z && tid < 64) {
        if (tid <= d) Ac[tid] = tid == 0 ? 1 : 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (int q = 0; q < d; q++) {
            i128 nv = 0;
            const bool act = tid <= q + 1 && tid <= d;
            if (act) nv = (tid > 0 ? Ac[tid - 1] : (i128)0) - (i128)ix.xz[q] * Ac[tid];
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (act) Ac[tid] = nv;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        if (tid < d) {
            // A_j[d-1] = 1, A_j[m-1] = A[m] + x_j A_j[m]
            const i128 xj = ix.xz[tid];
            i128 cur = 1;
            for (int m = d - 1; m >= 0; m--) {
                if (m < n_coef) ent[(size_t)m * d + tid] = cur;
                if (m > 0) cur = Ac[m] + xj * cur;
            }
        }
    } else if (do_z && tid < 64 + 4 * FS_MAXD + 32) {
        const int j = (tid - 64) >> 2, pq = (tid - 64) & 3;
        if (j < d) {
            uint32_t w[NL];
            fp_set(w, P.one);
            const uint32_t *row = inv + (size_t)ix.z[j] * n * NL;
            for (int q = pq; q < d; q += 4) {
                if (q == j) continue;
                uint32_t f[NL];
#pragma unroll
                for (int k = 0; k < NL; k++) f[k] = row[(size_t)ix.z[q] * NL + k];
                mont_mul(w, w, f, P);
            }
#pragma unroll
            for (int k = 0; k < NL; k++) part[((size_t)j * 4 + pq) * NL + k] = w[k];
        }
    } else if (do_zc && tid >= 256) {
        for (int e = tid - 256; e < nc * d; e += 1024 - 256) {
            const int i = e / d, j = e - i * d;
            const int64_t xi = ix.xzc[i];
            i128 v = 1;
            for (int q = 0; q < d; q++)
                if (q != j) v *= (i128)(xi - (int64_t)ix.xz[q]);
            ent[(size_t)(n_coef + i) * d + j] = v;
        }
    }
    __syncthreads();
    if (do_z && tid < d) {
        uint32_t a[NL], b[NL], c[NL];
#pragma unroll
        for (int k = 0; k < NL; k++) { a[k] = part[((size_t)tid * 4) * NL + k]; b[k] = part[((size_t)tid * 4 + 1) * NL + k]; }
        mont_mul(c, a, b, P);
#pragma unroll
        for (int k = 0; k < NL; k++) { a[k] = part[((size_t)tid * 4 + 2) * NL + k]; b[k] = part[((size_t)tid * 4 + 3) * NL + k]; }
        mont_mul(a, a, b, P);
        mont_mul(c, c, a, P);
#pragma unroll
        for (int k = 0; k < NL; k++) wj[(size_t)tid * NL + k] = c[k];
    }
    __syncthreads();
    // ---- digits: one thread per entry of the rows this launch owns -----------------------------------------------------
    const int row_lo = do_z ? 0 : n_coef, row_hi = do_zc ? n_out : n_coef;
    for (int e = tid + row_lo * d; e < row_hi * d; e += 1024) {
        const int i = e / d, l = e - i * d;
        i128 v = ent[e];
        const bool negv = v < 0;
        int carry = 0, kind;
        const int sl = fs_slot(pk, i, n_out, kind);
        bool lost = false;
#pragma unroll
        for (int b = 0; b < 16; b++) {
            int t = (int)((uint32_t)(v >> (8 * b)) & 0xffu) + carry;
            if (t > 127) { t -= 256; carry = 1; } else carry = 0;
            // a packed tile: digit group 1 of a merged row on M row + 8 of the piece of group 0; a single-group row has none
            if (kind == 0) a8[fs_digit_addr(sl, l, b, nkb)] = (uint8_t)(int8_t)t;
            else if (b < 8 || kind == 1) a8[fs_digit_addr(sl + (b < 8 ? 0 : 8), l, b & 7, nkb)] = (uint8_t)(int8_t)t;
            else lost |= t != 0;
        }
        if ((lost || carry != (negv ? 1 : 0)) && status) atomicOr(status, FS_OVERFLOW);
    }
    // ---- row constants: (0x80..80 * sum_l M[i][l] - bias sum) mod p as eight pairs [bias of the fold's columns + word] --------
    for (int i = tid + row_lo; i < row_hi; i += 1024) {
        int kind;
        const int sl = fs_slot(pk, i, n_out, kind);
        fs_row_constant(P, cs, ent + (size_t)i * d, d, crow + (size_t)sl * 16, kind);
        rowmode[sl] = i < n_coef ? -(i + 1) : (int32_t)ix.zc[i - n_coef] + 1;
    }
    if (do_z) {
        // T[l][q] = 2^(29 q) / den_l, canonical digits: mont_mul(w_l R, 2^(29 q)) = w_l 2^(29 q)
        for (int e = tid; e < d * NL; e += 1024) {
            const int l = e / NL, q = e - l * NL;
            uint32_t w[NL], two[NL], tq[NL];
#pragma unroll
            for (int k = 0; k < NL; k++) { w[k] = wj[(size_t)l * NL + k]; two[k] = (k == q) ? 1u : 0u; }
            mont_mul(tq, w, two, P);
#pragma unroll
            for (int k = 0; k < NL; k++) KT[((size_t)l * NL + q) * NL + k] = tq[k];
        }
    }
    if (do_z && ms) {
        // The division by den on the matrix cores (k_mm8f, MS): per term the A operand of the 32x32x32 products, [half][column] x 16 bytes
        // -- byte k of column c in half h is digit c of U_l[16 h + k], U_l[b] = 256^b / den_l as 32 balanced digits (of U or of U - p: one
        // of the two fits): piece h * 32 + c is what lane (c, h) reads -- then per term its 32 accumulator constants
        // 2^20 + byte c of (0x80..80 / den_l - sum_c 2^(20 + 8 c)) mod p, in the accumulators' order [half][register]: register i of a
        // lane of half h is column (i & 3) + 8 (i >> 2) + 4 h
        for (int e = tid; e < d * 32; e += 1024) {
            const int l = e >> 5, b = e & 31;
            uint32_t w[NL], two[NL], u[NL], uw[NW];
#pragma unroll
            for (int k = 0; k < NL; k++) { w[k] = wj[(size_t)l * NL + k]; two[k] = (k == (8 * b) / LB) ? 1u << ((8 * b) % LB) : 0u; }
            mont_mul(u, w, two, P);
            pack<NL, NW>(uw, u);
            int8_t dg[32];
            int carry = 0;
            for (int pass = 0; pass < 2; pass++) {
                // (second pass: U - p as the 256 bits of U + 2^256 - p, whose digits end in a carry)
                carry = 0;
                for (int c = 0; c < 32; c++) {
                    int t = (int)((uw[c >> 2] >> (8 * (c & 3))) & 0xffu) + carry;
                    if (t > 127) { t -= 256; carry = 1; } else carry = 0;
                    dg[c] = (int8_t)t;
                }
                if (carry == pass) break;
                if (pass == 0) {
                    unsigned cy = 0;
#pragma unroll
                    for (int k = 0; k < NW; k++) uw[k] = __builtin_addc(uw[k], cs.pneg[k], cy, &cy);
                } else if (status) atomicOr(status, FS_OVERFLOW);
            }
            for (int c = 0; c < 32; c++) ms[(size_t)((l * 2 + (b >> 4)) * 32 + c) * 16 + (b & 15)] = (uint8_t)dg[c];
        }
        for (int l = tid; l < d; l += 1024) {
            uint32_t w[NL], c80[NL], bm[NL], prod[NL], kk[NL], kw[NW];
#pragma unroll
            for (int k = 0; k < NL; k++) { w[k] = wj[(size_t)l * NL + k]; c80[k] = cs.ms_c80[k]; bm[k] = cs.ms_bias[k]; }
            mont_mul(prod, w, c80, P);
            fp_sub(kk, prod, bm, P);
            pack<NL, NW>(kw, kk);
            int32_t *ci = reinterpret_cast<int32_t *>(ms + (size_t)d * 1024) + l * 32;
            for (int c = 0; c < 32; c++) ci[16 * ((c >> 2) & 1) + 4 * (c >> 3) + (c & 3)] = FS_MS_BIAS + (int32_t)((kw[c >> 2] >> (8 * (c & 3))) & 0xffu);
        }
    }
}

// The rows of the compared senders before anybody knows who they will be: P[i][j] = prod_{q != j} (x_i - x_zq) for EVERY party i, its 16
// digits per entry laid out as the 8 NKB sixteen-byte pieces a row occupies in the image, and its row constant -- a candidate store
// indexed by party (k_mm8f gathers the rows it compares in its prologue: FsPick).  Depends on the first d arrivals alone.
__device__ __forceinline__ void fs_cand_body(uint8_t *fc_lds, const FpParams<9> &P, int n, const uint16_t *__restrict__ xs, const FsIdx &ix, int d, const FsConsts &cs,
                                             uint8_t *__restrict__ cand, uint32_t *__restrict__ cand_crow, int32_t *__restrict__ status) {
    i128 *ent = reinterpret_cast<i128 *>(fc_lds);                      // [n][d]
    const int tid = threadIdx.x, nkb = (d + 7) / 8;
    const size_t row_bytes = (size_t)nkb * 8 * 16;
    for (size_t i = tid; i < (size_t)n * row_bytes / 16; i += 1024) reinterpret_cast<uint4 *>(cand)[i] = make_uint4(0, 0, 0, 0);
    for (int e = tid; e < n * d; e += 1024) {
        const int i = e / d, j = e - i * d;
        const int64_t xi = xs[i];
        i128 v = 1;
        for (int q = 0; q < d; q++)
            if (q != j) v *= (i128)(xi - (int64_t)ix.xz[q]);
        ent[e] = v;
    }
    __syncthreads();
    for (int e = tid; e < n * d; e += 1024) {
        const int i = e / d, l = e - i * d;
        const i128 v = ent[e];
        const bool negv = v < 0;
        const int kb = l >> 3, gg = (l & 7) >> 1, el = l & 1;
        int carry = 0;
#pragma unroll
        for (int b = 0; b < 16; b++) {
            int t = (int)((uint32_t)(v >> (8 * b)) & 0xffu) + carry;
            if (t > 127) { t -= 256; carry = 1; } else carry = 0;
            const int grp = b >> 3, r7 = 7 - (b & 7), hi = r7 >> 2, bi = r7 & 3;
            cand[(size_t)i * row_bytes + (size_t)(((kb * 2 + grp) * 4 + gg) * 16) + 4 * (2 * hi + el) + bi] = (uint8_t)(int8_t)t;
        }
        if (carry != (negv ? 1 : 0) && status) atomicOr(status, FS_OVERFLOW);
    }
    for (int i = tid; i < n; i += 1024) fs_row_constant(P, cs, ent + (size_t)i * d, d, cand_crow + (size_t)i * 16);
}

__global__ void __launch_bounds__(1024) k_fs_build(const FpParams<9> P, const uint32_t *__restrict__ inv, int n, const FsIdx ix, int d, int nc, int n_coef,
                                                   int flags, const FsConsts cs, uint8_t *__restrict__ a8, uint32_t *__restrict__ crow, uint32_t *__restrict__ KT,
                                                   int32_t *__restrict__ rowmode, int32_t *__restrict__ z_dev, int32_t *__restrict__ status, const FsPack pk,
                                                   uint8_t *__restrict__ ms) {
    extern __shared__ __attribute__((aligned(16))) uint8_t fs_b_lds[];
    fs_build_body(fs_b_lds, P, inv, n, ix, d, nc, n_coef, flags, cs, a8, crow, KT, rowmode, z_dev, status, pk, ms);
}

__global__ void __launch_bounds__(1024) k_fs_cand(const FpParams<9> P, int n, const uint16_t *__restrict__ xs, const FsIdx ix, int d, const FsConsts cs,
                                                  uint8_t *__restrict__ cand, uint32_t *__restrict__ cand_crow, int32_t *__restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) uint8_t fs_c_lds[];
    fs_cand_body(fs_c_lds, P, n, xs, ix, d, cs, cand, cand_crow, status);
}

// What a decoder enqueues when its (degree + 1)-th column lands, as ONE launch of two workgroups: block 0 builds everything that depends on the
// arrivals alone (k_fs_build with FS_BUILD_Z), block 1 the candidate store (k_fs_cand) -- the two are independent, and as two launches
// the second waited for the first (8 us + a dispatch gap on the path of the column that completes the quorum).
__global__ void __launch_bounds__(1024) k_fs_build_z_cand(const FpParams<9> P, const uint32_t *__restrict__ inv, int n, const uint16_t *__restrict__ xs, const FsIdx ix, int d, int nc,
                                                          int n_coef, const FsConsts cs, uint8_t *__restrict__ a8, uint32_t *__restrict__ crow, uint32_t *__restrict__ KT,
                                                          int32_t *__restrict__ rowmode, int32_t *__restrict__ z_dev, uint8_t *__restrict__ cand, uint32_t *__restrict__ cand_crow,
                                                          int32_t *__restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) uint8_t fs_zc_lds[];
    if (blockIdx.x == 0) fs_build_body(fs_zc_lds, P, inv, n, ix, d, nc, n_coef, FS_BUILD_Z, cs, a8, crow, KT, rowmode, z_dev, status, FsPack{});
    else fs_cand_body(fs_zc_lds, P, n, xs, ix, d, cs, cand, cand_crow, status);
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
static int fs_num_cus() {
    static int n = 0;
    if (!n) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    }
    return n;
}

// Does [n_coef rows of N ; nc rows of P] over d arrivals of this point set fit the kernel?  The bounds hold for EVERY choice of
// arrivals: |coeff_m(A_j)| <= prod over the d - 1 largest points of (1 + x), |A_j(x_i)| <= the product of the d - 1 largest
// distances from a point, each distance taken by at most two points.
int fs_layout(hb_ctx *ctx, const PointTable *pt, int d, int nc, int n_coef, FsLayout *L) {
    if (ctx->n_limbs != 4 || !pt || !pt->usable || !pt->small) return HB_ERR_UNSUPPORTED;
    if (d < 4 || d > 22 || nc < 0 || nc > FS_MAXC || n_coef < 1 || n_coef > d) return HB_ERR_UNSUPPORTED;
    if (env_hook(ENV_NO_MFMA) || env_hook(ENV_NO_FUSED_SMALL) || env_hook(ENV_NO_QUICK) || !prescale_params(ctx)) return HB_ERR_UNSUPPORTED;
    // 128 * (16 digits of at most 128 in each of d terms) must stay below the accumulator bias
    if ((int64_t)d * 16 * 128 * 128 > MM8_BIAS) return HB_ERR_UNSUPPORTED;
    std::vector<uint16_t> xs(pt->xs);
    std::sort(xs.begin(), xs.end());
    double bits_n = 0.0, bits_p = 0.0;
    for (int k = 0; k < d - 1 && k < (int)xs.size(); k++) bits_n += log2(1.0 + xs[xs.size() - 1 - k]);
    const int R = xs.empty() ? 0 : xs.back() - xs.front();
    for (int k = 0; k < d - 1; k++) { const int dist = R - k / 2; if (dist < 1) break; bits_p += log2((double)dist); }
    if (bits_n > 124.5 || bits_p > 124.5) return HB_ERR_UNSUPPORTED;
    L->n = pt->n; L->d = d; L->nc = nc; L->n_coef = n_coef; L->n_out = n_coef + nc;
    L->nkb = (d + 7) / 8; L->n_rt = (L->n_out + 15) / 16;
    L->pk_nm = L->pk_ns = 0;
    memset(L->pk_single, 0, sizeof L->pk_single);
    if (fs_lds_bytes(L->n_rt, L->nkb) > FS_LDS_LIMIT) return HB_ERR_UNSUPPORTED;
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    L->o_a8 = 0;
    L->o_crow = al((size_t)L->n_rt * L->nkb * 2 * 64 * 16);
    L->o_kt = L->o_crow + al((size_t)L->n_rt * 16 * 16 * 4);
    L->o_mode = L->o_kt + al((size_t)d * 81 * 4);
    L->o_z = L->o_mode + al((size_t)L->n_rt * 16 * 4);
    L->o_ms = L->o_z + al((size_t)FS_MAXD * 4);
    L->need = L->o_ms + al((size_t)fs_ms_q(d) * 16);
    L->mscale = 0;
    L->o_cand = L->o_cand_crow = 0;
    if (pt->n <= FS_CAND_MAXN && nc > 0) {
        L->o_cand = L->need;
        L->o_cand_crow = L->o_cand + al((size_t)pt->n * L->nkb * 8 * 16);
        L->need = L->o_cand_crow + al((size_t)pt->n * 16 * 4);
    }
    return HB_OK;
}

// which coefficient rows of N have no digit above the eighth: small[m] = 1 iff every |coeff_m(A_j)| < 2^62, from the integers themselves
// (A(X) = prod (X - x_zq), then the synthetic divisions: the arithmetic of fs_build_body's first wave; the layout's bound keeps it in 128 bits)
static void fs_small_rows(const uint16_t *xz, int d, int n_coef, uint8_t *small) {
    i128 Ac[FS_MAXD + 1];
    for (int k = 0; k <= d; k++) Ac[k] = k == 0 ? 1 : 0;
    for (int q = 0; q < d; q++)
        for (int k = q + 1; k >= 0; k--) Ac[k] = (k > 0 ? Ac[k - 1] : (i128)0) - (i128)xz[q] * Ac[k];
    for (int m = 0; m < n_coef; m++) small[m] = 1;
    const i128 lim = (i128)1 << 62;
    for (int j = 0; j < d; j++) {
        i128 cur = 1;
        for (int m = d - 1; m >= 0; m--) {
            if (m < n_coef && (cur >= lim || cur <= -lim)) small[m] = 0;
            if (m > 0) cur = Ac[m] + (i128)xz[j] * cur;
        }
    }
}

bool fs_pack(const PointTable *pt, const int32_t *z, FsLayout *L) {
    L->pk_nm = L->pk_ns = 0;
    memset(L->pk_single, 0, sizeof L->pk_single);
    if (env_hook(ENV_NO_FUSED_PACK)) return false;
    uint16_t xz[FS_MAXD];
    uint8_t small[FS_MAXD];
    for (int i = 0; i < L->d; i++) { if (z[i] < 0 || z[i] >= L->n) return false; xz[i] = pt->xs[z[i]]; }
    fs_small_rows(xz, L->d, L->n_coef, small);
    FsPack pk;
    if (!fs_pack_decide(L->d, L->n_coef, L->nc, small, &pk)) return false;
    L->pk_nm = pk.nm; L->pk_ns = pk.ns;
    memcpy(L->pk_single, pk.single, sizeof pk.single);
    return true;
}

// An image that is built in one piece (a plan's, the one-shot check's) divides the received columns by den on the matrix cores, where the
// tables fit the LDS beside the rest; HB_NO_FUSED_MSCALE=1 keeps the T_q multiplication everywhere (what a decoder's launches do).
bool fs_mscale(FsLayout *L) {
    L->mscale = !env_hook(ENV_NO_FUSED_MSCALE) && fs_lds_bytes(L->n_rt, L->nkb, L->d) <= FS_LDS_LIMIT;
    return L->mscale != 0;
}

// enqueue the build into `base` (L.need bytes): FS_BUILD_Z needs z, FS_BUILD_ZC both (the rows of P depend on z too)
int fs_build(hb_ctx *ctx, const PointTable *pt, const int32_t *z, const int32_t *zc, const FsLayout &L, uint8_t *base, int flags, int32_t *status_dev, hipStream_t s) {
    const int n = L.n, d = L.d, nc = L.nc;
    FsIdx ix;
    memset(&ix, 0, sizeof ix);
    uint64_t seen[4] = {0, 0, 0, 0};            // (n <= 65535 in general: the bitmap covers the first 256, larger sets use the vector)
    std::vector<uint8_t> seen_big;
    if (n > 256) seen_big.assign((size_t)n, 0);
    auto mark = [&](int v) -> bool {
        if (v < 0 || v >= n) return false;
        if (n > 256) { if (seen_big[v]) return false; seen_big[v] = 1; return true; }
        if (seen[v >> 6] >> (v & 63) & 1) return false;
        seen[v >> 6] |= 1ull << (v & 63);
        return true;
    };
    for (int i = 0; i < d; i++) { if (!mark(z[i])) return fail(ctx, HB_ERR_BAD_ARG, "fused decode: arrival indices"); ix.z[i] = (uint16_t)z[i]; ix.xz[i] = pt->xs[z[i]]; }
    if (flags & FS_BUILD_ZC)
        for (int j = 0; j < nc; j++) { if (!mark(zc[j])) return fail(ctx, HB_ERR_BAD_ARG, "fused decode: compared indices"); ix.zc[j] = (uint16_t)zc[j]; ix.xzc[j] = pt->xs[zc[j]]; }
    const Mm8Shared *sh = nullptr;
    int rc = mm8_shared(ctx, &sh, s); if (rc) return rc;
    FsConsts cs;
    memcpy(cs.c80r, sh->c80r, sizeof cs.c80r);
    memcpy(cs.biasmod, sh->biasmod, sizeof cs.biasmod);
    memcpy(cs.biasmod_pm, sh->biasmod_pm, sizeof cs.biasmod_pm);
    memcpy(cs.biasmod_ps, sh->biasmod_ps, sizeof cs.biasmod_ps);
    memcpy(cs.ms_c80, sh->ms_c80, sizeof cs.ms_c80);
    memcpy(cs.ms_bias, sh->ms_bias, sizeof cs.ms_bias);
    memcpy(cs.pneg, sh->bp.pneg, sizeof cs.pneg);
    if (L.mscale && flags != (FS_BUILD_Z | FS_BUILD_ZC)) return fail(ctx, HB_ERR_BAD_ARG, "fused decode: the matrix-core division's tables are built with the whole image");
    FsPack pk;
    memset(&pk, 0, sizeof pk);
    if (L.pk_nm) {
        if (flags != (FS_BUILD_Z | FS_BUILD_ZC)) return fail(ctx, HB_ERR_BAD_ARG, "fused decode: a packed image is built in one piece");
        pk.nm = L.pk_nm; pk.ns = L.pk_ns;
        memcpy(pk.single, L.pk_single, sizeof pk.single);
    }
    const size_t lds = ((size_t)L.n_out * d + d + 1) * 16 + ((size_t)d * 9 + (size_t)d * 4 * 9) * 4;
    k_fs_build<<<1, 1024, lds, s>>>(ctx->pw, pt->inv, n, ix, d, nc, L.n_coef, flags, cs, base + L.o_a8, (uint32_t *)(base + L.o_crow), (uint32_t *)(base + L.o_kt),
                                    (int32_t *)(base + L.o_mode), (int32_t *)(base + L.o_z), status_dev, pk, L.mscale ? base + L.o_ms : nullptr);
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int fs_build_cand(hb_ctx *ctx, PointTable *pt, const int32_t *z, const FsLayout &L, uint8_t *base, int32_t *status_dev, hipStream_t s, bool with_z) {
    if (!L.o_cand) return fail(ctx, HB_ERR_BAD_ARG, "fused decode: no candidate store in this layout");
    if (!pt->xs_dev) {
        HB_HIP(ctx, hipMalloc(&pt->xs_dev, (size_t)pt->n * 2));
        int rc = upload_table(ctx, pt->xs_dev, pt->xs.data(), (size_t)pt->n * 2, s);      // (synchronises; once per point set)
        if (rc) { (void)hipFree(pt->xs_dev); pt->xs_dev = nullptr; return rc; }
    }
    FsIdx ix;
    memset(&ix, 0, sizeof ix);
    uint64_t seen[2] = {0, 0};                  // (a candidate store exists for at most 128 parties)
    for (int i = 0; i < L.d; i++) {
        const int v = z[i];
        if (v < 0 || v >= pt->n || (seen[v >> 6] >> (v & 63) & 1)) return fail(ctx, HB_ERR_BAD_ARG, "fused decode: arrival indices");
        seen[v >> 6] |= 1ull << (v & 63);
        ix.z[i] = (uint16_t)v; ix.xz[i] = pt->xs[v];
    }
    const Mm8Shared *sh = nullptr;
    int rc = mm8_shared(ctx, &sh, s); if (rc) return rc;
    FsConsts cs;
    memcpy(cs.c80r, sh->c80r, sizeof cs.c80r);
    memcpy(cs.biasmod, sh->biasmod, sizeof cs.biasmod);
    memset(cs.biasmod_pm, 0, sizeof cs.biasmod_pm);       // (no packed tile in an image whose compared rows are picked, and no matrix-core division)
    memset(cs.biasmod_ps, 0, sizeof cs.biasmod_ps);
    memset(cs.ms_c80, 0, sizeof cs.ms_c80);
    memset(cs.ms_bias, 0, sizeof cs.ms_bias);
    memset(cs.pneg, 0, sizeof cs.pneg);
    if (with_z) {
        const size_t lds_b = ((size_t)L.n_out * L.d + L.d + 1) * 16 + ((size_t)L.d * 9 + (size_t)L.d * 4 * 9) * 4, lds_c = (size_t)pt->n * L.d * 16;
        k_fs_build_z_cand<<<2, 1024, std::max(lds_b, lds_c), s>>>(ctx->pw, pt->inv, pt->n, pt->xs_dev, ix, L.d, L.nc, L.n_coef, cs, base + L.o_a8, (uint32_t *)(base + L.o_crow),
                                                                  (uint32_t *)(base + L.o_kt), (int32_t *)(base + L.o_mode), (int32_t *)(base + L.o_z), base + L.o_cand,
                                                                  (uint32_t *)(base + L.o_cand_crow), status_dev);
        HB_LAUNCH_CHECK(ctx);
        return HB_OK;
    }
    k_fs_cand<<<1, 1024, (size_t)pt->n * L.d * 16, s>>>(ctx->pw, pt->n, pt->xs_dev, ix, L.d, cs, base + L.o_cand, (uint32_t *)(base + L.o_cand_crow), status_dev);
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

static std::atomic<int> g_fs_last_pack{-1};       // k_mm8f's PK at the last fs_launch of the process (hb_debug_fs_last_pack)
static std::atomic<int> g_fs_last_mscale{-1};     // and whether it divided by den on the matrix cores (hb_debug_fs_last_mscale)

// The terms of the next unit dealt to the waves.  A wave's load in a unit: its passes (wave w takes pairs w, w + 8, ... of the 4 n_rt; a pass
// over a ragged last row tile with at most 8 rows reduces two of the four outputs a lane holds) plus its terms; measured on config 3's R2
// launch (scratch/fs_phase_timing.py) a pass is 9.5 k cycles of a wave's time and a term 3.6 k when two waves share the SIMD.  Each term goes
// to the wave with the least load so far (ties: the higher wave -- the older waves 0..3 win the issue arbitration anyway).
//
// A packed pass: by the phase ticks of a timing build (profiles/fs_pack.txt) 0.63 of a full pass with two reductions (R1: 60) and 0.78 with
// three (R2: 74) -- but at those weights the deal is the unpacked one, and the waves with a packed pass wait longest at the unit barrier
// (the ticks of a pass include what its SIMD partner issues meanwhile).  A sweep of the weight on the benchmark put both at 57 or below,
// where the waves with a packed pass take a term more and those with two full passes (or a full pass and three terms) one less.
//
// A term divided on the matrix cores (mscale): 2.4 k ticks against the multiplication's 3.6 k in the same waves of a timing build
// (profiles/fs_mscale.txt: R2 wave 5, ten tasks, 36.0 k -> 23.7 k), so 24 while a task was sixteen 16x16x64 MFMAs; as two 32x32x32 products
// the same ten tasks are 26.8 k -> 20.9 k in one session (profiles/fs_mscale32.txt), 2.1 k a task, so 20.  The benchmark does not tell
// 12 .. 36 apart (both files).
static FsSplit fs_split(int d, int n_rt, int n_out, int pk_nm, int pk_ns, bool mscale) {
    constexpr int PASS = 95, RAGGED = 70, PACKED2 = 50, PACKED3 = 55;
    const int TERM = mscale ? 20 : 36;
    const int packed = pk_ns ? PACKED3 : PACKED2;
    FsSplit sp;
    int load[FS_WAVES];
    const int n_pairs = FS_TPW * n_rt;
    const bool ragged = n_out - 16 * (n_rt - 1) <= 8;
    for (int w = 0; w < FS_WAVES; w++) {
        sp.terms[w] = 0;
        load[w] = 0;
        for (int pidx = w; pidx < n_pairs; pidx += FS_WAVES) {
            const int tl = n_rt == 2 ? (pidx >> 1) : pidx / n_rt;
            const int rt = n_rt == 2 ? ((pidx ^ (pidx >> 2)) & 1) : pidx - tl * n_rt;
            load[w] += (pk_nm && rt == n_rt - 1) ? packed : (ragged && rt == n_rt - 1) ? RAGGED : PASS;
        }
    }
    for (int l = 0; l < d; l++) {
        int best = FS_WAVES - 1;
        for (int w = FS_WAVES - 2; w >= 0; w--)
            if (load[w] < load[best]) best = w;
        sp.terms[best] |= 1u << l;
        load[best] += TERM;
    }
    return sp;
}

// the launch over a built image: rows with a store mode go to `out` (view ov, clipped at out_count), rows with a compare mode are
// checked against the rows of `cols` they name
int fs_launch(hb_ctx *ctx, const FsLayout &L, const uint8_t *base, const uint32_t *cols, hb_view cv, uint32_t *out, hb_view ov, int64_t out_count,
              int32_t *mismatch_dev, int32_t *first_bad_dev, uint32_t *bad_map_dev, int64_t C, hipStream_t s, const FsDone *done_p, const int32_t *pick_zc) {
    FsDone done;
    memset(&done, 0, sizeof done);
    if (done_p) done = *done_p;
    FsPick pick;
    memset(&pick, 0, sizeof pick);
    if (pick_zc) {
        if (L.pk_nm || L.mscale) return fail(ctx, HB_ERR_BAD_ARG, "fused decode: an image built in one piece has no rows to pick");
        if (!L.o_cand) return fail(ctx, HB_ERR_BAD_ARG, "fused decode: no candidate store to pick from");
        pick.cand = (const uint4 *)(base + L.o_cand); pick.cand_crow = (const uint32_t *)(base + L.o_cand_crow);
        pick.n_coef = L.n_coef; pick.nc = L.nc;
        for (int j = 0; j < L.nc; j++) pick.zc[j] = (uint16_t)pick_zc[j];
    }
    if (C <= 0) return HB_OK;
    const Mm8Shared *sh = nullptr;
    int rc = mm8_shared(ctx, &sh, s); if (rc) return rc;
    const int64_t n_units = (C + 63) / 64;
    int64_t blocks = fs_num_cus();
    if (blocks > n_units) blocks = n_units;
    blocks = mm8_trimmed_grid(n_units, blocks);          // (config 3: 249 of 256 -- seven CUs stay free for what other streams launch meanwhile)
    const size_t lds = fs_lds_bytes(L.n_rt, L.nkb, L.mscale ? L.d : 0);
    const FsSplit split = fs_split(L.d, L.n_rt, L.n_out, L.pk_nm, L.pk_ns, L.mscale != 0);
    const int pack = !L.pk_nm ? 0 : L.pk_ns ? 2 : 1;       // (k_mm8f's PK)
    g_fs_last_pack.store(pack);
    g_fs_last_mscale.store(L.mscale ? 1 : 0);
#define FS_LAUNCH(NKB, PK) do { if (L.mscale) FS_LAUNCH_(NKB, PK, true); else FS_LAUNCH_(NKB, PK, false); } while (0)
#define FS_LAUNCH_(NKB, PK, MSC)                                                                                                                   \
    do {                                                                                                                                   \
        static std::atomic<unsigned long long> attr_done{0};   /* one bit per device: the attribute is per device */                                                                                                     \
        if (!((attr_done.load() >> (ctx->device & 63)) & 1ull)) { HB_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(k_mm8f<NKB, PK, MSC>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); attr_done.fetch_or(1ull << (ctx->device & 63)); } \
        k_mm8f<NKB, PK, MSC><<<dim3((unsigned)blocks), dim3(64 * FS_WAVES), lds, s>>>((const int4 *)(base + L.o_a8), (const uint32_t *)(base + L.o_crow), sh->fold_dev,        \
            (const uint32_t *)(base + L.o_kt), ctx->psc, cols, cv.stride_c, cv.stride_l, (const int32_t *)(base + L.o_z), INT64_MAX, L.d, (const int32_t *)(base + L.o_mode), \
            out, ov.stride_c, ov.stride_l, out_count, mismatch_dev, first_bad_dev, bad_map_dev, L.n_out, L.n_rt, C, n_units, sh->bp, done, pick, split, \
            L.mscale ? (const v4i *)(base + L.o_ms) : nullptr); \
    } while (0)
    switch (L.nkb) {
        case 1: if (pack == 1) FS_LAUNCH(1, 1); else if (pack == 2) FS_LAUNCH(1, 2); else FS_LAUNCH(1, 0); break;
        case 2: if (pack == 1) FS_LAUNCH(2, 1); else if (pack == 2) FS_LAUNCH(2, 2); else FS_LAUNCH(2, 0); break;
        case 3: if (pack == 1) FS_LAUNCH(3, 1); else if (pack == 2) FS_LAUNCH(3, 2); else FS_LAUNCH(3, 0); break;
        default: return fail(ctx, HB_ERR_UNSUPPORTED, "fused decode: more than 24 terms");
    }
#undef FS_LAUNCH
#undef FS_LAUNCH_
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

}  // namespace hb

// the packing decision on its own (include/hbmpc_hip_debug.h): host arithmetic, no device
extern "C" int hb_debug_fs_pack_rows(int d, int n_coef, int nc, const uint8_t *small, int32_t *out) {
    hb::FsPack pk;
    const bool ok = d >= 1 && d <= hb::FS_MAXD && n_coef >= 1 && n_coef <= d && nc >= 0 && nc <= hb::FS_MAXC && hb::fs_pack_decide(d, n_coef, nc, small, &pk);
    if (!ok) memset(&pk, 0, sizeof pk);
    out[0] = pk.nm; out[1] = pk.ns;
    for (int k = 0; k < 8; k++) out[2 + k] = pk.single[k];
    return ok ? 1 : 0;
}
extern "C" int hb_debug_fs_pack_points(const int32_t *xz, int d, int n_coef, int nc, int32_t *out, uint8_t *small_out) {
    if (d < 1 || d > hb::FS_MAXD || n_coef < 1 || n_coef > d) return 0;
    uint16_t x16[hb::FS_MAXD];
    uint8_t small[hb::FS_MAXD];
    for (int i = 0; i < d; i++) x16[i] = (uint16_t)xz[i];
    hb::fs_small_rows(x16, d, n_coef, small);
    if (small_out) memcpy(small_out, small, (size_t)n_coef);
    return hb_debug_fs_pack_rows(d, n_coef, nc, small, out);
}
extern "C" int hb_debug_fs_last_pack(void) { return hb::g_fs_last_pack.load(); }
extern "C" int hb_debug_fs_last_mscale(void) { return hb::g_fs_last_mscale.load(); }
extern "C" int hb_debug_fs_slot(int nm, int ns, const int32_t *single, int i, int n_out, int32_t *kind) {
    hb::FsPack pk;
    memset(&pk, 0, sizeof pk);
    pk.nm = nm; pk.ns = ns;
    for (int k = 0; k < 8 && k < ns; k++) pk.single[k] = (uint8_t)single[k];
    int kd = 0;
    const int sl = hb::fs_slot(pk, i, n_out, kd);
    *kind = kd;
    return sl;
}

#ifdef HB_MM8_TIMING
extern "C" int hb_debug_fs_timing(unsigned long long *out, int count) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(hb::g_fs_t), sizeof(unsigned long long) * (size_t)count) == hipSuccess ? 0 : 1;
}
#endif

// hb_mimc.hip -- the MiMC block cipher of the reference's progs/mimc.py and progs/mimc_symmetric.py: the cleartext cipher
// (mimc_plain, progs/mimc.py:10-15, and the keystream of mimc_encrypt, progs/mimc_symmetric.py:10-16) as one compute kernel, and
// the cubing round of mimc_mpc / mimc_mpc_batch (progs/mimc.py:25-30, 46-55) as one fused pass -- restated on fp29.hpp, not
// translated.
//
//   F(x, k):  v <- x;  for c = 0 .. rounds - 1:  v <- (v + k + c)^3;   F = v + k          (rounds = 161 over BLS12-381 Fr)
//
// k_mimc_plain   out[i] = F(x_i, key_i) (+ addend_i | addend_i - F): x_i from an array or the counter start + i, key one element
//                for all or one an element.  2 rounds field multiplications an element with nothing but registers in between:
//                x and the running round constant key + c are kept in Montgomery form (+ mont(1) a round), every round is one square
//                and one product (mimc_chain), one conversion in and one out.  E = 1 or 2 independent elements a thread.
// MimcRoundRow   after the open of y = x - r:  x^3 = y^3 + 3 y^2 r + 3 y r2 + r3 by Horner, y (y (y + 3 r) + 3 r2) + r3 -- three
//                products -- and, in the same pass, the next round's array to open x^3 + (key + c + 1) - r_next (LAST: x^3 + key).
//                5 reads and one write an element (6 + 1 with a key per element); the round's share is never materialised.
// MimcFirstRow   x + key - r_0, the first array to open (x an array or the counters).
// A public constant is added to a Shamir share by every party alike, so the kernels do not ask which of x and key is shared.
//
// Operands and results are packed canonical residues.  The per-element bodies are HB_HD functions.  The two steps of the MPC round
// are rows (hb_rows.hpp): k_rows runs them on the device and hb_selftest_mimc runs the very same rows, addressing included, on the
// host.  k_mimc_plain keeps a kernel of its own (two elements a thread, another thread-to-element map); it only loads, calls the body
// and stores, and the self test runs the same body.
//
// Launch shape (all kernels): 256-thread workgroups, E elements a thread (E = 1 but for the paired cleartext variant), grid =
// ceil(count / (256 E)), no LDS, no grid stride, one launch a call.  A key for all is read from one address by every lane and made
// wave-uniform with readfirstlane (DeviceMem::same, as EwBinaryRow's broadcast operand): its digits and the round constant live in
// SGPRs.  The operands of a round are read once: the 32-byte width takes the non-temporal loads, as EwBeaverRow.
// Compiler's report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage) and the timings: DESIGN.md section 3k.
#include "hb_common.hpp"
#include "hb_rows.hpp"

using namespace hb;

namespace hb {

// ---------------------------------------------------------------- per-element bodies (host and device)
// r = i mod p, canonical, for an index 0 <= i < 2^63 (p may be as small as 13).  The digits of i times R^2: T < R p (i < 2^87 <= R,
// R^2 mod p < p), so REDC returns i R mod p below 2 p -- one conditional subtraction, as any mont_mul -- and a bare REDC takes the R off.
template <int NL> HB_HD void mimc_index(uint32_t (&r)[NL], int64_t i, const FpParams<NL> &P) {
    uint32_t d[NL], t[NL];
#pragma unroll
    for (int q = 0; q < NL; q++) d[q] = (q < 3) ? ((uint32_t)((uint64_t)i >> (LB * q)) & DMASK) : 0u;
    mont_mul<NL>(t, d, P.r2, P);
    from_mont<NL>(r, t, P);
}

// x of element i: the array's word, or start + i
template <int NL, int NW> HB_HD void mimc_input(uint32_t (&x)[NL], bool counter, const uint32_t (&xw)[NW], const uint32_t (&start)[NL], int64_t i, const FpParams<NL> &P) {
    if (counter) {
        uint32_t t[NL];
        mimc_index<NL>(t, i, P);
        fp_add<NL>(x, start, t, P);
    } else {
        unpack<NL, NW>(x, xw);
    }
}

// f[e] = F(x[e], k[e]) for E independent elements: canonical digits in and out.
// Bounds of a round.  v and the constant cm = (k + c) R are canonical Montgomery residues.  t = v + cm is taken digit by digit with
// no carry and no reduction: t[i] <= 2 (2^29 - 1), t < 2 p.  Column j of t * t holds at most NL products of 2 (2^29 - 1) * 2 (2^29 - 1),
// below 4 NL 2^58 -- four of the Lazy<NL>::GROUP = 7 (NL = 9) products a column may take (fp29.hpp:8).  REDC adds NL more and its
// neighbour's carry (< 2^36): 5 NL 2^58 + 2^36 < 2^64 for NL <= 9, so, as in mont_mul, no carry pass in front of REDC.  The value
// T = t^2 < 4 p^2, so REDC returns s < p (1 + 4 p / R) < 2 p (R = 2^(29 NL) >= 32 p): one conditional subtraction, s = t^2 / R canonical.
// s * t: columns below 2 NL 2^58 (+ NL 2^58 in REDC), T < 2 p^2, again one conditional subtraction: v' = t^3 / R^2 = ((v + cm) / R)^3 R.
// p = 2^256 - 189 with x = key = p - 1 is the largest case (tests/test_mimc_host.py).
template <int NL, int E>
HB_HD void mimc_chain(uint32_t (&f)[E][NL], const uint32_t (&x)[E][NL], const uint32_t (&k)[E][NL], int rounds, const FpParams<NL> &P) {
    uint32_t v[E][NL], cm[E][NL], km[E][NL];
#pragma unroll
    for (int e = 0; e < E; e++) {
        to_mont<NL>(v[e], x[e], P);
        to_mont<NL>(km[e], k[e], P);
        fp_set<NL>(cm[e], km[e]);
    }
#pragma unroll 1
    for (int c = 0; c < rounds; c++) {
#pragma unroll
        for (int e = 0; e < E; e++) {
            uint32_t t[NL], s[NL];
            uint64_t col[2 * NL];
#pragma unroll
            for (int i = 0; i < NL; i++) t[i] = v[e][i] + cm[e][i];
            col_zero(col);
            mac<NL>(col, t, t);
            redc<NL>(s, col, P);
            cond_sub_p<NL>(s, P);
            col_zero(col);
            mac<NL>(col, s, t);
            redc<NL>(v[e], col, P);
            cond_sub_p<NL>(v[e], P);
            fp_add<NL>(cm[e], cm[e], P.one, P);
        }
    }
#pragma unroll
    for (int e = 0; e < E; e++) {
        uint32_t t[NL];
        fp_add<NL>(t, v[e], km[e], P);
        from_mont<NL>(f[e], t, P);
    }
}

// o[e] = F(x, key) | addend + F | addend - F on packed words; x the array's words or start + idx[e]
template <int NL, int NW, int E>
HB_HD void mimc_plain_elem(uint32_t (&o)[E][NW], bool counter, const uint32_t (&xw)[E][NW], const uint32_t (&start)[NL], const int64_t (&idx)[E],
                           const uint32_t (&kw)[E][NW], bool has_addend, const uint32_t (&aw)[E][NW], bool subtract, int rounds, const FpParams<NL> &P) {
    uint32_t x[E][NL], k[E][NL], f[E][NL];
#pragma unroll
    for (int e = 0; e < E; e++) {
        mimc_input<NL, NW>(x[e], counter, xw[e], start, idx[e], P);
        unpack<NL, NW>(k[e], kw[e]);
    }
    mimc_chain<NL, E>(f, x, k, rounds, P);
#pragma unroll
    for (int e = 0; e < E; e++) {
        if (has_addend) {
            uint32_t a[NL], r[NL];
            unpack<NL, NW>(a, aw[e]);
            if (subtract) fp_sub<NL>(r, a, f[e], P); else fp_add<NL>(r, a, f[e], P);
            pack<NL, NW>(o[e], r);
        } else {
            pack<NL, NW>(o[e], f[e]);
        }
    }
}

// o = x + key - r0: the first array to open
template <int NL, int NW>
HB_HD void mimc_first_elem(uint32_t (&o)[NW], bool counter, const uint32_t (&xw)[NW], const uint32_t (&start)[NL], int64_t i, const uint32_t (&kw)[NW],
                           const uint32_t (&r0w)[NW], const FpParams<NL> &P) {
    uint32_t x[NL], k[NL], t[NL];
    mimc_input<NL, NW>(x, counter, xw, start, i, P);
    unpack<NL, NW>(k, kw);
    fp_add<NL>(t, x, k, P);
    unpack<NL, NW>(k, r0w);
    fp_sub<NL>(x, t, k, P);
    pack<NL, NW>(o, x);
}

// One cubing round after its open.  x^3 = (y + r)^3 = y (y (y + 3 r) + 3 r2) + r3 with y public, r, r2, r3 this party's shares of the
// round's cube (progs/mimc.py:29 and :53, regrouped): three products.  ym = y R; u = ym (y + 3 r) / R = y (y + 3 r);
// z = ym (u + 3 r2) / R; both results are plain residues, so nothing is converted back.
// Bounds.  s = y + 3 r is taken digit by digit with no carry and no reduction: s[i] <= 4 (2^29 - 1) < 2^31, s < 4 p.  Column j of
// ym * s holds at most NL products of (2^29 - 1) * 4 (2^29 - 1), below 4 NL 2^58: the unreduced multiple counts as four of the
// Lazy<NL>::GROUP = 7 (NL = 9) products a column may take (fp29.hpp:8).  REDC adds NL more and its neighbour's carry (< 2^36):
// 5 NL 2^58 + 2^36 < 2^64 for NL <= 9, so no carry pass in front of REDC.  T = ym s < 4 p^2: REDC returns u < p (1 + 4 p / R) < 2 p
// (R >= 32 p) with a top digit below 2^26: one conditional subtraction.  w = u + 3 r2 (u canonical) has the bounds of s, and
// z follows like u.  + r3, + key (+ c + 1, - r_next) are canonical additions.  p = 2^256 - 189 with every operand p - 1 is the
// largest case (tests/test_mimc_host.py).
// LAST: o = x^3 + key;  else o = x^3 + (key + cst) - r_next with cst = c + 1, the next round's masked input.
template <int NL, int NW, bool LAST>
HB_HD void mimc_round_elem(uint32_t (&o)[NW], const uint32_t (&yw)[NW], const uint32_t (&rw)[NW], const uint32_t (&r2w)[NW], const uint32_t (&r3w)[NW],
                           const uint32_t (&kw)[NW], const uint32_t (&cst)[NL], const uint32_t (&rnw)[NW], const FpParams<NL> &P) {
    uint32_t y[NL], ym[NL], a[NL], s[NL], u[NL], z[NL];
    uint64_t col[2 * NL];
    unpack<NL, NW>(y, yw);
    unpack<NL, NW>(a, rw);
    to_mont<NL>(ym, y, P);
#pragma unroll
    for (int i = 0; i < NL; i++) s[i] = y[i] + 3u * a[i];
    col_zero(col);
    mac<NL>(col, ym, s);
    redc<NL>(u, col, P);
    cond_sub_p<NL>(u, P);
    unpack<NL, NW>(a, r2w);
#pragma unroll
    for (int i = 0; i < NL; i++) s[i] = u[i] + 3u * a[i];
    col_zero(col);
    mac<NL>(col, ym, s);
    redc<NL>(z, col, P);
    cond_sub_p<NL>(z, P);
    unpack<NL, NW>(a, r3w);
    fp_add<NL>(u, z, a, P);
    unpack<NL, NW>(a, kw);
    if constexpr (LAST) {
        fp_add<NL>(z, u, a, P);
    } else {
        fp_add<NL>(s, a, cst, P);
        fp_add<NL>(y, u, s, P);
        unpack<NL, NW>(a, rnw);
        fp_sub<NL>(z, y, a, P);
    }
    pack<NL, NW>(o, z);
}

// ---------------------------------------------------------------- the rows of the MPC rounds (host and device, over a memory policy: hb_rows.hpp)
// A key for all is mem.same's element: wave-uniform on the device, its digits and the round constant in SGPRs.  What was just opened
// and the round's cube are read once (mem.once).  out may be any operand but a broadcast key: a row reads before it stores.
template <int NL> struct MimcFirstArgs { const uint32_t *x, *key, *r0; uint32_t *out; FpConst<NL> start; };

template <bool BCAST> struct MimcFirstRow {
    template <int NL, int NW, class Mem> HB_HD static void run(const MimcFirstArgs<NL> &A, int, int64_t i, int64_t, const Mem &mem, const FpParams<NL> &P) {
        uint32_t xw[NW], kw[NW], rw[NW], ow[NW];
        if (A.x) mem.load(xw, A.x, i);
        if constexpr (BCAST) mem.same(kw, A.key); else mem.load(kw, A.key, i);
        mem.once(rw, A.r0, i);
        mimc_first_elem<NL, NW>(ow, A.x == nullptr, xw, A.start.d, i, kw, rw, P);
        mem.store(A.out, i, ow);
    }
};

// cst = ctr + 1 mod p; LAST: r_next is not read
template <int NL> struct MimcRoundArgs { const uint32_t *y, *r, *r2, *r3, *key, *r_next; uint32_t *out; FpConst<NL> cst; };

template <bool LAST, bool BCAST> struct MimcRoundRow {
    template <int NL, int NW, class Mem> HB_HD static void run(const MimcRoundArgs<NL> &A, int, int64_t i, int64_t, const Mem &mem, const FpParams<NL> &P) {
        uint32_t yw[NW], rw[NW], r2w[NW], r3w[NW], kw[NW], rnw[NW], ow[NW];
        mem.once(yw, A.y, i); mem.once(rw, A.r, i); mem.once(r2w, A.r2, i);
        mem.once(r3w, A.r3, i);
        if constexpr (BCAST) mem.same(kw, A.key); else mem.load(kw, A.key, i);
        if constexpr (!LAST) mem.once(rnw, A.r_next, i);
        mimc_round_elem<NL, NW, LAST>(ow, yw, rw, r2w, r3w, kw, A.cst.d, rnw, P);
        mem.store(A.out, i, ow);
    }
};

// f(the row of (last, broadcast)): the one choice of the launch and of the self test
template <class F> static int with_round_row(bool last, bool bcast, F &&f) {
    if (last) return bcast ? f(MimcRoundRow<true, true>{}) : f(MimcRoundRow<true, false>{});
    return bcast ? f(MimcRoundRow<false, true>{}) : f(MimcRoundRow<false, false>{});
}

// ---------------------------------------------------------------- the cleartext cipher's kernel
// the key of element i; BCAST: element 0 for every lane, wave-uniform (DeviceMem::same) where UNIFORM -- which the paired kernel is
// not: in the 32-byte width the forced scalars of its two chains spilled 25 SGPRs; left to the compiler it spills none
template <int NW, bool BCAST, bool UNIFORM> __device__ __forceinline__ void mimc_load_key(uint32_t (&w)[NW], const uint32_t *key, int64_t i) {
    if constexpr (BCAST && UNIFORM) DeviceMem<NW>().same(w, key);
    else load_words<NW>(w, key + (BCAST ? 0 : i) * NW);
}

// Thread t of block b owns elements b 256 E + t + 256 e, e < E.  A slot past `count` repeats the thread's first element and is not
// stored.  No __restrict__: out may be x, addend or a per-element key (a thread reads all its elements before it writes any).
template <int NL, int NW, int E, bool BCAST>
__global__ void __launch_bounds__(256) k_mimc_plain(const FpParams<NL> P, const uint32_t *x, const FpConst<NL> start, const uint32_t *key, const uint32_t *addend,
                                                    int subtract, int rounds, uint32_t *out, int64_t count) {
    const int64_t first = (int64_t)blockIdx.x * (256 * E) + threadIdx.x;
    if (first >= count) return;
    int64_t idx[E];
    uint32_t xw[E][NW], kw[E][NW], aw[E][NW], ow[E][NW];
#pragma unroll
    for (int e = 0; e < E; e++) {
        const int64_t i = first + 256 * e;
        idx[e] = i < count ? i : first;
        if (x) load_words<NW>(xw[e], x + idx[e] * NW);
        mimc_load_key<NW, BCAST, E == 1>(kw[e], key, idx[e]);
        if (addend) load_words<NW>(aw[e], addend + idx[e] * NW);
    }
    mimc_plain_elem<NL, NW, E>(ow, x == nullptr, xw, start.d, idx, kw, addend != nullptr, aw, subtract != 0, rounds, P);
#pragma unroll
    for (int e = 0; e < E; e++)
        if (first + 256 * e < count) store_words<NW>(out + idx[e] * NW, ow[e]);
}

// ---------------------------------------------------------------- host side
// v mod p as digits (v < 2^63)
template <int NL> static FpConst<NL> mimc_small(const FpParams<NL> &P, uint64_t v) {
    bool below_2_64 = (P.p[2] >> 6) == 0;
    for (int i = 3; i < NL; i++) below_2_64 = below_2_64 && P.p[i] == 0;
    if (below_2_64) v %= (uint64_t)P.p[0] | ((uint64_t)P.p[1] << LB) | ((uint64_t)P.p[2] << (2 * LB));
    FpConst<NL> c;
    for (int q = 0; q < NL; q++) c.d[q] = (q < 3) ? ((uint32_t)(v >> (LB * q)) & DMASK) : 0u;
    return c;
}
// the counter's start from its packed words (NULL: 0); false if it is not below p
template <int NL> static bool mimc_start(FpConst<NL> &c, const FpParams<NL> &P, const uint64_t *start_host) {
    if (start_host) return host_digits<NL, words_of(NL)>(c.d, P, start_host);
    small_digits<NL>(c.d, 0);
    return true;
}

template <int NL, int NW>
static void launch_plain(const FpParams<NL> &P, const uint32_t *x, const FpConst<NL> &start, const uint32_t *key, bool bcast, const uint32_t *addend, int subtract,
                         int rounds, bool pair, uint32_t *out, int64_t count, unsigned blocks, hipStream_t s) {
    if (pair) {
        if (bcast) k_mimc_plain<NL, NW, 2, true><<<blocks, 256, 0, s>>>(P, x, start, key, addend, subtract, rounds, out, count);
        else k_mimc_plain<NL, NW, 2, false><<<blocks, 256, 0, s>>>(P, x, start, key, addend, subtract, rounds, out, count);
    } else {
        if (bcast) k_mimc_plain<NL, NW, 1, true><<<blocks, 256, 0, s>>>(P, x, start, key, addend, subtract, rounds, out, count);
        else k_mimc_plain<NL, NW, 1, false><<<blocks, 256, 0, s>>>(P, x, start, key, addend, subtract, rounds, out, count);
    }
}
// host: the rounds as the rows the device runs, the cleartext cipher as the same element function over `count` elements
template <int NL, int NW>
static int selftest_mimc(const uint64_t *p_limbs, int what, const uint64_t *const *ops, const uint64_t *start_host, bool bcast, int flags, int64_t arg,
                         uint64_t *out, int64_t count) {
    FpParams<NL> P;
    fp_params_from_limbs(P, p_limbs);
    FpConst<NL> start;
    if (!mimc_start(start, P, start_host)) return HB_ERR_BAD_ARG;
    uint32_t *o = u32(out);
    if (what == HB_MIMC_SELFTEST_PLAIN) {
        auto W = [](const uint64_t *base, int64_t i) -> const uint32_t (&)[NW] { return *reinterpret_cast<const uint32_t(*)[NW]>(reinterpret_cast<const uint32_t *>(base) + i * NW); };
        const uint32_t none[NW] = {};
        const bool counter = ops[0] == nullptr, has_addend = ops[2] != nullptr, subtract = (flags & HB_MIMC_SUB) != 0;
        if (flags & HB_MIMC_PAIR) {
            for (int64_t i = 0; i < count; i += 2) {
                int64_t idx[2] = {i, i + 1 < count ? i + 1 : i};
                uint32_t xw[2][NW], kw[2][NW], aw[2][NW], r[2][NW];
                for (int e = 0; e < 2; e++) {
                    memcpy(xw[e], counter ? none : W(ops[0], idx[e]), NW * 4);
                    memcpy(kw[e], W(ops[1], bcast ? 0 : idx[e]), NW * 4);
                    memcpy(aw[e], has_addend ? W(ops[2], idx[e]) : none, NW * 4);
                }
                mimc_plain_elem<NL, NW, 2>(r, counter, xw, start.d, idx, kw, has_addend, aw, subtract, (int)arg, P);
                for (int e = 0; e < 2; e++)
                    if (i + e < count) memcpy(o + (i + e) * NW, r[e], NW * 4);
            }
            return HB_OK;
        }
        for (int64_t i = 0; i < count; i++) {
            int64_t idx[1] = {i};
            uint32_t xw[1][NW], kw[1][NW], aw[1][NW], r[1][NW];
            memcpy(xw[0], counter ? none : W(ops[0], i), NW * 4);
            memcpy(kw[0], W(ops[1], bcast ? 0 : i), NW * 4);
            memcpy(aw[0], has_addend ? W(ops[2], i) : none, NW * 4);
            mimc_plain_elem<NL, NW, 1>(r, counter, xw, start.d, idx, kw, has_addend, aw, subtract, (int)arg, P);
            memcpy(o + i * NW, r[0], NW * 4);
        }
        return HB_OK;
    }
    if (what == HB_MIMC_SELFTEST_FIRST) {
        const MimcFirstArgs<NL> A = {u32(ops[0]), u32(ops[1]), u32(ops[2]), o, start};
        if (bcast) host_rows<MimcFirstRow<true>, NL, NW>(A, 1, count, P); else host_rows<MimcFirstRow<false>, NL, NW>(A, 1, count, P);
        return HB_OK;
    }
    const MimcRoundArgs<NL> A = {u32(ops[0]), u32(ops[1]), u32(ops[2]), u32(ops[3]), u32(ops[4]), u32(ops[5]), o, mimc_small<NL>(P, (uint64_t)arg + 1)};
    return with_round_row(ops[5] == nullptr, bcast, [&](auto row) { host_rows<decltype(row), NL, NW>(A, 1, count, P); return (int)HB_OK; });
}

}  // namespace hb

extern "C" {

int hb_mimc_plain(hb_ctx *ctx, const uint64_t *x_dev, const uint64_t *start_host, const uint64_t *key_dev, int key_broadcast, const uint64_t *addend_dev,
                  int flags, int rounds, uint64_t *out_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0 || (count > 0 && (!key_dev || !out_dev))) return HB_ERR_BAD_ARG;
    if (rounds < 1) return fail(ctx, HB_ERR_BAD_ARG, "hb_mimc_plain: rounds must be at least 1");
    if (flags & ~(HB_MIMC_SUB | HB_MIMC_PAIR)) return fail(ctx, HB_ERR_BAD_ARG, "hb_mimc_plain: unknown flag");
    if ((flags & HB_MIMC_SUB) && !addend_dev) return fail(ctx, HB_ERR_BAD_ARG, "hb_mimc_plain: HB_MIMC_SUB without an addend");
    if (key_broadcast && count > 1 && out_dev == key_dev) return fail(ctx, HB_ERR_BAD_ARG, "hb_mimc_plain: out aliases the broadcast key");
    FpConst<9> sw;
    FpConst<3> sn;
    if (!(ctx->n_limbs == 4 ? mimc_start(sw, ctx->pw, start_host) : mimc_start(sn, ctx->pn, start_host)))
        return fail(ctx, HB_ERR_BAD_ARG, "hb_mimc_plain: start is not below the modulus");
    if (count == 0) return HB_OK;
    const bool pair = (flags & HB_MIMC_PAIR) != 0;
    const int64_t per_block = pair ? 512 : 256, blocks = (count + per_block - 1) / per_block;
    if (blocks > 0x7fffffffLL) return fail(ctx, HB_ERR_UNSUPPORTED, "hb_mimc_plain: batch too large for one launch");
    hipStream_t s = (hipStream_t)stream;
    const uint32_t *x = (const uint32_t *)x_dev, *k = (const uint32_t *)key_dev, *a = (const uint32_t *)addend_dev;
    const int sub = (flags & HB_MIMC_SUB) != 0;
    HB_DISPATCH(ctx, (launch_plain<9, 8>(ctx->pw, x, sw, k, key_broadcast != 0, a, sub, rounds, pair, (uint32_t *)out_dev, count, (unsigned)blocks, s)),
                (launch_plain<3, 2>(ctx->pn, x, sn, k, key_broadcast != 0, a, sub, rounds, pair, (uint32_t *)out_dev, count, (unsigned)blocks, s)));
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

int hb_mimc_first(hb_ctx *ctx, const uint64_t *x_dev, const uint64_t *start_host, const uint64_t *key_dev, int key_broadcast, const uint64_t *r0_dev,
                  uint64_t *out_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0 || (count > 0 && (!key_dev || !r0_dev || !out_dev))) return HB_ERR_BAD_ARG;
    if (key_broadcast && count > 1 && out_dev == key_dev) return fail(ctx, HB_ERR_BAD_ARG, "hb_mimc_first: out aliases the broadcast key");
    FpConst<9> sw;
    FpConst<3> sn;
    if (!(ctx->n_limbs == 4 ? mimc_start(sw, ctx->pw, start_host) : mimc_start(sn, ctx->pn, start_host)))
        return fail(ctx, HB_ERR_BAD_ARG, "hb_mimc_first: start is not below the modulus");
    if (count == 0) return HB_OK;
    HB_ROW_BLOCKS(ctx, "hb_mimc_first");
    // (the start was refused above, ahead of the batch's size as ever; here it becomes the row's argument)
    auto fill = [&](auto &A, const auto &P) {
        A.x = u32(x_dev); A.key = u32(key_dev); A.r0 = u32(r0_dev); A.out = u32(out_dev);
        return mimc_start(A.start, P, start_host);
    };
    if (key_broadcast) return launch_rows<MimcFirstRow<true>, MimcFirstArgs>(ctx, fill, (unsigned)blocks, s, count);
    return launch_rows<MimcFirstRow<false>, MimcFirstArgs>(ctx, fill, (unsigned)blocks, s, count);
}

int hb_mimc_round(hb_ctx *ctx, const uint64_t *y_dev, const uint64_t *r_dev, const uint64_t *r2_dev, const uint64_t *r3_dev, const uint64_t *key_dev,
                  int key_broadcast, int64_t ctr, const uint64_t *r_next_dev, uint64_t *out_dev, int64_t count, void *stream) { HB_API_GUARD(ctx);
    if (!ctx || count < 0 || (count > 0 && (!y_dev || !r_dev || !r2_dev || !r3_dev || !key_dev || !out_dev))) return HB_ERR_BAD_ARG;
    if (ctr < 0 || ctr == INT64_MAX) return fail(ctx, HB_ERR_BAD_ARG, "hb_mimc_round: the round counter must be in [0, 2^63 - 1)");
    if (key_broadcast && count > 1 && out_dev == key_dev) return fail(ctx, HB_ERR_BAD_ARG, "hb_mimc_round: out aliases the broadcast key");
    if (count == 0) return HB_OK;
    HB_ROW_BLOCKS(ctx, "hb_mimc_round");
    auto fill = [&](auto &A, const auto &P) {
        A.y = u32(y_dev); A.r = u32(r_dev); A.r2 = u32(r2_dev); A.r3 = u32(r3_dev); A.key = u32(key_dev); A.r_next = u32(r_next_dev); A.out = u32(out_dev);
        A.cst = mimc_small(P, (uint64_t)ctr + 1);
        return true;
    };
    return with_round_row(r_next_dev == nullptr, key_broadcast != 0, [&](auto row) { return launch_rows<decltype(row), MimcRoundArgs>(ctx, fill, (unsigned)blocks, s, count); });
}

int hb_selftest_mimc(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *operands, const uint64_t *start, int key_broadcast, int flags,
                     int64_t arg, uint64_t *out, int64_t count) {
    if (!p_limbs || !operands || count < 0 || (count > 0 && !out) || (n_limbs != 1 && n_limbs != 4)) return HB_ERR_BAD_ARG;
    if (what == HB_MIMC_SELFTEST_PLAIN) {
        if (arg < 1 || arg > 0x7fffffffLL || (count > 0 && !operands[1]) || (flags & ~(HB_MIMC_SUB | HB_MIMC_PAIR)) || ((flags & HB_MIMC_SUB) && !operands[2])) return HB_ERR_BAD_ARG;
    } else if (what == HB_MIMC_SELFTEST_FIRST) {
        if (flags || !operands[1] || !operands[2]) return HB_ERR_BAD_ARG;
    } else if (what == HB_MIMC_SELFTEST_ROUND) {
        if (flags || arg < 0 || arg == INT64_MAX) return HB_ERR_BAD_ARG;
        for (int i = 0; i < 5; i++) if (!operands[i]) return HB_ERR_BAD_ARG;
    } else {
        return HB_ERR_BAD_ARG;
    }
    if (n_limbs == 4) return selftest_mimc<9, 8>(p_limbs, what, operands, start, key_broadcast != 0, flags, arg, out, count);
    return selftest_mimc<3, 2>(p_limbs, what, operands, start, key_broadcast != 0, flags, arg, out, count);
}

}  // extern "C"

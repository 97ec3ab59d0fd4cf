// hb_rows.hpp -- what the share-array step files share, one of each.
//   The helpers -- the read-once load, the small element helpers (word_bit, diff_elem, small_digits, FpConst), the host's digits of a
//   constant (host_digits, host_mont) and the argument checks of the entry points (u32, overlap, RowSpan / outputs_apart, modulus_bits,
//   HB_ROW_BLOCKS) -- serve all of them: hb_ew.hip, hb_fxp.hip, hb_bd.hip, hb_demux.hip, hb_div.hip, hb_fxsqrt.hip, hb_fxlog.hip, hb_fxtrig.hip, hb_fxatan.hip, hb_lt.hip, hb_eq.hip,
//   hb_jj.hip, hb_mimc.hip, hb_bf.hip, hb_off.hip, hb_offpow.hip, hb_offsb.hip, hb_mat.hip and hb_sort.hip.
//   The shape of a step -- the memory policies, k_rows, host_rows, launch_rows -- serves hb_ew.hip, hb_fxp.hip, hb_bd.hip, hb_demux.hip,
//   hb_div.hip, hb_fxsqrt.hip, hb_fxlog.hip, hb_fxtrig.hip, hb_fxatan.hip, hb_lt.hip, hb_eq.hip, hb_jj.hip, hb_mimc.hip, hb_bf.hip, hb_off.hip, hb_offpow.hip, hb_offsb.hip and hb_sort.hip.  Every step of
//   theirs is a row but for four kernels that keep a shape of their own: k_ew_inv, k_off_invsqrt_scale and k_off_degree_check (wave
//   sums: no lane may leave early) and k_mimc_plain (two elements a thread).  hb_mat.hip (tiles, LDS) uses the helpers alone.
//
// A step is a ROW: a type with
//     template <int NL, int NW, class Mem> HB_HD static void run(const Args &A, int y, int64_t i, int64_t count, const Mem &mem, const FpParams<NL> &P)
// that works element i of row y (a node, a triple, a plane, a product: whatever the step counts in blockIdx.y) -- which operands it
// loads, which element body it calls, where it stores.  Args is the step's argument struct, handed to the kernel by value; Mem is a
// memory policy: load / once (w, base, element index) and store (base, element index, w), element index = row * count + i; same (w,
// base), the element all of a launch share, and pair (x, y, base, even element index), two neighbours moved as one access.  k_rows
// runs a row on the device (256-thread workgroups, one element a thread in x, the row in blockIdx.y, no LDS, no grid stride), host_rows
// runs the same row on the host, so a host self test exercises the addressing the device runs, not a restatement of it.
//
// What stands in front of the row is written once too, as a STEP FUNCTION
//     template <class Run> static int xx_step(const Run &run, <the entry point's arguments without ctx and stream>)
// that holds the null checks, the parameter checks with their messages, the count == 0 return, the RowSpan lists and outputs_apart,
// the Args initialiser (or fill lambda) and the row count, and ends in run.rows<Row>(A, rows, count).  Run says where: DeviceRun
// (the context's field and stream; fail() sets the context's error text; rows() refuses a batch one launch cannot hold and calls
// launch_rows) for the extern "C" entry point, HostRun (the modulus' limbs; fail() is the code alone; rows() calls host_rows) for
// the case of hb_selftest_xx.  Both callers are one line, so the host self test runs the checks, the Args fill and the row count
// the device runs: an operand swapped in an initialiser, a wrong row count or a span list one row short shows without a GPU, and
// the self test refuses an output laid over an input as the entry point does (tests/row_refusal_cases.py).  hb_lt, hb_eq, hb_fxp,
// hb_bd, hb_div, hb_fxsqrt, hb_fxlog, hb_fxtrig, hb_fxatan, hb_sort and hb_demux have step functions; the other seven files still have entry point bodies and HB_ROW_BLOCKS.
#pragma once
#include "hb_common.hpp"

namespace hb {

// ---------------------------------------------------------------- element helpers (host and device)
// read-once operands (bit planes, triples, what was just opened): the 32-byte width takes the non-temporal loads
template <int NW> HB_HD void load_once(uint32_t (&w)[NW], const uint32_t *p) {
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (NW % 4 == 0) load_words_nt<NW>(w, p); else load_words<NW>(w, p);
#else
    load_words<NW>(w, p);
#endif
}

// bit i of the packed words (a chain of selects: the words stay in registers)
template <int NW> HB_HD uint32_t word_bit(const uint32_t (&cw)[NW], int i) {
    uint32_t w = 0;
#pragma unroll
    for (int q = 0; q < NW; q++) w = (q == (i >> 5)) ? cw[q] : w;
    return (w >> (i & 31)) & 1u;
}

// a field element as digits, handed to a kernel by value
template <int NL> struct FpConst { uint32_t d[NL]; };

// r = the small value v
template <int NL> HB_HD void small_digits(uint32_t (&r)[NL], uint32_t v) {
#pragma unroll
    for (int q = 0; q < NL; q++) r[q] = q == 0 ? v : 0u;
}

// o = v - a: a masked difference
template <int NL, int NW> HB_HD void diff_elem(uint32_t (&o)[NW], const uint32_t (&vw)[NW], const uint32_t (&aw)[NW], const FpParams<NL> &P) {
    uint32_t v[NL], a[NL], r[NL];
    unpack<NL, NW>(v, vw);
    unpack<NL, NW>(a, aw);
    fp_sub<NL>(r, v, a, P);
    pack<NL, NW>(o, r);
}

// ---------------------------------------------------------------- memory policies
template <int NW> struct DeviceMem {
    __device__ __forceinline__ void load(uint32_t (&w)[NW], const uint32_t *base, int64_t e) const { load_words<NW>(w, base + e * NW); }
    __device__ __forceinline__ void once(uint32_t (&w)[NW], const uint32_t *base, int64_t e) const { load_once<NW>(w, base + e * NW); }
    __device__ __forceinline__ void store(uint32_t *base, int64_t e, const uint32_t (&w)[NW]) const { store_words<NW>(base + e * NW, w); }
    // element 0 of base, the operand every element of the launch shares: every lane reads the one address (one transaction a wave)
    // and readfirstlane makes the words wave-uniform, so its digits live in SGPRs and its unpack is scalar work
    __device__ __forceinline__ void same(uint32_t (&w)[NW], const uint32_t *base) const {
        load_words<NW>(w, base);
#pragma unroll
        for (int q = 0; q < NW; q++) w[q] = __builtin_amdgcn_readfirstlane(w[q]);
    }
    // elements e and e + 1, e even: two 8-byte elements are one 16-byte access (the caller sees to it that base is 16-byte aligned)
    __device__ __forceinline__ void pair(uint32_t (&x)[NW], uint32_t (&y)[NW], const uint32_t *base, int64_t e) const {
        if constexpr (NW == 2) {
            const uint4 v = *reinterpret_cast<const uint4 *>(base + e * NW);
            x[0] = v.x; x[1] = v.y; y[0] = v.z; y[1] = v.w;
        } else {
            load_words<NW>(x, base + e * NW);
            load_words<NW>(y, base + (e + 1) * NW);
        }
    }
};
template <int NW> struct HostMem {
    void load(uint32_t (&w)[NW], const uint32_t *base, int64_t e) const { memcpy(w, base + e * NW, NW * 4); }
    void once(uint32_t (&w)[NW], const uint32_t *base, int64_t e) const { memcpy(w, base + e * NW, NW * 4); }
    void store(uint32_t *base, int64_t e, const uint32_t (&w)[NW]) const { memcpy(base + e * NW, w, NW * 4); }
    void same(uint32_t (&w)[NW], const uint32_t *base) const { memcpy(w, base, NW * 4); }
    void pair(uint32_t (&x)[NW], uint32_t (&y)[NW], const uint32_t *base, int64_t e) const {
        memcpy(x, base + e * NW, NW * 4);
        memcpy(y, base + (e + 1) * NW, NW * 4);
    }
};

// ---------------------------------------------------------------- a row on the device and on the host
template <class Row, int NL, int NW, class Args> __global__ void __launch_bounds__(256) k_rows(const FpParams<NL> P, const Args A, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    Row::template run<NL, NW>(A, (int)blockIdx.y, i, count, DeviceMem<NW>(), P);
}

template <class Row, int NL, int NW, class Args> void host_rows(const Args &A, int rows, int64_t count, const FpParams<NL> &P) {
    for (int y = 0; y < rows; y++)
        for (int64_t i = 0; i < count; i++) Row::template run<NL, NW>(A, y, i, count, HostMem<NW>(), P);
}

// ---------------------------------------------------------------- host side: argument checks
// packed words of the instantiation with NL digits: <9, 8> or <3, 2>
constexpr int words_of(int nl) { return nl == 9 ? 8 : 2; }

inline const uint32_t *u32(const void *p) { return (const uint32_t *)p; }
inline uint32_t *u32(void *p) { return (uint32_t *)p; }

inline int modulus_bits(const uint64_t *p_limbs, int n_limbs) {
    for (int l = n_limbs - 1; l >= 0; l--)
        if (p_limbs[l]) return 64 * l + 64 - __builtin_clzll(p_limbs[l]);
    return 0;
}
inline bool overlap(const void *x, int64_t x_bytes, const void *y, int64_t y_bytes) {
    const uintptr_t a = (uintptr_t)x, b = (uintptr_t)y;
    return x && y && a < b + (uintptr_t)y_bytes && b < a + (uintptr_t)x_bytes;
}

// one canonical element in host memory -> its digits; false if it is not below p
template <int NL, int NW> bool host_digits(uint32_t (&d)[NL], const FpParams<NL> &P, const uint64_t *host) {
    uint32_t w[NW];
    memcpy(w, host, NW * 4);
    unpack<NL, NW>(d, w);
    for (int i = NL - 1; i >= 0; i--)
        if (d[i] != P.p[i]) return d[i] < P.p[i];
    return false;
}
// the same -> its Montgomery digits
template <int NL, int NW> bool host_mont(uint32_t (&r)[NL], const FpParams<NL> &P, const uint64_t *host) {
    uint32_t d[NL];
    if (!host_digits<NL, NW>(d, P, host)) return false;
    to_mont<NL>(r, d, P);
    return true;
}

// `rows` rows of row_bytes each from p on; a null p is an operand the call does not take
struct RowSpan { const void *p; int64_t rows; };

// no output may lie over an input or over another output
inline bool outputs_apart(const RowSpan *outs, int n_outs, const RowSpan *ins, int n_ins, int64_t row_bytes) {
    for (int o = 0; o < n_outs; o++) {
        for (int i = 0; i < n_ins; i++)
            if (overlap(outs[o].p, outs[o].rows * row_bytes, ins[i].p, ins[i].rows * row_bytes)) return false;
        for (int o2 = o + 1; o2 < n_outs; o2++)
            if (overlap(outs[o].p, outs[o].rows * row_bytes, outs[o2].p, outs[o2].rows * row_bytes)) return false;
    }
    return true;
}

// ---------------------------------------------------------------- host side: the launch
// blocks of 256 elements in x, refused where one launch cannot hold them; s = the caller's stream (the files without step functions:
// DeviceRun::too_large is the same refusal, and the macro goes when the last of them has them)
#define HB_ROW_BLOCKS(ctx, name)                                                                                       \
    const int64_t blocks = (count + 255) / 256;                                                                        \
    if (blocks > 0x7fffffffLL) return fail(ctx, HB_ERR_UNSUPPORTED, name ": batch too large for one launch");          \
    hipStream_t s = (hipStream_t)stream

// Row over `grid` for the context's field, <9, 8> with ctx->pw or <3, 2> with ctx->pn, and the launch check.
template <class Row, class Args> int launch_rows(hb_ctx *ctx, const Args &A, dim3 grid, hipStream_t s, int64_t count) {
    if (ctx->n_limbs == 4) k_rows<Row, 9, 8><<<grid, 256, 0, s>>>(ctx->pw, A, count);
    else k_rows<Row, 3, 2><<<grid, 256, 0, s>>>(ctx->pn, A, count);
    HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}
// The same for a step whose argument struct ArgsT<NL> carries constants as digits of the field: fill(A, P) sets it up and returns
// false where a constant is refused (HB_ERR_BAD_ARG: the entry point adds its message).  An empty batch is checked and not launched.
template <class Row, template <int> class ArgsT, class Fill> int launch_rows(hb_ctx *ctx, Fill &&fill, dim3 grid, hipStream_t s, int64_t count) {
    if (ctx->n_limbs == 4) {
        ArgsT<9> A;
        if (!fill(A, ctx->pw)) return HB_ERR_BAD_ARG;
        if (count) k_rows<Row, 9, 8><<<grid, 256, 0, s>>>(ctx->pw, A, count);
    } else {
        ArgsT<3> A;
        if (!fill(A, ctx->pn)) return HB_ERR_BAD_ARG;
        if (count) k_rows<Row, 3, 2><<<grid, 256, 0, s>>>(ctx->pn, A, count);
    }
    if (count) HB_LAUNCH_CHECK(ctx);
    return HB_OK;
}

// ---------------------------------------------------------------- where a step function runs (the header comment has the shape)
// the device: the context's field (ctx->pw / ctx->pn as they stand: nothing is rebuilt a call) on stream s
struct DeviceRun {
    hb_ctx *ctx;
    hipStream_t s;
    const char *name;                                                           // the entry point's, for the refusals made here

    const uint64_t *modulus() const { return ctx->p_limbs; }
    int limbs() const { return ctx->n_limbs; }
    int bits() const { return modulus_bits(ctx->p_limbs, ctx->n_limbs); }
    int64_t elem_bytes() const { return 8 * (int64_t)ctx->n_limbs; }
    int fail(int code, const char *msg) const { return hb::fail(ctx, code, msg); }

    // blocks of 256 elements in x; where one launch cannot hold them the call is refused (the text is built on that path alone, so
    // the path of a launch stays a compare and inlines)
    static int64_t blocks(int64_t count) { return (count + 255) / 256; }
    static bool fits(int64_t count) { return blocks(count) <= 0x7fffffffLL; }
    __attribute__((noinline)) int too_large() const { return fail(HB_ERR_UNSUPPORTED, (std::string(name) + ": batch too large for one launch").c_str()); }

    template <class Row, class Args> int rows(const Args &A, int n_rows, int64_t count) const {
        if (!fits(count)) return too_large();
        return launch_rows<Row>(ctx, A, dim3((unsigned)blocks(count), (unsigned)n_rows), s, count);
    }
    template <class Row, template <int> class ArgsT, class Fill> int rows(Fill &&fill, int n_rows, int64_t count) const {
        if (!fits(count)) return too_large();
        return launch_rows<Row, ArgsT>(ctx, fill, dim3((unsigned)blocks(count), (unsigned)n_rows), s, count);
    }
};

// the host: FpParams from the modulus' limbs, the row walked by host_rows
struct HostRun {
    const uint64_t *p_limbs;
    int n_limbs;                                                                // 4 or 1: the self test's front has seen to it

    const uint64_t *modulus() const { return p_limbs; }
    int limbs() const { return n_limbs; }
    int bits() const { return modulus_bits(p_limbs, n_limbs); }
    int64_t elem_bytes() const { return 8 * (int64_t)n_limbs; }
    int fail(int code, const char *) const { return code; }

    // the row over the field of NL digits, its Args set up by fill(A, P) as in launch_rows' second form
    template <class Row, class ArgsN, int NL, class Fill> int walk(Fill &&fill, int n_rows, int64_t count) const {
        FpParams<NL> P;
        fp_params_from_limbs(P, p_limbs);
        ArgsN A;
        if (!fill(A, P)) return HB_ERR_BAD_ARG;
        host_rows<Row, NL, words_of(NL)>(A, n_rows, count, P);
        return HB_OK;
    }
    template <class Row, class Args> int rows(const Args &A0, int n_rows, int64_t count) const {
        const auto copy = [&](Args &A, const auto &) { A = A0; return true; };
        return n_limbs == 4 ? walk<Row, Args, 9>(copy, n_rows, count) : walk<Row, Args, 3>(copy, n_rows, count);
    }
    template <class Row, template <int> class ArgsT, class Fill> int rows(Fill &&fill, int n_rows, int64_t count) const {
        return n_limbs == 4 ? walk<Row, ArgsT<9>, 9>(fill, n_rows, count) : walk<Row, ArgsT<3>, 3>(fill, n_rows, count);
    }
};

}  // namespace hb

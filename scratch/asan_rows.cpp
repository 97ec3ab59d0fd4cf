// A stand-alone HOST program over hb_selftest_lt, hb_selftest_eq, hb_selftest_fxp, hb_selftest_bd, hb_selftest_div, hb_selftest_jj,
// hb_selftest_ew, hb_selftest_off, hb_selftest_mimc and hb_selftest_bf for AddressSanitizer and UBSan: the rows of csrc/hb_lt.hip,
// hb_eq.hip, hb_fxp.hip, hb_bd.hip, hb_div.hip, hb_jj.hip, hb_ew.hip, hb_off.hip, hb_mimc.hip and hb_bf.hip (hb_rows.hpp: host_rows runs
// what k_rows runs) compiled WITH the sanitizers into this program; the rest of the library comes from libhbmpc_hip.so as it is.  No
// GPU is touched.
//
//   C=honeybadgermpc_amd/csrc; hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-omit-frame-pointer scratch/asan_rows.cpp $C/hb_lt.hip $C/hb_eq.hip $C/hb_fxp.hip $C/hb_bd.hip $C/hb_div.hip \
//         $C/hb_jj.hip $C/hb_ew.hip $C/hb_off.hip $C/hb_mimc.hip $C/hb_bf.hip -Lhoneybadgermpc_amd/lib -lhbmpc_hip \
//         -Wl,-rpath,$PWD/honeybadgermpc_amd/lib -o scratch/asan_rows && scratch/asan_rows
//
// Every step of lt, eq and jj at count = 3, rows = 3 (hb_eq), a triples' row stride of count + 3 (hb_jj); one tree level each of hb_fxp,
// hb_bd and hb_div at count = 3; the element-wise, mul-add and MiMC rows at 1, 255, 256, 257 and 513 elements with a key or an operand
// for all (HostMem::same: ONE element on the heap) and one an element; a butterfly layer at k = 2, 4 and 1024 and every stride the GPU
// suite runs (HostMem::pair at stride 1 in the 8-byte width).  Both widths.  The self tests of lt, eq, fxp, bd and div run the step
// functions of hb_rows.hpp (the checks, the Args fill and the row count of the entry points), so each of these families also gets one
// call with an output over an input's last row and one with a parameter past its bound: both refused.  Every operand and output is a
// heap buffer of exactly the documented size, so a row that reads or writes one element past an array is a report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/hbmpc_hip.h"

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); fails++; } } while (0)

static uint64_t lcg = 88172645463325252ull;
static uint64_t next() { lcg ^= lcg << 13; lcg ^= lcg >> 7; lcg ^= lcg << 17; return lcg; }

static int NL;                                                             // 64-bit limbs an element: 4 or 1
// exactly `elems` elements of canonical residues (the top limb stays below the modulus')
struct Elems {
    uint64_t *p;
    explicit Elems(size_t elems) : p((uint64_t *)malloc(elems * NL * 8)) {
        for (size_t i = 0; i < elems * NL; i++) p[i] = (i % NL == (size_t)NL - 1) ? next() >> 4 : next();
    }
    ~Elems() { free(p); }
    operator const uint64_t *() const { return p; }
};
template <class T> struct Raw {
    T *p;
    explicit Raw(size_t n) : p((T *)calloc(n, sizeof(T))) {}
    ~Raw() { free(p); }
};

static const uint64_t BLS[4] = {0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull};
static const uint64_t P64[1] = {0xffffffffffffffc5ull};

static void less_than(const uint64_t *p, int L, int64_t n) {
    const int64_t prm[2][2] = {{L, HB_LT_DIRECT}, {L, HB_LT_REFERENCE}};
    Elems a(n), b(n), r(n), c(n), w(n), x(n), s(n), u(n), v(n), bits((size_t)L * n), o5(5 * n), o2(2 * n);
    Elems t0(n), t1(n), t2(n), t3(n), t4(n), t5(n), t6(n), t7(n);
    for (int has_b = 0; has_b < 2; has_b++) {
        Elems out(n);
        const uint64_t *ops[3] = {a, has_b ? b.p : nullptr, r};
        uint64_t *outs[1] = {out.p};
        CHECK(hb_selftest_lt(p, NL, HB_LT_SELFTEST_MASK, ops, prm[0], outs, n) == HB_OK);
    }
    for (int mode = 0; mode < 2; mode++) {
        Elems g((size_t)L * n), q((size_t)L * n);
        const uint64_t *ops[2] = {c, bits};
        uint64_t *outs[2] = {g.p, q.p};
        CHECK(hb_selftest_lt(p, NL, HB_LT_SELFTEST_LEAVES, ops, prm[mode], outs, n) == HB_OK);
    }
    {
        Elems ou(n), masked(2 * n);
        const uint64_t *ops[5] = {c, r, w, t0, t1};
        uint64_t *outs[2] = {ou.p, masked.p};
        CHECK(hb_selftest_lt(p, NL, HB_LT_SELFTEST_XOR_MASK, ops, prm[0], outs, n) == HB_OK);
    }
    {
        Elems ou(n), masked(5 * n);
        const uint64_t *ops[9] = {c, r, x, s, bits, t0, t1, t2, t3};
        uint64_t *outs[2] = {ou.p, masked.p};
        CHECK(hb_selftest_lt(p, NL, HB_LT_SELFTEST_DMASK, ops, prm[1], outs, n) == HB_OK);
    }
    {
        Elems ov(n), d0(n), masked(2 * n);
        const uint64_t *ops[11] = {o5, u, bits, t0, t1, t2, t3, t4, t5, t6, t7};
        uint64_t *outs[3] = {ov.p, d0.p, masked.p};
        CHECK(hb_selftest_lt(p, NL, HB_LT_SELFTEST_MID, ops, prm[1], outs, n) == HB_OK);
    }
    {
        Elems out(n);
        const uint64_t *ops[6] = {o2, u, v, t0, t1, t2};
        uint64_t *outs[1] = {out.p};
        CHECK(hb_selftest_lt(p, NL, HB_LT_SELFTEST_XOR_FINISH, ops, prm[0], outs, n) == HB_OK);
    }
    {                                                                       // refused by the step function: masked over the last row of s_bits; L one short
        Elems ou(n);
        const uint64_t *ops[9] = {c, r, x, s, bits, t0, t1, t2, t3};
        uint64_t *outs[2] = {ou.p, bits.p + (size_t)(L - 1) * n * NL};
        const int64_t shortL[2] = {L - 1, HB_LT_REFERENCE};
        CHECK(hb_selftest_lt(p, NL, HB_LT_SELFTEST_DMASK, ops, prm[1], outs, n) == HB_ERR_BAD_ARG);
        Elems masked(5 * n);
        outs[1] = masked.p;
        CHECK(hb_selftest_lt(p, NL, HB_LT_SELFTEST_DMASK, ops, shortL, outs, n) == HB_ERR_BAD_ARG);
    }
}

static void equality(const uint64_t *p, int64_t rows, int64_t n) {
    const int64_t rc = rows * n, prm[2][2] = {{rows, HB_EQ_BIT}, {rows, HB_EQ_REFERENCE}};
    std::vector<uint64_t> nr(NL, 0);
    nr[0] = 5;
    Elems x(n), y(n), r(rc), rp(rc), bits(rc), o4(4 * rc), o2(2 * rc), c(rc);
    Elems t0(rc), t1(rc), t2(rc), t3(rc), t4(rc), t5(rc), t6(rc), t7(rc);
    memset(c.p + (size_t)(n + 1) * NL, 0, NL * 8);                         // one c of the middle row is 0
    {
        Raw<int8_t> out(n);
        const uint64_t *ops[1] = {x};
        void *outs[1] = {out.p};
        CHECK(hb_selftest_eq(p, NL, HB_EQ_SELFTEST_LEGENDRE, ops, prm[0], outs, n) == HB_OK);
    }
    for (int has_y = 0; has_y < 2; has_y++) {
        Elems masked(4 * rc);
        const uint64_t *ops[8] = {x, has_y ? y.p : nullptr, r, rp, t0, t1, t2, t3};
        void *outs[1] = {masked.p};
        CHECK(hb_selftest_eq(p, NL, HB_EQ_SELFTEST_MASK1, ops, prm[0], outs, n) == HB_OK);
    }
    {
        Elems masked2(2 * rc), dr(rc);
        const uint64_t *ops[11] = {o4, t0, t1, t2, t3, t4, t5, bits, t6, t7, nr.data()};
        void *outs[2] = {masked2.p, dr.p};
        CHECK(hb_selftest_eq(p, NL, HB_EQ_SELFTEST_MID, ops, prm[0], outs, n) == HB_OK);
    }
    for (int alias = 0; alias < 2; alias++) {                               // c a fresh array, then c = dr
        Elems dr(rc), out(rc);
        const uint64_t *ops[5] = {o2, dr, t0, t1, t2};
        void *outs[1] = {alias ? dr.p : out.p};
        CHECK(hb_selftest_eq(p, NL, HB_EQ_SELFTEST_CSHARE, ops, prm[0], outs, n) == HB_OK);
    }
    for (int mode = 0; mode < 2; mode++) {
        Elems factor(rc);
        Raw<int32_t> zero_rows(rows);
        const uint64_t *ops[3] = {c, bits, nr.data()};
        void *outs[2] = {factor.p, zero_rows.p};
        CHECK(hb_selftest_eq(p, NL, HB_EQ_SELFTEST_FINISH, ops, prm[mode], outs, n) == HB_OK);
        CHECK(zero_rows.p[0] == 0 && zero_rows.p[1] == 1 && zero_rows.p[2] == 0);
        for (int l = 0; l < NL; l++) CHECK(factor.p[(size_t)(n + 1) * NL + l] == 0);
    }
    {                                                                       // refused by the step function: masked2 over the last row of qc; no rows
        Elems dr(rc);
        const uint64_t *ops[11] = {o4, t0, t1, t2, t3, t4, t5, bits, t6, t7, nr.data()};
        void *outs[2] = {t7.p + (size_t)(rows - 1) * n * NL, dr.p};
        const int64_t none[2] = {0, HB_EQ_BIT};
        CHECK(hb_selftest_eq(p, NL, HB_EQ_SELFTEST_MID, ops, prm[0], outs, n) == HB_ERR_BAD_ARG);
        Elems masked2(2 * rc);
        outs[0] = masked2.p;
        CHECK(hb_selftest_eq(p, NL, HB_EQ_SELFTEST_MID, ops, none, outs, n) == HB_ERR_BAD_ARG);
    }
}

// hb_fxp.hip, hb_bd.hip, hb_div.hip: one level of each family's tree through its step functions (carry level of 3 nodes, prefix level 0
// of m = 3, OR level 0 of 2 planes), then the same call with the output over the last row of an input and with a parameter past its bound
static void tree_levels(const uint64_t *p, int64_t n) {
    Elems g(3 * n), q(3 * n), opened(4 * n), ta(2 * n), tb(2 * n), tab(2 * n);
    {
        Elems masked(4 * n);
        const uint64_t *ops[4] = {g, q, ta, tb};
        uint64_t *outs[1] = {masked.p}, *over[1] = {tb.p + (size_t)n * NL};
        const int64_t level[5] = {0, 0, 0, 3, 0}, wide[5] = {0, 0, 0, 258, 0};
        CHECK(hb_selftest_fxp(p, NL, HB_FXP_SELFTEST_CARRY_MASK, ops, level, outs, n) == HB_OK);
        CHECK(hb_selftest_fxp(p, NL, HB_FXP_SELFTEST_CARRY_MASK, ops, level, over, n) == HB_ERR_BAD_ARG);
        CHECK(hb_selftest_fxp(p, NL, HB_FXP_SELFTEST_CARRY_MASK, ops, wide, outs, n) == HB_ERR_BAD_ARG);
        Elems g_out(2 * n), p_out(2 * n);
        const uint64_t *cops[6] = {opened, g, q, ta, tb, tab};
        uint64_t *couts[2] = {g_out.p, p_out.p};
        CHECK(hb_selftest_fxp(p, NL, HB_FXP_SELFTEST_CARRY_COMBINE, cops, level, couts, n) == HB_OK);
    }
    {
        Elems masked(2 * n), g2(2 * n), q2(2 * n);
        const uint64_t *ops[4] = {g2, q2, ta, tb};
        uint64_t *outs[1] = {masked.p}, *over[1] = {q2.p + (size_t)n * NL};
        const int64_t level[2] = {3, 0}, none[2] = {3, 1};
        CHECK(hb_selftest_bd(p, NL, HB_BD_SELFTEST_PREFIX_MASK, ops, level, outs, n) == HB_OK);
        CHECK(hb_selftest_bd(p, NL, HB_BD_SELFTEST_PREFIX_MASK, ops, level, over, n) == HB_ERR_BAD_ARG);
        CHECK(hb_selftest_bd(p, NL, HB_BD_SELFTEST_PREFIX_MASK, ops, none, outs, n) == HB_ERR_BAD_ARG);
        const uint64_t *cops[4] = {opened, ta, tb, tab};
        uint64_t *couts[2] = {g2.p, q2.p};
        CHECK(hb_selftest_bd(p, NL, HB_BD_SELFTEST_PREFIX_COMBINE, cops, level, couts, n) == HB_OK);
    }
    {
        Elems masked(2 * n), y(2 * n);
        const uint64_t *ops[3] = {y, ta, tb};
        uint64_t *outs[1] = {masked.p}, *over[1] = {y.p + (size_t)n * NL};
        const int64_t level[5] = {2, 0, 1, 0, 0}, none[5] = {257, 0, 1, 0, 0};
        CHECK(hb_selftest_div(p, NL, HB_DIV_SELFTEST_OR_MASK, ops, level, outs, n) == HB_OK);
        CHECK(hb_selftest_div(p, NL, HB_DIV_SELFTEST_OR_MASK, ops, level, over, n) == HB_ERR_BAD_ARG);
        CHECK(hb_selftest_div(p, NL, HB_DIV_SELFTEST_OR_MASK, ops, none, outs, n) == HB_ERR_BAD_ARG);
        const uint64_t *cops[4] = {opened, ta, tb, tab};
        uint64_t *couts[1] = {y.p};
        CHECK(hb_selftest_div(p, NL, HB_DIV_SELFTEST_OR_COMBINE, cops, level, couts, n) == HB_OK);
    }
}

static void jubjub(const uint64_t *p, int64_t m) {
    const int64_t stride = m + 3, K = 3;
    std::vector<uint64_t> a(p, p + NL), d(NL, 0);
    a[0] -= 1;                                                             // a = -1
    d[0] = 2;
    Elems x1(m), y1(m), x2(m), y2(m), rx(m), ry(m), one_n(1), one_x(1), one_y(1);
    for (int flags = 0; flags < 4; flags++) {
        Elems out(2 * m);
        const uint64_t *ops[3] = {(flags & HB_JJ_SCALAR_BROADCAST) ? one_n.p : rx.p, (flags & HB_JJ_POINT_BROADCAST) ? one_x.p : x1.p,
                                  (flags & HB_JJ_POINT_BROADCAST) ? one_y.p : y1.p};
        CHECK(hb_selftest_jj(p, NL, HB_JJ_SELFTEST_SCALAR_MUL, ops, a.data(), d.data(), flags, 0, out.p, m) == HB_OK);
    }
    {
        Elems out(3 * K * m);
        const uint64_t *ops[2] = {x1, y1};
        CHECK(hb_selftest_jj(p, NL, HB_JJ_SELFTEST_DOUBLE_TABLE, ops, a.data(), nullptr, 0, K, out.p, m) == HB_OK);
    }
    {                                                                      // rows 0..3 of the triples: the last row holds m elements, no more
        Elems tp(3 * stride + m), tq(3 * stride + m), out(8 * m);
        const uint64_t *ops[6] = {x1, y1, x2, y2, tp, tq};
        CHECK(hb_selftest_jj(p, NL, HB_JJ_SELFTEST_MASK, ops, nullptr, nullptr, 0, stride, out.p, m) == HB_OK);
    }
    {                                                                      // rows 0..6
        Elems A(8 * m), tp(6 * stride + m), tq(6 * stride + m), tpq(6 * stride + m), out(6 * m);
        const uint64_t *ops[6] = {A, tp, tq, tpq, rx, ry};
        CHECK(hb_selftest_jj(p, NL, HB_JJ_SELFTEST_STAGE1, ops, nullptr, nullptr, 0, stride, out.p, m) == HB_OK);
    }
    Elems tp(8 * stride + m), tq(8 * stride + m), tpq(8 * stride + m);       // rows 0..8
    {
        Elems B(6 * m), out(6 * m);
        const uint64_t *ops[6] = {B, tp, tq, tpq, rx, ry};
        CHECK(hb_selftest_jj(p, NL, HB_JJ_SELFTEST_STAGE2, ops, nullptr, d.data(), 0, stride, out.p, m) == HB_OK);
    }
    {
        Elems C(4 * m), out(2 * m);
        const uint64_t *ops[4] = {C, tp, tq, tpq};
        CHECK(hb_selftest_jj(p, NL, HB_JJ_SELFTEST_STAGE3, ops, nullptr, nullptr, 0, stride, out.p, m) == HB_OK);
    }
    {
        Elems inv(2 * m), uv(2 * m), out(2 * m);
        const uint64_t *ops[2] = {inv, uv};
        CHECK(hb_selftest_jj(p, NL, HB_JJ_SELFTEST_SCALE, ops, nullptr, nullptr, 0, 0, out.p, m) == HB_OK);
    }
}

static const int64_t COUNTS[5] = {1, 255, 256, 257, 513};

static void elementwise(const uint64_t *p, int64_t n) {
    Elems a(n), b(n), one(1), d(n), e(n), tp(n), tq(n), tpq(n);
    for (int op = HB_EW_ADD; op <= HB_EW_NEG; op++)
        for (int bcast = 0; bcast < (op == HB_EW_NEG ? 1 : 2); bcast++)
            for (int alias = 0; alias < 3; alias++) {                       // out a fresh array, a itself, b itself (where b is an array)
                if (alias == 2 && (bcast || op == HB_EW_NEG)) continue;
                Elems x(n), y(n), out(n);
                const uint64_t *ops[2] = {x, op == HB_EW_NEG ? nullptr : bcast ? one.p : y.p};
                CHECK(hb_selftest_ew(p, NL, op | (bcast ? HB_EW_SELFTEST_BROADCAST : 0), ops, alias == 0 ? out.p : alias == 1 ? x.p : y.p, n) == HB_OK);
            }
    Elems out(n);
    const uint64_t *ops[5] = {d, e, tp, tq, tpq};
    CHECK(hb_selftest_ew(p, NL, HB_EW_SELFTEST_BEAVER, ops, out.p, n) == HB_OK);
}

static void mul_add(const uint64_t *p, int64_t n) {
    for (int shape = 0; shape < 3; shape++) {                               // plain; b is a (the square); out is c
        Elems a(n), b(n), c(n), out(n);
        const uint64_t *ops[3] = {a, shape == 1 ? a.p : b.p, c};
        CHECK(hb_selftest_off(p, NL, HB_OFF_SELFTEST_MUL_ADD, ops, shape == 2 ? c.p : out.p, n) == HB_OK);
    }
}

static void mimc_rounds(const uint64_t *p, int64_t n) {
    std::vector<uint64_t> start(p, p + NL);
    start[0] -= 3;                                                         // the counters wrap
    Elems x(n), r0(n), y(n), r(n), r2(n), r3(n), rn(n), keys(n), key(1);
    for (int bcast = 0; bcast < 2; bcast++) {
        const uint64_t *k = bcast ? key.p : keys.p;
        for (int counter = 0; counter < 2; counter++) {
            Elems out(n);
            const uint64_t *ops[3] = {counter ? nullptr : x.p, k, r0};
            CHECK(hb_selftest_mimc(p, NL, HB_MIMC_SELFTEST_FIRST, ops, counter ? start.data() : nullptr, bcast, 0, 0, out.p, n) == HB_OK);
        }
        for (int last = 0; last < 2; last++)
            for (int64_t ctr : {(int64_t)0, (int64_t)1 << 62}) {
                Elems out(n);
                const uint64_t *ops[6] = {y, r, r2, r3, k, last ? nullptr : rn.p};
                CHECK(hb_selftest_mimc(p, NL, HB_MIMC_SELFTEST_ROUND, ops, nullptr, bcast, 0, ctr, out.p, n) == HB_OK);
            }
    }
}

static void butterfly(const uint64_t *p, int64_t k, int a) {
    const int64_t half = k / 2;
    Elems in(k), bits(half), tp(half), tq(half), tpq(half), d(half), e(half);
    for (int has_bits = 0; has_bits < 2; has_bits++) {
        Elems masked(has_bits ? k : half);
        const uint64_t *ops[4] = {in, has_bits ? bits.p : nullptr, has_bits ? tp.p : nullptr, tq};
        CHECK(hb_selftest_bf(p, NL, HB_BF_SELFTEST_MASK, ops, k, a, masked.p) == HB_OK);
    }
    Elems out(k);
    const uint64_t *ops[6] = {in, d, e, tp, tq, tpq};
    CHECK(hb_selftest_bf(p, NL, HB_BF_SELFTEST_SWITCH, ops, k, a, out.p) == HB_OK);
}

int main() {
    for (int wide = 1; wide >= 0; wide--) {
        NL = wide ? 4 : 1;
        const uint64_t *p = wide ? BLS : P64;
        less_than(p, wide ? 255 : 64, 3);
        equality(p, 3, 3);
        tree_levels(p, 3);
        jubjub(p, 3);
        for (int64_t n : COUNTS) { elementwise(p, n); mul_add(p, n); mimc_rounds(p, n); }
        butterfly(p, 2, 0);
        for (int a : {0, 1}) butterfly(p, 4, a);
        for (int a : {0, 5, 9}) butterfly(p, 1024, a);
    }
    printf(fails ? "asan_rows: %d check(s) FAILED\n" : "asan_rows ok\n", fails);
    return fails ? 1 : 0;
}

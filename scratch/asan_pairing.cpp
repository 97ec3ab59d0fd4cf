// A stand-alone HOST program over hb_selftest_pairing for AddressSanitizer and UBSan: the bodies of csrc/hb_fq12_elem.hpp and csrc/hb_pair.hip
// (the tower, the Miller loop over a prepared table, the final exponentiation, the verdict) compiled WITH the sanitizers into this program;
// the rest of the library (hb_selftest_g1 for the points) comes from libhbmpc_hip.so as it is.  No GPU is touched.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         scratch/asan_pairing.cpp honeybadgermpc_amd/csrc/hb_pair.hip -Lhoneybadgermpc_amd/lib -lhbmpc_hip \
//         -Wl,-rpath,$PWD/honeybadgermpc_amd/lib -o scratch/asan_pairing && scratch/asan_pairing
//
// Every buffer has exactly the size the self test may touch, so a word too many is a report.  The table's coefficients are not a real G2
// point's (preparing one is the Python model's work): any 204 residues below Q drive the same loads, products and stores, and the algebra is
// checked by what holds for every table: the tower's laws on random operands, FE(a) FE(1 / a) = 1, the Frobenius laws, an all-identity
// item is 1 and accepted, a live item is not, and a skipped pair leaves the other pair's value.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/hbmpc_hip.h"

static const uint64_t GEN[12] = {0xfb3af00adb22c6bbull, 0x6c55e83ff97a1aefull, 0xa14e3a3f171bac58ull, 0xc3688c4f9774b905ull, 0x2695638c4fa9ac0full, 0x17f1d3a73197d794ull,
                                 0xcaa232946c5e7e1ull,  0xd03cc744a2888ae4ull, 0xdb18cb2c04b3edull,   0xfcf5e095d5d00af6ull, 0xa09e30ed741d8ae4ull, 0x8b3f481e3aaa0f1ull};

struct Buf {
    uint64_t *p;
    size_t words;
    explicit Buf(size_t w) : p((uint64_t *)aligned_alloc(16, ((w ? w : 2) * 8 + 15) / 16 * 16)), words(w) { memset(p, 0, (w ? w : 2) * 8); }
    ~Buf() { free(p); }
};

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); fails++; } } while (0)

static uint64_t lcg = 88172645463325252ull;
static uint64_t next() { lcg ^= lcg << 13; lcg ^= lcg >> 7; lcg ^= lcg << 17; return lcg; }
// residues below 2^380 < Q
static void fill_residues(uint64_t *p, size_t n) {
    for (size_t i = 0; i < n; i++) {
        for (int k = 0; k < 6; k++) p[6 * i + k] = next();
        p[6 * i + 5] &= 0x0fffffffffffffffull;
    }
}
static int tower(int op, const Buf &a, const Buf *b, int64_t arg, Buf &out, int64_t count) {
    const uint64_t *ops[5] = {a.p, b ? b->p : nullptr, nullptr, nullptr, nullptr};
    return hb_selftest_pairing(HB_PAIR_SELFTEST_TOWER, ops, op, arg, out.p, count);
}
static bool is_one(const uint64_t *gt) {
    if (gt[0] != 1) return false;
    for (int i = 1; i < 72; i++) if (gt[i]) return false;
    return true;
}

int main() {
    const int N = 3;
    Buf a(N * 72), b(N * 72), c(N * 72), r0(N * 72), r1(N * 72), r2(N * 72);
    fill_residues(a.p, N * 12);
    fill_residues(b.p, N * 12);
    fill_residues(c.p, N * 12);
    // every operation once, into a buffer of exactly its size
    for (int op = 0; op <= HB_PAIR_OP_FQ12_CYCLO_SQR; op++) {
        const bool two = op == HB_PAIR_OP_FQ2_MUL || op == HB_PAIR_OP_FQ6_MUL || op == HB_PAIR_OP_FQ12_MUL || op == HB_PAIR_OP_FQ6_MUL_BY_01 || op == HB_PAIR_OP_FQ6_MUL_BY_1 ||
                         op == HB_PAIR_OP_FQ12_MUL_BY_014;
        CHECK(tower(op, a, two ? &b : nullptr, op == HB_PAIR_OP_FQ12_FROBENIUS ? 1 : 0, r0, N) == HB_OK);
    }
    // (a b) c == a (b c); a^2 == a a; a / a == 1
    CHECK(tower(HB_PAIR_OP_FQ12_MUL, a, &b, 0, r0, N) == HB_OK && tower(HB_PAIR_OP_FQ12_MUL, r0, &c, 0, r1, N) == HB_OK);
    CHECK(tower(HB_PAIR_OP_FQ12_MUL, b, &c, 0, r0, N) == HB_OK && tower(HB_PAIR_OP_FQ12_MUL, a, &r0, 0, r2, N) == HB_OK);
    CHECK(memcmp(r1.p, r2.p, N * 72 * 8) == 0);
    CHECK(tower(HB_PAIR_OP_FQ12_SQR, a, nullptr, 0, r0, N) == HB_OK && tower(HB_PAIR_OP_FQ12_MUL, a, &a, 0, r1, N) == HB_OK && memcmp(r0.p, r1.p, N * 72 * 8) == 0);
    CHECK(tower(HB_PAIR_OP_FQ12_INV, a, nullptr, 0, r0, N) == HB_OK && tower(HB_PAIR_OP_FQ12_MUL, a, &r0, 0, r1, N) == HB_OK);
    for (int i = 0; i < N; i++) CHECK(is_one(r1.p + 72 * i));
    // Frobenius: 1 then 2 is 3; twelve times is the identity
    CHECK(tower(HB_PAIR_OP_FQ12_FROBENIUS, a, nullptr, 1, r0, N) == HB_OK && tower(HB_PAIR_OP_FQ12_FROBENIUS, r0, nullptr, 2, r1, N) == HB_OK);
    CHECK(tower(HB_PAIR_OP_FQ12_FROBENIUS, a, nullptr, 3, r2, N) == HB_OK && memcmp(r1.p, r2.p, N * 72 * 8) == 0);
    memcpy(r0.p, a.p, N * 72 * 8);
    for (int k = 0; k < 12; k++) { CHECK(tower(HB_PAIR_OP_FQ12_FROBENIUS, r0, nullptr, 1, r1, N) == HB_OK); memcpy(r0.p, r1.p, N * 72 * 8); }
    CHECK(memcmp(r0.p, a.p, N * 72 * 8) == 0);
    // FE(a) FE(1 / a) == 1, FE(a) != 1
    CHECK(tower(HB_PAIR_OP_FQ12_FINAL_EXP, a, nullptr, 0, r0, 1) == HB_OK && !is_one(r0.p));
    CHECK(tower(HB_PAIR_OP_FQ12_INV, a, nullptr, 0, r1, 1) == HB_OK && tower(HB_PAIR_OP_FQ12_FINAL_EXP, r1, nullptr, 0, r2, 1) == HB_OK);
    CHECK(tower(HB_PAIR_OP_FQ12_MUL, r0, &r2, 0, r1, 1) == HB_OK && is_one(r1.p));
    // a table, a Miller loop with its final exponentiation, a verdict
    const size_t tw = (size_t)hb_pair_table_bytes() / 8;
    Buf coeffs(204 * 12), table(tw), table2(tw);
    fill_residues(coeffs.p, 204 * 2);
    {
        const uint64_t *ops[5] = {coeffs.p, nullptr, nullptr, nullptr, nullptr};
        CHECK(hb_selftest_pairing(HB_PAIR_SELFTEST_PREPARE, ops, 0, 0, table.p, 1) == HB_OK);
        fill_residues(coeffs.p, 204 * 2);
        CHECK(hb_selftest_pairing(HB_PAIR_SELFTEST_PREPARE, ops, 0, 0, table2.p, 1) == HB_OK);
    }
    // items of K = 2 points: (g, 2 g), (identity, identity), (identity, g)
    Buf k(4), two_g(12), pts(3 * 2 * 12);
    k.p[0] = 2;
    {
        const uint64_t *ops[6] = {k.p, GEN, nullptr, nullptr, nullptr, nullptr};
        CHECK(hb_selftest_g1(HB_G1_SELFTEST_SCALAR_MUL, ops, 0, 0, two_g.p, 1) == HB_OK);
    }
    memcpy(pts.p, GEN, 96);
    memcpy(pts.p + 12, two_g.p, 96);
    memcpy(pts.p + 5 * 12, GEN, 96);
    {
        const uint64_t *ops[5] = {pts.p, table.p, table2.p, nullptr, nullptr};
        Buf gt(3 * 72), gt1(72), verdict(2);                               // three int32 verdicts and the counter: 16 bytes
        CHECK(hb_selftest_pairing(HB_PAIR_SELFTEST_PRODUCT, ops, 2, HB_PAIR_GT, gt.p, 3) == HB_OK);
        CHECK(!is_one(gt.p) && is_one(gt.p + 72) && !is_one(gt.p + 144));
        CHECK(hb_selftest_pairing(HB_PAIR_SELFTEST_PRODUCT, ops, 2, HB_PAIR_VERDICT, verdict.p, 3) == HB_OK);
        const int32_t *v = (const int32_t *)verdict.p;
        CHECK(v[0] == 0 && v[1] == 1 && v[2] == 0 && v[3] == 2);
        // K = 1 over the second column alone equals the third item's value: the first pair there is skipped
        Buf col(12);
        memcpy(col.p, GEN, 96);
        const uint64_t *ops1[5] = {col.p, table2.p, nullptr, nullptr, nullptr};
        CHECK(hb_selftest_pairing(HB_PAIR_SELFTEST_PRODUCT, ops1, 1, HB_PAIR_GT, gt1.p, 1) == HB_OK);
        CHECK(memcmp(gt1.p, gt.p + 144, 72 * 8) == 0);
    }
    printf(fails ? "asan_pairing: %d check(s) FAILED\n" : "asan_pairing ok\n", fails);
    return fails ? 1 : 0;
}

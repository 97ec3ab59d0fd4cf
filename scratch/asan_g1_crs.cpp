// A stand-alone HOST program over hb_selftest_g1_crs for AddressSanitizer and UBSan: the bodies of csrc/hb_crs.hip (tables, quotient, a
// lane's units, the tree steps of the split path over an array in place of LDS) compiled WITH the sanitizers into this program; the rest of
// the library (Fq's and GF(R)'s parameters, hb_g1_table_bytes, hb_selftest_g1) comes from libhbmpc_hip.so as it is.  No GPU is touched.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         scratch/asan_g1_crs.cpp honeybadgermpc_amd/csrc/hb_crs.hip -Lhoneybadgermpc_amd/lib -lhbmpc_hip \
//         -Wl,-rpath,$PWD/honeybadgermpc_amd/lib -o scratch/asan_g1_crs && scratch/asan_g1_crs
//
// Every buffer has exactly the size the self test may touch, so a word too many is a report.  Checks: every split and both window widths give
// the same words; rows beyond a workgroup's last group; U < S; U no multiple of S; the quotient's last lane.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/hbmpc_hip.h"

static const uint64_t GEN[12] = {0xfb3af00adb22c6bbull, 0x6c55e83ff97a1aefull, 0xa14e3a3f171bac58ull, 0xc3688c4f9774b905ull, 0x2695638c4fa9ac0full, 0x17f1d3a73197d794ull,
                                 0xcaa232946c5e7e1ull,  0xd03cc744a2888ae4ull, 0xdb18cb2c04b3edull,   0xfcf5e095d5d00af6ull, 0xa09e30ed741d8ae4ull, 0x8b3f481e3aaa0f1ull};
static const uint64_t RM1[4] = {0xffffffff00000000ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull};

// 16-byte aligned storage of exactly `words` 64-bit words (tables go through 16-byte accesses)
struct Buf {
    uint64_t *p;
    explicit Buf(size_t words) : p((uint64_t *)aligned_alloc(16, ((words ? words : 2) * 8 + 15) / 16 * 16)) { memset(p, 0, (words ? words : 2) * 8); }
    ~Buf() { free(p); }
};

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); fails++; } } while (0)

static uint64_t lcg = 88172645463325252ull;
static uint64_t next() { lcg ^= lcg << 13; lcg ^= lcg >> 7; lcg ^= lcg << 17; return lcg; }

int main() {
    // bases: k g for small k, through the scalar multiplication of the library
    const int N = 3;
    const uint64_t mult[2][N] = {{1, 2, 3}, {5, 7, 11}};
    Buf bases[2] = {Buf(N * 12), Buf(N * 12)};
    for (int f = 0; f < 2; f++) {
        Buf k(N * 4);
        for (int i = 0; i < N; i++) k.p[4 * i] = mult[f][i];
        const uint64_t *ops[6] = {k.p, GEN, nullptr, nullptr, nullptr, nullptr};
        CHECK(hb_selftest_g1(HB_G1_SELFTEST_SCALAR_MUL, ops, HB_G1_POINT_BROADCAST, 0, bases[f].p, N) == HB_OK);
    }
    std::vector<uint64_t> first;
    for (int c : {8, 4}) {
        const size_t tw = (size_t)hb_g1_table_bytes(c) / 8;
        Buf tg(N * tw), th(N * tw);
        const uint64_t *b0[4] = {bases[0].p, nullptr, nullptr, nullptr}, *b1[4] = {bases[1].p, nullptr, nullptr, nullptr};
        CHECK(hb_selftest_g1_crs(HB_G1_CRS_SELFTEST_TABLE, b0, 0, c, tg.p, N) == HB_OK);
        CHECK(hb_selftest_g1_crs(HB_G1_CRS_SELFTEST_TABLE, b1, 0, c, th.p, N) == HB_OK);
        // rows x terms: 5 x 3 over two families (U = 192 at c = 8: no multiple of 128), 5 x 1 over one (U = 32 < 256 at c = 8)
        for (int shape = 0; shape < 2; shape++) {
            const int rows = 5, terms = shape ? 1 : 3;
            Buf a((size_t)rows * terms * 4), b((size_t)rows * terms * 4);
            lcg = 88172645463325252ull + shape;
            for (int i = 0; i < rows * terms * 4; i++) { a.p[i] = next(); b.p[i] = next(); }
            memcpy(a.p, RM1, 32);                                          // R - 1
            memset(a.p + 4, 0xff, 32 * (terms > 1));                       // 2^256 - 1
            memset(b.p, 0, 32);                                            // 0
            std::vector<uint64_t> ref;
            for (int S : {1, 2, 64, 128, 256, 0}) {
                Buf out((size_t)rows * 12);
                const uint64_t *ops[4] = {tg.p, shape ? nullptr : th.p, a.p, shape ? nullptr : b.p};
                CHECK(hb_selftest_g1_crs(HB_G1_CRS_SELFTEST_MSM, ops, c | S << 8, (int64_t)terms | (int64_t)N << 32, out.p, rows) == HB_OK);
                if (ref.empty()) ref.assign(out.p, out.p + rows * 12);
                CHECK(memcmp(ref.data(), out.p, rows * 96) == 0);
            }
            if (!shape) {
                if (first.empty()) first = ref;
                CHECK(first == ref);                                       // both window widths
            }
        }
    }
    // the quotient: B = 3 polynomials of t + 1 = 3 coefficients at n = 5 points; phi = (X - x) q + rem at X = 1 is checked in integers mod 2^64
    {
        const int B = 3, n = 5, nc = 3;
        Buf phi(B * nc * 4), xs(n * 4), out((size_t)B * n * (nc - 1) * 4 + (size_t)B * n * 4);
        for (int i = 0; i < B * nc; i++) phi.p[4 * i] = next() >> 8;
        for (int i = 0; i < n; i++) xs.p[4 * i] = i;
        const uint64_t *ops[4] = {phi.p, xs.p, nullptr, nullptr};
        CHECK(hb_selftest_g1_crs(HB_G1_CRS_SELFTEST_QUOTIENT, ops, nc, n, out.p, B) == HB_OK);
        // x = 0: q = (phi_1, phi_2), rem = phi_0
        for (int b = 0; b < B; b++) {
            const uint64_t *q = out.p + (size_t)(b * n) * (nc - 1) * 4, *rem = out.p + (size_t)B * n * (nc - 1) * 4 + (size_t)(b * n) * 4;
            CHECK(q[0] == phi.p[(b * nc + 1) * 4] && q[4] == phi.p[(b * nc + 2) * 4] && rem[0] == phi.p[b * nc * 4]);
        }
        Buf rem_only((size_t)B * n * 4);                                   // t = 0 writes only rem
        CHECK(hb_selftest_g1_crs(HB_G1_CRS_SELFTEST_QUOTIENT, ops, 1, n, rem_only.p, B) == HB_OK);
    }
    printf(fails ? "asan_g1_crs: %d check(s) FAILED\n" : "asan_g1_crs ok\n", fails);
    return fails ? 1 : 0;
}

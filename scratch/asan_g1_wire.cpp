// A stand-alone HOST program over hb_selftest_g1_wire for AddressSanitizer and UBSan: the bodies of csrc/hb_g1_wire_elem.hpp and
// csrc/hb_g1_wire.hip (the square root, phi, the membership test, decompression, compression) and the load-time derivation of their
// constants compiled WITH the sanitizers into this program; the rest of the library comes from libhbmpc_hip.so as it is.  No GPU is touched.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         scratch/asan_g1_wire.cpp honeybadgermpc_amd/csrc/hb_g1_wire.hip -Lhoneybadgermpc_amd/lib -lhbmpc_hip \
//         -Wl,-rpath,$PWD/honeybadgermpc_amd/lib -o scratch/asan_g1_wire && scratch/asan_g1_wire
//
// Every buffer has exactly the size the self test may touch (the counts are chosen so that each size is a multiple of the 16 bytes
// aligned_alloc wants), so a byte too many is a report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../include/hbmpc_hip.h"

static const uint64_t GEN[12] = {0xfb3af00adb22c6bbull, 0x6c55e83ff97a1aefull, 0xa14e3a3f171bac58ull, 0xc3688c4f9774b905ull, 0x2695638c4fa9ac0full, 0x17f1d3a73197d794ull,
                                 0xcaa232946c5e7e1ull,  0xd03cc744a2888ae4ull, 0xdb18cb2c04b3edull,   0xfcf5e095d5d00af6ull, 0xa09e30ed741d8ae4ull, 0x8b3f481e3aaa0f1ull};
static const uint64_t QM2[6] = {0xb9feffffffffaaa9ull, 0x1eabfffeb153ffffull, 0x6730d2a0f6b0f624ull, 0x64774b84f38512bfull, 0x4b1ba7b6434bacd7ull, 0x1a0111ea397fe69aull};

struct Buf {
    uint8_t *p;
    size_t bytes;
    explicit Buf(size_t n) : p((uint8_t *)aligned_alloc(16, n)), bytes(n) {
        if (n % 16) { printf("a buffer of %zu bytes is no multiple of 16\n", n); exit(2); }
        memset(p, 0, n);
    }
    ~Buf() { free(p); }
    uint64_t *w() const { return (uint64_t *)p; }
};

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); fails++; } } while (0)

static int run(int what, const Buf &in, int flags, Buf &out, int64_t count) {
    const uint64_t *ops[1] = {in.w()};
    return hb_selftest_g1_wire(what, ops, flags, 0, out.w(), count);
}

int main() {
    // points: the generator, the identity, (0, 2) of order 3, the generator again
    Buf pts(4 * 96), flags(4 * 4), enc(4 * 48), back(4 * 48);
    memcpy(pts.p, GEN, 96);
    pts.w()[2 * 12 + 6] = 2;
    memcpy(pts.p + 3 * 96, GEN, 96);
    CHECK(run(HB_G1_WIRE_SELFTEST_SUBGROUP, pts, 0, flags, 4) == HB_OK);
    const int32_t *f = (const int32_t *)flags.p;
    CHECK(f[0] == 1 && f[1] == 1 && f[2] == 0 && f[3] == 1);
    CHECK(run(HB_G1_WIRE_SELFTEST_COMPRESS, pts, 0, enc, 4) == HB_OK);
    CHECK(enc.p[0] == 0x97 && enc.p[47] == 0xbb);                              // 0x80 | 0x17: the generator's y is the smaller root
    CHECK(enc.p[48] == 0xc0 && enc.p[96] == 0x80 && enc.p[96 + 47] == 0);
    for (int i = 1; i < 48; i++) CHECK(enc.p[48 + i] == 0);
    // decompression of three encodings: out = 3 points, 3 statuses and the counter: 304 bytes
    Buf three(3 * 48), out(3 * 96 + 3 * 4 + 4);
    memcpy(three.p, enc.p, 3 * 48);
    CHECK(run(HB_G1_WIRE_SELFTEST_DECOMPRESS, three, 0, out, 3) == HB_OK);
    const int32_t *st = (const int32_t *)(out.p + 3 * 96);
    CHECK(st[0] == HB_G1_WIRE_OK && st[1] == HB_G1_WIRE_OK && st[2] == HB_G1_WIRE_OK && st[3] == 0);
    CHECK(memcmp(out.p, pts.p, 3 * 96) == 0);
    CHECK(run(HB_G1_WIRE_SELFTEST_DECOMPRESS, three, 1, out, 3) == HB_OK);
    CHECK(st[0] == HB_G1_WIRE_OK && st[1] == HB_G1_WIRE_OK && st[2] == HB_G1_WIRE_NOT_IN_SUBGROUP && st[3] == 1);
    CHECK(memcmp(out.p, pts.p, 2 * 96) == 0);
    for (int i = 0; i < 96; i++) CHECK(out.p[2 * 96 + i] == 0);
    // the other root, the flags, x not below Q
    three.p[0] |= 0x20;
    three.p[48] = 0x40;
    memset(three.p + 96, 0xff, 48);
    three.p[96] = 0x9f;
    CHECK(run(HB_G1_WIRE_SELFTEST_DECOMPRESS, three, 0, out, 3) == HB_OK);
    CHECK(st[0] == HB_G1_WIRE_OK && st[1] == HB_G1_WIRE_NOT_COMPRESSED && st[2] == HB_G1_WIRE_X_NOT_BELOW_Q && st[3] == 2);
    CHECK(memcmp(out.p, GEN, 48) == 0 && memcmp(out.p + 48, GEN + 6, 48) != 0);
    {
        Buf neg(96), e1(48);                                                   // and back: the sign flag is set
        memcpy(neg.p, out.p, 96);
        CHECK(run(HB_G1_WIRE_SELFTEST_COMPRESS, neg, 0, e1, 1) == HB_OK && memcmp(e1.p, three.p, 48) == 0);
    }
    three.p[48] = 0xe0;
    CHECK(run(HB_G1_WIRE_SELFTEST_DECOMPRESS, three, 0, out, 3) == HB_OK && st[1] == HB_G1_WIRE_BAD_IDENTITY);
    // the bare pieces: sqrt(4) = +-2, sqrt(Q - 1) does not exist (Q = 3 mod 4), sqrt(0) = 0; phi has order 3
    Buf a(4 * 48), roots(4 * 48 + 4 * 4);
    a.w()[0] = 4;
    memcpy(a.p + 48, QM2, 48);
    a.w()[6] += 1;
    a.w()[18] = 9;
    CHECK(run(HB_G1_WIRE_SELFTEST_SQRT, a, 0, roots, 4) == HB_OK);
    const int32_t *sq = (const int32_t *)(roots.p + 4 * 48);
    CHECK(sq[0] == 1 && sq[1] == 0 && sq[2] == 1 && sq[3] == 1);
    CHECK(roots.w()[0] == 2 || roots.w()[0] == QM2[0]);
    CHECK(roots.w()[18] == 3 || roots.w()[18] == QM2[0] - 1);
    for (int i = 6; i < 18; i++) CHECK(roots.w()[i] == 0);
    Buf p1(4 * 96), p2(4 * 96), p3(4 * 96);
    CHECK(run(HB_G1_WIRE_SELFTEST_PHI, pts, 0, p1, 4) == HB_OK && run(HB_G1_WIRE_SELFTEST_PHI, p1, 0, p2, 4) == HB_OK && run(HB_G1_WIRE_SELFTEST_PHI, p2, 0, p3, 4) == HB_OK);
    CHECK(memcmp(p3.p, pts.p, 4 * 96) == 0 && memcmp(p1.p, pts.p, 48) != 0 && memcmp(p1.p + 48, pts.p + 48, 48) == 0);
    // refusals: a misaligned operand, an unknown operation
    {
        const uint64_t *ops[1] = {(const uint64_t *)(pts.p + 8)};
        CHECK(hb_selftest_g1_wire(HB_G1_WIRE_SELFTEST_SUBGROUP, ops, 0, 0, flags.w(), 1) == HB_ERR_BAD_ARG);
        CHECK(run(99, pts, 0, flags, 1) == HB_ERR_BAD_ARG);
    }
    printf(fails ? "asan_g1_wire: %d check(s) FAILED\n" : "asan_g1_wire ok\n", fails);
    return fails ? 1 : 0;
}

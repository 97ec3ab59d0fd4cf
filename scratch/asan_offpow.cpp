// A stand-alone HOST program over hb_selftest_off_powers for AddressSanitizer and UBSan: the two rows of csrc/hb_offpow.hip (hb_rows.hpp:
// host_rows runs what k_rows runs, index arithmetic included) compiled WITH the sanitizers into this program; the rest of the library
// comes from libhbmpc_hip.so as it is.  No GPU is touched.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         scratch/asan_offpow.cpp honeybadgermpc_amd/csrc/hb_offpow.hip \
//         -Lhoneybadgermpc_amd/lib -lhbmpc_hip -Wl,-rpath,$PWD/honeybadgermpc_amd/lib -o scratch/asan_offpow && scratch/asan_offpow
//
// Every level of k = 2, 3, 5, 8, 9 at count = 1, 3, 65 in both layouts and both widths.  The powers array, the masks and the outputs are
// heap buffers of exactly count k and count w elements, so a cell addressed one element past an array is a report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

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
};

static const uint64_t BLS[4] = {0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull};
static const uint64_t P64[1] = {0xffffffffffffffc5ull};

static void levels(const uint64_t *p, int64_t count, int k, bool item_major) {
    const int64_t is = item_major ? k : 1, ps = item_major ? 1 : count;
    Elems powers((size_t)count * k);
    for (int m = 1; m < k;) {
        const int w = m < k - m ? m : k - m;
        Elems r2t((size_t)count * w), rt((size_t)count * w), opened((size_t)count * w), out((size_t)count * w);
        CHECK(hb_selftest_off_powers(p, NL, HB_OFF_POWERS_SELFTEST_MASK, powers.p, is, ps, nullptr, r2t.p, m, w, out.p, count) == HB_OK);
        CHECK(hb_selftest_off_powers(p, NL, HB_OFF_POWERS_SELFTEST_FINISH, powers.p, is, ps, opened.p, rt.p, m, w, nullptr, count) == HB_OK);
        // refused before anything is addressed
        CHECK(hb_selftest_off_powers(p, NL, HB_OFF_POWERS_SELFTEST_MASK, powers.p, is, ps, nullptr, r2t.p, m, m + 1, out.p, count) == HB_ERR_BAD_ARG);
        CHECK(hb_selftest_off_powers(p, NL, HB_OFF_POWERS_SELFTEST_MASK, powers.p, is, ps, nullptr, r2t.p, m, w, powers.p, count) == HB_ERR_BAD_ARG);
        CHECK(hb_selftest_off_powers(p, NL, HB_OFF_POWERS_SELFTEST_FINISH, powers.p, is, ps, powers.p + (size_t)m * ps * NL, rt.p, m, w, nullptr, count) == HB_ERR_BAD_ARG);
        m += w;
    }
}

int main() {
    for (int width = 0; width < 2; width++) {
        NL = width ? 1 : 4;
        const uint64_t *p = width ? P64 : BLS;
        for (int64_t count : {1, 3, 65})
            for (int k : {2, 3, 5, 8, 9})
                for (int item_major = 0; item_major < 2; item_major++) levels(p, count, k, item_major != 0);
        CHECK(hb_selftest_off_powers(p, NL, HB_OFF_POWERS_SELFTEST_MASK, nullptr, 4, 1, nullptr, nullptr, 2, 2, nullptr, 0) == HB_OK);
    }
    printf(fails ? "asan_offpow: %d check(s) FAILED\n" : "asan_offpow ok\n", fails);
    return fails ? 1 : 0;
}

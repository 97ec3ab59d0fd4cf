// A stand-alone HOST program over hb_selftest_off_share_bits for AddressSanitizer and UBSan: the two rows of csrc/hb_offsb.hip (hb_rows.hpp:
// host_rows runs what k_rows runs, index arithmetic included) compiled WITH the sanitizers into this program; the rest of the library
// comes from libhbmpc_hip.so as it is.  No GPU is touched.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         scratch/asan_offsb.cpp honeybadgermpc_amd/csrc/hb_offsb.hip \
//         -Lhoneybadgermpc_amd/lib -lhbmpc_hip -Wl,-rpath,$PWD/honeybadgermpc_amd/lib -o scratch/asan_offsb && scratch/asan_offsb
//
// Leaves at count = 1, 3, 65 and the finish over 1, 3, 65 candidates with index lists that are empty, single, whole, reversed, repeated and
// partly out of range, in both widths.  The planes, the index and the outputs are heap buffers of exactly L count, k and L k elements, so
// a cell addressed one element past an array -- or through an index that is out of range -- is a report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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
    size_t n;
    explicit Elems(size_t elems) : p((uint64_t *)malloc(elems * NL * 8 + 1)), n(elems) {          // + 1: malloc(0) may return null
        for (size_t i = 0; i < elems * NL; i++) p[i] = (i % NL == (size_t)NL - 1) ? next() >> 4 : next();
    }
    bool zero(size_t e) const {
        for (int l = 0; l < NL; l++) if (p[e * NL + l]) return false;
        return true;
    }
    ~Elems() { free(p); }
};

static const uint64_t BLS[4] = {0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull};
static const uint64_t P64[1] = {0xffffffffffffffc5ull};

static void leaves(const uint64_t *p, int L, int64_t count) {
    Elems bits((size_t)L * count), g((size_t)L * count), q((size_t)L * count);
    uint64_t bound[4] = {next(), next(), next(), next() >> 2};
    if (NL == 1) bound[0] = next();
    CHECK(hb_selftest_off_share_bits(p, NL, HB_OFF_SB_SELFTEST_LEAVES, bits.p, L, nullptr, 0, nullptr, g.p, q.p, count) == HB_OK);
    CHECK(hb_selftest_off_share_bits(p, NL, HB_OFF_SB_SELFTEST_LEAVES, bits.p, L, bound, 0, nullptr, g.p, q.p, count) == HB_OK);
    // refused before anything is addressed
    CHECK(hb_selftest_off_share_bits(p, NL, HB_OFF_SB_SELFTEST_LEAVES, bits.p, L - 1, nullptr, 0, nullptr, g.p, q.p, count) == HB_ERR_BAD_ARG);
    CHECK(hb_selftest_off_share_bits(p, NL, HB_OFF_SB_SELFTEST_LEAVES, bits.p, L, nullptr, 0, nullptr, g.p, g.p, count) == HB_ERR_BAD_ARG);
    CHECK(hb_selftest_off_share_bits(p, NL, HB_OFF_SB_SELFTEST_LEAVES, bits.p, L, nullptr, 0, nullptr, bits.p, q.p, count) == HB_ERR_BAD_ARG);
    if (NL == 4) {
        bound[3] = 1ull << 63;
        CHECK(hb_selftest_off_share_bits(p, NL, HB_OFF_SB_SELFTEST_LEAVES, bits.p, L, bound, 0, nullptr, g.p, q.p, count) == HB_ERR_BAD_ARG);
    }
}

static void finish(const uint64_t *p, int L, int64_t candidates, const std::vector<int64_t> &index) {
    const int64_t k = (int64_t)index.size();
    Elems bits((size_t)L * candidates), r((size_t)k), r_bits((size_t)L * k);
    int64_t *idx = (int64_t *)malloc(k * 8 + 1);                            // exactly k entries
    for (int64_t j = 0; j < k; j++) idx[j] = index[j];
    CHECK(hb_selftest_off_share_bits(p, NL, HB_OFF_SB_SELFTEST_FINISH, bits.p, L, nullptr, candidates, idx, r.p, r_bits.p, k) == HB_OK);
    for (int64_t j = 0; j < k; j++) {
        const bool inside = index[j] >= 0 && index[j] < candidates;
        bool same = true;                                                  // the gathered planes, or zeros
        for (int q = 0; q < L; q++)
            for (int l = 0; l < NL; l++)
                same = same && r_bits.p[((size_t)q * k + j) * NL + l] == (inside ? bits.p[((size_t)q * candidates + index[j]) * NL + l] : 0);
        CHECK(same);
        if (!inside) CHECK(r.zero(j));
    }
    if (k) {
        CHECK(hb_selftest_off_share_bits(p, NL, HB_OFF_SB_SELFTEST_FINISH, bits.p, L + 1, nullptr, candidates, idx, r.p, r_bits.p, k) == HB_ERR_BAD_ARG);
        CHECK(hb_selftest_off_share_bits(p, NL, HB_OFF_SB_SELFTEST_FINISH, bits.p, L, nullptr, candidates, idx, r_bits.p, r_bits.p, k) == HB_ERR_BAD_ARG);
        if (candidates)                                                    // (planes of no candidate have no extent to lie over)
            CHECK(hb_selftest_off_share_bits(p, NL, HB_OFF_SB_SELFTEST_FINISH, bits.p, L, nullptr, candidates, idx, r.p, bits.p, k) == HB_ERR_BAD_ARG);
        CHECK(hb_selftest_off_share_bits(p, NL, HB_OFF_SB_SELFTEST_FINISH, bits.p, L, nullptr, -1, idx, r.p, r_bits.p, k) == HB_ERR_BAD_ARG);
    }
    free(idx);
}

int main() {
    for (int width = 0; width < 2; width++) {
        NL = width ? 1 : 4;
        const uint64_t *p = width ? P64 : BLS;
        const int L = width ? 64 : 255;
        for (int64_t count : {1, 3, 65}) {
            leaves(p, L, count);
            std::vector<int64_t> all, reversed;
            for (int64_t c = 0; c < count; c++) { all.push_back(c); reversed.push_back(count - 1 - c); }
            finish(p, L, count, {});
            finish(p, L, count, {count - 1});
            finish(p, L, count, all);
            finish(p, L, count, reversed);
            finish(p, L, count, {0, 0, count - 1, 0, count / 2, count / 2});
            finish(p, L, count, {0, -1, count, count - 1, (int64_t)1 << 40, INT64_MIN, INT64_MAX, count + 1});
        }
        finish(p, L, 0, {0, 1, -1});                                       // no candidates: every slot is zeros, the planes are not read
        CHECK(hb_selftest_off_share_bits(p, NL, HB_OFF_SB_SELFTEST_LEAVES, nullptr, L, nullptr, 0, nullptr, nullptr, nullptr, 0) == HB_OK);
        CHECK(hb_selftest_off_share_bits(p, NL, HB_OFF_SB_SELFTEST_FINISH, nullptr, L, nullptr, 0, nullptr, nullptr, nullptr, 0) == HB_OK);
    }
    printf(fails ? "asan_offsb: %d check(s) FAILED\n" : "asan_offsb ok\n", fails);
    return fails ? 1 : 0;
}

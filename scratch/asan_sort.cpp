// A stand-alone HOST program over hb_selftest_sort for AddressSanitizer and UBSan: the rows of csrc/hb_sort.hip (hb_rows.hpp:
// host_rows runs what k_rows runs) compiled WITH the sanitizers into this program; the rest of the library comes from
// libhbmpc_hip.so as it is.  No GPU is touched.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         scratch/asan_sort.cpp honeybadgermpc_amd/csrc/hb_sort.hip \
//         -Lhoneybadgermpc_amd/lib -lhbmpc_hip -Wl,-rpath,$PWD/honeybadgermpc_amd/lib -o scratch/asan_sort && scratch/asan_sort
//
// Every layer of the merge exchange over n = 13, 16 and 5 rows, batch 3, width 3, both element widths; the self test runs the step
// functions of the entry points (hb_rows.hpp), so every layer also gets a swap mask with out over tq's last element and one with
// width 0: both refused.  Every operand and output is a
// heap buffer of exactly the documented size, so a row that reads or writes one element past an array is a report; the last
// comparator of the last array ends at the table's last row in the layers that reach row n - 1.
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
// exactly `elems` elements of canonical residues (the top limb stays below the modulus'); no element at all where elems == 0
struct Elems {
    uint64_t *p;
    explicit Elems(size_t elems) : p((uint64_t *)malloc(elems * NL * 8 + (elems ? 0 : 1))) {
        for (size_t i = 0; i < elems * NL; i++) p[i] = (i % NL == (size_t)NL - 1) ? next() >> 4 : next();
    }
    ~Elems() { free(p); }
    operator const uint64_t *() const { return p; }
};

static const uint64_t BLS[4] = {0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull};
static const uint64_t P64[1] = {0xffffffffffffffc5ull};

static void layer(const uint64_t *p, int64_t n, int64_t batch, int64_t width, int a, int64_t r, int64_t d, int64_t cnt, int64_t k, int64_t kappa) {
    const int64_t prm[9] = {n, batch, width, a, r, d, cnt, k, kappa}, slots = batch * cnt, plane = batch * n;
    Elems table(width * plane), bits((k + kappa) * slots), c(slots), r1(slots), carry(slots), tp(width * slots), tq(width * slots), tpq(width * slots);
    Elems opened(2 * width * slots), inv(1);
    {
        Elems masked(slots), o1(slots);
        const uint64_t *ops[2] = {table, bits};
        uint64_t *outs[2] = {masked.p, o1.p};
        CHECK(hb_selftest_sort(p, NL, HB_SORT_SELFTEST_CMP_MASK, ops, prm, outs) == HB_OK);
    }
    {
        Elems out(2 * width * slots);
        const uint64_t *ops[7] = {table, c, r1, carry, tp, tq, inv};
        uint64_t *outs[1] = {out.p};
        CHECK(hb_selftest_sort(p, NL, HB_SORT_SELFTEST_SWAP_MASK, ops, prm, outs) == HB_OK);
    }
    {
        const uint64_t *ops[4] = {opened, tp, tq, tpq};
        uint64_t *outs[1] = {table.p};
        CHECK(hb_selftest_sort(p, NL, HB_SORT_SELFTEST_SWAP_FINISH, ops, prm, outs) == HB_OK);
    }
    if (slots > 0) {                                                        // refused by the step function: out over the last element of tq; no width
        Elems out(2 * width * slots);
        const uint64_t *ops[7] = {table, c, r1, carry, tp, tq, inv};
        uint64_t *outs[1] = {tq.p + (size_t)(width * slots - 1) * NL};
        const int64_t flat[9] = {n, batch, 0, a, r, d, cnt, k, kappa};
        CHECK(hb_selftest_sort(p, NL, HB_SORT_SELFTEST_SWAP_MASK, ops, prm, outs) == HB_ERR_BAD_ARG);
        outs[0] = out.p;
        CHECK(hb_selftest_sort(p, NL, HB_SORT_SELFTEST_SWAP_MASK, ops, flat, outs) == HB_ERR_BAD_ARG);
    }
}

// the layers of Algorithm M with their closed counts
static void network(const uint64_t *p, int64_t n, int64_t batch, int64_t width, int64_t k, int64_t kappa) {
    int t = 0;
    while (((int64_t)1 << t) < n) t++;
    for (int a = t - 1; a >= 0; a--) {
        const int64_t pp = (int64_t)1 << a;
        for (int j = t; j > a; j--) {                                       // j == t: the layer (p, 0, p); then q = 2^j
            const int64_t r = j == t ? 0 : pp, d = j == t ? pp : ((int64_t)1 << j) - pp, m = n - d > 0 ? n - d : 0;
            const int64_t full = m / (2 * pp), rem = m % (2 * pp);
            const int64_t cnt = full * pp + (r == 0 ? (rem < pp ? rem : pp) : (rem > pp ? rem - pp : 0));
            if (d < n) layer(p, n, batch, width, a, r, d, cnt, k, kappa);
        }
    }
}

int main() {
    for (int wide = 1; wide >= 0; wide--) {
        NL = wide ? 4 : 1;
        const uint64_t *p = wide ? BLS : P64;
        network(p, 13, 3, 3, 8, 8);
        network(p, 16, 1, 1, 8, 8);
        network(p, 5, 2, 2, wide ? 64 : 16, wide ? 32 : 16);
        layer(p, 2, 1, 1, 0, 0, 1, 1, 8, 8);
        layer(p, 2, 1, 3, 0, 0, 1, 0, 8, 8);
    }
    printf(fails ? "asan_sort: %d check(s) FAILED\n" : "asan_sort ok\n", fails);
    return fails ? 1 : 0;
}

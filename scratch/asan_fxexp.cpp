// A stand-alone HOST program over hb_selftest_fxexp for AddressSanitizer and UBSan: the rows and step functions of csrc/hb_fxexp.hip
// (hb_rows.hpp: host_rows runs what k_rows runs) compiled WITH the sanitizers into this program; the rest of the library comes from
// libhbmpc_hip.so as it is.  No GPU is touched.
//
//   C=honeybadgermpc_amd/csrc; hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-omit-frame-pointer scratch/asan_fxexp.cpp $C/hb_fxexp.hip -Lhoneybadgermpc_amd/lib -lhbmpc_hip \
//         -Wl,-rpath,$PWD/honeybadgermpc_amd/lib -o scratch/asan_fxexp && scratch/asan_fxexp
//
// The fused last level at the merges (1,1), (2,1), (2,2), (4,3), (4,4) and a group of one bit, alone and three groups a launch, with
// tables of arbitrary residues, of short constants and with zero entries; products to truncation masks for 1 to 5 products; the tree
// step for 1 to 5 rows with and without a carried factor, at count = 3 and both widths; one call each with an output over an input's
// last row and with a parameter past its bound: both refused.  Every operand and output is a heap buffer of exactly the documented
// size, so a row that reads or writes one element past an array is a report.
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

struct Field { int nl; uint64_t p[4]; };

// `elems` canonical residues on the heap, exactly sized: the top limb stays below the modulus' so every value is below p
static uint64_t *residues(const Field &F, int64_t elems) {
    uint64_t *b = (uint64_t *)malloc(sizeof(uint64_t) * F.nl * (elems ? elems : 1));
    for (int64_t e = 0; e < elems; e++)
        for (int l = 0; l < F.nl; l++) b[e * F.nl + l] = l == F.nl - 1 ? next() % F.p[l] : next();
    return b;
}

static int call(const Field &F, int what, std::vector<const uint64_t *> ops, std::vector<int64_t> prm, uint64_t *o0, uint64_t *o1, int64_t count) {
    ops.resize(8, nullptr);
    prm.resize(51, 0);
    uint64_t *outs[2] = {o0, o1};
    return hb_selftest_fxexp(F.p, F.nl, what, ops.data(), prm.data(), outs, count);
}

int main() {
    const Field fields[2] = {{4, {0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull}}, {1, {0xffffffffffffffc5ull, 0, 0, 0}}};
    const int64_t count = 3;
    const int merges[6][2] = {{1, 1}, {2, 1}, {2, 2}, {4, 3}, {4, 4}, {1, 0}};
    for (const Field &F : fields) {
        for (int first = 0; first < 6; first++)
            for (int n_groups : {1, 3}) {
                std::vector<int64_t> prm = {n_groups, 2, n_groups + 1};
                int64_t open_rows = 0, prod_rows = 0, entries = 0;
                for (int g = 0; g < n_groups; g++) {
                    const int wl = merges[(first + g) % 6][0], wh = merges[(first + g) % 6][1];
                    if (wh == 0) prm.insert(prm.end(), {1, 0, 1, 0, entries, g});      // plane 1 of two
                    else {
                        prm.insert(prm.end(), {wl, wh, open_rows, prod_rows, entries, g});
                        open_rows += (1 << wl) + (1 << wh);
                        prod_rows += 1 << (wl + wh);
                    }
                    entries += 1 << (wl + wh);
                }
                uint64_t *bits = residues(F, 2 * count), *opened = residues(F, open_rows * count), *ta = residues(F, open_rows * count), *tab = residues(F, prod_rows * count);
                uint64_t *tables = residues(F, entries), *na = residues(F, 2 * count), *nb = residues(F, 2 * count);
                uint64_t *masked = residues(F, 4 * count), *kept = residues(F, (n_groups + 1) * count);
                for (int64_t e = 0; e < entries; e++) {                            // a third of the entries 0, a third short constants
                    if (e % 3 == 0) memset(tables + e * F.nl, 0, sizeof(uint64_t) * F.nl);
                    if (e % 3 == 1 && F.nl == 4) tables[e * 4 + 2] = tables[e * 4 + 3] = 0, tables[e * 4 + 1] &= 7;
                }
                const uint64_t *o = open_rows ? opened : nullptr, *a = open_rows ? ta : nullptr, *ab = open_rows ? tab : nullptr;
                CHECK(call(F, HB_FXEXP_SELFTEST_FINISH_LOOKUP_MASK, {bits, o, a, ab, tables, na, nb}, prm, masked, kept, count) == HB_OK);
                if (open_rows) {
                    CHECK(call(F, HB_FXEXP_SELFTEST_FINISH_LOOKUP_MASK, {bits, o, a, ab, tables, na, nb}, prm, masked, opened + (open_rows - 1) * count * F.nl, count) ==
                          HB_ERR_BAD_ARG);
                    std::vector<int64_t> bad = prm;
                    bad[2] = 0;                                                    // no room for a slot
                    CHECK(call(F, HB_FXEXP_SELFTEST_FINISH_LOOKUP_MASK, {bits, o, a, ab, tables, na, nb}, bad, masked, kept, count) == HB_ERR_BAD_ARG);
                }
                for (uint64_t *q : {bits, opened, ta, tab, tables, na, nb, masked, kept}) free(q);
            }
        const int width = F.nl == 4 ? 134 : 38, kappa = F.nl == 4 ? 32 : 8, m = F.nl == 4 ? 66 : 18;
        for (int products : {1, 2, 3, 4, 5}) {
            uint64_t *opened = residues(F, 2 * products * count), *ta = residues(F, products * count), *tb = residues(F, products * count), *tab = residues(F, products * count);
            uint64_t *bits = residues(F, (int64_t)products * (width + kappa) * count), *masked = residues(F, products * count), *s = residues(F, products * count);
            CHECK(call(F, HB_FXEXP_SELFTEST_PRODUCTS_TRUNC, {opened, ta, tb, tab, bits}, {products, width, m, kappa}, masked, s, count) == HB_OK);
            CHECK(call(F, HB_FXEXP_SELFTEST_PRODUCTS_TRUNC, {opened, ta, tb, tab, bits}, {products, width, m, kappa}, masked, tab + (products - 1) * count * F.nl, count) ==
                  HB_ERR_BAD_ARG);
            CHECK(call(F, HB_FXEXP_SELFTEST_PRODUCTS_TRUNC, {opened, ta, tb, tab, bits}, {products, width, width, kappa}, masked, s, count) == HB_ERR_BAD_ARG);
            for (uint64_t *q : {opened, ta, tb, tab, bits, masked, s}) free(q);
        }
        uint64_t *inv = residues(F, 1);
        for (int rows : {1, 2, 3, 4, 5})
            for (int carried : {0, 1}) {
                const int values = rows + carried, pairs = values / 2, odd = values & 1;
                uint64_t *opened = residues(F, rows * count), *s = residues(F, rows * count), *carry = residues(F, count), *ta = residues(F, pairs * count), *tb = residues(F, pairs * count);
                uint64_t *masked = residues(F, 2 * pairs * count), *kept = residues(F, count);
                const uint64_t *c = carried ? carry : nullptr, *a = pairs ? ta : nullptr, *b = pairs ? tb : nullptr;
                CHECK(call(F, HB_FXEXP_SELFTEST_TREE_STEP, {opened, s, inv, c, a, b}, {rows, m}, pairs ? masked : nullptr, odd ? kept : nullptr, count) == HB_OK);
                if (odd) CHECK(call(F, HB_FXEXP_SELFTEST_TREE_STEP, {opened, s, inv, c, a, b}, {rows, m}, pairs ? masked : nullptr, s + (rows - 1) * count * F.nl, count) == HB_ERR_BAD_ARG);
                CHECK(call(F, HB_FXEXP_SELFTEST_TREE_STEP, {opened, s, inv, c, a, b}, {129, m}, pairs ? masked : nullptr, odd ? kept : nullptr, count) == HB_ERR_BAD_ARG);
                for (uint64_t *q : {opened, s, carry, ta, tb, masked, kept}) free(q);
            }
        free(inv);
    }
    if (fails) printf("asan_fxexp: %d check(s) FAILED\n", fails);
    else printf("asan_fxexp: every step ran and every refusal held\n");
    return fails ? 1 : 0;
}

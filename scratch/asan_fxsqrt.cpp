// A stand-alone HOST program over hb_selftest_fxsqrt for AddressSanitizer and UBSan: the rows and step functions of csrc/hb_fxsqrt.hip
// (hb_rows.hpp: host_rows runs what k_rows runs) compiled WITH the sanitizers into this program; the rest of the library comes from
// libhbmpc_hip.so as it is.  No GPU is touched.
//
//   C=honeybadgermpc_amd/csrc; hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-omit-frame-pointer scratch/asan_fxsqrt.cpp $C/hb_fxsqrt.hip -Lhoneybadgermpc_amd/lib -lhbmpc_hip \
//         -Wl,-rpath,$PWD/honeybadgermpc_amd/lib -o scratch/asan_fxsqrt && scratch/asan_fxsqrt
//
// The scale step at 1, 2, 7, 8, 15, 22 and 63 planes with one and two sets of weights (the last group of the lazy sum short, full and
// absent), the first approximation, and the truncation step in every mode with one and two products, at count = 3 and both widths;
// one call each with an output over an input's last row and with a parameter past its bound: both refused.  Every operand and output
// is a heap buffer of exactly the documented size, so a row that reads or writes one element past an array is a report.
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
    prm.resize(4, 0);
    uint64_t *outs[2] = {o0, o1};
    return hb_selftest_fxsqrt(F.p, F.nl, what, ops.data(), prm.data(), outs, count);
}

int main() {
    const Field fields[2] = {{4, {0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull}}, {1, {0xffffffffffffffc5ull, 0, 0, 0}}};
    const int64_t count = 3;
    for (const Field &F : fields) {
        const int m = F.nl == 4 ? 140 : 61;
        for (int n : {1, 2, 7, 8, 15, 22, 63})
            for (int sets : {1, 2}) {
                uint64_t *x = residues(F, count), *y = residues(F, n * count), *w = residues(F, sets * n), *ta = residues(F, count), *tb = residues(F, count);
                uint64_t *masked = residues(F, 2 * count), *kept = residues(F, (1 + sets) * count);
                CHECK(call(F, HB_FXSQRT_SELFTEST_NORM_MASK, {x, y, w, ta, tb}, {n, sets}, masked, kept, count) == HB_OK);
                if (n == 7) {
                    CHECK(call(F, HB_FXSQRT_SELFTEST_NORM_MASK, {x, y, w, ta, tb}, {n, sets}, y + (n - 1) * count * F.nl - F.nl, kept, count) == HB_ERR_BAD_ARG);
                    CHECK(call(F, HB_FXSQRT_SELFTEST_NORM_MASK, {x, y, w, ta, tb}, {n, 3}, masked, kept, count) == HB_ERR_BAD_ARG);
                }
                for (uint64_t *b : {x, y, w, ta, tb, masked, kept}) free(b);
            }
        {
            uint64_t *opened = residues(F, 2 * count), *ta = residues(F, count), *tb = residues(F, count), *tab = residues(F, count), *a = residues(F, 1), *b = residues(F, 1);
            uint64_t *na = residues(F, count), *nb = residues(F, count), *masked = residues(F, 2 * count), *h = residues(F, count);
            CHECK(call(F, HB_FXSQRT_SELFTEST_FIRST, {opened, ta, tb, tab, a, b, na, nb}, {}, masked, h, count) == HB_OK);
            CHECK(call(F, HB_FXSQRT_SELFTEST_FIRST, {opened, ta, tb, tab, a, b, na, nb}, {}, masked, nb, count) == HB_ERR_BAD_ARG);
            for (uint64_t *q : {opened, ta, tb, tab, a, b, na, nb, masked, h}) free(q);
        }
        uint64_t *inv = residues(F, 1), *cst = residues(F, 1);
        for (int rows : {1, 2}) {                                                  // GH: one row reads the kept h, two rows read none
            uint64_t *opened = residues(F, rows * count), *s = residues(F, rows * count), *h = residues(F, count), *ta = residues(F, count), *tb = residues(F, count);
            uint64_t *masked = residues(F, 2 * count), *kept = residues(F, 2 * count);
            CHECK(call(F, HB_FXSQRT_SELFTEST_TRUNC_STEP, {opened, s, inv, nullptr, rows == 1 ? h : nullptr, ta, tb}, {HB_FXSQRT_GH, rows, 3, m}, masked, kept, count) == HB_OK);
            CHECK(call(F, HB_FXSQRT_SELFTEST_TRUNC_STEP, {opened, s, inv, nullptr, h, ta, tb}, {HB_FXSQRT_GH, rows, 3, m}, masked, s + (rows - 1) * count * F.nl, count) ==
                  HB_ERR_BAD_ARG);
            CHECK(call(F, HB_FXSQRT_SELFTEST_TRUNC_STEP, {opened, s, inv, nullptr, h, ta, tb}, {HB_FXSQRT_GH, 3, 3, m}, masked, kept, count) == HB_ERR_BAD_ARG);
            for (uint64_t *q : {opened, s, h, ta, tb, masked, kept}) free(q);
        }
        for (int which : {1, 2, 3}) {
            const int products = which == 3 ? 2 : 1;
            uint64_t *opened = residues(F, count), *s = residues(F, count), *gh = residues(F, 2 * count), *ta = residues(F, products * count), *tb = residues(F, products * count);
            uint64_t *masked = residues(F, 2 * products * count);
            CHECK(call(F, HB_FXSQRT_SELFTEST_TRUNC_STEP, {opened, s, inv, cst, gh, ta, tb}, {HB_FXSQRT_R, 1, which, m}, masked, nullptr, count) == HB_OK);
            CHECK(call(F, HB_FXSQRT_SELFTEST_TRUNC_STEP, {opened, s, inv, cst, gh, ta, tb}, {HB_FXSQRT_R, 1, which, m}, gh + count * F.nl, nullptr, count) == HB_ERR_BAD_ARG);
            for (uint64_t *q : {opened, s, gh, ta, tb, masked}) free(q);
            uint64_t *o2 = residues(F, products * count), *s2 = residues(F, products * count), *tw = residues(F, products * count);
            ta = residues(F, products * count), tb = residues(F, products * count), masked = residues(F, 2 * products * count);
            CHECK(call(F, HB_FXSQRT_SELFTEST_TRUNC_STEP, {o2, s2, inv, nullptr, tw, ta, tb}, {HB_FXSQRT_OUT, products, which, m}, masked, nullptr, count) == HB_OK);
            CHECK(call(F, HB_FXSQRT_SELFTEST_TRUNC_STEP, {o2, s2, inv, nullptr, tw, ta, tb}, {HB_FXSQRT_OUT, products, which, 0}, masked, nullptr, count) == HB_ERR_BAD_ARG);
            for (uint64_t *q : {o2, s2, tw, ta, tb, masked}) free(q);
        }
        free(inv), free(cst);
    }
    if (fails) printf("asan_fxsqrt: %d check(s) FAILED\n", fails);
    else printf("asan_fxsqrt: every step ran and every refusal held\n");
    return fails ? 1 : 0;
}

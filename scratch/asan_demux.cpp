// A stand-alone HOST program over hb_selftest_demux for AddressSanitizer and UBSan: the three rows of csrc/hb_demux.hip (hb_rows.hpp:
// host_rows runs what k_rows runs, the wiring and the index arithmetic included) compiled WITH the sanitizers into this program; the
// rest of the library comes from libhbmpc_hip.so as it is.  No GPU is touched.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         scratch/asan_demux.cpp honeybadgermpc_amd/csrc/hb_demux.hip \
//         -Lhoneybadgermpc_amd/lib -lhbmpc_hip -Wl,-rpath,$PWD/honeybadgermpc_amd/lib -o scratch/asan_demux && scratch/asan_demux
//
// The leaves, and the mask and the finish of every level of m = 2 .. 12, at count = 1, 3 and 65 in both widths.  The wiring is restated
// here (groups paired from the least significant, an odd last one carried) to size the buffers: bits, groups, ta, tab, the opened
// array and the outputs are heap buffers of exactly m, sum of products, sum (2^wl + 2^wh), sum 2^(wl + wh) rows of count elements,
// so a cell addressed one element past an array is a report.  The self test runs the step functions of the entry points
// (hb_rows.hpp): every level also gets a finish with groups over tab's last row, and every m a level it does not have: both refused.
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
    explicit Elems(size_t elems) : p((uint64_t *)malloc(elems * NL * 8 + 1)) {                     // + 1: malloc(0) may return null
        for (size_t i = 0; i < elems * NL; i++) p[i] = (i % NL == (size_t)NL - 1) ? next() >> 4 : next();
    }
    ~Elems() { free(p); }
};

static const uint64_t BLS[4] = {0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull};
static const uint64_t P64[1] = {0xffffffffffffffc5ull};

int main() {
    for (int width = 0; width < 2; width++) {
        NL = width ? 1 : 4;
        const uint64_t *p = width ? P64 : BLS;
        for (int64_t count : {1, 3, 65}) {
            {
                Elems bits(count), out(2 * count);
                const uint64_t *ops[1] = {bits.p};
                uint64_t *outs[1] = {out.p};
                const int64_t params[2] = {1, 0};
                CHECK(hb_selftest_demux(p, NL, HB_DEMUX_SELFTEST_LEAVES, ops, params, outs, count) == HB_OK);
            }
            for (int m = 2; m <= 12; m++) {
                // the wiring: per level the rows opened and the products
                std::vector<int> widths(m, 1), opened, products;
                while (widths.size() > 1) {
                    std::vector<int> next_w;
                    int o = 0, q = 0;
                    for (size_t k = 0; 2 * k + 1 < widths.size(); k++) {
                        o += (1 << widths[2 * k]) + (1 << widths[2 * k + 1]);
                        q += 1 << (widths[2 * k] + widths[2 * k + 1]);
                        next_w.push_back(widths[2 * k] + widths[2 * k + 1]);
                    }
                    if (widths.size() & 1) next_w.push_back(widths.back());
                    opened.push_back(o), products.push_back(q);
                    widths = next_w;
                }
                size_t rows = 0;
                for (int q : products) rows += q;
                CHECK(products.back() == 1 << m);
                Elems bits((size_t)m * count), groups(rows * count);
                for (size_t level = 0; level < opened.size(); level++) {
                    Elems ta((size_t)opened[level] * count), tab((size_t)products[level] * count), masked((size_t)opened[level] * count);
                    const int64_t params[2] = {m, (int64_t)level};
                    const uint64_t *mask_ops[3] = {bits.p, groups.p, ta.p};
                    uint64_t *mask_outs[1] = {masked.p};
                    CHECK(hb_selftest_demux(p, NL, HB_DEMUX_SELFTEST_MASK, mask_ops, params, mask_outs, count) == HB_OK);
                    const uint64_t *fin_ops[3] = {masked.p, ta.p, tab.p};
                    uint64_t *fin_outs[1] = {groups.p};
                    CHECK(hb_selftest_demux(p, NL, HB_DEMUX_SELFTEST_FINISH, fin_ops, params, fin_outs, count) == HB_OK);
                    uint64_t *over[1] = {tab.p + (size_t)(products[level] - 1) * count * NL};     // groups over the last row of tab: refused
                    CHECK(hb_selftest_demux(p, NL, HB_DEMUX_SELFTEST_FINISH, fin_ops, params, over, count) == HB_ERR_BAD_ARG);
                }
                const int64_t bad[2] = {m, (int64_t)opened.size()};
                const uint64_t *ops[3] = {bits.p, groups.p, bits.p};
                uint64_t *outs[1] = {groups.p};
                CHECK(hb_selftest_demux(p, NL, HB_DEMUX_SELFTEST_MASK, ops, bad, outs, count) == HB_ERR_BAD_ARG);
            }
        }
    }
    printf(fails ? "asan_demux: %d FAILED\n" : "asan_demux: ok\n", fails);
    return fails ? 1 : 0;
}

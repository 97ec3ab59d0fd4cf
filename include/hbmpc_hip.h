/*
 * hbmpc_hip.h -- C ABI of libhbmpc_hip.so: the MI355X (gfx950) implementation of
 * HoneyBadgerMPC's batch share-reconstruction arithmetic.
 *
 * This is the drop-in boundary for the reference's NTL/Cython extension
 * `honeybadgermpc.ntl` (reference: honeybadgermpc/ntl/hbmpc_ntl_helpers.pyx,
 * re-exported by honeybadgermpc/ntl/__init__.py:1).  Each entry point names the
 * reference interface it replaces.  The reference marshals Python ints to NTL ZZ_p
 * through little-endian bytes (pyx:20-29); here a field element is the same
 * little-endian integer in a fixed width:
 *
 *     4 x uint64_t (32 bytes) for a context created with n_limbs = 4 (p < 2^256)
 *     1 x uint64_t ( 8 bytes) for a context created with n_limbs = 1 (p < 2^64)
 *
 * Conventions
 *   - plain C types only; no torch / HIP types in signatures.  `stream` is a
 *     hipStream_t passed as void* (NULL = the default stream).
 *   - `*_dev` pointers are DEVICE pointers owned by the caller (e.g. a torch tensor's
 *     data_ptr()); everything else (points x, exponents zs, omega, the modulus) is a
 *     small HOST array copied at call time.
 *   - all element values are canonical residues in [0, p) on output; inputs may be any
 *     value < 2^(64*n_limbs) ("reduced on entry", pyx:31-32).
 *   - every function returns an hb_status; nothing throws or aborts.  Work is enqueued
 *     on `stream`; functions that must report a data-dependent result (singular matrix,
 *     validation mismatch) synchronise that stream before returning and say so below.
 *   - a context is bound to one device; one process per GPU is the intended use.
 */
#ifndef HBMPC_HIP_H
#define HBMPC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    HB_OK = 0,
    HB_ERR_SINGULAR = 1,     /* Vandermonde matrix not invertible / repeated point -> InterpolationError (pyx:167-169) */
    HB_ERR_BAD_ARG = 2,      /* ValueError-class problems (pyx:44,62) */
    HB_ERR_UNSUPPORTED = 3,  /* even modulus, size beyond a kernel's limits */
    HB_ERR_NO_DEVICE = 4,    /* no usable gfx950 device: the product path fails loudly, there is no CPU fallback */
    HB_ERR_HIP = 5,          /* a HIP runtime call failed; see hb_last_error() */
    HB_ERR_MISMATCH = 6,     /* hb_batch_open: re-encoded guess disagrees with a received column (reed_solomon.py:316-326) */
    HB_ERR_RETRY = 7         /* hb_probe_feed: the launch was void (a workgroup of a probe over several workgroups waited in vain for another: they
                                talk through memory and need each other resident); nothing was fed, the probe has been reset -- feed the whole list
                                again, after hb_probe_workgroups(pr, 0) if the chip is crowded */
} hb_status;

typedef struct hb_ctx hb_ctx;        /* modulus + Montgomery constants + device + table cache */
typedef struct hb_matrix hb_matrix;  /* a device-resident n_out x n_in matrix over GF(p) in kernel layout */

/* element layout selector for batched buffers: element (c, l) of a C x L batch lives at
 * base + (c*stride_c + l*stride_l) elements.  Chunk-major [C][L] is {L, 1}; party-major /
 * coefficient-major [L][C] is {1, C} (the layout R1/R2 messages travel in,
 * batch_reconstruction.py:165-167). */
typedef struct {
    int64_t stride_c;
    int64_t stride_l;
} hb_view;

/* ---- library / context ------------------------------------------------------------ */
int hb_version(void);
int hb_device_count(void);
/* Replaces ZZ_p::init(modulus) at the top of every pyx entry point (pyx:107,220,250,...). */
int hb_ctx_create(hb_ctx **out, const uint64_t *p_limbs, int n_limbs, int device);
void hb_ctx_destroy(hb_ctx *ctx);
const char *hb_last_error(const hb_ctx *ctx);
/* Tables derived from point sets (V, V^-1, error-locator bases, index maps) are cached per context, keyed by the
 * sorted point set, and bounded: once more than a cap of entries (192; HB_CACHE_CAP in the environment) are
 * resident, the least recently used ones are dropped on entry to the next call.  hb_ctx_cache_clear drops them all
 * (synchronises the device); hb_ctx_cache_entries reports how many are resident.  The reference keeps one
 * process-global FFT base-case cache flushed on modulus change (rsdecode_impl.h:18-20,52-65). */
int hb_ctx_cache_clear(hb_ctx *ctx);
int hb_ctx_cache_entries(const hb_ctx *ctx);
int hb_elem_bytes(const hb_ctx *ctx);

/* device-memory helpers for callers that have no allocator of their own */
int hb_malloc(hb_ctx *ctx, void **dptr, size_t bytes);
int hb_free(hb_ctx *ctx, void *dptr);
int hb_memcpy_h2d(hb_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes, void *stream);
int hb_memcpy_d2h(hb_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes, void *stream);
int hb_stream_sync(hb_ctx *ctx, void *stream);

/* ---- tables ------------------------------------------------------------------------ */
/* V[i][l] = x_i^l, n x d.  Replaces set_vm_matrix (rsdecode_impl.h:23-36).  The two point-set constructors hand out
 * shared, reference-counted tables: release every handle with hb_matrix_destroy. */
int hb_vand_matrix_create(hb_ctx *ctx, const uint64_t *x_host, int n, int d, hb_matrix **out, void *stream);
/* V(x)^-1, k x k.  Replaces vandermonde_inverse (rsdecode_impl.h:97-122).  Synchronises;
 * returns HB_ERR_SINGULAR when two points coincide mod p. */
int hb_vand_inverse_create(hb_ctx *ctx, const uint64_t *x_host, int k, hb_matrix **out, void *stream);
/* arbitrary matrix from host canonical elements, row-major n_out x n_in */
int hb_matrix_from_host(hb_ctx *ctx, const uint64_t *m_host, int n_out, int n_in, hb_matrix **out, void *stream);
/* copy a matrix back to host canonical row-major (testing / vandermonde_inverse's legacy dump, pyx:115-132) */
int hb_matrix_to_host(hb_ctx *ctx, const hb_matrix *m, uint64_t *m_host, void *stream);
void hb_matrix_destroy(hb_matrix *m);

/* ---- the hot kernel: batched mat-vec over GF(p) ---------------------------------------
 * out(c, i) = sum_l M[i][l] * in(c, in_rows ? in_rows[l] : l)     c < C, i < n_out
 * Replaces NTL mat_ZZ_p mul at pyx:183 and pyx:237.  in_rows (host, n_in ints or NULL)
 * selects which rows of a party-major buffer feed the product (the arrival set z of
 * IncrementalDecoder, reed_solomon.py:305-313). */
int hb_matvec(hb_ctx *ctx, const hb_matrix *m, const uint64_t *in_dev, hb_view in, const int32_t *in_rows,
              uint64_t *out_dev, hb_view out, int64_t C, void *stream);
/* Same product, but instead of storing, compare row i (for every i in check_rows[0..n_check))
 * with expect(c, i) and OR 1 into *mismatch_dev on any difference.  Replaces the Python
 * loop reed_solomon.py:316-319.  Asynchronous. */
int hb_matvec_check(hb_ctx *ctx, const hb_matrix *m, const uint64_t *in_dev, hb_view in, const int32_t *in_rows,
                    const uint64_t *expect_dev, hb_view expect, const int32_t *check_rows, int n_check,
                    int32_t *mismatch_dev, int64_t C, void *stream);

/* to_ZZ_p for packed batches (hbmpc_ntl_helpers.pyx:31-32: every value entering the reference's boundary is reduced
 * mod p): out[i] = in[i] mod p for `count` packed elements of any word content (in == out allowed).  *changed_dev, when
 * given, is incremented once per element that was not already canonical.  The kernels behind every other entry point
 * expect canonical residues; list-of-int inputs are reduced by the Python glue, packed numpy / torch batches pass through
 * this call.  Asynchronous. */
int hb_reduce(hb_ctx *ctx, const uint64_t *in_dev, uint64_t *out_dev, int64_t count, int32_t *changed_dev, void *stream);

/* ---- element-wise arithmetic on share arrays (hb_ew.hip) ---------------------------------------------------------
 * What an MPC program does between its opens, on the packed buffers the opens read and write.  Operands are canonical
 * residues (every output of this library is; hb_reduce makes foreign buffers so) and so are the results.  All three entry
 * points are asynchronous on `stream`, allocate nothing, and accept count == 0 (nothing is launched).  Null pointers with
 * count > 0, a negative count and an unknown op return HB_ERR_BAD_ARG without launching. */
#define HB_EW_ADD 0
#define HB_EW_SUB 1
#define HB_EW_MUL 2
#define HB_EW_NEG 3
/* out[i] = a[i] op b[i] for `count` elements; HB_EW_NEG: out[i] = -a[i] (b_dev ignored).  b_broadcast != 0: b_dev is ONE
 * element used for every i (a public scalar times a share array, a share array plus a public constant).  out_dev may be
 * a_dev or b_dev (not a broadcast b_dev with count > 1).  Replaces the element loops of ShareArray.__add__ / __sub__ /
 * __mul__ (progs/mixins/dataflow.py) and of the local product of DoubleSharingMultiplyArrays
 * (progs/mixins/share_arithmetic.py:96-98). */
int hb_ew_op(hb_ctx *ctx, int op, const uint64_t *a_dev, const uint64_t *b_dev, int b_broadcast, uint64_t *out_dev, int64_t count,
             void *stream);
/* The step of a Beaver multiplication after its two opens, fused: out[i] = d[i] e[i] + d[i] q[i] + e[i] p[i] + pq[i]
 * (d = x - p and e = y - q opened, (p, q, pq) this party's shares of a triple).  Replaces the list comprehension of
 * BeaverMultiplyArrays (progs/mixins/share_arithmetic.py:43).  out_dev may be any of the inputs. */
int hb_ew_beaver(hb_ctx *ctx, const uint64_t *d_dev, const uint64_t *e_dev, const uint64_t *p_dev, const uint64_t *q_dev,
                 const uint64_t *pq_dev, uint64_t *out_dev, int64_t count, void *stream);
/* out[i] = 1 / in[i], batched (Montgomery's trick over tiles of the array; in == out allowed).  Replaces `1 / sig` for every
 * opened sig of InvertShareArray (progs/mixins/share_arithmetic.py:133).  A zero has no inverse: its output is 0, the
 * other elements are unaffected, and *zeros_dev (when given; the caller zeroes it) is increased by the number of zeros
 * met -- the caller decides whether that is field.py:126's ZeroDivisionError. */
int hb_ew_inv(hb_ctx *ctx, const uint64_t *in_dev, uint64_t *out_dev, int64_t count, int32_t *zeros_dev, void *stream);

/* ---- power mixing (hb_pm.hip) -------------------------------------------------------------------------------------
 * Replaces the NTL program apps/asynchromix/cpp/compute-power-sums.cpp (computePowers :17-84, runWithInputs :192-238) that
 * apps/asynchromix/powermixing.py:49-59 shells out to once a client, and the files of its phases 1 and 3 (:35-45, :84-90).
 * c_dev [M]: the opened a_c - b_c; powers_dev [M][k]: this party's shares of b_c^1 .. b_c^k.  With u_j = [b^j] / j! ([b^0] = 1)
 * and v_i = c^i / i!, [a^m] = m! (u * v)[m]: a convolution.  hb_pm_powers writes this party's shares of a_c^1 .. a_c^k
 * (out_dev [M][k], what computePowers returns); hb_pm_power_sums their sums over the M clients (sums_dev [k], the .sums file).
 * method: HB_PM_DIRECT (tiled triangular convolution, any odd prime), HB_PM_NTT (2M forward transforms of order N = the power
 * of two above 2k, one multiply-accumulate pass, one inverse transform: omega_host a primitive N-th root of unity and
 * order == N, else HB_ERR_UNSUPPORTED), HB_PM_AUTO (the NTT path when a usable omega is given and k > HB_PM_CROSSOVER, else the
 * direct path).  Both paths give the same canonical residues.  Asynchronous on `stream` (the first call for a given k builds the
 * factorial tables and synchronises once).  M == 0 writes zeros.  k <= 0, k >= p, a negative M and null pointers return
 * HB_ERR_BAD_ARG before any launch.  Neither call changes its inputs; the outputs must not overlap them.
 * Working set: clients are taken in slabs, so the temporaries -- 2 (k + 1) + 2 N elements a client of a slab (2 (k + 1) on the
 * direct path), at most 256 MiB a slab (one client's worth if that is more), plus (1024 / ceil(N / 256) + 2) N elements of
 * partial sums -- do not grow with M.  They are kept with the context per stream and returned by hb_ctx_cache_clear. */
#define HB_PM_AUTO 0
#define HB_PM_DIRECT 1
#define HB_PM_NTT 2
/* HB_PM_AUTO takes the NTT path for k above this while N fits the batched LDS transform (N <= 2048 for 32-byte elements, 8192 for
 * 8-byte ones).  Measured, profiles/power_mixing.txt (M = k, BLS12-381 Fr): direct / NTT time 0.74 at k = 256, 1.64 at k = 320 (the direct
 * kernel takes a second tile of outputs from k = 257), 3.4 at k = 1023; above the LDS order the transforms run one polynomial at a time
 * and the direct path is 40x (k = 1024) to 4x (k = 4096) faster. */
#define HB_PM_CROSSOVER 256
int hb_pm_power_sums(hb_ctx *ctx, const uint64_t *c_dev, const uint64_t *powers_dev, int64_t M, int k, int method,
                     const uint64_t *omega_host, int order, uint64_t *sums_dev, void *stream);
int hb_pm_powers(hb_ctx *ctx, const uint64_t *c_dev, const uint64_t *powers_dev, int64_t M, int k, uint64_t *out_dev, void *stream);

/* ---- root finding: power sums -> messages (hb_rf.hip) ---------------------------------------------------------------
 * Replaces apps/asynchromix/solver/solver.py:20 solve() and the FLINT program behind it (apps/asynchromix/solver/solver.cpp).
 * hb_rf_newton: sums_dev [k] = S_1 .. S_k -> coeffs_dev [k + 1], the monic polynomial with those power sums (coefficient of x^i at
 * i) by Newton's identities: one workgroup, k dependent steps in one launch; asynchronous on `stream`.
 * hb_rf_roots: coeffs_dev [k + 1], monic -> roots_dev [k], the roots with multiplicity in the order found, *n_roots_host = k; or
 * *n_roots_host = -1 (and HB_OK) when the polynomial is not a product of k linear factors -- decided, not assumed: see hb_rf.hip.
 * `seed` chooses the random shifts of the equal-degree splitting (a counter-based generator on (seed, level, node, draw)); the set
 * of roots does not depend on it.  THIS CALL OWNS THE LEVEL LOOP AND SYNCHRONISES `stream` ONCE A LEVEL of the split tree, and once
 * for each multiplicity, to read the degrees of the factors -- some 10 + the largest multiplicity waits at k = 1024 -- and once
 * before it returns: the roots are complete when it does.  A node that no shift splits in 64 draws gives HB_ERR_HIP (probability
 * 2^-64 a node for p > 64; cannot happen below, where every shift is tried).
 * k < 1, k >= p, null pointers: HB_ERR_BAD_ARG; k > HB_RF_MAX_K: HB_ERR_UNSUPPORTED (a GCD keeps both remainders, 2 (k + 1)
 * coefficients of 36 bytes, in one compute unit's LDS: 74 KB at 1024, two workgroups a unit).  Temporaries (the k x k reduction
 * table is the largest: 38 MB at k = 1024) are kept with the context per stream and returned by hb_ctx_cache_clear. */
#define HB_RF_MAX_K 1024
/* nodes of the split tree at or below this degree run their whole chain in one launch of one workgroup each */
#define HB_RF_SMALL_DEGREE 32
int hb_rf_newton(hb_ctx *ctx, const uint64_t *sums_dev, int k, uint64_t *coeffs_dev, void *stream);
int hb_rf_roots(hb_ctx *ctx, const uint64_t *coeffs_dev, int k, uint64_t seed, uint64_t *roots_dev, int32_t *n_roots_host, void *stream);

/* ---- the butterfly (switching) network (hb_bf.hip) ------------------------------------------------------------------
 * One layer of apps/asynchromix/butterfly_network.py:9-53 (batch_switch and the loops that deal its inputs): k inputs, k a power
 * of two, stride 2^log2_stride, k / 2 switches.  Switch j takes x = in[xi], y = in[yi], xi = ((j >> a) << (a + 1)) | (j & (2^a - 1)),
 * yi = xi | 2^a (a = log2_stride), a shared sign b_j in {1, -1} and one triple (p_j, q_j, pq_j); m = b_j (x - y) is one Beaver
 * multiplication and out[2j] = (x + y + m) / 2, out[2j + 1] = (x + y - m) / 2.
 * hb_bf_mask, before the open: masked_dev[j] = bits[j] - p[j] and masked_dev[k / 2 + j] = in[xi] - in[yi] - q[j] (k elements, one
 * array to open); bits_dev == NULL (the signs' differences were opened in advance): masked_dev[j] = in[xi] - in[yi] - q[j] alone
 * (k / 2 elements; p_dev is not read).  hb_bf_switch, after it: d_dev, e_dev [k / 2] the opened halves; writes out_dev [k].
 * Operands and results are canonical residues; bits_dev, p_dev, q_dev, pq_dev, d_dev, e_dev hold k / 2 elements each.  Both calls
 * are asynchronous on `stream`, one launch each, allocate nothing and leave their inputs unchanged.  HB_ERR_BAD_ARG before any
 * launch: null pointers, k not a power of two or below 2, log2_stride outside [0, log2(k)), out_dev / masked_dev overlapping
 * in_dev (a layer is not in place: ping-pong two buffers). */
int hb_bf_mask(hb_ctx *ctx, const uint64_t *in_dev, const uint64_t *bits_dev, const uint64_t *p_dev, const uint64_t *q_dev, int64_t k,
               int log2_stride, uint64_t *masked_dev, void *stream);
int hb_bf_switch(hb_ctx *ctx, const uint64_t *in_dev, const uint64_t *d_dev, const uint64_t *e_dev, const uint64_t *p_dev,
                 const uint64_t *q_dev, const uint64_t *pq_dev, int64_t k, int log2_stride, uint64_t *out_dev, void *stream);

/* ---- the MiMC block cipher (hb_mimc.hip) -----------------------------------------------------------------------------
 * progs/mimc.py:10-15 (mimc_plain), :25-30 and :46-55 (the cubing round of mimc_mpc and mimc_mpc_batch), and the keystream of
 * progs/mimc_symmetric.py:10-16, 19-28.  F(x, k): v = x; rounds times v = (v + k + c)^3 for c = 0, 1, ...; F = v + k.
 * Everywhere: operands and results are canonical residues; key_dev holds ONE element for all (key_broadcast != 0) or `count` of them;
 * x_dev == NULL means the counters x_i = start + i, start_host one canonical element in host memory (NULL: 0; not below the modulus:
 * HB_ERR_BAD_ARG).  A public constant is added to a Shamir share alike by every party, so no call asks whether x or key is shared.
 * hb_mimc_plain, the cleartext cipher in one launch: out[i] = F(x_i, key_i); with addend_dev, addend[i] + F (mimc_encrypt) or, with
 *   HB_MIMC_SUB, addend[i] - F (its inverse).  HB_MIMC_PAIR: two elements a thread instead of one, same results (DESIGN.md 3k has
 *   the timings of both).  rounds < 1: HB_ERR_BAD_ARG.
 * hb_mimc_first: out[i] = x_i + key_i - r0[i], the first array an MPC evaluation opens.
 * hb_mimc_round, after the open of round ctr: y_dev the opened x - r; r_dev, r2_dev, r3_dev this party's shares of the round's
 *   cube (r, r^2, r^3); x3 = y^3 + 3 y^2 r + 3 y r2 + r3.  out[i] = x3 + (key_i + ctr + 1) - r_next[i], the next round's array to
 *   open; r_next_dev == NULL (the last round): out[i] = x3 + key_i.  ctr < 0: HB_ERR_BAD_ARG.
 * All three are asynchronous on `stream`, one launch each, and allocate nothing.  HB_ERR_BAD_ARG before any launch: null pointers
 * (with count > 0: an empty array may have none), a negative count, unknown flags, HB_MIMC_SUB without an addend.  count == 0 returns HB_OK and launches nothing; more than
 * 2^31 - 1 workgroups: HB_ERR_UNSUPPORTED.  In place: out_dev may be any of the arrays of `count` elements a call reads (x, addend,
 * a key per element, y, r, r2, r3, r_next, r0: a thread reads its elements before it writes them) but not a broadcast key when
 * count > 1; partial overlaps are the caller's to avoid. */
#define HB_MIMC_SUB 1
#define HB_MIMC_PAIR 2
int hb_mimc_plain(hb_ctx *ctx, const uint64_t *x_dev, const uint64_t *start_host, const uint64_t *key_dev, int key_broadcast,
                  const uint64_t *addend_dev, int flags, int rounds, uint64_t *out_dev, int64_t count, void *stream);
int hb_mimc_first(hb_ctx *ctx, const uint64_t *x_dev, const uint64_t *start_host, const uint64_t *key_dev, int key_broadcast,
                  const uint64_t *r0_dev, uint64_t *out_dev, int64_t count, void *stream);
int hb_mimc_round(hb_ctx *ctx, const uint64_t *y_dev, const uint64_t *r_dev, const uint64_t *r2_dev, const uint64_t *r3_dev,
                  const uint64_t *key_dev, int key_broadcast, int64_t ctr, const uint64_t *r_next_dev, uint64_t *out_dev, int64_t count,
                  void *stream);

/* ---- the Jubjub curve (hb_jj.hip) --------------------------------------------------------------------------------------
 * The twisted Edwards curve a x^2 + y^2 = 1 + d x^2 y^2 of elliptic_curve.py: Point.__mul__ (:102-122) and the doubling chain of
 * share_mul (progs/jubjub.py:280-286) in the clear, and SharedPoint.add (progs/jubjub.py:87-113) on share arrays.  Points are two
 * arrays of canonical residues (x, y); a_host and d_host are ONE canonical element each in host memory (missing where the call
 * says it needs one, or not below the modulus: HB_ERR_BAD_ARG).  The curve must be complete (a a square, d a non-square) and the
 * points on it: nothing here checks that, and off the curve a denominator may vanish (its result is then 0).
 * hb_jj_scalar_mul: (outx, outy)[i] = n_i (x_i, y_i) in one launch; n_broadcast / point_broadcast != 0: element 0 serves every i.
 *   Scalars are canonical residues (any value below the modulus); n_i = 0 gives (0, 1).
 * hb_jj_double_table: (xs, ys)[j][i] = 2^j (x_i, y_i) for j < rows, arrays of rows * count elements, row-major; zs_dev is scratch of
 *   the same size.  Four launches: the projective rows, ONE hb_ew_inv over every Z (zeros_dev as hb_ew_inv takes it, or NULL) and two
 *   hb_ew_op products.  rows < 1: HB_ERR_BAD_ARG.
 * The addition of m pairs of SHARED points, for curves with a = -1 (the reference's law):
 *     x3 = (x1 y2 + y1 x2) / (1 + d x1 x2 y1 y2),   y3 = (y1 y2 + x1 x2) / (1 - d x1 x2 y1 y2)
 *   consumes 9 Beaver triples and 2 random shares (rx, ry) a pair.  p_dev, q_dev, pq_dev: this party's shares of the triples' first
 *   factors, second factors and products; triple k of pair i at element k * trip_stride + i (trip_stride >= m, else HB_ERR_BAD_ARG).
 *   Triple k multiplies: 0 x1 x2, 1 y1 y2, 2 x1 y2, 3 y1 x2, 4 xp yp, 5 nx rx, 6 ny ry, 7 dx rx, 8 dy ry (xp = x1 x2, yp = y1 y2,
 *   nx = x1 y2 + y1 x2, ny = yp + xp, dx = 1 + d xp yp, dy = 1 - d xp yp).  Between the calls the caller opens what a call wrote:
 *   hb_jj_add_mask    writes a_dev [8][m]: rows 2k, 2k + 1 the masked factors of products k = 0..3
 *   hb_jj_add_stage1  opened A -> b_dev [6][m]: the masked factors of products 4..6
 *   hb_jj_add_stage2  opened B -> uv_dev [2][m] = ([nx rx], [ny ry]), kept by the caller, and c_dev [4][m]: products 7, 8
 *   hb_jj_add_stage3  opened C -> d_dev [2][m]: the shares of sig_x = dx rx, sig_y = dy ry
 *   hb_jj_add_finish  opened D -> x3 = uv[0] / sig_x, y3 = uv[1] / sig_y: hb_ew_inv over the 2 m sigs into inv_dev (scratch, [2][m];
 *                     a zero sig -- r = 0 or operands off the curve -- is counted in *zeros_dev as hb_ew_inv counts) and one scaling launch.
 *   One launch each (finish: two), asynchronous on `stream`, nothing allocated.  Every output is an array of its own, distinct from
 *   what the call reads.  Null pointers with m > 0 and a negative m: HB_ERR_BAD_ARG; m == 0 returns HB_OK and launches nothing. */
int hb_jj_scalar_mul(hb_ctx *ctx, const uint64_t *n_dev, int n_broadcast, const uint64_t *x_dev, const uint64_t *y_dev, int point_broadcast,
                     const uint64_t *a_host, const uint64_t *d_host, uint64_t *outx_dev, uint64_t *outy_dev, int64_t count, void *stream);
int hb_jj_double_table(hb_ctx *ctx, const uint64_t *x_dev, const uint64_t *y_dev, const uint64_t *a_host, int rows, uint64_t *xs_dev,
                       uint64_t *ys_dev, uint64_t *zs_dev, int64_t count, int32_t *zeros_dev, void *stream);
int hb_jj_add_mask(hb_ctx *ctx, const uint64_t *x1_dev, const uint64_t *y1_dev, const uint64_t *x2_dev, const uint64_t *y2_dev,
                   const uint64_t *p_dev, const uint64_t *q_dev, int64_t trip_stride, uint64_t *a_dev, int64_t m, void *stream);
int hb_jj_add_stage1(hb_ctx *ctx, const uint64_t *a_open_dev, const uint64_t *p_dev, const uint64_t *q_dev, const uint64_t *pq_dev,
                     int64_t trip_stride, const uint64_t *rx_dev, const uint64_t *ry_dev, uint64_t *b_dev, int64_t m, void *stream);
int hb_jj_add_stage2(hb_ctx *ctx, const uint64_t *b_open_dev, const uint64_t *p_dev, const uint64_t *q_dev, const uint64_t *pq_dev,
                     int64_t trip_stride, const uint64_t *rx_dev, const uint64_t *ry_dev, const uint64_t *d_host, uint64_t *uv_dev,
                     uint64_t *c_dev, int64_t m, void *stream);
int hb_jj_add_stage3(hb_ctx *ctx, const uint64_t *c_open_dev, const uint64_t *p_dev, const uint64_t *q_dev, const uint64_t *pq_dev,
                     int64_t trip_stride, uint64_t *d_dev, int64_t m, void *stream);
int hb_jj_add_finish(hb_ctx *ctx, const uint64_t *d_open_dev, const uint64_t *uv_dev, uint64_t *inv_dev, uint64_t *x3_dev, uint64_t *y3_dev,
                     int64_t m, int32_t *zeros_dev, void *stream);

/* ---- BLS12-381 G1 and the linear polynomial commitment (hb_g1.hip) -----------------------------------------------------
 * The group the reference's poly_commit_lin.py commits in (betterpairing.G1): E: y^2 = x^3 + 4 over the 381-bit field GF(Q), written
 * additively here.  Every call takes a four-limb context whose modulus is the group order R = Subgroup.BLS12_381 (anything else:
 * HB_ERR_BAD_ARG).  A point is 12 words: x then y, 6 little-endian words each, canonical residues below Q; the identity is all zeros.
 * Scalars are the context's elements, read as plain 256-bit integers (any value).  Points are taken as they come: what is off the
 * curve gives a meaningless result, never a fault; hb_g1_check tells.  NOTHING here tests membership of the subgroup of order R:
 * hb_g1_scalar_mul by R (identity out <=> member) is that test.
 * hb_g1_scalar_mul: out[i] = k_i P_i; k_broadcast / point_broadcast != 0: element 0 serves every i.  One launch.
 * hb_g1_add: out[i] = P_i + Q_i, or P_i - Q_i with subtract != 0.  Complete: identity, equal and opposite operands included.
 * hb_g1_check: flags[i] = 1 if P_i is the identity, or has both coordinates below Q and lies on the curve; else 0.
 * hb_g1_table: the fixed-base window table of ONE base (12 words in HOST memory; the identity or a point off the curve:
 *   HB_ERR_BAD_ARG) for window width 4 or 8, into table_dev, a device buffer of hb_g1_table_bytes(window) bytes (0 for another width)
 *   aligned to 16 bytes.  Its layout is the library's own.  Synchronises the stream once (the base's upload), then one launch.
 * hb_g1_commit: out[i] = a_i g + b_i h from the tables of g and h (built with the same window): the dealer's commitments.
 * hb_g1_eval: out[b] = sum_j index^j cs[b][j] for `count` vectors of n_coef commitments (cs: count * n_coef points), by Horner's
 *   rule; index < 2^32 (else HB_ERR_BAD_ARG); index = 0 gives cs[b][0].
 * hb_g1_verify: verdict[b] = 1 if every commitment of item b passes hb_g1_check's test and sum_j index^j cs[b][j] = s_b g + w_b h,
 *   else 0; *rejected_dev (an int32 the caller has zeroed) grows by the number of rejected items.  One launch, no inversion.
 * All: asynchronous on `stream` (but hb_g1_table's upload), nothing allocated; count == 0 returns HB_OK and launches nothing. */
int hb_g1_scalar_mul(hb_ctx *ctx, const uint64_t *k_dev, int k_broadcast, const uint64_t *p_dev, int point_broadcast, uint64_t *out_dev,
                     int64_t count, void *stream);
int hb_g1_add(hb_ctx *ctx, const uint64_t *p_dev, const uint64_t *q_dev, int subtract, uint64_t *out_dev, int64_t count, void *stream);
int hb_g1_check(hb_ctx *ctx, const uint64_t *p_dev, int32_t *flags_dev, int64_t count, void *stream);
int64_t hb_g1_table_bytes(int window);
int hb_g1_table(hb_ctx *ctx, const uint64_t *base_host, int window, void *table_dev, void *stream);
int hb_g1_commit(hb_ctx *ctx, const void *tg_dev, const void *th_dev, int window, const uint64_t *a_dev, const uint64_t *b_dev,
                 uint64_t *out_dev, int64_t count, void *stream);
int hb_g1_eval(hb_ctx *ctx, const uint64_t *cs_dev, int n_coef, uint64_t index, uint64_t *out_dev, int64_t count, void *stream);
int hb_g1_verify(hb_ctx *ctx, const void *tg_dev, const void *th_dev, int window, const uint64_t *cs_dev, int n_coef, uint64_t index,
                 const uint64_t *s_dev, const uint64_t *w_dev, int32_t *verdict_dev, int32_t *rejected_dev, int64_t count, void *stream);
/* Multi-scalar multiplication in G1 (hb_msm.hip): out[m] = sum_k s[m][k] P[m][k] for `rows` rows of `terms` terms; what the reference's
 * interpolate_g1_at_x (betterpairing.py:800) computes with Lagrange weights for scalars.  s_dev: rows * terms scalars, plain 256-bit
 * integers; p_dev: `terms` points shared by every row (points_per_row == 0) or rows * terms points; out_dev: `rows` affine points.
 * method: 0 auto (by `terms`), 1 direct (a full scalar multiplication a term, summed by a tree in LDS), 2 bucket (windows of 8 bits:
 *   one mixed addition a term a window; buckets summed without a serial chain; see hb_msm.hip).  All give the same words.
 * chunk: the terms one workgroup of the bucket path takes: 0 = the default (4096), else a multiple of 64 in [64, 4096].
 * workspace_dev: hb_g1_msm_workspace_bytes(rows, terms, method, chunk) bytes (0 for arguments hb_g1_msm refuses), aligned to 16 bytes,
 *   the library's while the call's launches run; its content afterwards means nothing.
 * HB_ERR_BAD_ARG: a null pointer, a negative count, another method or chunk, a workspace too small, out overlapping s, P or the
 *   workspace.  rows == 0 launches nothing; terms == 0 fills out with identities.  Three launches on `stream`, nothing allocated.
 *   A call on the bucket path ends in 248 dependent doublings a row: it is never faster than one hb_g1_scalar_mul of a wave. */
int64_t hb_g1_msm_workspace_bytes(int64_t rows, int64_t terms, int method, int chunk);
int hb_g1_msm(hb_ctx *ctx, const uint64_t *s_dev, const uint64_t *p_dev, int points_per_row, uint64_t *out_dev, int64_t rows, int64_t terms,
              int method, int chunk, void *workspace_dev, int64_t workspace_bytes, void *stream);
/* The prover of the constant-size (KZG) polynomial commitment in G1 (hb_crs.hip): the reference's poly_commit_const.py commit and
 * create_witness, sums of powers of the FIXED bases gs[j] = alpha^j g, hs[j] = alpha^j h of a common reference string.  The verifier
 * (verify_eval, batch_verify_eval) needs a pairing -- G2, Fq12 -- and is NOT in this library.
 * hb_g1_crs_table: the window tables of n_bases bases (n_bases * 12 words in HOST memory; an identity or a point off the curve among
 *   them: HB_ERR_BAD_ARG, as hb_g1_table) for window width 4 or 8 into tables_dev, n_bases * hb_g1_table_bytes(window) bytes aligned to
 *   16: table k stands at byte k * hb_g1_table_bytes(window) in hb_g1_table's layout, so each is also a table for hb_g1_commit and
 *   hb_g1_verify.  n_bases <= 4096.  Returns once bases_host is the caller's again (one synchronisation, for the upload); then ONE
 *   launch, a base a workgroup, on `stream`.
 * hb_kzg_quotient: synthetic division in GF(R) for count_polys polynomials of n_coef = t + 1 >= 1 coefficients (phi_dev: count_polys *
 *   n_coef canonical residues, lowest first) by X - xs[i] for n_points points (xs_dev: canonical residues):
 *   q[b][i][t-1] = phi[b][t], q[b][i][j-1] = phi[b][j] + xs[i] q[b][i][j], rem[b][i] = phi[b][0] + xs[i] q[b][i][0] = phi_b(xs[i]).
 *   q_dev: count_polys * n_points * t elements (unused, and may be NULL, for t = 0), rem_dev: count_polys * n_points; canonical.
 *   (phi_b(X) - rem[b][i]) = (X - xs[i]) sum_j q[b][i][j] X^j: q holds the exponents of the witness, rem the share.  One launch.
 * hb_g1_crs_msm: out[m] = sum_{k < terms} a[m][k] G_k + b[m][k] H_k over the first `terms` of the n_bases tables at tg_dev and th_dev
 *   (both built with `window`); th_dev and b_dev both NULL: one family.  a_dev, b_dev: rows * terms scalars, plain 256-bit integers.
 *   One mixed addition a non-zero window digit, no doubling.  split: the lanes that share a row, a power of two in [1, 256] (1: a row a
 *   lane, no LDS; above: a tree in LDS ends the row), or 0 for the library's rule (hb_crs.hip: CRS_FILL_LANES).  Every split and both
 *   widths give the same words.  One launch.
 * All three, HB_ERR_BAD_ARG: a null pointer, a negative count, a window other than 4 or 8, terms > n_bases, n_bases > 4096, another
 *   split, an output overlapping an input.  A zero count returns HB_OK and launches nothing; terms == 0 fills out with identities.
 *   Nothing is allocated; everything is asynchronous on `stream` but the table's upload.  A context over R in four limbs, as all of G1. */
int hb_g1_crs_table(hb_ctx *ctx, const uint64_t *bases_host, int64_t n_bases, int window, void *tables_dev, void *stream);
int hb_kzg_quotient(hb_ctx *ctx, const uint64_t *phi_dev, int n_coef, const uint64_t *xs_dev, int64_t n_points, uint64_t *q_dev,
                    uint64_t *rem_dev, int64_t count_polys, void *stream);
int hb_g1_crs_msm(hb_ctx *ctx, const void *tg_dev, const void *th_dev, int64_t n_bases, int window, const uint64_t *a_dev,
                  const uint64_t *b_dev, int64_t terms, int split, uint64_t *out_dev, int64_t rows, void *stream);
/* G1 points from the wire (hb_g1_wire.hip): the 48-byte compressed encoding of the reference's Rust crate and a test of membership in
 * the subgroup of order R that needs no full-width scalar multiplication.  An encoding is big-endian x; in byte 0, 0x80 always set
 * (compressed), 0x40 the identity (x = 0, no sign), 0x20 set when y > (Q - 1) / 2.
 * hb_g1_subgroup: flags[i] = 1 if P_i passes hb_g1_check's test AND (P_i is the identity or phi(P_i) = -[x^2] P_i), else 0;
 *   phi(x, y) = (beta x, y) the curve's endomorphism, x = 0xd201000000010000 the curve's parameter: true exactly for the points of the
 *   subgroup (Scott, eprint 2021/1130).  126 doublings and 10 additions an element in Jacobian coordinates, no inversion.  One launch.
 * hb_g1_decompress: bytes_dev = count * 48 bytes, aligned to 16 (another alignment: HB_ERR_BAD_ARG) -> out_dev, `count` points as all
 *   of G1 takes them, and status_dev[i], the FIRST check item i fails in the order of the codes below (HB_G1_WIRE_NOT_IN_SUBGROUP
 *   only with check_subgroup != 0: hb_g1_subgroup's test in the same launch).  A rejected item's point is all zeros, as the
 *   identity's is: the status tells them apart.  *rejected_dev is incremented once a rejected item (the caller zeroes it).  y is
 *   rhs^((Q + 1) / 4) with rhs = x^3 + 4, accepted iff y^2 = rhs.  x = 0 with either sign IS a point ((0, +-2), of order 3).  One launch.
 * hb_g1_compress: bytes_dev (count * 48 bytes, aligned to 16) = the encodings of `count` points.  The coordinates are written as they
 *   stand (all zeros: the identity); hb_g1_check tells whether they are a point.  One launch.
 * All: asynchronous on `stream`, nothing allocated; count == 0 returns HB_OK and launches nothing; an output overlapping an input:
 *   HB_ERR_BAD_ARG.  The exponent (Q + 1) / 4, (Q - 1) / 2 and beta are derived from or checked against Q once a process (4 e = Q + 1,
 *   beta^3 = 1, beta != 1, phi(G) = -[x^2] G on the generator, sqrt(4) = +-2); a failed check: HB_ERR_UNSUPPORTED from all three. */
#define HB_G1_WIRE_OK 0
#define HB_G1_WIRE_NOT_COMPRESSED 1
#define HB_G1_WIRE_BAD_IDENTITY 2
#define HB_G1_WIRE_X_NOT_BELOW_Q 3
#define HB_G1_WIRE_NOT_ON_CURVE 4
#define HB_G1_WIRE_NOT_IN_SUBGROUP 5
int hb_g1_subgroup(hb_ctx *ctx, const uint64_t *p_dev, int32_t *flags_dev, int64_t count, void *stream);
int hb_g1_decompress(hb_ctx *ctx, const void *bytes_dev, int check_subgroup, uint64_t *out_dev, int32_t *status_dev, int32_t *rejected_dev,
                     int64_t count, void *stream);
int hb_g1_compress(hb_ctx *ctx, const uint64_t *p_dev, void *bytes_dev, int64_t count, void *stream);

/* ---- pairings against prepared G2 points (hb_pair.hip) ------------------------------------------------------------------
 * The verifier of the KZG commitment (poly_commit_const.py:28-44): products of BLS12-381 pairings whose G2 arguments are fixed.  A G2
 * point is PREPARED on the host (bls12_381_pairing.prepare_g2: the 68 line-coefficient triples of the ate loop, 63 doublings and 5
 * additions in the order the loop reads them) and uploaded once; the device does no G2 arithmetic.  A GT element is 72 words: twelve
 * canonical residues below Q of 6 little-endian words each, in the order c0.c0.c0, c0.c0.c1, c0.c1.c0, ..., c1.c2.c1 of the tower
 * Fq2 = Fq[u]/(u^2 + 1), Fq6 = Fq2[v]/(v^3 - 1 - u), Fq12 = Fq6[w]/(w^2 - v).  It is the reference crate's pairing value: the Miller
 * value to the power 3 (Q^12 - 1) / R.
 * hb_pair_table_bytes: the bytes of one prepared table (its layout belongs to the library).
 * hb_pair_prepare: n_coeffs = 204 Fq2 coefficients in HOST memory (68 triples; an Fq2 is c0 then c1, 6 words each, below Q; another
 *   count or a residue not below Q: HB_ERR_BAD_ARG) into table_dev, hb_pair_table_bytes() bytes.  Returns once coeffs_host is the caller's
 *   again (one synchronisation, for the upload).
 * hb_pair_product: out[m] = FE(prod_k ML(P[m][k], Q_k)) for k < K, 1 <= K <= 4: tables_dev a HOST array of K device tables, points_dev
 *   (count, K, 12) words as all of G1 takes points; an identity point contributes 1.  mode = HB_PAIR_GT: out_dev receives the GT elements,
 *   72 words an item (flags_dev and rejected_dev unused).  mode = HB_PAIR_VERDICT: flags_dev[m] = 1 if the product is 1 and every point
 *   of the item passes hb_g1_check's test, else 0, and *rejected_dev is incremented once a rejected item (the caller zeroes it; out_dev
 *   unused).  Membership of a point in the subgroup of order R is NOT checked.  One launch.
 * HB_ERR_BAD_ARG: a null pointer, a negative count, K outside 1..4, another mode, an output overlapping an input.  A zero count returns
 *   HB_OK and launches nothing.  Nothing is allocated on the device; everything is asynchronous on `stream` but the table's upload.  A
 *   context over R in four limbs, as all of G1. */
#define HB_PAIR_GT 0
#define HB_PAIR_VERDICT 1
int64_t hb_pair_table_bytes(void);
int hb_pair_prepare(hb_ctx *ctx, const uint64_t *coeffs_host, int64_t n_coeffs, void *table_dev, void *stream);
int hb_pair_product(hb_ctx *ctx, const void *const *tables_dev, int K, const uint64_t *points_dev, int mode, uint64_t *out_dev,
                    int32_t *flags_dev, int32_t *rejected_dev, int64_t count, void *stream);

/* ---- fixed-point arithmetic on shares (hb_fxp.hip) --------------------------------------------------------------------
 * progs/fixedpoint.py ("Secure Computation With Fixed-Point Numbers", Catrina and Saxena): random2m (:91-98), trunc_pr (:108-120),
 * get_carry_bit / bit_ltl (:131-172), div2m (:184-193), trunc (:208-211) and FixedPoint.ltz (:266-268) for arrays of `count` values.
 * Everywhere: operands and results are canonical residues.  A value has k bits, m of them are cut off, kappa is the statistical
 * security parameter.  Preprocessed random bit shares are bit planes: bits_dev holds rows of `count` elements, row i this party's
 * shares of bit i of every element's mask.  Arrays of several rows are row-major with `count` elements a row.
 * hb_fxp_mask: r1 = sum_{i<m} 2^i b_i and r2 = sum_{i<k+kappa-m} 2^i b_{m+i} by Horner over k + kappa rows of bits_dev.
 *   x_dev given: masked_dev[i] = x_i + 2^(k-1) + r1 + 2^m r2, the array to open, and r1_dev[i] = r1.  x_dev == NULL (random2m alone):
 *   masked_dev[i] = r2, r1_dev[i] = r1.  HB_ERR_BAD_ARG unless 0 < m < k, kappa >= 0 and k + kappa + 1 <= bits(p) - 1 (the masked
 *   value c < 2^(k+kappa+1) must not wrap).  masked_dev may be x_dev; r1_dev is an array of its own.
 * hb_fxp_trunc_pr, after the open: out[i] = (x_i - (c_i mod 2^m) + r1_i) 2^(-m).  inv2m_host: ONE canonical element in host
 *   memory, 2^(-m) mod p (not below the modulus: HB_ERR_BAD_ARG).  0 < m <= bits(p) - 2.  out_dev may be x_dev, c_dev or r1_dev.
 * hb_fxp_ltl_leaves: the leaves of the carry tree of c2 + (2^m - 1 - r1) + 1, c2 = c mod 2^m public, from rows 0..m-1 of bits_dev
 *   (no product: bit a of c2 selects).  g_dev, p_dev [m + 1][count]: row j < m for bit i = m - 1 - j, (g, p) = (1 - b_i, b_i) where
 *   bit i of c is set and (0, 1 - b_i) where it is not; row m the low carry (1, 0).
 * One level of the carry tree, (g1, p1) o (g2, p2) = (g1 + p1 g2, p1 p2) on adjacent rows 2j, 2j + 1 of `nodes` rows; an odd last row
 *   moves up unchanged.  Node j spends triples 2j (p1 g2) and 2j + 1 (p1 p2) of the level: ta_dev, tb_dev, tab_dev hold this party's
 *   shares of the first factors, second factors and products, one row a triple.  root != 0 (nodes must be 2): only g is wanted,
 *   one triple.
 *   hb_fxp_carry_mask     masked_dev rows 2t, 2t + 1 = p1 - ta[t], (t even: g2, t odd: p2) - tb[t]: the level's ONE array to open
 *   hb_fxp_carry_combine  opened_dev = that array opened; g_out_dev, p_out_dev [ceil(nodes / 2)][count] (root: g_out_dev [count],
 *                         p_out_dev ignored).  The outputs are arrays of their own.  nodes < 2: HB_ERR_BAD_ARG.
 * hb_fxp_div2m_finish: u = 1 - carry, a2 = (c mod 2^m) - r1 + 2^m u.  mode HB_FXP_MOD: out = a2 = [x mod 2^m] (x_dev may be NULL);
 *   HB_FXP_TRUNC: out = (x - a2) 2^(-m); HB_FXP_NEG_TRUNC: its negation (ltz for m = k - 1).  out_dev may be any input array.
 * All are asynchronous on `stream`, one launch each, and allocate nothing.  HB_ERR_BAD_ARG before any launch: null pointers (with
 * count > 0), a negative count, parameters out of range.  count == 0 returns HB_OK and launches nothing. */
#define HB_FXP_MOD 0
#define HB_FXP_TRUNC 1
#define HB_FXP_NEG_TRUNC 2
int hb_fxp_mask(hb_ctx *ctx, const uint64_t *x_dev, const uint64_t *bits_dev, int k, int m, int kappa, uint64_t *masked_dev,
                uint64_t *r1_dev, int64_t count, void *stream);
int hb_fxp_trunc_pr(hb_ctx *ctx, const uint64_t *x_dev, const uint64_t *c_dev, const uint64_t *r1_dev, int m, const uint64_t *inv2m_host,
                    uint64_t *out_dev, int64_t count, void *stream);
int hb_fxp_ltl_leaves(hb_ctx *ctx, const uint64_t *c_dev, const uint64_t *bits_dev, int m, uint64_t *g_dev, uint64_t *p_dev, int64_t count,
                      void *stream);
int hb_fxp_carry_mask(hb_ctx *ctx, const uint64_t *g_dev, const uint64_t *p_dev, int nodes, int root, const uint64_t *ta_dev,
                      const uint64_t *tb_dev, uint64_t *masked_dev, int64_t count, void *stream);
int hb_fxp_carry_combine(hb_ctx *ctx, const uint64_t *opened_dev, const uint64_t *g_dev, const uint64_t *p_dev, int nodes, int root,
                         const uint64_t *ta_dev, const uint64_t *tb_dev, const uint64_t *tab_dev, uint64_t *g_out_dev, uint64_t *p_out_dev,
                         int64_t count, void *stream);
int hb_fxp_div2m_finish(hb_ctx *ctx, const uint64_t *x_dev, const uint64_t *c_dev, const uint64_t *r1_dev, const uint64_t *carry_dev, int m,
                        const uint64_t *inv2m_host, int mode, uint64_t *out_dev, int64_t count, void *stream);

/* ---- oblivious sort of shared values: one layer of compare-exchanges (hb_sort.hip) --------------------------------------------
 * The three fused steps between the opens of a layer of Batcher's merge exchange (Knuth 5.2.2, Algorithm M).  table_dev holds
 * `width` columns (1..256) of `batch` arrays of n rows, column-major: element w (batch n) + b n + i is row i of array b in column w;
 * column 0 is the key.  A layer (a, r, d, cnt) compares, in every array, rows lo(e) and lo(e) + d for e < cnt with
 * lo(e) = ((e >> a) << (a + 1)) | (e & (2^a - 1)) | r, and leaves the smaller key in row lo(e).  Slot s of the layer is comparator
 * s % cnt of array s / cnt; every other array has rows of `slots` = batch cnt elements, row-major.  HB_ERR_BAD_ARG unless
 * 2 <= n <= 2^31, batch >= 1, 0 <= a <= 30, r is 0 or 2^a, d is a positive odd multiple of 2^a (which makes the layer a matching:
 * no row belongs to two comparators), lo(cnt - 1) + d < n, and batch n <= 2^40.  The comparison is that of hb_fxp_* with m = k - 1: the
 * difference of two keys is a signed k-bit value.
 * hb_sort_cmp_mask: d = key[lo] - key[hi] and the mask of hb_fxp_mask over the slot's k + kappa rows of bits_dev:
 *   masked_dev[s] = d + 2^(k-1) + r1 + 2^(k-1) r2, the array to open, and r1_dev[s] = r1.  k >= 2, kappa >= 0, k + kappa + 1 <= bits(p) - 1.
 *   masked_dev and r1_dev are arrays of their own.  The table is not written.
 * hb_sort_swap_mask, after the carry tree's root (hb_fxp_ltl_leaves, hb_fxp_carry_mask / hb_fxp_carry_combine over the opened c):
 *   u = 1 - [key_lo < key_hi], the HB_FXP_NEG_TRUNC result of hb_fxp_div2m_finish on (d, c, r1, carry) at m = k - 1 mapped to 1 - b and
 *   not stored; out_dev rows 2w, 2w + 1 = u - p_w, (table[w][lo] - table[w][hi]) - q_w for w < width: the layer's second array to open,
 *   [2 width][slots].  p_dev, q_dev [width][slots]: the first and second factors of one triple a slot and column.  inv2m_host: ONE
 *   canonical element in host memory, 2^(-(k-1)) mod p.  Equal keys give u = 1.  out_dev is an array of its own; the table is not written.
 * hb_sort_swap_finish: opened_dev = that array opened; for every slot and column m = de + dq + ep + pq (hb_ew_beaver), then
 *   table[w][lo] -= m and table[w][hi] += m IN PLACE (safe: the layer is a matching).  Rows outside the layer's comparators are not
 *   written.  The table does not overlap the other arrays.
 * All are asynchronous on `stream`, one launch each, and allocate nothing.  cnt == 0 returns HB_OK and launches nothing. */
int hb_sort_cmp_mask(hb_ctx *ctx, const uint64_t *table_dev, int64_t n, int64_t batch, int a, int64_t r, int64_t d, int64_t cnt,
                     const uint64_t *bits_dev, int k, int kappa, uint64_t *masked_dev, uint64_t *r1_dev, void *stream);
int hb_sort_swap_mask(hb_ctx *ctx, const uint64_t *table_dev, int width, int64_t n, int64_t batch, int a, int64_t r, int64_t d, int64_t cnt,
                      const uint64_t *c_dev, const uint64_t *r1_dev, const uint64_t *carry_dev, const uint64_t *p_dev, const uint64_t *q_dev,
                      int k, const uint64_t *inv2m_host, uint64_t *out_dev, void *stream);
int hb_sort_swap_finish(hb_ctx *ctx, uint64_t *table_dev, int width, int64_t n, int64_t batch, int a, int64_t r, int64_t d, int64_t cnt,
                        const uint64_t *opened_dev, const uint64_t *p_dev, const uint64_t *q_dev, const uint64_t *pq_dev, void *stream);

/* ---- bit decomposition of shared values (hb_bd.hip) ------------------------------------------------------------------------
 * Shares of the low m bits of a signed k-bit value (Catrina and de Hoogh's BitDec on the masks above), for arrays of `count` values:
 * after the open of c = x + 2^(k-1) + r1 + 2^m r2 (hb_fxp_mask) they are the bits of c2 + (2^m - 1 - r1) + 1 mod 2^m, c2 = c mod 2^m
 * public, rows 0..m-1 of bits_dev the bit shares of r1.  A Sklansky prefix network over N = m - 1 (generate, propagate) planes, least
 * significant first, keeps every carry; arrays of several rows are row-major with `count` elements a row.
 * hb_bd_leaves: g_dev, p_dev [m - 1][count], row i from bit i of c and row i of bits_dev with no product: (1 - b_i, b_i) where the bit
 *   is set, (0, 1 - b_i) where it is not; the carry-in 1 is folded into row 0: (g_0 + p_0, 0).  m == 1: nothing is launched.
 * One level of the network (0 <= level < ceil(log2(m - 1))).  Node y = 0, 1, ... is row j = ((y >> level) << (level + 1)) |
 *   (1 << level) | (y & ((1 << level) - 1)) while j <= m - 2, its partner q = ((j >> level) << level) - 1, and (g_j, p_j) <-
 *   (g_j + p_j g_q, p_j p_q).  The nodes y < 2^level are g-only: one product, p_j is left as it is.  With G = min(2^level, nodes) the
 *   g-only node y uses triple row y, the full node y rows G + 2 (y - G) [p_j g_q] and G + 2 (y - G) + 1 [p_j p_q]; ta_dev, tb_dev,
 *   tab_dev hold this party's shares of the first factors, second factors and products, one row a triple.
 *   hb_bd_prefix_mask     masked_dev rows 2t, 2t + 1 = p_j - ta[t], (g_q | p_q) - tb[t]: the level's ONE array to open
 *   hb_bd_prefix_combine  opened_dev = that array opened; g_dev and p_dev are updated IN PLACE at the level's nodes, every other row is
 *                         left untouched.
 * The sum bits: s_0 = a_0 xor b_0, s_i = p_i + C_i - 2 p_i C_i with p_i the leaf's propagate of bit i (recomputed from c_dev and
 *   bits_dev) and C_i = row i - 1 of g_dev after the last level; triple row i - 1 for bit i.
 *   hb_bd_sum_mask        masked_dev rows 2t, 2t + 1 = p_{t+1} - ta[t], g[t] - tb[t], t < m - 1.  m == 1: nothing is launched.
 *   hb_bd_sum_combine     out_dev [m][count], row i this party's share of bit i; an array of its own.  m == 1: opened_dev, g_dev and the
 *                         triples are not looked at.
 * All are asynchronous on `stream`, one launch each, and allocate nothing.  HB_ERR_BAD_ARG before any launch: m outside 0 < m <=
 * bits(p) - 2, more than 256 planes, a level the network does not have, null pointers (with count > 0), a negative count, an output
 * that overlaps an input.  count == 0 returns HB_OK and launches nothing. */
int hb_bd_leaves(hb_ctx *ctx, const uint64_t *c_dev, const uint64_t *bits_dev, int m, uint64_t *g_dev, uint64_t *p_dev, int64_t count, void *stream);
int hb_bd_prefix_mask(hb_ctx *ctx, const uint64_t *g_dev, const uint64_t *p_dev, int m, int level, const uint64_t *ta_dev, const uint64_t *tb_dev,
                      uint64_t *masked_dev, int64_t count, void *stream);
int hb_bd_prefix_combine(hb_ctx *ctx, const uint64_t *opened_dev, uint64_t *g_dev, uint64_t *p_dev, int m, int level, const uint64_t *ta_dev,
                         const uint64_t *tb_dev, const uint64_t *tab_dev, int64_t count, void *stream);
int hb_bd_sum_mask(hb_ctx *ctx, const uint64_t *c_dev, const uint64_t *bits_dev, const uint64_t *g_dev, int m, const uint64_t *ta_dev,
                   const uint64_t *tb_dev, uint64_t *masked_dev, int64_t count, void *stream);
int hb_bd_sum_combine(hb_ctx *ctx, const uint64_t *opened_dev, const uint64_t *c_dev, const uint64_t *bits_dev, const uint64_t *g_dev, int m,
                      const uint64_t *ta_dev, const uint64_t *tb_dev, const uint64_t *tab_dev, uint64_t *out_dev, int64_t count, void *stream);

/* ---- one-hot demultiplexer of shared index bits (hb_demux.hip) ---------------------------------------------------------------
 * From this party's shares of the m bits of an index s = sum_i 2^i b_i (rows of bits_dev, least significant first, 1 <= m <= 12),
 * shares of e_j = [s == j], j < 2^m, for arrays of `count` indices; arrays of several rows are row-major with `count` elements a row.
 * Level 0 starts from m groups of width 1; a level merges the groups (0, 1), (2, 3), .. counted from the least significant by a Beaver
 * outer product -- a low group of wl bits with one-hot vector A and a high group of wh bits with vector B give
 * out[hi 2^wl + lo] = A[lo] B[hi] -- and carries an odd last group unchanged: ceil(log2 m) levels.  A width-1 group is never stored, its
 * vector (1 - b, b) is read from the bit plane.  Merged groups live in groups_dev, [sum over the levels of their products][count]: a
 * level writes its merges in order from the row where the levels before it ended, and the last level's 2^m rows are the result.
 * hb_demux_leaves  m == 1: out_dev [2][count] = (1 - b, b).
 * hb_demux_mask    out_dev [sum (2^wl + 2^wh)][count], the level's ONE array to open: for each merge in order 2^wl rows A[lo] - P[lo],
 *                  then 2^wh rows B[hi] - Q[hi]; ta_dev holds this party's shares of P then Q in exactly that row order.  groups_dev may
 *                  be NULL at level 0 (every factor is a bit plane).
 * hb_demux_finish  opened_dev = that array opened, tab_dev [sum 2^(wl + wh)][count] the triples' products, merge by merge, row
 *                  hi 2^wl + lo = P[lo] Q[hi]: the level's rows of groups_dev = d_lo e_hi + d_lo Q_hi + e_hi P_lo + PQ.  Rows of other
 *                  levels are left untouched.
 * All are asynchronous on `stream`, one launch each, and allocate nothing.  HB_ERR_BAD_ARG before any launch: m outside 1 .. 12, a
 * level the wiring does not have, null pointers (with count > 0), a negative count, an output that overlaps an input;
 * HB_ERR_UNSUPPORTED: a batch too large for one launch.  count == 0 returns HB_OK and launches nothing. */
int hb_demux_leaves(hb_ctx *ctx, const uint64_t *bits_dev, uint64_t *out_dev, int64_t count, void *stream);
int hb_demux_mask(hb_ctx *ctx, const uint64_t *bits_dev, const uint64_t *groups_dev, int m, int level, const uint64_t *ta_dev, uint64_t *out_dev,
                  int64_t count, void *stream);
int hb_demux_finish(hb_ctx *ctx, const uint64_t *opened_dev, const uint64_t *ta_dev, const uint64_t *tab_dev, int m, int level, uint64_t *groups_dev,
                    int64_t count, void *stream);

/* ---- division of shared fixed-point numbers by a shared divisor (hb_div.hip) ----------------------------------------------
 * Catrina and Saxena's FPDiv / AppRcr / Norm for signed k-bit values with f fractional bits, for arrays of `count` values; everything
 * between two opens is one launch.  Operands and results are canonical residues; arrays of several rows are row-major with `count`
 * elements a row; ta_dev, tb_dev, tab_dev hold this party's shares of the first factors, second factors and products, one row a triple.
 * One level of a Sklansky prefix OR over n_planes planes (0 <= level < ceil(log2 n_planes)), the wiring of hb_bd_prefix_*: node t is
 *   network plane j = ((t >> level) << (level + 1)) | (1 << level) | (t & ((1 << level) - 1)) while j <= n_planes - 1, its partner
 *   q = ((j >> level) << level) - 1, and y_j <- y_j + y_q - [y_j y_q]: one triple a node, triple row t for node t.  from_top != 0:
 *   network plane r is row n_planes - 1 - r of y_dev, so row i ends as the OR of rows i and above; else row r, the OR of rows r and below.
 *   hb_div_or_mask     masked_dev rows 2t, 2t + 1 = y_j - ta[t], y_q - tb[t]: the level's ONE array to open
 *   hb_div_or_combine  opened_dev = that array opened; y_dev is updated IN PLACE at the level's nodes, every other row is left untouched
 * hb_div_pair_mask: masked_dev rows 0, 1 = x - ta, y - tb (one row each): the masked pair of ONE product [x y] as one array to open.
 * hb_div_norm_mask: y_dev the prefix OR from the top of the bits of x.  v_dev = sum_i 2^(n_planes-1-i) (y_i - y_{i+1}) (no product), and
 *   masked_dev rows 0, 1 = x - ta[0], v - tb[0] and, with u_dev (the sign bit; NULL: unsigned), rows 2, 3 = u - ta[1], v - tb[1].
 * hb_div_product_step: opened_dev [2 products][count] the masked pairs opened.  Beaver-combines them, applies the step's affine map and
 *   writes what the next open needs:
 *     HB_DIV_SIGN   products = 1 [u b], aux_dev = b: out0 = b - 2 [u b]
 *     HB_DIV_NORM   products = 2 [x v], [u v] (or 1: unsigned), aux_dev = v: c = [x v], v' = v - 2 [u v] (unsigned: v).  With nxt_a_dev and
 *                   nxt_b_dev (the next triple's factors, one row each) and cst_host = alpha': out0 rows 0, 1 = (alpha' - 2 c) - nxt_a,
 *                   v' - nxt_b; with both NULL: out0 rows 0, 1 = c, v'.
 *     HB_DIV_FIRST  products = 2 [b w], [a w], cst_host = alpha = 2^(2f): out1 row 1 = alpha - [b w]; Y = [a w] is masked for truncation:
 *                   out0 row 0 = Y + 2^(width-1) + r1 + 2^m r2, out1 row 0 = Y + r1, from bits_dev [width + kappa][count]
 *     HB_DIV_TRUNC  products = 1 or 2: product r is masked for truncation from rows r (width + kappa) .. of bits_dev: out0 row r the masked
 *                   value, out1 row r = product + r1
 *   The masks are hb_fxp_mask's and width, m, kappa are checked as it checks k, m, kappa.  cst_host: one element in host memory.
 * hb_div_trunc_step: opened_dev, s_dev [rows][count] the masked values opened and the kept product + r1; t_r = (s_r - (opened_r mod 2^m))
 *   2^(-m), inv2m_host = 2^(-m) mod p (one element in host memory).
 *     HB_DIV_T_RESULT  rows = 1, products = 0: out = t_0
 *     HB_DIV_T_RECIP   rows = 1, products = 2: out rows 0..3 = ext0 - ta[0], t_0 - tb[0], ext1 - ta[1], t_0 - tb[1]
 *     HB_DIV_T_GOLD    x = t_1 (rows = 2) or x_dev (rows = 1); alpha_host = 2^(2f): out rows 0, 1 = t_0 - ta[0], alpha + x - tb[0] and, with
 *                      products = 2, rows 2, 3 = x - ta[1], x - tb[1]
 * All are asynchronous on `stream`, one launch each, and allocate nothing.  HB_ERR_BAD_ARG before any launch: an unknown mode, counts a
 * mode does not take, a level the network does not have, more than 256 planes, a truncation the modulus has no room for, a constant
 * not below the modulus, null pointers (with count > 0), a negative count, an output that overlaps an input or another output.
 * count == 0 returns HB_OK and launches nothing. */
#define HB_DIV_SIGN 0
#define HB_DIV_NORM 1
#define HB_DIV_FIRST 2
#define HB_DIV_TRUNC 3
#define HB_DIV_T_RESULT 0
#define HB_DIV_T_RECIP 1
#define HB_DIV_T_GOLD 2
int hb_div_pair_mask(hb_ctx *ctx, const uint64_t *x_dev, const uint64_t *y_dev, const uint64_t *ta_dev, const uint64_t *tb_dev, uint64_t *masked_dev,
                     int64_t count, void *stream);
int hb_div_or_mask(hb_ctx *ctx, const uint64_t *y_dev, int n_planes, int level, int from_top, const uint64_t *ta_dev, const uint64_t *tb_dev,
                   uint64_t *masked_dev, int64_t count, void *stream);
int hb_div_or_combine(hb_ctx *ctx, const uint64_t *opened_dev, uint64_t *y_dev, int n_planes, int level, int from_top, const uint64_t *ta_dev,
                      const uint64_t *tb_dev, const uint64_t *tab_dev, int64_t count, void *stream);
int hb_div_norm_mask(hb_ctx *ctx, const uint64_t *x_dev, const uint64_t *y_dev, int n_planes, const uint64_t *u_dev, const uint64_t *ta_dev,
                     const uint64_t *tb_dev, uint64_t *masked_dev, uint64_t *v_dev, int64_t count, void *stream);
int hb_div_product_step(hb_ctx *ctx, int mode, int products, const uint64_t *opened_dev, const uint64_t *ta_dev, const uint64_t *tb_dev,
                        const uint64_t *tab_dev, const uint64_t *aux_dev, const uint64_t *cst_host, const uint64_t *nxt_a_dev,
                        const uint64_t *nxt_b_dev, const uint64_t *bits_dev, int width, int m, int kappa, uint64_t *out0_dev, uint64_t *out1_dev,
                        int64_t count, void *stream);
int hb_div_trunc_step(hb_ctx *ctx, int mode, int rows, int products, const uint64_t *opened_dev, const uint64_t *s_dev, int m,
                      const uint64_t *inv2m_host, const uint64_t *alpha_host, const uint64_t *x_dev, const uint64_t *ext0_dev,
                      const uint64_t *ext1_dev, const uint64_t *ta_dev, const uint64_t *tb_dev, uint64_t *out_dev, int64_t count, void *stream);

/* ---- square root and inverse square root of shared fixed-point numbers (hb_fxsqrt.hip) -----------------------------------------
 * The steps of progs/fixedpoint_sqrt.py that the division does not already have, for arrays of `count` unsigned k-bit values with f
 * fractional bits (N = k - 1, beta = 2^N); the reference has no square root.  Operands and results are canonical residues; arrays of
 * several rows are row-major, [rows][count].  "Products to truncation mask" is hb_div_product_step(HB_DIV_TRUNC) and the last step
 * hb_div_trunc_step(HB_DIV_T_RESULT).
 * hb_fxsqrt_norm_mask: y_dev [n_planes][count] the prefix OR from the top of the bits of x; weights_dev [sets][n_planes] (sets = 1 or 2)
 *   the PUBLIC D_i = W_i - W_{i-1} mod p, one element each, the same for every element of the batch.  kept_dev [1 + sets][count] =
 *   v = sum_i 2^(n_planes-1-i) (y_i - y_{i+1}), then T_s = sum_i D_{s,i} y_i = sum_i W_{s,i} (y_i - y_{i+1}); masked_dev rows 0, 1 = x - ta,
 *   v - tb: the masked pair of [x v] as ONE array to open.
 * hb_fxsqrt_first: opened_dev [2][count] that pair opened; c = [x v] by the Beaver combine with (ta, tb, tab), y0 = a - b c with the
 *   constants a_host, b_host (one element each, host memory); h_dev = y0, masked_dev rows 0, 1 = c - nxt_a, y0 - nxt_b: the masked pair
 *   of [c y0] as ONE array to open.
 * hb_fxsqrt_trunc_step: opened_dev, s_dev [rows][count] the masked truncations opened and the kept product + r1; t_r = (s_r - (opened_r
 *   mod 2^m)) inv2m with inv2m_host = 2^(-m) (one element, host memory), and
 *     HB_FXSQRT_GH   rows = 2: (g, h) = (t_0, t_1); rows = 1: g = t_0, h = kept_in_dev [1][count].  which = 3.  kept_out_dev [2][count] =
 *                    g, h; masked_dev rows 0, 1 = g - ta, h - tb
 *     HB_FXSQRT_R    rows = 1, kept_in_dev [2][count] = g, h, cst_host = 3 beta: r = cst - t_0; which = 1: masked_dev = g - ta[0], r - tb[0];
 *                    which = 2: h - ta[0], r - tb[0]; which = 3: both pairs, g's first (rows 0..3, two triples)
 *     HB_FXSQRT_OUT  rows = 1 (which = 1 or 2) or 2 (which = 3), kept_in_dev [rows][count] the kept weights: masked_dev rows 2q, 2q + 1 =
 *                    t_q - ta[q], kept_in[q] - tb[q]
 * All are asynchronous on `stream`, one launch each, and allocate nothing.  HB_ERR_BAD_ARG before any launch: an unknown mode, counts a
 * mode does not take, more than 256 planes, m outside 0 < m <= bits(p) - 2, a constant not below the modulus, null pointers (with
 * count > 0), a negative count, an output that overlaps an input or another output.  count == 0 returns HB_OK and launches nothing. */
#define HB_FXSQRT_GH 0
#define HB_FXSQRT_R 1
#define HB_FXSQRT_OUT 2
int hb_fxsqrt_norm_mask(hb_ctx *ctx, const uint64_t *x_dev, const uint64_t *y_dev, int n_planes, const uint64_t *weights_dev, int sets,
                        const uint64_t *ta_dev, const uint64_t *tb_dev, uint64_t *masked_dev, uint64_t *kept_dev, int64_t count, void *stream);
int hb_fxsqrt_first(hb_ctx *ctx, const uint64_t *opened_dev, const uint64_t *ta_dev, const uint64_t *tb_dev, const uint64_t *tab_dev,
                    const uint64_t *a_host, const uint64_t *b_host, const uint64_t *nxt_a_dev, const uint64_t *nxt_b_dev, uint64_t *masked_dev,
                    uint64_t *h_dev, int64_t count, void *stream);
int hb_fxsqrt_trunc_step(hb_ctx *ctx, int mode, int rows, int which, const uint64_t *opened_dev, const uint64_t *s_dev, int m,
                         const uint64_t *inv2m_host, const uint64_t *cst_host, const uint64_t *kept_in_dev, const uint64_t *ta_dev,
                         const uint64_t *tb_dev, uint64_t *masked_dev, uint64_t *kept_out_dev, int64_t count, void *stream);

/* ---- base-2 and natural exponential of shared fixed-point numbers (hb_fxexp.hip) --------------------------------------------------
 * The steps of progs/fixedpoint_exp.py that the demultiplexer and the division do not already have, for arrays of `count` values; the
 * reference has no exponential.  Operands and results are canonical residues; arrays of several rows are row-major, [rows][count].
 * The last truncation is hb_div_trunc_step(HB_DIV_T_RESULT).
 * hb_fxexp_finish_lookup_mask: n_groups (1 .. 8) groups of index bits whose LAST demultiplexer level was just opened.  desc_host holds 6
 *   ints a group: wl, wh, open_off, prod_off, table_off, slot.  The group's last merge joins a low factor of wl bits and a high one of wh
 *   bits (1 <= wl, wh; wl + wh <= 12); rows open_off .. of opened_dev and of ta_dev are the 2^wl low rows and then the 2^wh high rows of
 *   the level's opened array and of the triple's factors (hb_demux_mask's numbering), rows prod_off .. of tab_dev the 2^(wl + wh) triple
 *   products, elements table_off .. of tables_dev the group's PUBLIC table T (one element an entry, the same for every element of the
 *   batch).  F = sum_y T_y (d_lo e_hi + d_lo Q_hi + e_hi P_lo + PQ_y), y = hi 2^wl + lo: the table read at the one-hot vector, which is never
 *   written.  wl = 1, wh = 0 is a group of ONE bit: open_off is its plane of bits_dev, and F = T_0 + (T_1 - T_0) b.  kept_dev [kept_rows][count]
 *   row slot = F; for slot < 2 pairs also masked_dev [2 pairs][count] row slot = F - (slot even ? nxt_a : nxt_b)[slot / 2], nxt_a_dev,
 *   nxt_b_dev [pairs][count] the factors of the next triples.  Rows of kept and masked that no group of the call names are left alone.
 * hb_fxexp_products_trunc: 1 <= products <= 128.  opened_dev [2 products][count] the masked pairs opened, ta, tb, tab [products][count]:
 *   v_r by the Beaver combine, then its truncation mask from planes r (width + kappa) .. of bits_dev: masked_dev [products][count] =
 *   v_r + 2^(width-1) + r1 + 2^m r2 to open, s_dev [products][count] = v_r + r1.
 * hb_fxexp_tree_step: 1 <= rows <= 128.  opened_dev, s_dev [rows][count] as above: t_j = (s_j - (opened_j mod 2^m)) inv2m with inv2m_host =
 *   2^(-m) (one element, host memory).  The values are t_0 .. t_(rows-1) and, if carry_dev is not NULL, carry_dev [count] after them; pair
 *   q of them goes to masked_dev rows 2q, 2q + 1 = v_2q - ta[q], v_(2q+1) - tb[q], and an odd last value to kept_dev [count].
 * All are asynchronous on `stream`, one launch each, and allocate nothing.  HB_ERR_BAD_ARG before any launch: counts or widths outside the
 * ranges above, two groups in one slot, a slot at or above kept_rows, a truncation the modulus has no room for, a constant not below the
 * modulus, null pointers (with count > 0), a negative count, an output that overlaps an input or another output.  count == 0 returns
 * HB_OK and launches nothing. */
int hb_fxexp_finish_lookup_mask(hb_ctx *ctx, const uint64_t *bits_dev, const uint64_t *opened_dev, const uint64_t *ta_dev, const uint64_t *tab_dev,
                                const uint64_t *tables_dev, int n_groups, const int *desc_host, const uint64_t *nxt_a_dev, const uint64_t *nxt_b_dev,
                                int pairs, uint64_t *masked_dev, uint64_t *kept_dev, int kept_rows, int64_t count, void *stream);
int hb_fxexp_products_trunc(hb_ctx *ctx, int products, const uint64_t *opened_dev, const uint64_t *ta_dev, const uint64_t *tb_dev,
                            const uint64_t *tab_dev, const uint64_t *bits_dev, int width, int m, int kappa, uint64_t *masked_dev, uint64_t *s_dev,
                            int64_t count, void *stream);
int hb_fxexp_tree_step(hb_ctx *ctx, int rows, const uint64_t *opened_dev, const uint64_t *s_dev, int m, const uint64_t *inv2m_host,
                       const uint64_t *carry_dev, const uint64_t *ta_dev, const uint64_t *tb_dev, uint64_t *masked_dev, uint64_t *kept_dev,
                       int64_t count, void *stream);

/* ---- base-2, natural and public-base logarithm of shared fixed-point numbers (hb_fxlog.hip) --------------------------------------
 * The steps of progs/fixedpoint_log.py that the division, the square root and the exponential do not already have, for arrays of
 * `count` unsigned k-bit values with f fractional bits (N = k - 1, beta = 2^N); the reference has no logarithm.  Operands and results
 * are canonical residues; arrays of several rows are row-major, [rows][count].  The scale step is hb_fxsqrt_norm_mask with the weights
 * of the integer part and of Y = beta [x != 0]; "products to truncation masks" is hb_fxexp_products_trunc.  A polynomial of degree d, 2
 * <= d <= 64, in t = 4 c - 3 Y is evaluated from the powers t^1 .. t^d, power j in row j - 1 of powers_dev [d][count]; level l = 1 ..
 * ceil(log2 d) forms the powers half < j <= min(2 half, d), half = 2^(l-1), product q of it being [t^half t^(q+1)].
 * hb_fxlog_first: opened_dev [2][count] the masked pair of [x v] opened; c = [x v] by the Beaver combine with (ta, tb, tab), t = 4 c -
 *   3 ybig; row 0 of powers_dev = t, masked_dev rows 0, 1 = t - nxt_a, t - nxt_b: the masked pair of [t t] as ONE array to open.
 * hb_fxlog_level: 1 <= level < ceil(log2 d).  opened_dev, s_dev [n][count], n the powers of `level`: the masked truncations opened
 *   and the kept product + r1; power half + 1 + q = (s_q - (opened_q mod 2^m)) inv2m with inv2m_host = 2^(-m) (one element, host memory)
 *   goes to row half + q of powers_dev, and masked_dev rows 2q, 2q + 1 = t^(2 half) - ta[q], t^(q+1) - tb[q] for the products of level
 *   + 1 (ta, tb one row a product).  Rows below half of powers_dev are read.
 * hb_fxlog_poly_mask: after the LAST level's open; opened_dev, s_dev, m_in, inv2m_host as above for that level, powers_dev rows below
 *   its half read.  L = coef[0] ybig + sum_{j=1..d} coef[j] t^j with coef_dev [d + 1] PUBLIC, one element each, the same for every
 *   element of the batch; bits_dev [width + kappa][count]: masked_dev = L + 2^(width-1) + r1 + 2^m_out r2 to open, s_out_dev = L + r1.
 * hb_fxlog_finish: out = (s - (opened mod 2^m)) inv2m + ipart.
 * All are asynchronous on `stream`, one launch each, and allocate nothing.  HB_ERR_BAD_ARG before any launch: d or level outside the
 * ranges above, m outside 0 < m <= bits(p) - 2, a truncation the modulus has no room for, a constant not below the modulus, null
 * pointers (with count > 0), a negative count, an output that overlaps an input or another output.  count == 0 returns HB_OK and
 * launches nothing. */
int hb_fxlog_first(hb_ctx *ctx, const uint64_t *opened_dev, const uint64_t *ta_dev, const uint64_t *tb_dev, const uint64_t *tab_dev,
                   const uint64_t *ybig_dev, const uint64_t *nxt_a_dev, const uint64_t *nxt_b_dev, uint64_t *masked_dev, uint64_t *powers_dev,
                   int64_t count, void *stream);
int hb_fxlog_level(hb_ctx *ctx, int level, int d, const uint64_t *opened_dev, const uint64_t *s_dev, int m, const uint64_t *inv2m_host,
                   const uint64_t *ta_dev, const uint64_t *tb_dev, uint64_t *masked_dev, uint64_t *powers_dev, int64_t count, void *stream);
int hb_fxlog_poly_mask(hb_ctx *ctx, int d, const uint64_t *opened_dev, const uint64_t *s_dev, int m_in, const uint64_t *inv2m_host,
                       const uint64_t *powers_dev, const uint64_t *ybig_dev, const uint64_t *coef_dev, const uint64_t *bits_dev, int width,
                       int m_out, int kappa, uint64_t *masked_dev, uint64_t *s_out_dev, int64_t count, void *stream);
int hb_fxlog_finish(hb_ctx *ctx, const uint64_t *opened_dev, const uint64_t *s_dev, int m, const uint64_t *inv2m_host,
                    const uint64_t *ipart_dev, uint64_t *out_dev, int64_t count, void *stream);

/* ---- sine and cosine of shared fixed-point numbers (hb_fxtrig.hip) ----------------------------------------------------------------
 * The steps of progs/fixedpoint_trig.py that the demultiplexer and the exponential do not already have, for arrays of `count` values;
 * the reference has no circular functions.  Operands and results are canonical residues; arrays of several rows are row-major,
 * [rows][count].  A complex value is two rows, re (the cosine side) and then im.  A MODE says which components a level of the product
 * tree keeps and how many triples a complex product takes: 0, both, THREE (Karatsuba: p0 = a.re b.re, p1 = a.im b.im, p2 = (a.re + a.im)
 * (b.re + b.im); re = p0 - p1, im = p2 - p0 - p1); 1, re alone, the first TWO of them (re = p0 - p1); 2, im alone, all
 * THREE (im = p2 - p0 - p1): a component kept alone is, share for share, the one kept beside the other.  With tp triples a product, triple r = tp q + t of product q takes rows 2 r and 2 r + 1 of a
 * masked array [2 tp products][count]: operand a's value minus ta[r], operand b's minus tb[r] (hb_fxexp_products_trunc's convention);
 * the values are re, im and (modes 0 and 2) re + im.
 * hb_fxtrig_finish_lookup_mask: hb_fxexp_finish_lookup_mask's descriptors and operands; entries table_off .. of tables_dev are the group's
 *   cos table, 2^(wl + wh) entries, and right after it its sin table, both read through the SAME one-hot vector in one pass over opened,
 *   ta and tab.  Entries are signed: any canonical residue; one whose negative has fewer digits costs those.  A group of ONE bit (wl = 1,
 *   wh = 0) has four entries C0, C1, S0, S1.  kept_dev [2 kept_slots][count] rows 2 slot, 2 slot + 1 = re, im; for slot < 2 pairs the value
 *   is operand slot & 1 of product slot / 2 of a level in `mode` and its masked rows go to masked_dev [2 tp pairs][count] against
 *   nxt_a_dev, nxt_b_dev [tp pairs][count].  split = 1, 2, 4, 8 or 16: the lanes an element's high indices are dealt to, summed across
 *   the lanes at the end; every split gives the same bits.  Rows that no group of the call names are left alone.
 * hb_fxtrig_cproducts_trunc: 1 <= products <= 64 complex products in `mode`.  opened_dev [2 tp products][count] the masked operands
 *   opened, ta, tb, tab [tp products][count]; the kept components v (comps = 2 in mode 0, else 1; row comps q + c) and their truncation
 *   masks from planes row (width + kappa) .. of bits_dev: masked_dev [comps products][count] = v + 2^(width-1) + r1 + 2^m r2 to open,
 *   s_dev likewise = v + r1.
 * hb_fxtrig_tree_step: opened_dev, s_dev [rows][count], 1 <= rows <= 128: t_j = (s_j - (opened_j mod 2^m)) inv2m with inv2m_host = 2^(-m)
 *   (one element, host memory).  final = 1: kept_dev [rows][count] = t, the results; no carry.  final = 0: rows is even, the complex
 *   values are (t_0, t_1), (t_2, t_3) .. and, if carry_dev is not NULL, carry_dev [2][count] after them; value u is operand u & 1 of
 *   product u / 2 of the next level, whose mode is `mode`: its masked rows go to masked_dev against ta_dev, tb_dev [tp pairs][count], and
 *   an odd last value to kept_dev [2][count].
 * All are asynchronous on `stream`, one launch each, and allocate nothing.  HB_ERR_BAD_ARG before any launch: counts, widths, a mode or
 * a split outside the ranges above, two groups in one slot, a slot at or above kept_slots, a truncation the modulus has no room for, a
 * constant not below the modulus, null pointers (with count > 0), a negative count, an output that overlaps an input or another
 * output.  count == 0 returns HB_OK and launches nothing. */
int hb_fxtrig_finish_lookup_mask(hb_ctx *ctx, const uint64_t *bits_dev, const uint64_t *opened_dev, const uint64_t *ta_dev, const uint64_t *tab_dev,
                                 const uint64_t *tables_dev, int n_groups, const int *desc_host, const uint64_t *nxt_a_dev, const uint64_t *nxt_b_dev,
                                 int pairs, int mode, int split, uint64_t *masked_dev, uint64_t *kept_dev, int kept_slots, int64_t count, void *stream);
int hb_fxtrig_cproducts_trunc(hb_ctx *ctx, int products, int mode, const uint64_t *opened_dev, const uint64_t *ta_dev, const uint64_t *tb_dev,
                              const uint64_t *tab_dev, const uint64_t *bits_dev, int width, int m, int kappa, uint64_t *masked_dev, uint64_t *s_dev,
                              int64_t count, void *stream);
int hb_fxtrig_tree_step(hb_ctx *ctx, int rows, int final, const uint64_t *opened_dev, const uint64_t *s_dev, int m, const uint64_t *inv2m_host,
                        const uint64_t *carry_dev, int mode, const uint64_t *ta_dev, const uint64_t *tb_dev, uint64_t *masked_dev, uint64_t *kept_dev,
                        int64_t count, void *stream);

/* ---- arctangent and atan2 of shared fixed-point numbers (hb_fxatan.hip) -----------------------------------------------------------
 * The steps of progs/fixedpoint_atan.py between the opens of the comparison, the division and hb_fxexp_products_trunc, for arrays of
 * `count` pairs (y, x) of signed k-bit values with f fractional bits (N = k - 1, beta = 2^N); the reference has no arctangent.  Operands
 * and results are canonical residues; arrays of several rows are row-major, [rows][count].  A sign bit s stands for sigma = 1 - 2 s.
 * An odd polynomial of degree d, 3 <= d <= 63 odd, J = (d - 1) / 2, in t = 2^shift q is evaluated from the odd powers t^(2j+1), row j of
 * powers_dev [J + 1][count], and the squares u^(2^l), u = [t t]: level 0 forms u; level l = 1 .. levels = bit_length(J) forms t^(2j+1),
 * 2^(l-1) <= j < min(2^l, J + 1), as [t^(2j+1-2^l) u^(2^(l-1))] (product q = j - 2^(l-1)) and, last and only if l < levels, u^(2^l) =
 * [u^(2^(l-1)) u^(2^(l-1))]; every product is truncated by N bits.
 * hb_fxatan_sign_mask: s_dev [2][count] = (sx, sy); masked_dev [6][count] = sx - ta[0], x - tb[0], sy - ta[1], y - tb[1], sigma_y - ta[2],
 *   sx - tb[2]: the masked pairs of [sx x], [sy y] and g = [sigma_y sx] as ONE array to open.
 * hb_fxatan_abs: opened_dev [6][count] that array opened, ta, tb, tab [3][count]; |x| = x - 2 [sx x], |y| = y - 2 [sy y], g, w = |x| - |y|;
 *   bits_dev [k + kappa][count]: masked_dev [1][count] = w + 2^(k-1) + r1 + 2^(k-1) r2, the comparison's array to open; kept_dev
 *   [5][count] = |x|, |y|, g, w, r1.
 * hb_fxatan_select_mask: c = [w < 0]; masked_dev [4][count] = c - ta[0], w - tb[0], sigma_c - ta[1], sigma_x - tb[1].
 * hb_fxatan_select: opened_dev [4][count], ta, tb, tab [2][count]; out_dev [3][count] = num = |y| + [c w], den = |x| - [c w], e1 =
 *   [sigma_c sigma_x].
 * hb_fxatan_first: t = 2^shift q, 0 <= shift <= 255; row 0 of powers_dev = t; masked_dev [4][count] = t - ta[0], t - tb[0], sigma_y -
 *   ta[1], e1 - tb[1]: the masked pairs of [t t] and E = [sigma_y e1].
 * hb_fxatan_level: 0 <= level < levels.  opened_dev, s_dev [n][count], n the products of `level`: the masked truncations opened and the
 *   kept product + r1, truncated as (s - (opened mod 2^m)) inv2m with inv2m_host = 2^(-m) (one element, host memory); the odd powers go
 *   to their rows of powers_dev, and masked_dev rows 2q, 2q + 1 are the masked pair of product q of level + 1 against ta[q], tb[q].
 * hb_fxatan_poly_mask: after the LAST level's open; L = sum_{j=0..J} coef[j] t^(2j+1) with coef_dev [J + 1] PUBLIC, one element each;
 *   bits_dev [width + kappa][count]: masked_dev = L + 2^(width-1) + r1 + 2^m_out r2 to open, s_out_dev = L + r1.
 * hb_fxatan_assemble: a = (s - (opened mod 2^m)) inv2m; E = [sigma_y e1] from eopened_dev [2][count] (rows 2, 3 of the first step's array,
 *   opened) and its triple (ea, eb, eab); masked_dev [2][count] = E - ta, a - tb; c_dev = A g + B (sigma_y - E), cst_host = (A, B), two
 *   elements in host memory.
 * hb_fxatan_finish: out = c + [E a] by the Beaver combine of opened_dev [2][count] with (ta, tb, tab).
 * All are asynchronous on `stream`, one launch each, and allocate nothing.  HB_ERR_BAD_ARG before any launch: d, level or shift outside
 * the ranges above, m outside 0 < m <= bits(p) - 2, a truncation the modulus has no room for, a constant not below the modulus, null
 * pointers (with count > 0), a negative count, an output that overlaps an input or another output.  count == 0 returns HB_OK and
 * launches nothing. */
int hb_fxatan_sign_mask(hb_ctx *ctx, const uint64_t *s_dev, const uint64_t *x_dev, const uint64_t *y_dev, const uint64_t *ta_dev,
                        const uint64_t *tb_dev, uint64_t *masked_dev, int64_t count, void *stream);
int hb_fxatan_abs(hb_ctx *ctx, const uint64_t *opened_dev, const uint64_t *ta_dev, const uint64_t *tb_dev, const uint64_t *tab_dev,
                  const uint64_t *x_dev, const uint64_t *y_dev, const uint64_t *bits_dev, int k, int kappa, uint64_t *masked_dev,
                  uint64_t *kept_dev, int64_t count, void *stream);
int hb_fxatan_select_mask(hb_ctx *ctx, const uint64_t *c_dev, const uint64_t *w_dev, const uint64_t *sx_dev, const uint64_t *ta_dev,
                          const uint64_t *tb_dev, uint64_t *masked_dev, int64_t count, void *stream);
int hb_fxatan_select(hb_ctx *ctx, const uint64_t *opened_dev, const uint64_t *ta_dev, const uint64_t *tb_dev, const uint64_t *tab_dev,
                     const uint64_t *ax_dev, const uint64_t *ay_dev, uint64_t *out_dev, int64_t count, void *stream);
int hb_fxatan_first(hb_ctx *ctx, const uint64_t *q_dev, int shift, const uint64_t *sy_dev, const uint64_t *e1_dev, const uint64_t *ta_dev,
                    const uint64_t *tb_dev, uint64_t *masked_dev, uint64_t *powers_dev, int64_t count, void *stream);
int hb_fxatan_level(hb_ctx *ctx, int level, int d, const uint64_t *opened_dev, const uint64_t *s_dev, int m, const uint64_t *inv2m_host,
                    const uint64_t *ta_dev, const uint64_t *tb_dev, uint64_t *masked_dev, uint64_t *powers_dev, int64_t count, void *stream);
int hb_fxatan_poly_mask(hb_ctx *ctx, int d, const uint64_t *opened_dev, const uint64_t *s_dev, int m_in, const uint64_t *inv2m_host,
                        const uint64_t *powers_dev, const uint64_t *coef_dev, const uint64_t *bits_dev, int width, int m_out, int kappa,
                        uint64_t *masked_dev, uint64_t *s_out_dev, int64_t count, void *stream);
int hb_fxatan_assemble(hb_ctx *ctx, const uint64_t *opened_dev, const uint64_t *s_dev, int m, const uint64_t *inv2m_host,
                       const uint64_t *eopened_dev, const uint64_t *ea_dev, const uint64_t *eb_dev, const uint64_t *eab_dev,
                       const uint64_t *sy_dev, const uint64_t *g_dev, const uint64_t *cst_host, const uint64_t *ta_dev, const uint64_t *tb_dev,
                       uint64_t *masked_dev, uint64_t *c_dev, int64_t count, void *stream);
int hb_fxatan_finish(hb_ctx *ctx, const uint64_t *opened_dev, const uint64_t *ta_dev, const uint64_t *tb_dev, const uint64_t *tab_dev,
                     const uint64_t *c_dev, uint64_t *out_dev, int64_t count, void *stream);

/* ---- equality of shared values (hb_eq.hip)---------------------------------------------------------------------------------
 * The Equality mixin of progs/mixins/share_comparison.py:9-80, the probabilistic Legendre-symbol test, for arrays of `count` pairs
 * and `rows` test bits a pair.  Everywhere: operands and results are canonical residues; preprocessing arrives as planes, rows of
 * `count` elements, row j holding test bit j's value of every element; arrays of several rows are row-major.  Test bit j opens
 * c = diff r + _b rp^2 with _b = nr - (nr - 1) b, nr a public quadratic non-residue (that it is one is the caller's business), and its
 * factor is affine in [b] with coefficients chosen by L = legendre(c).
 * hb_legendre: out_dev[i] = legendre(a_i) in {-1, 0, 1}, one int8 an element: a^((p-1)/2) by a sliding-window chain whose schedule
 *   is derived from p on the host and is the same for every lane.  A zero element gives 0 without running the chain.
 * hb_eq_mask1: diff = x - y (y_dev == NULL: diff = x).  masked_dev [4][rows][count] = diff - pa, r - qa, rp - pb, rp - qb: the ONE
 *   array to open before the products diff r (triple a) and rp rp (triple b).  masked_dev is an array of its own.
 * hb_eq_mid: opened_dev = that array opened.  dr_dev [rows][count] = [diff r], masked2_dev [2][rows][count] = _b - pc, [rp^2] - qc:
 *   the array to open before the product _b rp^2 (triple c).  nr_host: ONE canonical element in host memory (0, 1 or not below the
 *   modulus: HB_ERR_BAD_ARG).  The outputs are arrays of their own.
 * hb_eq_cshare: opened2_dev = masked2 opened.  c_dev [rows][count] = [diff r] + [_b rp^2], the third array to open; c_dev may be dr_dev.
 * hb_eq_finish: c_dev = that array opened.  factor_dev [rows][count]:
 *   HB_EQ_BIT        (1 - L) / 2 + L [b]: a share of 1 (the bit agrees with "equal") or 0; nr_host is not read
 *   HB_EQ_REFERENCE  L (nr + L) / 2 - (L (nr - 1) / 2) [b]: the reference's (L / 2) (_b + L)
 *   c = 0 (L = 0): the factor written is 0 and zero_rows_dev[row] = 1; rows without a zero are not written, so the caller zeroes
 *   zero_rows_dev [rows] (int32) first.  factor_dev may be c_dev or bits_dev.
 * All are asynchronous on `stream`, one launch each, and allocate nothing.  1 <= rows <= 4096.  HB_ERR_BAD_ARG before any launch:
 * null pointers (with count > 0), a negative count, parameters out of range.  count == 0 launches nothing. */
#define HB_EQ_BIT 0
#define HB_EQ_REFERENCE 1
int hb_legendre(hb_ctx *ctx, const uint64_t *a_dev, int8_t *out_dev, int64_t count, void *stream);
int hb_eq_mask1(hb_ctx *ctx, const uint64_t *x_dev, const uint64_t *y_dev, const uint64_t *r_dev, const uint64_t *rp_dev, const uint64_t *pa_dev,
                const uint64_t *qa_dev, const uint64_t *pb_dev, const uint64_t *qb_dev, uint64_t *masked_dev, int rows, int64_t count, void *stream);
int hb_eq_mid(hb_ctx *ctx, const uint64_t *opened_dev, const uint64_t *pa_dev, const uint64_t *qa_dev, const uint64_t *pqa_dev, const uint64_t *pb_dev,
              const uint64_t *qb_dev, const uint64_t *pqb_dev, const uint64_t *bits_dev, const uint64_t *pc_dev, const uint64_t *qc_dev,
              const uint64_t *nr_host, uint64_t *masked2_dev, uint64_t *dr_dev, int rows, int64_t count, void *stream);
int hb_eq_cshare(hb_ctx *ctx, const uint64_t *opened2_dev, const uint64_t *dr_dev, const uint64_t *pc_dev, const uint64_t *qc_dev,
                 const uint64_t *pqc_dev, uint64_t *c_dev, int rows, int64_t count, void *stream);
int hb_eq_finish(hb_ctx *ctx, const uint64_t *c_dev, const uint64_t *bits_dev, int mode, const uint64_t *nr_host, uint64_t *factor_dev,
                 int32_t *zero_rows_dev, int rows, int64_t count, void *stream);

/* ---- less-than of shared field elements (hb_lt.hip) ----------------------------------------------------------------------
 * The LessThan mixin of progs/mixins/share_comparison.py:83-212 (Reistad 2007) for arrays of `count` pairs a, b < (p - 1) / 2.
 * Everywhere: operands and results are canonical residues, L is the bit length of the modulus (anything else: HB_ERR_BAD_ARG), bit
 * shares arrive as planes [L][count], row i this party's shares of bit i (least significant first) of every element's mask; arrays
 * of several rows are row-major with `count` elements a row.  The protocol opens c = 2 (a - b) + r and [a < b] = c_0 xor r_0 xor
 * [r > c]; the tree between hb_lt_leaves and the steps after it is hb_fxp_carry_mask / hb_fxp_carry_combine over L rows.
 * hb_lt_mask: masked_dev[i] = 2 (a_i - b_i) + r_i, the array to open (b_dev == NULL: 2 a_i + r_i).
 * hb_lt_leaves: g_dev, p_dev [L][count], row j for bit i = L - 1 - j of the opened c against row i of r_bits_dev, no product:
 *   HB_LT_DIRECT     c_i = 0: (r_i, 1 - r_i); c_i = 1: (0, r_i).      The root's g is [r > c], a bit.
 *   HB_LT_REFERENCE  c_i = 0: (r_i, 1 + r_i); c_i = 1: (0, 2 - r_i).  The root's g is the reference's x (_compute_x, :137-163).
 * hb_lt_xor_mask (DIRECT, w_dev the root's g): u_dev[i] = c_0 ? 1 - r_0 : r_0 (r0_dev: row 0 of the bit planes) and masked_dev
 *   [2][count] = u - pa, w - qa, the array to open before the product u w.
 * hb_lt_dmask (REFERENCE, x_dev the root's g; s_dev, s_bits_dev the second mask and its bit planes): u_dev as above and masked_dev
 *   [5][count] = s + x, u - pa, s_0 - qa, s_1 - pb, s_2 - qb with s_0, s_1, s_2 rows 0, L - 1, L - 2 of s_bits_dev (:178-182): ONE
 *   array to open, d = s + x and the masked operands of u s_0 (triple a) and s_1 s_2 (triple b).
 * hb_lt_mid: opened_dev = that array opened.  v_dev = u + s_0 - 2 [u s_0], d0_dev = the reference's [d_0] (:186-199), masked_dev
 *   [2][count] = v - pc, d_0 - qc, the array to open before the product v d_0 (triple c).
 * hb_lt_xor_finish (both modes): opened_dev [2][count] = the last array opened; out = u + v - 2 [u v] with the triple (p, q, pq) whose
 *   factors masked u and v (REFERENCE: u_dev, v_dev are hb_lt_mid's v_dev, d0_dev).
 * All are asynchronous on `stream`, one launch each, and allocate nothing.  Every output is an array of its own: one that overlaps
 * an input or another output is HB_ERR_BAD_ARG, as are null pointers (with count > 0), a negative count and an unknown mode, before
 * any launch.  count == 0 returns HB_OK and launches nothing. */
#define HB_LT_DIRECT 0
#define HB_LT_REFERENCE 1
int hb_lt_mask(hb_ctx *ctx, const uint64_t *a_dev, const uint64_t *b_dev, const uint64_t *r_dev, uint64_t *masked_dev, int64_t count, void *stream);
int hb_lt_leaves(hb_ctx *ctx, const uint64_t *c_dev, const uint64_t *r_bits_dev, int L, int mode, uint64_t *g_dev, uint64_t *p_dev, int64_t count,
                 void *stream);
int hb_lt_xor_mask(hb_ctx *ctx, const uint64_t *c_dev, const uint64_t *r0_dev, const uint64_t *w_dev, const uint64_t *pa_dev, const uint64_t *qa_dev,
                   uint64_t *u_dev, uint64_t *masked_dev, int64_t count, void *stream);
int hb_lt_dmask(hb_ctx *ctx, const uint64_t *c_dev, const uint64_t *r0_dev, const uint64_t *x_dev, const uint64_t *s_dev, const uint64_t *s_bits_dev, int L,
                const uint64_t *pa_dev, const uint64_t *qa_dev, const uint64_t *pb_dev, const uint64_t *qb_dev, uint64_t *u_dev, uint64_t *masked_dev,
                int64_t count, void *stream);
int hb_lt_mid(hb_ctx *ctx, const uint64_t *opened_dev, const uint64_t *u_dev, const uint64_t *s_bits_dev, int L, const uint64_t *pa_dev,
              const uint64_t *qa_dev, const uint64_t *pqa_dev, const uint64_t *pb_dev, const uint64_t *qb_dev, const uint64_t *pqb_dev, const uint64_t *pc_dev,
              const uint64_t *qc_dev, uint64_t *v_dev, uint64_t *d0_dev, uint64_t *masked_dev, int64_t count, void *stream);
int hb_lt_xor_finish(hb_ctx *ctx, const uint64_t *opened_dev, const uint64_t *u_dev, const uint64_t *v_dev, const uint64_t *p_dev, const uint64_t *q_dev,
                     const uint64_t *pq_dev, uint64_t *out_dev, int64_t count, void *stream);

/* ---- the offline phase: RanDouSha, triples and random bits (hb_off.hip) -----------------------------------------------------
 * The local arithmetic of offline_randousha.py:34-232; the protocol itself is honeybadgermpc_amd/offline.py.  Operands and results are
 * canonical residues; every call is one launch, asynchronous on `stream`; count == 0 returns HB_OK and launches nothing; null
 * pointers (with count > 0), a negative count and an unknown mode are HB_ERR_BAD_ARG before any launch.
 * hb_off_mul_add: out[i] = a[i] b[i] + c[i] in one pass, the masked local product of both generators (a b + r_2t, u u + r_2t).
 *   b_dev may be a_dev and out_dev may be any of the inputs.
 * hb_off_invsqrt_scale: the finish of generate_bits.  x_dev holds the opened u^2, u_dev this party's shares, w(x) = x^(-1/2):
 *   HB_OFF_PM1  out = u w (a share of +-1, what the reference returns)      HB_OFF_01  out = (u w + 1) / 2 (a share of 0 or 1)
 *   u_dev == NULL: out = w.  With p - 1 = q 2^s and c = z^q for the smallest non-residue z >= 2, w = x^((q-1)/2) c^e for the unique
 *   e in [0, 2^(s-1)) with x^q c^(2e) = 1: the inverse of exactly the root hb_sqrt_mod returns.  status_dev is int32[2], zeroed by
 *   the caller: [0] += the number of x = 0, [1] += the number of non-residues; their outputs are 0 and the other elements are
 *   unaffected (the convention of hb_ew_inv).  The first call of a context builds a table of s elements and synchronises once.
 * hb_off_degree_check: the checkers' verdict.  coeffs_dev is [n][2k], coefficient-major: row e holds coefficient e of the k
 *   interpolated t-sharings, then of the k 2t-sharings (what one hb_matvec with the inverse Vandermonde matrix over the received
 *   [n][2k] block writes).  counters_dev is int32[3], zeroed by the caller: [0] += columns j < k whose polynomial is not of exact
 *   degree t (coefficient t zero, or any coefficient above it non-zero), [1] += the same for the 2t-sharings and degree 2t,
 *   [2] += columns whose two constant terms differ.  2 t < n, else HB_ERR_BAD_ARG. */
#define HB_OFF_PM1 0
#define HB_OFF_01 1
int hb_off_mul_add(hb_ctx *ctx, const uint64_t *a_dev, const uint64_t *b_dev, const uint64_t *c_dev, uint64_t *out_dev, int64_t count, void *stream);
int hb_off_invsqrt_scale(hb_ctx *ctx, const uint64_t *x_dev, const uint64_t *u_dev, int mode, uint64_t *out_dev, int64_t count, int32_t *status_dev,
                         void *stream);
int hb_off_degree_check(hb_ctx *ctx, const uint64_t *coeffs_dev, int n, int64_t k, int t, int32_t *counters_dev, void *stream);
/* Shared powers and cubes (hb_offpow.hip; offline.py generate_powers, generate_cubes): the two launches of one doubling level.
 * powers_dev holds the powers of `count` items: power e (1-based) of item c is element c item_stride + (e - 1) power_stride, strides
 * in elements and >= 1 -- (k, 1) is item-major, (1, count) power-major.  With powers 1 .. m held, level (m, w), 1 <= w <= m, makes
 * powers m + 1 .. m + w.  The masked, opened and mask arrays are contiguous, element c w + j for item c and product j < w.
 * hb_off_pow_mask:   out[c w + j] = P[c][m] P[c][j + 1] + r2t[c w + j]; powers_dev is only read.
 * hb_off_pow_finish: P[c][m + 1 + j] = opened[c w + j] - rt[c w + j]; nothing else of powers_dev is written.
 * HB_ERR_BAD_ARG before any launch: a null operand with count w > 0, count < 0, m < 1, w < 1, w > m, a stride below 1, strides under
 * which two cells of the count x (m + w) block share an element, out_dev over the block or over r2t_dev, opened_dev or rt_dev over
 * the written columns.  count == 0 returns HB_OK and launches nothing. */
int hb_off_pow_mask(hb_ctx *ctx, const uint64_t *powers_dev, int64_t item_stride, int64_t power_stride, const uint64_t *r2t_dev, int m, int w,
                    uint64_t *out_dev, int64_t count, void *stream);
int hb_off_pow_finish(hb_ctx *ctx, const uint64_t *opened_dev, const uint64_t *rt_dev, uint64_t *powers_dev, int64_t item_stride, int64_t power_stride,
                      int m, int w, int64_t count, void *stream);
/* Share bits (hb_offsb.hip; offline.py share_bits_round, generate_share_bits): a random residue shared with its bit planes, by rejection
 * of bitwise-shared candidates.  L is the bit length of the modulus; bits_dev holds planes [L][candidates], row i this party's shares
 * of bit i (least significant first) of every candidate r = sum_i 2^i b_i < 2^L.
 * hb_off_sb_leaves: g_dev, p_dev [L][count], row y for bit i = L - 1 - y of a PUBLIC bound against row i of bits_dev (count candidates),
 *   the HB_LT_DIRECT leaves of hb_lt_leaves: bound bit 0: (b, 1 - b); 1: (0, b).  The root's g of the carry tree over them is
 *   [r > bound].  bound_limbs: n_limbs limbs in HOST memory, below 2^L; NULL: p - 1, so that the root is [r >= p].  No array of the
 *   bound is read or made.
 * hb_off_sb_finish: for every output slot j < count with c = index_dev[j] (int64, device): r_bits_dev[q][j] = bits_dev[q][c] for every
 *   plane q, and r_dev[j] = sum_q 2^q bits_dev[q][c] mod p, in one pass over the planes.  An index outside [0, candidates) is never
 *   used as an address: that slot gets zeros in r_dev and in every plane.  Indices may repeat and come in any order.
 * One launch each, asynchronous on `stream`, no allocation.  HB_ERR_BAD_ARG before any launch: a null operand where there is work,
 * a negative count or candidates, L not the bit length of the modulus, a bound of 2^L or more, an output over an input or over the
 * other output.  count == 0 returns HB_OK and launches nothing. */
int hb_off_sb_leaves(hb_ctx *ctx, const uint64_t *bits_dev, int L, const uint64_t *bound_limbs, uint64_t *g_dev, uint64_t *p_dev, int64_t count,
                     void *stream);
int hb_off_sb_finish(hb_ctx *ctx, const uint64_t *bits_dev, int L, int64_t candidates, const int64_t *index_dev, uint64_t *r_dev, uint64_t *r_bits_dev,
                     int64_t count, void *stream);

/* ---- products of share matrices (hb_mat.hip) --------------------------------------------------------------------------------
 * hb_mat_mul: out[b] = A[b] B[b] (op) C[b] for b < batch; A is m x k, B is k x n, C and out are m x n, all row-major packed canonical
 * residues, batches back to back.  op: HB_MAT_NONE (c_dev is not read), HB_MAT_ADD (A B + C), HB_MAT_SUB (A B - C): the epilogue is
 * part of the launch.  Asynchronous on `stream`.  batch, m or n equal to 0 launches nothing; k == 0 gives 0 (op) C.  out_dev may be
 * c_dev.  HB_ERR_BAD_ARG before any launch: out_dev equal to a_dev or b_dev, a null pointer with a non-empty shape, a negative size,
 * an unknown c_op, c_dev == NULL with c_op != HB_MAT_NONE.
 * One launch and no allocation, except when the output gives at most 64 workgroups (tiles of 16 x 32 over all batches) and
 * k >= 2048: then the inner dimension is cut into slices, a first launch writes partial products to a scratch slot kept with the
 * context per stream and a second adds them and applies the epilogue, both on `stream`.  That slot never exceeds 512 tiles:
 * 8 MiB for 32-byte elements, 2 MiB for 8-byte ones; it goes with hb_ctx_cache_clear and with the context.  The result is the same
 * bit for bit either way.
 * hb_mat_constants: out[0..HB_MAT_CONSTANTS) = tile rows, tile columns, tile depth, products between two carry passes, products
 * between two reductions (both for the element width n_limbs), and the split rule: least k, most workgroups, target workgroups. */
#define HB_MAT_NONE 0
#define HB_MAT_ADD  1
#define HB_MAT_SUB  2
#define HB_MAT_CONSTANTS 8
int hb_mat_mul(hb_ctx *ctx, const uint64_t *a_dev, const uint64_t *b_dev, const uint64_t *c_dev, int c_op,
               uint64_t *out_dev, int64_t batch, int m, int k, int n, void *stream);
int hb_mat_constants(int n_limbs, int32_t *out);

/* ---- the robust path of IncrementalDecoder without plans (hb_quick.hip)-------------------------------------------
 * A decoder that is working its way past faulty senders sees every arrival set once: these entry points build what they
 * need on the device and enqueue it; none of them creates tables on the host. */
/* decoder.decode_batch over the arrivals z[0..d) + encoder.encode_batch + the compare loop with the later arrivals zc[0..nc)
 * (reed_solomon.py:305-326) as one launch: cols_dev is the party-major buffer [n][C] (row j = what party j sent), x_host the n
 * party points; coefficients go chunk-major to coeffs_dev ((C, d) elements; NULL: validate only).  On a disagreement
 * status_dev[0] |= 1 and status_dev[1] = min(status_dev[1], first disagreeing chunk - chunk_lo); the caller initialises both (0, INT32_MAX)
 * and reads them after synchronising.  Only the chunks [chunk_lo, chunk_hi) are read, written and compared (a decoder that has accepted
 * its first polynomials goes on from there).  z and zc are disjoint party indices.  Asynchronous.  HB_ERR_UNSUPPORTED outside the
 * full-size matrix-core kernel's range (narrow contexts, p outside [2^254, 0x7f 2^248), d < 4 or > 128, repeated points):
 * callers use an open plan then. */
int hb_quick_interp_check(hb_ctx *ctx, const uint64_t *x_host, int n, const int32_t *z, int d, const int32_t *zc, int nc,
                          const uint64_t *cols_dev, int64_t C, int64_t chunk_lo, int64_t chunk_hi, uint64_t *coeffs_dev, int32_t *status_dev,
                          void *stream);
/* The same, and every disagreeing chunk rather than only the first: bit (c - chunk_lo) of bad_map_dev (uint32 words, at least
 * ceil((chunk_hi - chunk_lo + 31) / 32) + 1 of them, zeroed by the caller) is set for every chunk c some compared column disagrees on.
 * A decoder whose liars corrupt one late chunk each reads the whole list off one launch (reed_solomon.py:334-365 walks the
 * polynomials in order; the candidates of one interpolation set do not change when a COMPARED sender is expelled).
 * bad_map_dev = NULL: hb_quick_interp_check. */
int hb_quick_interp_check_map(hb_ctx *ctx, const uint64_t *x_host, int n, const int32_t *z, int d, const int32_t *zc, int nc,
                              const uint64_t *cols_dev, int64_t C, int64_t chunk_lo, int64_t chunk_hi, uint64_t *coeffs_dev, int32_t *status_dev,
                              uint32_t *bad_map_dev, void *stream);

/* The optimistic step of ONE IncrementalDecoder (reed_solomon.py:305-330) in two halves, on wide contexts (points that are small
 * integers -- the production points 1 .. n -- on the small-entry kernel, hb_mfma_fused.hip; any other point set on the full-size one
 * with hb_quick_interp_check's device-built image): what depends on the first d arrivals alone is built when the d-th column lands
 * (hb_quick_dec_arrivals: enqueued, nothing waited for), and when the last column lands hb_quick_dec_decide builds the rows of the
 * compared senders, launches decode + validate (hb_mfma_fused.hip) over chunks [chunk_lo, chunk_hi) of the party-major buffer and
 * WAITS for the verdict, which the kernel hands over in pinned memory: *flag != 0 -- some compared column disagrees, *first = the
 * first disagreeing chunk - chunk_lo (INT32_MAX when none).  n_coef = d: all coefficients go chunk-major to coeffs_dev ((C, d)
 * elements); n_coef = 1: only the constant terms, to coeffs_dev[0 .. C) (what R1 forwards, batch_reconstruction.py:194).
 * HB_ERR_UNSUPPORTED from _create / _arrivals (narrow contexts, repeated points, fewer than 4 coefficients, more than 128, moduli
 * outside the matrix-core kernels' range): use an open plan. */
typedef struct hb_quick_dec hb_quick_dec;
int hb_quick_dec_create(hb_ctx *ctx, const uint64_t *x_host, int n, hb_quick_dec **out, void *stream);
int hb_quick_dec_arrivals(hb_quick_dec *qd, const int32_t *z, int d, int nc, int n_coef, void *stream);
int hb_quick_dec_decide(hb_quick_dec *qd, const int32_t *zc, int nc, const uint64_t *cols_dev, int64_t C, int64_t chunk_lo, int64_t chunk_hi,
                        uint64_t *coeffs_dev, int32_t *flag, int32_t *first, void *stream);
/* hb_quick_dec_decide in its two halves: _launch enqueues (the compared senders' rows, decode + validate) and returns, _verdict waits for
 * the last launch's verdict.  Between the two the calling thread is free (the next round's decoder, the next messages). */
int hb_quick_dec_launch(hb_quick_dec *qd, const int32_t *zc, int nc, const uint64_t *cols_dev, int64_t C, int64_t chunk_lo, int64_t chunk_hi,
                        uint64_t *coeffs_dev, void *stream);
int hb_quick_dec_verdict(hb_quick_dec *qd, int32_t *flag, int32_t *first);
/* on: hb_quick_dec_arrivals enqueues its build on a stream of the decoder's own (the caller's stream is busy with something the build does
 * not depend on -- it reads no column) and the next launch waits for it; off (default): in order on the caller's stream */
int hb_quick_dec_beside(hb_quick_dec *qd, int on);
void hb_quick_dec_destroy(hb_quick_dec *qd);

/* ---- IncrementalDecoder's optimistic phase as an object (hb_dec.hip) ------------------------------------------------------------
 * Replaces, for one round of one open, the state machine of IncrementalDecoder.add (reed_solomon.py:367-403) up to its first verdict:
 * _validate / duplicate and confirmed-error filtering (:288-300, :369-372), the optimistic decode + re-encode from the first degree + 1
 * arrivals (:305-313), the comparison of the later arrivals (:316-326) and the quorum test degree + 1 + max_errors - |confirmed|
 * (:302-303, :328-330) -- as batch_reconstruct drives it, one add() per received message (batch_reconstruction.py:43-61).
 * The host announces arrivals BY INDEX: party idx's column has landed in row idx of the party-major buffer cols_dev [n][C].  The
 * object enqueues what depends on the first degree + 1 arrivals when the last of them is announced, launches decode + validate when
 * the quorum is complete and waits for the verdict (pinned memory; the stream is not synchronised).  A decoder object is reusable:
 * hb_dec_begin starts the next round (another buffer, another set of confirmed errors).
 *   n_coef = degree + 1: all coefficients, chunk-major (C, degree + 1) to coeffs_dev;  n_coef = 1: the constant terms only, (C) elements
 *   (what R1 forwards, batch_reconstruction.py:194).  excluded[0..n_excluded): senders confirmed in error before this round
 *   (their arrivals are ignored; each lowers the quorum by one).
 * hb_dec_create / hb_dec_begin return HB_ERR_UNSUPPORTED for contexts / point sets / shapes outside the plan-free kernels
 * (hb_quick_dec_*'s conditions; also max_errors - n_excluded < 1: nothing to compare) -- callers keep their own path for those. */
#define HB_DEC_COLLECTING 0   /* more columns needed */
#define HB_DEC_DONE 1         /* every compared column agreed: the results are in coeffs_dev */
#define HB_DEC_DISAGREE 2     /* a compared column differs from the guess (reed_solomon.py:321-326): the robust phase takes over from
                                 hb_dec_arrivals_list; with n_coef = degree + 1 the refuted guess is in coeffs_dev and hb_dec_verdict
                                 gives the first disagreeing chunk */
#define HB_DEC_UNSUPPORTED 3  /* found at the (degree + 1)-th arrival: decode the arrival list another way */
#define HB_DEC_PENDING 4      /* only with HB_DEC_OPT_DEFER: decode + validate is enqueued, its verdict not read yet (hb_dec_settle) */
typedef struct hb_dec hb_dec;
int hb_dec_create(hb_ctx *ctx, const uint64_t *x_host, int n, int degree, int max_errors, hb_dec **out, void *stream);
int hb_dec_begin(hb_dec *dec, const uint64_t *cols_dev, int64_t C, int n_coef, uint64_t *coeffs_dev, const int32_t *excluded, int n_excluded,
                 void *stream);
/* one arrival: returns the state (HB_DEC_*) after it, or -(hb_status) on an error.  A sender already counted or excluded is ignored;
 * so is every arrival once the state has left HB_DEC_COLLECTING.  The call that completes the quorum returns when the verdict is in. */
int hb_dec_arrived1(hb_dec *dec, int32_t idx);
/* Options of the rounds to come (they hold across hb_dec_begin):
 *   HB_DEC_OPT_DEFER   the arrival that completes the quorum enqueues decode + validate and returns HB_DEC_PENDING instead of waiting;
 *                      hb_dec_settle waits for that verdict and returns the state it leads to (HB_DEC_DONE / HB_DEC_DISAGREE; any other
 *                      state as it is; -(hb_status) on an error).  While the state is HB_DEC_PENDING further arrivals are NOT counted
 *                      (hb_dec_arrived1 returns HB_DEC_PENDING): the caller keeps them and, after a HB_DEC_DISAGREE, hands them to its
 *                      robust phase in order.  What batch_reconstruct gains: its two rounds are subscribed up front
 *                      (batch_reconstruction.py:158-176), so the next round's decoder can be made, and its first messages taken, while
 *                      this round's launch runs.
 *   HB_DEC_OPT_BESIDE  the caller's stream is busy while this round's columns come in (the open's encode; the previous round's launch):
 *                      what depends on the first degree + 1 arrivals is built on a stream of the decoder's own, beside that work, and
 *                      the decode launch waits for it (hb_quick_dec_beside).  On an idle stream the dependency between two queues costs
 *                      more than the build: leave it off there. */
#define HB_DEC_OPT_DEFER 1
#define HB_DEC_OPT_BESIDE 2
int hb_dec_options(hb_dec *dec, int flags);
int hb_dec_settle(hb_dec *dec);
/* a burst of arrivals in order; stops at the first one that changes the state (*consumed = how many were taken) */
int hb_dec_arrived(hb_dec *dec, const int32_t *idx, int count, int32_t *consumed, int32_t *state);
int hb_dec_verdict(const hb_dec *dec, int32_t *state, int32_t *first_bad);
/* the senders counted so far, in arrival order (reed_solomon.py's _z): *count of them, the first min(cap, *count) copied */
int hb_dec_arrivals_list(const hb_dec *dec, int32_t *out, int cap, int32_t *count);
void hb_dec_destroy(hb_dec *dec);

/* ---- a candidate's waiting phase (hb_dec.hip) ------------------------------------------------------------------------------------
 * IncrementalDecoder's robust phase (reed_solomon.py:334-346) accepts a robust decode only once |z| - |errors| >= degree + 1 + max_errors -
 * |confirmed| and otherwise waits with nothing changed.  A decoder that holds CANDIDATES for the polynomial that disagreed -- polynomials few
 * enough arrived senders contradict; device.py _candidate_cap proves that such a candidate decides the reference's verdicts -- has ONE question
 * per arrival until then: does the new sender's symbol of that chunk equal the candidate's value at its point?  This object asks it: it keeps
 * the candidates' values at the n points (host), fetches the new sender's symbol (hb_symbols_fetch) and counts.  values_host [n_cands][n][limbs],
 * contradictions[c] = senders that already contradict candidate c, zlen = arrivals so far, n_cands <= 8.  hb_wait_arrived1 returns HB_WAIT_ON
 * (keep waiting), HB_WAIT_EVENT (a candidate can be accepted, or none is left: the wait is over, read hb_wait_result and act) or -(hb_status).
 * Gao's rule for how many contradictions a candidate may have: max(floor((|z| - degree - 1) / 2), max_errors - n_confirmed). */
#define HB_WAIT_ON 0
#define HB_WAIT_EVENT 1
typedef struct hb_wait hb_wait;
int hb_wait_create(hb_ctx *ctx, int n, hb_wait **out);
int hb_wait_begin(hb_wait *w, const uint64_t *cols_dev, int64_t C, int64_t chunk, int degree, int max_errors, int zlen, int n_cands,
                  const uint64_t *values_host, const int32_t *contradictions, void *stream);
int hb_wait_arrived1(hb_wait *w, int32_t idx, int n_confirmed);
int hb_wait_result(const hb_wait *w, int cand, int32_t *standing, int32_t *senders, int cap, int32_t *count);
void hb_wait_destroy(hb_wait *w);

/* The symbols of polynomial `chunk` in the columns of parties idx[0..count) (each in [0, n), count <= 64) of the party-major buffer cols_dev [n][C], to
 * out_host[count][limbs]: what IncrementalDecoder compares a new sender's share with (reed_solomon.py:318-321, data[i] against the guess) when
 * the guess is a candidate for ONE polynomial (device.py _candidate_cap).  One launch that writes pinned memory the call polls: the answer
 * is on the host a few microseconds after the columns are, where a synchronous 32-byte copy costs a stream synchronisation. */
int hb_symbols_fetch(hb_ctx *ctx, const uint64_t *cols_dev, int n, int64_t C, int64_t chunk, const int32_t *idx, int count, uint64_t *out_host, void *stream);
/* A candidate polynomial (coeffs_dev: d packed coefficients) against the received symbols of its chunk: the values it takes at the n party points
 * -> out_values_host[n][limbs] (the host keeps them for the senders still to come) and, per party, whether the symbol of `chunk` in its row of
 * the party-major buffer differs -> out_differs_host[n] (rows of parties that have not arrived hold whatever they hold: the caller looks at the
 * arrived ones).  IncrementalDecoder's comparison of the guess with the received shares (reed_solomon.py:316-326) for ONE polynomial: one launch, the
 * answer through pinned memory.  n <= 1024 (HB_ERR_UNSUPPORTED above). */
int hb_candidate_check(hb_ctx *ctx, const uint64_t *x_host, int n, const uint64_t *coeffs_dev, int d, const uint64_t *cols_dev, int64_t C, int64_t chunk,
                       uint64_t *out_values_host, uint8_t *out_differs_host, void *stream);
/* plumbing: `stream` goes on only after everything enqueued on `after` so far (an event of the context) */
int hb_stream_after(hb_ctx *ctx, void *stream, void *after);
/* plumbing: the context's side stream (made on first use, highest priority, non-blocking) -- where hb_dec / hb_quick_dec build beside a busy caller's
 * stream (HB_DEC_OPT_BESIDE) and where a caller may feed its probes (hb_probe_feed's `stream`): ONE for the context, a process has few hardware queues */
int hb_side_stream(hb_ctx *ctx, void **stream);

/* gao_interpolate for ONE codeword, incremental in its points (rsdecode_impl.h:325-363 as GaoRobustDecoder.robust_decode
 * runs it per polynomial, reed_solomon.py:151-186, 334-365): the probe keeps a reduced basis of the interpolation module of
 * the points fed so far (Koetter / Welch-Berlekamp; one workgroup, O(n') multiplications per new point) and decides exactly
 * as the reference's Gao does, beyond the unique-decoding radius included. */
typedef struct hb_probe hb_probe;
int hb_probe_create(hb_ctx *ctx, const uint64_t *x_host, int n, int k, hb_probe **out, void *stream);
/* feed element `poly` of the columns of parties idx[0..count) of the party-major buffer cols_dev [n][C] (arrival order, each party
 * once); with decide != 0 synchronise and report: *ok = the codeword decodes over everything fed, err_mask[0..n) = 1 at the
 * parties that are roots of the error locator (reed_solomon.py:174-184). */
int hb_probe_feed(hb_probe *pr, const int32_t *idx, int count, const uint64_t *cols_dev, int64_t C, int64_t poly, int decide,
                  int32_t *ok, uint8_t *err_mask, void *stream);
int hb_probe_reset(hb_probe *pr);          /* start over: another polynomial, or another arrival list */
/* workgroups a launch of this probe spreads over from now on (the probe must be reset: hb_probe_reset, or a HB_ERR_RETRY just returned): 0 = the
 * fewest the point set allows (1 up to 128 points, 2 above), otherwise 1 or 2 .. 8.  HB_ERR_BAD_ARG for a count the point set does not allow. */
int hb_probe_workgroups(hb_probe *pr, int wgs);
int hb_probe_points_fed(hb_probe *pr);
void hb_probe_destroy(hb_probe *pr);

/* ---- reference-shaped entry points (chunk-major buffers, tables cached in ctx) -------- */
/* vandermonde_batch_evaluate (pyx:199-244): polys_dev [C][d] -> out_dev [C][n] */
int hb_vandermonde_batch_evaluate(hb_ctx *ctx, const uint64_t *x_host, int n, const uint64_t *polys_dev,
                                  int64_t C, int d, uint64_t *out_dev, void *stream);
/* vandermonde_batch_interpolate (pyx:139-197): data_dev [C][k] -> out_dev [C][k]; HB_ERR_SINGULAR */
int hb_vandermonde_batch_interpolate(hb_ctx *ctx, const uint64_t *x_host, int k, const uint64_t *data_dev,
                                     int64_t C, uint64_t *out_dev, void *stream);
/* fft / partial_fft / fft_batch_evaluate (pyx:246-316, rsdecode_impl.h:125-192):
 * coeffs_dev [C][d] -> out_dev [C][k], out[c][i] = sum_{j<min(d,order)} coeffs[c][j] * omega^(i*j), i < k <= order */
int hb_fft_batch_evaluate(hb_ctx *ctx, const uint64_t *omega_host, int order, const uint64_t *coeffs_dev,
                          int64_t C, int d, int k, uint64_t *out_dev, void *stream);
/* fft_interpolate / fft_batch_interpolate (pyx:318-381, rsdecode_impl.h:194-265):
 * ys_dev [C][k] at points omega^zs[i] -> out_dev [C][k].  HB_ERR_SINGULAR for repeated zs. */
int hb_fft_batch_interpolate(hb_ctx *ctx, const uint64_t *omega_host, int order, const int32_t *zs_host, int k,
                             const uint64_t *ys_dev, int64_t C, uint64_t *out_dev, void *stream);
/* gao_interpolate, batched over C codewords sharing the same points (pyx:389-439,
 * rsdecode_impl.h:281-405).  ys_dev [C][npts]; coeffs_dev [C][k]; errloc_dev [C][npts+1]
 * (un-normalised EEA cofactor, errloc_len_dev[c] = deg+1); ok_dev[c] = 1 on success. */
int hb_gao_decode(hb_ctx *ctx, const uint64_t *x_host, int npts, int k, const uint64_t *ys_dev, int64_t C,
                  uint64_t *coeffs_dev, uint64_t *errloc_dev, int32_t *errloc_len_dev, uint8_t *ok_dev, void *stream);
/* Welch-Berlekamp (reed_solomon_wb.py:129-151), batched.  ys_dev [C][n], present_dev [C][n]
 * (0 = erasure).  coeffs_dev [C][k] zero padded, coeff_len_dev[c] = length after stripping
 * trailing zeros (polynomial.py:14-20), status_dev[c]: 0 ok, 1 "found no divisors!",
 * 2 "No solution", 3 too few points.  Words with at most floor((n' - k) / 2) errors over their n' surviving
 * points are settled by Gao's kernels (there the reference's solver can only return the closest codeword's
 * polynomial): complete words; words that all lost the SAME symbols (the protocol's case: the parties that
 * have not arrived, reed_solomon.py:201-204) as one batch over the points that are left; and, round 6, a batch
 * with up to 64 distinct patterns cut by pattern (groups of at least 64 codewords).  Every other word -- more
 * errors, small groups, also those Gao would still decode because the message has leading zeros -- goes through
 * the reference's own elimination, its descending-e loop and its particular solution (reed_solomon_wb.py:79-127,
 * 157-273).  The call returns with its last launch enqueued when Gao's kernels settled the whole batch. */
int hb_wb_decode(hb_ctx *ctx, const uint64_t *x_host, int n, int k, const uint64_t *ys_dev,
                 const uint8_t *present_dev, int64_t C, uint64_t *coeffs_dev, int32_t *coeff_len_dev,
                 int32_t *status_dev, void *stream);

/* sqrt_mod (pyx:441-444, NTL SqrRootMod), batched: out[i]^2 == a[i] (mod p), ok[i] = 0 for a non-residue.
 * Which of the two roots is returned is not pinned by the reference (tests/test_ntl.py:331-341). */
int hb_sqrt_mod(hb_ctx *ctx, const uint64_t *a_dev, int64_t C, uint64_t *out_dev, uint8_t *ok_dev, void *stream);

/* ---- one party's fault-free batch open -------------------------------------------------
 * The compute of batch_reconstruct (batch_reconstruction.py:158-227) for one party when no
 * received column is wrong: R1 encode; R1 optimistic decode + validating re-encode + compare
 * (reed_solomon.py:305-330); constant terms -> R2 message; R2 decode + re-encode + compare;
 * flatten.  3 batch encodes + 2 batch decodes, all on device.
 *   plan: created once per (points, arrival set); shares_dev [B]; r1_out_dev [n][C] party-major;
 *   r1_cols_dev / r2_cols_dev [n][C] party-major received columns; r2_msg_dev [C];
 *   result_dev [B].  C = ceil(B / d).
 * The hb_open_r* calls are asynchronous; hb_open_status synchronises and returns HB_OK or HB_ERR_MISMATCH. */
typedef struct hb_open_plan hb_open_plan;
int hb_open_plan_create(hb_ctx *ctx, int n, int d, int use_omega_powers, const uint64_t *x_host,
                        const uint64_t *omega_host, int order, const int32_t *z_host /* d arrivals used to decode */,
                        const int32_t *zc_host /* later arrivals to validate */, int n_check, int64_t max_B,
                        hb_open_plan **out, void *stream);
int hb_open_r1_encode(hb_open_plan *plan, const uint64_t *shares_dev, int64_t B, uint64_t *r1_out_dev, void *stream);
int hb_open_r1_decode(hb_open_plan *plan, const uint64_t *r1_cols_dev, int64_t B, uint64_t *r2_msg_dev, void *stream);
int hb_open_r2_decode(hb_open_plan *plan, const uint64_t *r2_cols_dev, int64_t B, uint64_t *result_dev, void *stream);
int hb_open_status(hb_open_plan *plan, void *stream);
/* Options.  HB_OPEN_OPT_VALIDATE_ARRIVED_ONLY (default 0): the reference re-encodes the guess at ALL n
 * points (encoder.encode_batch, reed_solomon.py:313) and then compares the columns that arrive; with
 * the option on, only output tiles containing a compared row are re-encoded.  Same accept/reject
 * decision, less arithmetic; off by default so that an open performs the reference's 3 full encodes.
 * HB_OPEN_OPT_MATRIX_CORES (default 1): when the Vandermonde entries fit 16 signed base-256 digits and
 * 2^254 <= p < 2^256 (the reference's BLS12-381 scalar field with the default points 1..n), the R1 encode
 * and the validating re-encode run as an exact int8 GEMM on the matrix cores (csrc/hb_mfma.hip); 0 forces
 * the integer-VALU kernels.  Results are bit-identical either way.  get_option reports whether the
 * matrix-core path is in use for this plan (0 when the plan's shapes do not qualify).
 * HB_OPEN_OPT_FUSED_VALIDATE (default 1): plans on the matrix cores with at least 4 coefficients and 4 points decode AND
 * validate in one launch of the full-size matrix-core kernel: the value the guess takes at a later
 * arrival's point is a linear function of the arrival set, V[zc] (Vinv y) = (V[zc] Vinv) y, so the rows [Vinv rows wanted ;
 * V[zc] Vinv] applied to the received columns give the coefficients and the predictions to compare (reference:
 * decoder.decode_batch + encoder.encode_batch + compare, reed_solomon.py:300-323; same canonical values, same accept /
 * reject).  The two matrices are built on the device when the plan is created (hb_quick.hip: enqueued, nothing waited for);
 * where that builder does not apply (p >= 0x7f 2^248, repeated points) they are built through the host (1-2.5 ms) when the plan
 * decodes for the third time, or at once when the option is set to 1.
 * At points that are distinct integers below 2^16 (the production points 1 .. n; 4 <= d <= 22) the two products factor as
 * [N ; P] (y ./ den) with matrices of small INTEGERS (numerators of the Lagrange basis and its values at the compared points):
 * such plans decode + validate on the small-entry kernel with the division by den_j inside it (csrc/hb_mfma_fused.hip) -- value 2
 * selects the full-size kernel for them all the same.
 * 0: decode, then re-encode all n points (NTT or mat-vec) and compare.  get_option: 0 = off / unavailable, 1 = on (full-size
 * kernel), 3 = on (small-entry kernel). */
#define HB_OPEN_OPT_VALIDATE_ARRIVED_ONLY 1
#define HB_OPEN_OPT_MATRIX_CORES 2
#define HB_OPEN_OPT_FUSED_VALIDATE 3
int hb_open_plan_set_option(hb_open_plan *plan, int option, int value);
int hb_open_plan_get_option(hb_open_plan *plan, int option, int *value);
void hb_open_plan_destroy(hb_open_plan *plan);

/* host-side self test of the radix-2^29 arithmetic templates (no GPU needed):
 * out = a*b mod p computed with the same code the kernels use. */
int hb_selftest_mulmod(const uint64_t *p_limbs, int n_limbs, const uint64_t *a, const uint64_t *b, uint64_t *out);
/* host-side run of the element-wise kernels' bodies (no GPU needed): the same per-element functions hb_ew_op,
 * hb_ew_beaver and hb_ew_inv launch, over `count` packed elements of host memory.
 *   what = HB_EW_ADD | SUB | MUL (operands[0] = a, [1] = b; or-ed with HB_EW_SELFTEST_BROADCAST: b is one element),
 *          HB_EW_NEG (operands[0] = a),
 *          HB_EW_SELFTEST_BEAVER (operands[0..4] = d, e, p, q, pq),
 *          HB_EW_SELFTEST_INV (operands[0] = in, walked tile by tile and lane by lane as the kernel's waves do;
 *          operands[1], when not NULL, points at one uint64_t that receives the number of zeros met). */
#define HB_EW_SELFTEST_BEAVER 4
#define HB_EW_SELFTEST_INV 5
#define HB_EW_SELFTEST_BROADCAST 0x100
int hb_selftest_ew(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *operands, uint64_t *out, int64_t count);
/* host-side run of the power-mixing kernels' bodies (no GPU needed), walked tile by tile and lane by lane as the kernels' workgroups
 * walk them, over host memory: c_host [M], powers_host [M][k].
 *   what = HB_PM_SELFTEST_SUMS    out [k]: the direct path's power sums, partial sums over `group` clients each added up afterwards
 *          HB_PM_SELFTEST_POWERS  out [M][k]: the direct path with groups of one client
 *          HB_PM_SELFTEST_TABLES  out [2][M][k + 1]: u (1, [b^j] / j!) and then v (c^i / i!) as the table kernels build them
 *          HB_PM_SELFTEST_MAC     c_host = U, powers_host = V, both [M][k]: out [k] = sum_c U[c][f] V[c][f] as the NTT path's
 *                                 multiply-accumulate and reduction passes compute it (any k; the first three need k < p)
 *          HB_PM_SELFTEST_CONV    c_host = u, powers_host = v, both [M][k + 1], taken as they are: out [k], out[m - 1] =
 *                                 sum_c sum_{j <= m} u[c][j] v[c][m - j] through the direct kernel's staging and windows (any k) */
#define HB_PM_SELFTEST_SUMS 0
#define HB_PM_SELFTEST_POWERS 1
#define HB_PM_SELFTEST_TABLES 2
#define HB_PM_SELFTEST_MAC 3
#define HB_PM_SELFTEST_CONV 4
int hb_selftest_pm(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *c_host, const uint64_t *powers_host, int64_t M, int k,
                   int64_t group, uint64_t *out);
/* host-side run of the butterfly kernels' bodies (no GPU needed) over host memory, switch by switch:
 *   what = HB_BF_SELFTEST_MASK    operands[0..3] = in [k], bits, p, q [k / 2]: out as hb_bf_mask writes masked_dev (operands[1] NULL:
 *                                 the k / 2 data-dependent elements alone)
 *          HB_BF_SELFTEST_SWITCH  operands[0..5] = in [k], d, e, p, q, pq [k / 2]: out [k] as hb_bf_switch writes out_dev
 *          HB_BF_SELFTEST_INDEX   no operands: out[2j] = xi, out[2j + 1] = yi of switch j as plain 64-bit integers (k of them)
 *          HB_BF_SELFTEST_HALVE   operands[0] = v [k], any k >= 0, log2_stride ignored: out[i] = v[i] / 2 as the switch halves its sums */
#define HB_BF_SELFTEST_MASK 0
#define HB_BF_SELFTEST_SWITCH 1
#define HB_BF_SELFTEST_INDEX 2
#define HB_BF_SELFTEST_HALVE 3
int hb_selftest_bf(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *operands, int64_t k, int log2_stride, uint64_t *out);
/* host-side run of the MiMC kernels' bodies (no GPU needed) over host memory, element by element; start, key_broadcast and flags as
 * the device calls take them:
 *   what = HB_MIMC_SELFTEST_PLAIN  operands[0..2] = x (NULL: the counters start + i), key, addend (or NULL); arg = rounds: out as
 *                                  hb_mimc_plain writes out_dev (HB_MIMC_PAIR: through the two-element body)
 *          HB_MIMC_SELFTEST_ROUND  operands[0..5] = y, r, r2, r3, key, r_next (NULL: the last round); arg = ctr: as hb_mimc_round
 *          HB_MIMC_SELFTEST_FIRST  operands[0..2] = x (or NULL), key, r0: as hb_mimc_first */
#define HB_MIMC_SELFTEST_PLAIN 0
#define HB_MIMC_SELFTEST_ROUND 1
#define HB_MIMC_SELFTEST_FIRST 2
int hb_selftest_mimc(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *operands, const uint64_t *start, int key_broadcast,
                     int flags, int64_t arg, uint64_t *out, int64_t count);
/* host-side run of the Jubjub kernels' bodies (no GPU needed) over host memory, element by element; a, d one canonical element each
 * (NULL where `what` does not use it); arrays of several rows are row-major with `count` elements a row:
 *   what = HB_JJ_SELFTEST_SCALAR_MUL    operands[0..2] = n, x, y; flags = HB_JJ_SCALAR_BROADCAST | HB_JJ_POINT_BROADCAST; a, d;
 *                                       out [2][count] = the x row, then the y row, as hb_jj_scalar_mul writes them
 *          HB_JJ_SELFTEST_DOUBLE_TABLE  operands[0..1] = x, y; arg = rows; a; out [3][rows][count]: the PROJECTIVE rows the kernel writes
 *                                       (Montgomery residues of X, Y, Z: x = X / Z, y = Y / Z)
 *          HB_JJ_SELFTEST_MASK          operands[0..5] = x1, y1, x2, y2, p, q; arg = trip_stride; out [8][count]
 *          HB_JJ_SELFTEST_STAGE1        operands[0..5] = opened A, p, q, pq, rx, ry; arg = trip_stride; out [6][count]
 *          HB_JJ_SELFTEST_STAGE2        operands[0..5] = opened B, p, q, pq, rx, ry; arg = trip_stride; d; out [2][count] uv, then [4][count] C
 *          HB_JJ_SELFTEST_STAGE3        operands[0..3] = opened C, p, q, pq; arg = trip_stride; out [2][count]
 *          HB_JJ_SELFTEST_SCALE         operands[0..1] = the inverted sigs [2][count], uv [2][count]; out [2][count] = x3, y3 */
#define HB_JJ_SCALAR_BROADCAST 1
#define HB_JJ_POINT_BROADCAST 2
#define HB_JJ_SELFTEST_SCALAR_MUL 0
#define HB_JJ_SELFTEST_DOUBLE_TABLE 1
#define HB_JJ_SELFTEST_MASK 2
#define HB_JJ_SELFTEST_STAGE1 3
#define HB_JJ_SELFTEST_STAGE2 4
#define HB_JJ_SELFTEST_STAGE3 5
#define HB_JJ_SELFTEST_SCALE 6
int hb_selftest_jj(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *operands, const uint64_t *a, const uint64_t *d,
                   int flags, int64_t arg, uint64_t *out, int64_t count);
/* host-side run of the G1 kernels' bodies (no GPU needed) over host memory, item by item; points, scalars and tables as the device
 * calls take them (a table: hb_g1_table_bytes(window) bytes, 16-byte aligned); also checks the literal constants of Fq against Q:
 *   what = HB_G1_SELFTEST_FQ_MUL      operands[0..1] = a, b: 6 words an element, below Q; out = a b mod Q, 6 words an element
 *          HB_G1_SELFTEST_SCALAR_MUL  operands[0..1] = k, P; flags = HB_G1_SCALAR_BROADCAST | HB_G1_POINT_BROADCAST; out = points
 *          HB_G1_SELFTEST_ADD         operands[0..1] = P, Q; flags = HB_G1_SUBTRACT, as hb_g1_add;
 *                                     | HB_G1_GENERAL: through the Jacobian + Jacobian formula, both operands moved off Z = 1;
 *                                     | HB_G1_DOUBLE: out = 2 P through the doubling formula (Q unused)
 *          HB_G1_SELFTEST_CHECK       operands[0] = P; out = `count` int32 flags
 *          HB_G1_SELFTEST_TABLE       operands[0] = the base; arg = window; count = 1; out = the table
 *          HB_G1_SELFTEST_COMMIT      operands[0..3] = a, b, table of g, table of h; arg = window
 *          HB_G1_SELFTEST_EVAL        operands[0] = cs; flags = n_coef; arg = index
 *          HB_G1_SELFTEST_VERIFY      operands[0..4] = cs, s, w, table of g, table of h; flags = n_coef | window << 16; arg = index;
 *                                     out = `count` int32 verdicts, then the int32 count of rejected items */
#define HB_G1_SCALAR_BROADCAST 1
#define HB_G1_POINT_BROADCAST 2
#define HB_G1_SUBTRACT 1
#define HB_G1_GENERAL 2
#define HB_G1_DOUBLE 4
#define HB_G1_SELFTEST_FQ_MUL 0
#define HB_G1_SELFTEST_SCALAR_MUL 1
#define HB_G1_SELFTEST_ADD 2
#define HB_G1_SELFTEST_CHECK 3
#define HB_G1_SELFTEST_TABLE 4
#define HB_G1_SELFTEST_COMMIT 5
#define HB_G1_SELFTEST_EVAL 6
#define HB_G1_SELFTEST_VERIFY 7
int hb_selftest_g1(int what, const uint64_t *const *operands, int flags, int64_t arg, uint64_t *out, int64_t count);
/* host-side run of hb_g1_msm (no GPU needed) over host memory: the per-lane steps of its kernels (the digit of a term, the walk of a
 * bucket's list, b * B_b, a tree step, the fold, the row's Horner end) driven lane by lane, workgroup by workgroup, with arrays in place
 * of LDS.  Arguments as hb_g1_msm; method = 3 (here only): the bucket path with EVERY non-empty bucket summed by the whole workgroup. */
int hb_selftest_g1_msm(const uint64_t *s, const uint64_t *p, int points_per_row, uint64_t *out, int64_t rows, int64_t terms, int method,
                       int chunk);
/* host-side run of the bodies of hb_crs.hip (no GPU needed) over host memory; arguments are checked as the device calls check them:
 *   what = HB_G1_CRS_SELFTEST_TABLE     operands[0] = `count` bases; arg = window; out = `count` tables, as hb_g1_crs_table lays them out
 *          HB_G1_CRS_SELFTEST_QUOTIENT  operands[0..1] = phi, xs; flags = n_coef; arg = n_points; count = polynomials;
 *                                       out = q (count * n_points * (n_coef - 1) elements), then rem (count * n_points)
 *          HB_G1_CRS_SELFTEST_MSM       operands[0..3] = tables of G, tables of H or NULL, a, b or NULL; flags = window | split << 8;
 *                                       arg = terms | n_bases << 32; count = rows; out = points.  split > 1 drives a workgroup lane by
 *                                       lane: every lane's units, the tree steps over an array in place of LDS, the first lanes' stores */
#define HB_G1_CRS_SELFTEST_TABLE 0
#define HB_G1_CRS_SELFTEST_QUOTIENT 1
#define HB_G1_CRS_SELFTEST_MSM 2
int hb_selftest_g1_crs(int what, const uint64_t *const *operands, int flags, int64_t arg, uint64_t *out, int64_t count);
/* host-side run of the bodies of hb_g1_wire.hip (no GPU needed) over host memory, item by item; operands and out aligned to 16 bytes
 * (else HB_ERR_BAD_ARG); arg = 0; the constants are derived and checked as for the device calls (a failed check: HB_ERR_UNSUPPORTED):
 *   what = HB_G1_WIRE_SELFTEST_SUBGROUP    operands[0] = points; out = `count` int32 flags
 *          HB_G1_WIRE_SELFTEST_DECOMPRESS  operands[0] = count * 48 bytes; flags = check_subgroup; out = `count` points (12 words each),
 *                                          then `count` int32 statuses, then the int32 count of rejected items
 *          HB_G1_WIRE_SELFTEST_COMPRESS    operands[0] = points; out = count * 48 bytes
 *          HB_G1_WIRE_SELFTEST_SQRT        operands[0] = a: 6 words an element, below Q; out = `count` roots a^((Q + 1) / 4) (6 words
 *                                          each, zeros where a is no square), then `count` int32 flags: 1 a square, 0 not
 *          HB_G1_WIRE_SELFTEST_PHI         operands[0] = points; out = (beta x, y) of each */
#define HB_G1_WIRE_SELFTEST_SUBGROUP 0
#define HB_G1_WIRE_SELFTEST_DECOMPRESS 1
#define HB_G1_WIRE_SELFTEST_COMPRESS 2
#define HB_G1_WIRE_SELFTEST_SQRT 3
#define HB_G1_WIRE_SELFTEST_PHI 4
int hb_selftest_g1_wire(int what, const uint64_t *const *operands, int flags, int64_t arg, uint64_t *out, int64_t count);
/* host-side run of the bodies of hb_pair.hip and hb_fq12_elem.hpp (no GPU needed) over host memory, item by item; also derives the
 * Frobenius constants from Q and compares them with the literals (a difference: HB_ERR_BAD_ARG whatever is asked):
 *   what = HB_PAIR_SELFTEST_TOWER    operands[0..1] = a, b: 72 words an item, residues below Q; flags = HB_PAIR_OP_*; out = 72 words an
 *                                    item.  An operation of Fq2 or Fq6 works on the leading coordinates and copies the rest of a.
 *                                    MUL_BY_01 / MUL_BY_1 / MUL_BY_014 take their sparse factor's Fq2 coefficients from the head of b.
 *                                    FROBENIUS: arg = 1, 2 or 3.  FINAL_EXP: out = a^(3 (Q^12 - 1) / R).
 *                                    CYCLO_SQR: Granger and Scott's squaring, a square only for a in the cyclotomic subgroup.
 *                                    flags also takes the three Fq operations of hbmpc_hip_debug.h (coordinate 0 alone).
 *          HB_PAIR_SELFTEST_PREPARE  operands[0] = the 204 Fq2 coefficients hb_pair_prepare takes; count = 1; out = the table
 *          HB_PAIR_SELFTEST_PRODUCT  operands[0] = points (count, K, 12), operands[1..K] = tables; flags = K; arg = mode; out = GT
 *                                    elements, or `count` int32 verdicts then the int32 count of rejected items */
#define HB_PAIR_SELFTEST_TOWER 0
#define HB_PAIR_SELFTEST_PREPARE 1
#define HB_PAIR_SELFTEST_PRODUCT 2
#define HB_PAIR_OP_FQ2_MUL 0
#define HB_PAIR_OP_FQ2_SQR 1
#define HB_PAIR_OP_FQ2_MUL_NR 2
#define HB_PAIR_OP_FQ2_INV 3
#define HB_PAIR_OP_FQ6_MUL 4
#define HB_PAIR_OP_FQ6_MUL_BY_01 5
#define HB_PAIR_OP_FQ6_MUL_BY_1 6
#define HB_PAIR_OP_FQ6_MUL_NR 7
#define HB_PAIR_OP_FQ6_INV 8
#define HB_PAIR_OP_FQ12_MUL 9
#define HB_PAIR_OP_FQ12_SQR 10
#define HB_PAIR_OP_FQ12_MUL_BY_014 11
#define HB_PAIR_OP_FQ12_CONJ 12
#define HB_PAIR_OP_FQ12_FROBENIUS 13
#define HB_PAIR_OP_FQ12_INV 14
#define HB_PAIR_OP_FQ12_FINAL_EXP 15
#define HB_PAIR_OP_FQ12_CYCLO_SQR 16
int hb_selftest_pairing(int what, const uint64_t *const *operands, int flags, int64_t arg, uint64_t *out, int64_t count);
/* host-side run of the fixed-point kernels' bodies (no GPU needed) over host memory, element by element.  params = {k, m, kappa,
 * nodes or mode, root}; parameters are checked as the device calls check them:
 *   what = HB_FXP_SELFTEST_MASK     operands[0..1] = x (or NULL), bits [k + kappa][count]; outs[0..1] as hb_fxp_mask writes masked_dev, r1_dev
 *          HB_FXP_SELFTEST_TRUNC_PR operands[0..3] = x, c, r1, inv2m (one element); outs[0]
 *          HB_FXP_SELFTEST_LEAVES   operands[0..1] = c, bits [m][count]; outs[0..1] = g, p [m + 1][count]
 *          HB_FXP_SELFTEST_CARRY_MASK     operands[0..3] = g, p, ta, tb; outs[0] as hb_fxp_carry_mask writes masked_dev
 *          HB_FXP_SELFTEST_CARRY_COMBINE  operands[0..5] = opened, g, p, ta, tb, tab; outs[0..1] = g_out, p_out (root: outs[1] unused)
 *          HB_FXP_SELFTEST_FINISH   operands[0..4] = x (NULL with HB_FXP_MOD), c, r1, carry, inv2m; params[3] = mode; outs[0] */
#define HB_FXP_SELFTEST_MASK 0
#define HB_FXP_SELFTEST_TRUNC_PR 1
#define HB_FXP_SELFTEST_LEAVES 2
#define HB_FXP_SELFTEST_CARRY_MASK 3
#define HB_FXP_SELFTEST_CARRY_COMBINE 4
#define HB_FXP_SELFTEST_FINISH 5
int hb_selftest_fxp(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *operands, const int64_t *params,
                    uint64_t *const *outs, int64_t count);
/* host-side run of the bit decomposition kernels' bodies (no GPU needed) over host memory, a whole level or step at a time.
 * params = {m, level}; parameters are checked as the device calls check them:
 *   what = HB_BD_SELFTEST_LEAVES          operands[0..1] = c, bits [m - 1][count]; outs[0..1] = g, p [m - 1][count]
 *          HB_BD_SELFTEST_PREFIX_MASK     operands[0..3] = g, p, ta, tb; outs[0] as hb_bd_prefix_mask writes masked_dev
 *          HB_BD_SELFTEST_PREFIX_COMBINE  operands[0..3] = opened, ta, tb, tab; outs[0..1] = g, p, updated in place
 *          HB_BD_SELFTEST_SUM_MASK        operands[0..4] = c, bits [m][count], g, ta, tb; outs[0] as hb_bd_sum_mask writes masked_dev
 *          HB_BD_SELFTEST_SUM_COMBINE     operands[0..6] = opened, c, bits [m][count], g, ta, tb, tab; outs[0] = the m planes */
#define HB_BD_SELFTEST_LEAVES 0
#define HB_BD_SELFTEST_PREFIX_MASK 1
#define HB_BD_SELFTEST_PREFIX_COMBINE 2
#define HB_BD_SELFTEST_SUM_MASK 3
#define HB_BD_SELFTEST_SUM_COMBINE 4
int hb_selftest_bd(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *operands, const int64_t *params,
                   uint64_t *const *outs, int64_t count);
/* host-side run of the demultiplexer's rows (no GPU needed) over host memory, a whole step at a time, with the index arithmetic and the
 * argument checks of the entry points.  params = {m, level}:
 *   what = HB_DEMUX_SELFTEST_LEAVES  operands[0] = bits [1][count]; outs[0] [2][count]; params are not read
 *          HB_DEMUX_SELFTEST_MASK    operands[0..2] = bits [m][count], groups, ta; outs[0] as hb_demux_mask writes out_dev
 *          HB_DEMUX_SELFTEST_FINISH  operands[0..2] = opened, ta, tab; outs[0] = groups, the level's rows updated in place */
#define HB_DEMUX_SELFTEST_LEAVES 0
#define HB_DEMUX_SELFTEST_MASK 1
#define HB_DEMUX_SELFTEST_FINISH 2
int hb_selftest_demux(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *operands, const int64_t *params,
                      uint64_t *const *outs, int64_t count);
/* host-side run of the division kernels' bodies (no GPU needed) over host memory, a whole level or step at a time; parameters are
 * checked as the device calls check them:
 *   what = HB_DIV_SELFTEST_OR_MASK       params = {n_planes, level, from_top}; operands[0..2] = y, ta, tb; outs[0] as hb_div_or_mask writes
 *                                        masked_dev
 *          HB_DIV_SELFTEST_OR_COMBINE    params as above; operands[0..3] = opened, ta, tb, tab; outs[0] = y, updated in place
 *          HB_DIV_SELFTEST_NORM_MASK     params = {n_planes}; operands[0..4] = x, y, u (or NULL), ta, tb; outs[0..1] = masked, v
 *          HB_DIV_SELFTEST_PRODUCT_STEP  params = {mode, products, width, m, kappa}; operands[0..8] = opened, ta, tb, tab, aux, cst (one
 *                                        element), nxt_a, nxt_b, bits (NULL where the mode reads none); outs[0..1] = out0, out1
 *          HB_DIV_SELFTEST_TRUNC_STEP    params = {mode, rows, products, m}; operands[0..8] = opened, s, inv2m, alpha (one element each), x,
 *                                        ext0, ext1, ta, tb; outs[0]
 *          HB_DIV_SELFTEST_PAIR_MASK     operands[0..3] = x, y, ta, tb; outs[0] as hb_div_pair_mask writes masked_dev */
#define HB_DIV_SELFTEST_OR_MASK 0
#define HB_DIV_SELFTEST_OR_COMBINE 1
#define HB_DIV_SELFTEST_NORM_MASK 2
#define HB_DIV_SELFTEST_PRODUCT_STEP 3
#define HB_DIV_SELFTEST_TRUNC_STEP 4
#define HB_DIV_SELFTEST_PAIR_MASK 5
int hb_selftest_div(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *operands, const int64_t *params,
                    uint64_t *const *outs, int64_t count);
/* host-side run of the square root kernels' steps (no GPU needed) over host memory, a whole step at a time; parameters and overlaps
 * are checked as the device calls check them:
 *   what = HB_FXSQRT_SELFTEST_NORM_MASK   params = {n_planes, sets}; operands[0..4] = x, y, weights, ta, tb; outs[0..1] = masked, kept
 *          HB_FXSQRT_SELFTEST_FIRST       operands[0..7] = opened, ta, tb, tab, a, b (one element each), nxt_a, nxt_b; outs[0..1] = masked, h
 *          HB_FXSQRT_SELFTEST_TRUNC_STEP  params = {mode, rows, which, m}; operands[0..6] = opened, s, inv2m, cst (one element each; cst NULL
 *                                         where the mode reads none), kept_in, ta, tb; outs[0..1] = masked, kept_out */
#define HB_FXSQRT_SELFTEST_NORM_MASK 0
#define HB_FXSQRT_SELFTEST_FIRST 1
#define HB_FXSQRT_SELFTEST_TRUNC_STEP 2
int hb_selftest_fxsqrt(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *operands, const int64_t *params,
                       uint64_t *const *outs, int64_t count);
/* host-side run of the exponential kernels' steps (no GPU needed) over host memory, a whole step at a time; parameters and overlaps are
 * checked as the device calls check them:
 *   what = HB_FXEXP_SELFTEST_FINISH_LOOKUP_MASK  params = {n_groups, pairs, kept_rows, then desc: 6 ints a group}; operands[0..6] = bits,
 *                                                opened, ta, tab, tables, nxt_a, nxt_b; outs[0..1] = masked, kept
 *          HB_FXEXP_SELFTEST_PRODUCTS_TRUNC      params = {products, width, m, kappa}; operands[0..4] = opened, ta, tb, tab, bits; outs[0..1]
 *                                                = masked, s
 *          HB_FXEXP_SELFTEST_TREE_STEP           params = {rows, m}; operands[0..5] = opened, s, inv2m (one element), carry (or NULL), ta, tb;
 *                                                outs[0..1] = masked, kept */
#define HB_FXEXP_SELFTEST_FINISH_LOOKUP_MASK 0
#define HB_FXEXP_SELFTEST_PRODUCTS_TRUNC 1
#define HB_FXEXP_SELFTEST_TREE_STEP 2
int hb_selftest_fxexp(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *operands, const int64_t *params,
                      uint64_t *const *outs, int64_t count);
/* host-side run of the logarithm kernels' steps (no GPU needed) over host memory, a whole step at a time; parameters and overlaps are
 * checked as the device calls check them (params has five entries; those a step does not read are 0):
 *   what = HB_FXLOG_SELFTEST_FIRST      operands[0..6] = opened, ta, tb, tab, ybig, nxt_a, nxt_b; outs[0..1] = masked, powers (row 0 written)
 *          HB_FXLOG_SELFTEST_LEVEL      params = {level, d, m}; operands[0..4] = opened, s, inv2m (one element), ta, tb; outs[0..1] = masked,
 *                                       powers [d][count], updated in place
 *          HB_FXLOG_SELFTEST_POLY_MASK  params = {d, m_in, width, m_out, kappa}; operands[0..6] = opened, s, inv2m (one element), powers, ybig,
 *                                       coef [d + 1], bits; outs[0..1] = masked, s_out
 *          HB_FXLOG_SELFTEST_FINISH     params = {m}; operands[0..3] = opened, s, inv2m (one element), ipart; outs[0] = out */
#define HB_FXLOG_SELFTEST_FIRST 0
#define HB_FXLOG_SELFTEST_LEVEL 1
#define HB_FXLOG_SELFTEST_POLY_MASK 2
#define HB_FXLOG_SELFTEST_FINISH 3
int hb_selftest_fxlog(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *operands, const int64_t *params,
                      uint64_t *const *outs, int64_t count);
/* host-side run of the sine and cosine kernels' steps (no GPU needed) over host memory, a whole step at a time; parameters and overlaps
 * are checked as the device calls check them:
 *   what = HB_FXTRIG_SELFTEST_FINISH_LOOKUP_MASK  params = {n_groups, pairs, kept_slots, mode, split, then desc: 6 ints a group};
 *                                                 operands[0..6] = bits, opened, ta, tab, tables, nxt_a, nxt_b; outs[0..1] = masked, kept
 *          HB_FXTRIG_SELFTEST_CPRODUCTS_TRUNC     params = {products, mode, width, m, kappa}; operands[0..4] = opened, ta, tb, tab, bits;
 *                                                 outs[0..1] = masked, s
 *          HB_FXTRIG_SELFTEST_TREE_STEP           params = {rows, final, m, mode}; operands[0..5] = opened, s, inv2m (one element), carry (or
 *                                                 NULL), ta, tb; outs[0..1] = masked, kept */
#define HB_FXTRIG_SELFTEST_FINISH_LOOKUP_MASK 0
#define HB_FXTRIG_SELFTEST_CPRODUCTS_TRUNC 1
#define HB_FXTRIG_SELFTEST_TREE_STEP 2
int hb_selftest_fxtrig(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *operands, const int64_t *params,
                       uint64_t *const *outs, int64_t count);
/* host-side run of the arctangent kernels' steps (no GPU needed) over host memory, a whole step at a time; parameters and overlaps are
 * checked as the device calls check them (params has five entries; those a step does not read are 0):
 *   what = HB_FXATAN_SELFTEST_SIGN_MASK    operands[0..4] = s, x, y, ta, tb; outs[0] = masked
 *          HB_FXATAN_SELFTEST_ABS          params = {k, kappa}; operands[0..6] = opened, ta, tb, tab, x, y, bits; outs[0..1] = masked, kept
 *          HB_FXATAN_SELFTEST_SELECT_MASK  operands[0..4] = c, w, sx, ta, tb; outs[0] = masked
 *          HB_FXATAN_SELFTEST_SELECT       operands[0..5] = opened, ta, tb, tab, ax, ay; outs[0] = out
 *          HB_FXATAN_SELFTEST_FIRST        params = {shift}; operands[0..4] = q, sy, e1, ta, tb; outs[0..1] = masked, powers (row 0 written)
 *          HB_FXATAN_SELFTEST_LEVEL        params = {level, d, m}; operands[0..4] = opened, s, inv2m (one element), ta, tb; outs[0..1] =
 *                                          masked, powers [J + 1][count], updated in place
 *          HB_FXATAN_SELFTEST_POLY_MASK    params = {d, m_in, width, m_out, kappa}; operands[0..5] = opened, s, inv2m (one element), powers,
 *                                          coef [J + 1], bits; outs[0..1] = masked, s_out
 *          HB_FXATAN_SELFTEST_ASSEMBLE     params = {m}; operands[0..11] = opened, s, inv2m (one element), eopened, ea, eb, eab, sy, g, cst
 *                                          (two elements), ta, tb; outs[0..1] = masked, c
 *          HB_FXATAN_SELFTEST_FINISH       operands[0..4] = opened, ta, tb, tab, c; outs[0] = out */
#define HB_FXATAN_SELFTEST_SIGN_MASK 0
#define HB_FXATAN_SELFTEST_ABS 1
#define HB_FXATAN_SELFTEST_SELECT_MASK 2
#define HB_FXATAN_SELFTEST_SELECT 3
#define HB_FXATAN_SELFTEST_FIRST 4
#define HB_FXATAN_SELFTEST_LEVEL 5
#define HB_FXATAN_SELFTEST_POLY_MASK 6
#define HB_FXATAN_SELFTEST_ASSEMBLE 7
#define HB_FXATAN_SELFTEST_FINISH 8
int hb_selftest_fxatan(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *operands, const int64_t *params,
                       uint64_t *const *outs, int64_t count);
/* host-side run of the equality kernels' bodies (no GPU needed) over host memory, element by element.  params = {rows, mode}:
 *   what = HB_EQ_SELFTEST_LEGENDRE  operands[0] = a; outs[0] = int8 [count]
 *          HB_EQ_SELFTEST_MASK1     operands[0..7] = x, y (or NULL), r, rp, pa, qa, pb, qb; outs[0] as hb_eq_mask1 writes masked_dev
 *          HB_EQ_SELFTEST_MID       operands[0..10] = opened, pa, qa, pqa, pb, qb, pqb, bits, pc, qc, nr (one element); outs[0..1] = masked2, dr
 *          HB_EQ_SELFTEST_CSHARE    operands[0..4] = opened2, dr, pc, qc, pqc; outs[0] = c
 *          HB_EQ_SELFTEST_FINISH    operands[0..2] = c, bits, nr (one element; may be NULL with HB_EQ_BIT); outs[0] = factor,
 *                                   outs[1] = zero_rows, int32 [rows], zeroed by the caller */
#define HB_EQ_SELFTEST_LEGENDRE 0
#define HB_EQ_SELFTEST_MASK1 1
#define HB_EQ_SELFTEST_MID 2
#define HB_EQ_SELFTEST_CSHARE 3
#define HB_EQ_SELFTEST_FINISH 4
int hb_selftest_eq(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *operands, const int64_t *params, void *const *outs,
                   int64_t count);
/* host-side run of the less-than kernels' bodies (no GPU needed) over host memory, element by element.  params = {L, mode}; L and
 * the mode are checked as the device calls check them where the step reads them:
 *   what = HB_LT_SELFTEST_MASK        operands[0..2] = a, b (or NULL), r; outs[0]
 *          HB_LT_SELFTEST_LEAVES      operands[0..1] = c, r_bits [L][count]; outs[0..1] = g, p [L][count]
 *          HB_LT_SELFTEST_XOR_MASK    operands[0..4] = c, r_0, w, pa, qa; outs[0..1] = u, masked [2][count]
 *          HB_LT_SELFTEST_DMASK       operands[0..8] = c, r_0, x, s, s_bits [L][count], pa, qa, pb, qb; outs[0..1] = u, masked [5][count]
 *          HB_LT_SELFTEST_MID         operands[0..10] = opened [5][count], u, s_bits [L][count], pa, qa, pqa, pb, qb, pqb, pc, qc;
 *                                     outs[0..2] = v, d_0, masked [2][count]
 *          HB_LT_SELFTEST_XOR_FINISH  operands[0..5] = opened [2][count], u, v, p, q, pq; outs[0] */
#define HB_LT_SELFTEST_MASK 0
#define HB_LT_SELFTEST_LEAVES 1
#define HB_LT_SELFTEST_XOR_MASK 2
#define HB_LT_SELFTEST_DMASK 3
#define HB_LT_SELFTEST_MID 4
#define HB_LT_SELFTEST_XOR_FINISH 5
int hb_selftest_lt(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *operands, const int64_t *params, uint64_t *const *outs,
                   int64_t count);
/* host-side run of the offline kernels' bodies (no GPU needed) over host memory, element by element:
 *   what = HB_OFF_SELFTEST_MUL_ADD       operands[0..2] = a, b, c; out may be any of them
 *          HB_OFF_SELFTEST_INVSQRT       or-ed with (mode << 8): operands[0] = x, [1] = u (or NULL: out = w), [2] = two uint64 words
 *                                        that receive the status counts (or NULL)
 *          HB_OFF_SELFTEST_DEGREE_CHECK  operands[0] = coeffs [n][2 count], [1] = two uint64 words {n, t}; count = k; out = the three
 *                                        counts as uint64 words */
#define HB_OFF_SELFTEST_MUL_ADD 0
#define HB_OFF_SELFTEST_INVSQRT 1
#define HB_OFF_SELFTEST_DEGREE_CHECK 2
int hb_selftest_off(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *operands, uint64_t *out, int64_t count);
/* host-side run of the two rows of hb_offpow.hip (no GPU needed) over host memory, with the index arithmetic and the argument checks of
 * the entry points:
 *   what = HB_OFF_POWERS_SELFTEST_MASK    as hb_off_pow_mask: r = r2t, out = the masked products; x is not read
 *          HB_OFF_POWERS_SELFTEST_FINISH  as hb_off_pow_finish: x = opened, r = rt; out is not written */
#define HB_OFF_POWERS_SELFTEST_MASK 0
#define HB_OFF_POWERS_SELFTEST_FINISH 1
int hb_selftest_off_powers(const uint64_t *p_limbs, int n_limbs, int what, uint64_t *powers, int64_t item_stride, int64_t power_stride, const uint64_t *x,
                           const uint64_t *r, int m, int w, uint64_t *out, int64_t count);
/* host-side run of the two rows of hb_offsb.hip (no GPU needed) over host memory, with the index arithmetic and the argument checks of
 * the entry points:
 *   what = HB_OFF_SB_SELFTEST_LEAVES  as hb_off_sb_leaves: bits [L][count], bound_limbs (or NULL: p - 1); out0, out1 = g, p [L][count];
 *                                     candidates and index are not read
 *          HB_OFF_SB_SELFTEST_FINISH  as hb_off_sb_finish: bits [L][candidates], index [count]; out0 = r [count], out1 = r_bits [L][count];
 *                                     bound_limbs is not read */
#define HB_OFF_SB_SELFTEST_LEAVES 0
#define HB_OFF_SB_SELFTEST_FINISH 1
int hb_selftest_off_share_bits(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *bits, int L, const uint64_t *bound_limbs, int64_t candidates,
                               const int64_t *index, uint64_t *out0, uint64_t *out1, int64_t count);
/* host-side run of the root-finding kernels' bodies (no GPU needed) over host memory, phase by phase as the kernels' workgroups walk
 * them.  For tests only: not a fallback.
 *   what = HB_RF_SELFTEST_NEWTON  operands[0] = sums [k]; params = {k}; out [k + 1] as hb_rf_newton writes coeffs_dev
 *          HB_RF_SELFTEST_STEP    operands[0..2] = s [d + 1] (monic), h [d], a [1]; params = {d, mul}; out [d] = h^2 (x + a)^mul mod s,
 *                                 one step of the chain as a node of degree d takes it (table, tiled square and reduction above
 *                                 HB_RF_SMALL_DEGREE, the one-workgroup step at or below)
 *          HB_RF_SELFTEST_GCD     operands[0..1] = A [da + 1], B [db + 1], db <= da; params = {da, db}; out [da + 2]: word 0 = the degree,
 *                                 elements 1 .. the monic gcd
 *          HB_RF_SELFTEST_SHIFT   params = {seed, level, node, draw}; out [1] = the shift
 *          HB_RF_SELFTEST_ROOTS   operands[0] = coeffs [k + 1]; params = {k, seed}; out [k + 1]: the first 8 bytes = the number of roots
 *                                 (-1: not a product of linear factors), elements 1 .. the roots in the order found: the whole level
 *                                 loop of hb_rf_roots over host memory (its levels, rounds and nodes: hb_debug_rf_stats) */
#define HB_RF_SELFTEST_NEWTON 0
#define HB_RF_SELFTEST_STEP 1
#define HB_RF_SELFTEST_GCD 2
#define HB_RF_SELFTEST_SHIFT 3
#define HB_RF_SELFTEST_ROOTS 4
int hb_selftest_rf(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *operands, const int64_t *params, uint64_t *out);
/* host-side run of the matrix-product kernels' bodies (no GPU needed) over host memory, workgroup by workgroup and lane by lane.
 * For tests only: not a fallback.  what = the epilogue (HB_MAT_NONE / ADD / SUB), or-ed with nothing (the unsplit launch),
 * HB_MAT_SELFTEST_SPLIT (params[4] slices of whole tile depths, then the reduction launch) or HB_MAT_SELFTEST_AUTO (the rule
 * hb_mat_mul applies).  operands[0..2] = A, B, C; params = {batch, m, k, n, slices}; the argument table of hb_mat_mul. */
#define HB_MAT_SELFTEST_SPLIT 0x100
#define HB_MAT_SELFTEST_AUTO 0x200
int hb_selftest_mat(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *operands,
                    const int64_t *params, uint64_t *out);
/* host-side run of the sorting kernels' rows (no GPU needed) over host memory, slot by slot, with the index arithmetic and the
 * argument checks of the entry points.  params = {n, batch, width, a, r, d, cnt, k, kappa}; slots = batch cnt:
 *   what = HB_SORT_SELFTEST_CMP_MASK     operands[0..1] = table (column 0 is read), bits [k + kappa][slots]; outs[0..1] = masked, r1
 *          HB_SORT_SELFTEST_SWAP_MASK    operands[0..6] = table, c, r1, carry, p [width][slots], q, inv2m (one element); outs[0] [2 width][slots]
 *          HB_SORT_SELFTEST_SWAP_FINISH  operands[0..3] = opened [2 width][slots], p, q, pq; outs[0] = the table, updated in place */
#define HB_SORT_SELFTEST_CMP_MASK 0
#define HB_SORT_SELFTEST_SWAP_MASK 1
#define HB_SORT_SELFTEST_SWAP_FINISH 2
int hb_selftest_sort(const uint64_t *p_limbs, int n_limbs, int what, const uint64_t *const *operands, const int64_t *params,
                     uint64_t *const *outs);

#ifdef __cplusplus
}
#endif
#endif /* HBMPC_HIP_H */

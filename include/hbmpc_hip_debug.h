/*
 * hbmpc_hip_debug.h -- diagnostic entry points of libhbmpc_hip.so used by scratch/ scripts and a few white-box tests.
 * NOT part of the drop-in surface declared in hbmpc_hip.h; signatures may change between rounds.
 */
#ifndef HBMPC_HIP_DEBUG_H
#define HBMPC_HIP_DEBUG_H

#include "hbmpc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*  * hb_debug_mm8_*: the int8 matrix-core mat-vec of csrc/hb_mfma.hip on its own -- table for the points
 * x_host (n points, d terms), then out(c, i) = sum_l x_i^l in(c, l) with explicit views; HB_ERR_UNSUPPORTED
 * when the shapes do not qualify.  hb_debug_occupancy: resident workgroups per CU the runtime reports for
 * the second-generation kernels at a given inner dimension. */
int hb_debug_mm8_create(hb_ctx *ctx, const uint64_t *x_host, int n, int d, void **out);
int hb_debug_mm8_apply(hb_ctx *ctx, void *mat, const void *in_dev, int64_t in_sc, int64_t in_sl, int64_t in_count,
                       void *out_dev, int64_t out_sc, int64_t out_sl, int64_t out_count, int64_t n_chunks,
                       const int32_t *check_mask_dev, int32_t *mismatch_dev);
int hb_debug_occupancy(int n_in, int nl, int *mv3, int *dc);
/* The library reads its environment hooks (HB_NO_QUICK, HB_GAO_PAIR, ...: DESIGN.md section 7) once, at the first question any of them is
 * asked.  A test that flips one inside a process calls this to have them read again. */
void hb_debug_reload_env(void);
/* Cap, in bytes, on the per-slab temporaries of hb_pm_power_sums / hb_pm_powers (hbmpc_hip.h; 256 MiB): a test sets a small one to put
 * a slab boundary inside a small client count.  0 restores the default.  Process-wide. */
void hb_debug_pm_slab_bytes(int64_t bytes);
/* What the last hb_rf_roots of the process did: out[0..7] = levels of the split tree, kernel launches, stream synchronisations, rounds of
 * the repeated-root loop, and -- in profile mode only -- microseconds in the chains, in the GCDs and divisions, and waiting for the
 * degrees; out[7] = nodes processed over all levels.  Profile mode waits for the stream after every stage so that the time can be
 * charged to it: for scratch/time_solver.py, not for timing the call as a whole.  Process-wide.
 * hb_selftest_rf(HB_RF_SELFTEST_ROOTS), the same level loop over host memory, publishes its levels, rounds and nodes here too (the
 * other five are zero: it launches and waits for nothing), so a test can hold the device's walk against the host's. */
void hb_debug_rf_stats(int64_t *out);
void hb_debug_rf_profile(int on);
/* How hb_mat_mul cuts the inner dimension: 0 its own rule (hbmpc_hip.h), 1 slices of one tile depth whenever the output gives few
 * enough workgroups (a small shape takes the split path), -1 never.  Process-wide. */
void hb_debug_mat_split(int mode);
/* Which kernel an hb_matvec / hb_matvec_check of C chunks over this handle launches, asked of the launch's own rule (launch_matvec,
 * hb_core.hip; the geometry of hb_mfma_wide.hip with its per-matrix and per-context memo): out[0] = 0 the integer kernel k_matvec, 1 the
 * full-size matrix-core kernel k_mm8w in its unit launch, 2 its balanced launch k_mm8w_flat; out[1..7] = rows a row tile, row tiles,
 * K-blocks, K-blocks peeled, chunk tiles a unit, row tiles a row group, ring slots (all 0 with out[0] = 0; k_mm8w<CHECK, PEEL, K> has
 * PEEL = out[4], K = out[1] / 4).  Builds the handle's int8 image if no launch has yet -- exactly as the first launch would, the
 * environment hooks of that moment included -- and launches no mat-vec.  out: int32[8], host. */
int hb_debug_matvec_route(hb_ctx *ctx, const hb_matrix *m, int64_t C, int32_t *out);
/* Which path an hb_fft_batch_evaluate of this order with d coefficients and k outputs a polynomial takes, asked of the call's own rule
 * (fft_route, hb_ntt.hip: the call itself decides there), the environment hooks of the moment included; no launch.  out[0] = 0 the
 * Vandermonde mat-vec at the powers of omega (d = 0: the outputs are zero-filled instead), 1 the whole transform in LDS (k_ntt_lds), 2 the four-step transform over it, 3 the stage
 * loop over HBM (HB_NTT_STAGE_LOOP=1, orders beyond 2^22); out[1], out[2] = n1, n2 of the four-step (else 0); out[3] = polynomials a
 * workgroup of the LDS launch takes when the batch holds at least as many (else 0).  The same argument checks as the call: HB_ERR_BAD_ARG
 * where it would refuse.  out: int32[4], host. */
int hb_debug_fft_route(hb_ctx *ctx, int order, int d, int k, int32_t *out);
/* The packed last row tile of the fused decode + validate kernel (csrc/hb_mfma_fused.hip, FsPack), host arithmetic only.
 * hb_debug_fs_pack_rows: the decision for an image of n_coef coefficient rows (small[i] != 0: row i has no digit above the eighth) and nc
 * compared rows over d terms; returns 1 if the last tile packs, out[0] = merged rows, out[1] = single-group rows, out[2..9] = the
 * coefficient rows that are the single-group ones.  hb_debug_fs_pack_points: the same from the arrival points themselves (xz: d distinct
 * integers below 2^16); small_out (n_coef bytes, may be null) receives the flags it derived.  hb_debug_fs_slot: the image slot
 * (16 row tile + M row) of matrix row i under such a decision, *kind = 0 unpacked, 1 merged (digit group 1 on M row + 8), 2 single-group.
 * hb_debug_fs_last_pack: the form of the last row tile at the process's last launch of the kernel -- 0 unpacked, 1 merged outputs alone,
 * 2 merged outputs and single-group rows; -1 before any launch.
 * hb_debug_fs_last_mscale: 1 if that launch divided the received columns by den on the matrix cores, 0 if by the T_q multiplication
 * (HB_NO_FUSED_MSCALE=1, a decoder's launch, tables that do not fit the LDS); -1 before any launch. */
int hb_debug_fs_pack_rows(int d, int n_coef, int nc, const uint8_t *small, int32_t *out);
int hb_debug_fs_pack_points(const int32_t *xz, int d, int n_coef, int nc, int32_t *out, uint8_t *small_out);
int hb_debug_fs_slot(int nm, int ns, const int32_t *single, int i, int n_out, int32_t *kind);
int hb_debug_fs_last_pack(void);
int hb_debug_fs_last_mscale(void);
/* The tower bodies of csrc/hb_fq12_elem.hpp on the DEVICE, one operation a launch: what hb_selftest_pairing(HB_PAIR_SELFTEST_TOWER) runs
 * on the host (the same function, pair_tower_elem), so that the device build of the Fq, Fq2, Fq6 and Fq12 code can be fed chosen operands
 * instead of what a Miller loop happens to produce.  k_pair_op: 64-lane workgroups, one item a lane, as k_pair_product.
 *   op     an HB_PAIR_OP_* of hbmpc_hip.h (arg as there: the Frobenius power, else 0) or one of the three Fq operations below, which
 *          work on coordinate 0 of a (and of b) and copy the other eleven coordinates of a through:
 *            HB_PAIR_OP_FQ_MUL       a0 b0 mod Q: to Montgomery form, one fq_mul, back; arg = 0
 *            HB_PAIR_OP_FQ_MUL_LAZY  arg = 16 log2(ka) + log2(kb), ka, kb in {1, 2, 4, 8}: ka a0 and kb b0 formed by fq_add_lazy doublings of
 *                                    the Montgomery residues (no conditional subtraction: the Karatsuba factor sums of the tower, up to
 *                                    8 Q), ONE fq_mul, back: ka kb a0 b0 mod Q
 *            HB_PAIR_OP_FQ_INV       1 / a0 mod Q, 0 -> 0; arg = 0
 *          The self test takes these three op codes too.
 *   a_dev, b_dev, out_dev  72 words an item, twelve residues; b_dev is read by the two-operand operations only (may be null otherwise)
 *   status_dev[i] = 1 if every residue of item i that was read is below Q, else 0 and the item's output is zero-filled
 * HB_ERR_BAD_ARG: an unknown op, an arg the op does not take, a null pointer, a negative count, a pointer not aligned to 16 bytes, an
 * output overlapping an input or the other output.  A zero count returns HB_OK and launches nothing.  A context over R in four limbs, as
 * hb_pair_product; asynchronous on `stream`, nothing allocated. */
#define HB_PAIR_OP_FQ_MUL 17
#define HB_PAIR_OP_FQ_MUL_LAZY 18
#define HB_PAIR_OP_FQ_INV 19
int hb_debug_pair_op(hb_ctx *ctx, int op, int64_t arg, const uint64_t *a_dev, const uint64_t *b_dev, uint64_t *out_dev, int32_t *status_dev, int64_t count, void *stream);
/* The bare square root and endomorphism of csrc/hb_g1_wire_elem.hpp on the DEVICE: the per-item functions of the self test's
 * HB_G1_WIRE_SELFTEST_SQRT and HB_G1_WIRE_SELFTEST_PHI cases (`what` is one of the two), 256-lane workgroups, one item a lane.
 *   SQRT  in_dev: 6 words an item, a residue a; out_dev: 6 words, a^((Q + 1) / 4) if that squares to a, else zero; flags_dev[i] = 1 a
 *         square, 0 not, -1 a not below Q (output zero)
 *   PHI   in_dev, out_dev: 12 words an item, a point (x, y) -> (beta x, y); flags_dev is not used and may be null
 * HB_ERR_BAD_ARG: another `what`, a null pointer, a negative count, a pointer not aligned to 16 bytes, overlapping buffers.  A zero count
 * returns HB_OK and launches nothing.  A context over R in four limbs. */
int hb_debug_g1_wire_op(hb_ctx *ctx, int what, const uint64_t *in_dev, uint64_t *out_dev, int32_t *flags_dev, int64_t count, void *stream);


#ifdef __cplusplus
}
#endif
#endif /* HBMPC_HIP_DEBUG_H */

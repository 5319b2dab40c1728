/*
 * ultrare_attr_train.h -- in-training attribute unlearning (csrc/attr_train.hip): part of the C ABI of libultrare_hip.so, included by
 * ultrare_hip.h.  New symbols; URE_ABI_VERSION is unchanged, as for the other CSR entries.  The reference adds, at every optimizer
 * step, eta * mmd_loss(U[user1], U[user2]) ('d2d') or eta * trace(U^T Lap U) ('u2u') over the batch's distinct users of two attribute
 * groups (utils.py:46-111).  The rows of a step and their counts change every step, so they live in device memory: nothing below
 * takes a count from the host, and nothing is read back.  The arithmetic is stated in numpy in ultrare_amd/attr_train.py
 * (selection, validity, hand-off) and ultrare_amd/attr_unlearn.py (the losses); DESIGN.md 4.29.
 *
 * counts (device) int32 [2] = (n1, n2) of the step, m = n1 + n2; cap1, cap2 (host) >= 1 are the capacities: n1 <= cap1, n2 <= cap2
 * (a larger count is read as the capacity), cap = cap1 + cap2, 2 <= cap <= 2^31 - 65.  rows (device) int32 [cap]: the first n1 the
 * source group S, the next n2 the target group T; what follows is not read.  Grids and scratch are planned from the capacities
 * (ure_attr_scratch(cap, d) bytes: ure_mmd_scratch's layout at m = cap, never quadratic in cap; -1 for a shape the calls refuse).
 * valid (device) int32 [1] is 1 when n1 >= 1 and n2 >= 1 and -- for the MMD -- the bandwidth is positive and finite, else 0: the
 * step's term is then skipped (value 0, gradient +0.0) where the reference would produce NaN.
 * The results are a function of (counts, capacities, d, the data) alone: a fixed summation order, no floating-point atomics, equal
 * bytes on any stream.  Argument checks come before any HIP call; the memory contract is DESIGN 4.20's (every byte of every output
 * written, nothing read that the call did not write, scratch exactly the sizer's).  Nothing synchronises.
 */
#ifndef ULTRARE_ATTR_TRAIN_H
#define ULTRARE_ATTR_TRAIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Once per epoch.  off (device) int64 [n_user + 1] and tag (device) int32 [nnz] are a shard's CSR and the step of every CSR entry
 * (ure_gcn_gather_tags); group (device) int8 [n_user]: 0 none, 1 source, 2 target.  masks (device) uint32 [n_user][words],
 * words = ceil(steps / 32): bit s of user u is set iff group[u] != 0 and u has an entry with tag == s (a tag outside [0, steps) sets
 * nothing); rows of any length; every word is written. */
int ure_attr_step_masks(const int64_t *off, const int32_t *tag, const int8_t *group, int64_t n_user, int64_t nnz, int32_t steps, uint32_t *masks,
                        void *stream);
/* Per step.  rows [cap1 + cap2] = the users of group 1 whose bit `step` is set, in ascending id, then those of group 2, in ascending
 * id; the entries behind them are written -1; counts = (n1, n2).  An ordered compaction by prefix sums: no atomics.  scratch:
 * ure_attr_select_scratch(n_user) bytes. */
int64_t ure_attr_select_scratch(int64_t n_user);
int ure_attr_select(const uint32_t *masks, const int8_t *group, int64_t n_user, int32_t steps, int32_t step, int64_t cap1, int64_t cap2, int32_t *rows,
                    int32_t *counts, void *scratch, int64_t scratch_bytes, void *stream);

int64_t ure_attr_scratch(int64_t cap, int32_t d);
/* *bandwidth (device float64) = fix_sigma when fix_sigma > 0, else ure_mmd_bandwidth's closed form over the m selected rows (0.0 for
 * m < 2); *valid as above (the MMD's). */
int ure_attr_bandwidth(const float *X, int64_t ld, int32_t d, const int32_t *rows, const int32_t *counts, int64_t cap1, int64_t cap2, double fix_sigma,
                       double *bandwidth, int32_t *valid, void *scratch, int64_t scratch_bytes, void *stream);
/* ure_mmd_bandwidth + ure_mmd_loss_grad at the step's counts: the same tile arithmetic, the coefficients 2 / n1^2, 2 / n2^2 and
 * -2 / (n1 n2) derived on the device, tiles past m contributing exact zeros.  sums (device float64 [4]) as ure_mmd_loss_grad's; grad
 * (device float32 [cap x d]): rows at or beyond m are +0.0.  When *valid is 0, sums and grad are +0.0 throughout.  bandwidth
 * (device float64, optional) receives the bandwidth used.  acc (device float64, optional, in place): the loss
 * sums[0] / n1^2 + sums[1] / n2^2 - sums[2] / (n1 n2) - sums[3] / (n1 n2) is added to it only when valid; skipped (device int32,
 * optional, in place) is advanced by one only when not. */
int ure_attr_mmd_loss_grad(const float *X, int64_t ld, int32_t d, const int32_t *rows, const int32_t *counts, int64_t cap1, int64_t cap2,
                           double kernel_mul, int32_t kernel_num, double fix_sigma, double *bandwidth, double *sums, float *grad, int32_t *valid,
                           double *acc, int32_t *skipped, void *scratch, int64_t scratch_bytes, void *stream);
/* ure_u2u_loss_grad at the step's counts: *value (device float64; 0.0 when not valid), grad, valid (n1 >= 1 and n2 >= 1), acc and
 * skipped as above. */
int ure_attr_u2u_loss_grad(const float *X, int64_t ld, int32_t d, const int32_t *rows, const int32_t *counts, int64_t cap1, int64_t cap2, double *value,
                           float *grad, int32_t *valid, double *acc, int32_t *skipped, void *scratch, int64_t scratch_bytes, void *stream);
/* The hand-off, in place: G[rows[i]][c] = fl(G[rows[i]][c] + fl(eta * grad[i][c])) for i < n1 + n2, c < d, and only when *valid;
 * every other byte of G (device float32 [n_rows] rows of stride ldg >= d) is untouched.  A row id outside [0, n_rows) is passed
 * over. */
int ure_attr_add_grad(float *G, int64_t ldg, int64_t n_rows, int32_t d, const int32_t *rows, const int32_t *counts, int64_t cap, const int32_t *valid,
                      const float *grad, float eta, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ULTRARE_ATTR_TRAIN_H */

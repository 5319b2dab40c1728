/*
 * ultrare_bpr.h -- BPR training with device-side negative sampling (csrc/bpr.hip): part of the C ABI of libultrare_hip.so,
 * included by ultrare_hip.h.  New symbols; URE_ABI_VERSION is unchanged, as for the other CSR entries.  The arithmetic is stated
 * in numpy in ultrare_amd/bpr.py and the kernels are held to it: integers and the gradient walks bit for bit, the coefficient w
 * to one float32 ulp of its float64 value.
 *
 * The graph is ultrare_gcn.h's (CSR: off_u, col, row_u, pos; CSC: off_i, row, to_csr) with, beside it, the users' DISTINCT items
 * (off_d [n_user + 1] int64, col_d [nnz_d] int32, ascending inside a user: the CSR itself when no pair repeats).  A batch is
 * the set of CSR entries q with tag[q] == step (ure_gcn_gather_tags); every entry is a positive (u, i) = (row_u[q], col[q]) and has
 * one negative item neg[q] per epoch.  Per step, for x_q = s(u, i) - s(u, neg_q) over the final tables: the loss is
 * sum_q -log sigmoid(x_q) and its gradient with respect to x_q is w_q = -1 / (1 + exp(x_q)).
 *
 * As in ultrare_gcn.h: every float operation is ONE float32 operation rounded on its own, a chain stays in one lane in ascending
 * entry position, a row -- however long -- stays with its group of d / 4 lanes; no floating-point atomics, nothing summed
 * across workgroups (but the float64 loss, by ure_gcn_step_loss); integer atomics only in the sort's histograms, whose sums do
 * not depend on their order.  n_user, n_item, nnz in 1 .. 2^31 - 1; d a power of two in 4 .. 256; an index outside its range is
 * read as the nearest valid one.  Argument checks come before any HIP call.  Memory contract: DESIGN.md 4.20 (ure_bpr_index
 * takes scratch of ure_bpr_index_scratch bytes).  Nothing synchronises.
 */
#ifndef ULTRARE_BPR_H
#define ULTRARE_BPR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The negatives of one epoch, for all nnz CSR entries.  With u = row_u[q], p = pos[q] (the entry's FILE position), c = u's
 * distinct items and m = n_item - len(c), in wrapping uint64 arithmetic:
 *   mix(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; z ^ (z >> 31)
 *   z = mix(key + 0x9E3779B97F4A7C15 * (1 + (epoch << 32) + p));  r = ((z >> 32) * m) >> 32;  neg[q] = r + #{t : c[t] - t <= r}
 * -- the r-th item u has no triple for, uniform over them, whatever the launch shape.  A user with m = 0 (callers refuse it)
 * gets n_item - 1.  neg must not overlap an input. */
int ure_bpr_sample(const int64_t *off_d, const int32_t *col_d, int64_t nnz_d, const int32_t *row_u, const int32_t *pos, int64_t nnz,
                   int64_t n_user, int64_t n_item, uint64_t key, int32_t epoch, int32_t *neg, void *stream);
/* Bytes of scratch ure_bpr_index needs (0 for sizes it refuses). */
int64_t ure_bpr_index_scratch(int64_t nnz, int64_t n_item);
/* The entries grouped by negative item -- the stable sort of q = 0 .. nnz - 1 by neg[q]: map_n [nnz] the CSR positions (ascending
 * inside an item), off_n [n_item + 1] the items' offsets into it, usr_n[t] = row_u[map_n[t]].  An LSD radix sort with 8-bit
 * digits, ceil(log2(n_item) / 8) passes (at least one), on the device and deterministic.  Outputs, inputs and scratch must not
 * overlap. */
int ure_bpr_index(const int32_t *neg, const int32_t *row_u, int64_t nnz, int64_t n_item, int64_t *off_n, int32_t *map_n, int32_t *usr_n,
                  void *scratch, int64_t scratch_bytes, void *stream);
/* The coefficient pass over the CSR entries k = 0 .. nnz - 1.  For an entry of the batch (tag[k] == step): s_pos and s_neg = the
 * bytes ure_score gives ONE model (U, V) at (row[k], col[k]) and (row[k], neg[k]) (csrc/score_dot.h), x[k] = fl(s_pos - s_neg),
 * w[k] = (float)(-1.0 / (1.0 + exp((double)x[k]))) -- within one float32 ulp of the real value; exactly -0.5f at x = 0.  Every
 * other entry gets +0.0 in w and x.  pos_out, neg_out (optional, [nnz]): the two scores, +0.0 outside the batch. */
int ure_bpr_coef(const int32_t *row, const int32_t *col, const int32_t *neg, const int32_t *tag, int64_t nnz, int32_t step, const float *U,
                 const float *V, int64_t n_user, int64_t n_item, int32_t d, float *w, float *x, float *pos_out, float *neg_out, void *stream);
/* The user walk.  For user r and column c, over the row's CSR entries k in ascending position that are in the batch, from +0.0f:
 * g = fl(g + fl(w[k] * fl(V[col[k]][c] - V[neg[k]][c]))); G[r][c] = g, +0.0 in every byte for a row without an entry in the batch.
 * row_loss (optional, float64 [n_user]): the chain from 0.0 over the same entries of max(-x, 0) + log1p(exp(-|x|)) at
 * (double)x[k].  G must not overlap V. */
int ure_bpr_grad_user(const int64_t *off, const int32_t *col, const int32_t *neg, const int32_t *tag, const float *w, const float *x,
                      int64_t n_user, int64_t n_item, int64_t nnz, int32_t step, const float *V, int32_t d, float *G, double *row_loss,
                      void *stream);
/* The item walk, one launch: for item r and column c ONE chain from +0.0f.  First the item's CSC entries k in ascending position
 * whose CSR position q = to_csr[k] is in the batch: g = fl(g + fl(w[q] * U[row[k]][c])); then, in the same accumulator, the
 * item's entries t of the negative index in ascending position whose q = map_n[t] is in the batch:
 * g = fl(g + fl(fl(-w[q]) * U[usr_n[t]][c])).  G[r][c] = g, +0.0 in every byte for a row with neither.  G must not overlap U. */
int ure_bpr_grad_item(const int64_t *off_i, const int32_t *row, const int32_t *to_csr, const int64_t *off_n, const int32_t *map_n,
                      const int32_t *usr_n, const int32_t *tag, const float *w, int64_t n_item, int64_t n_user, int64_t nnz, int32_t step,
                      const float *U, int32_t d, float *G, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ULTRARE_BPR_H */

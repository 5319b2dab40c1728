/*
 * ultrare_gcn.h -- the LightGCN backbone (csrc/gcn.hip): part of the C ABI of libultrare_hip.so, included by ultrare_hip.h.
 * New symbols; URE_ABI_VERSION is unchanged, as for the other CSR entries.  The reference has no such source (its README
 * names the backbone as the next one); the arithmetic is stated in numpy in ultrare_amd/lightgcn.py and the kernels are held
 * to it bit for bit.
 *
 * A shard's graph is held twice on the device, as for ure_csr_cost: off [n_dst + 1] int64 and idx [nnz] int32 of the rows of
 * one side (CSR: a user's items; CSC: an item's users), entries of a row in a FIXED order (lightgcn.Graph: by (row, index,
 * file position); a repeated pair is two entries).  s (float32 per node) = (float)(1 / sqrt((double)deg)), 0 for a node
 * without entries: made by the host, an input here.  Tables are row-major [rows][d] float32, d a power of two in 4 .. 256.
 *
 * Every float operation below is ONE float32 operation rounded on its own (no fma); the chain of a (row, column) stays in one
 * lane and is never split or reordered; a row -- however long -- stays with the one group of d / 4 lanes that owns it.  No
 * floating-point atomics, nothing is summed across workgroups (but the float64 loss, in its stated order): a row's bytes depend
 * on its own entries and the source table alone, on any stream.  n_dst, n_src, nnz in 1 .. 2^31 - 1 (a kernel argument must
 * not be NULL: an empty graph passes one unused entry and nnz = 0 is refused); an index outside [0, n_src) is read as the
 * nearest valid one (callers check their graphs).  Argument checks come before any HIP call.  None of the entries needs
 * scratch memory, so there are no sizers.  Memory contract: DESIGN.md 4.20; ure_gcn_sgd_step and ure_gcn_step_loss are
 * in-place entries.  Nothing synchronises.
 */
#ifndef ULTRARE_GCN_H
#define ULTRARE_GCN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One propagation, serving both sides and both directions.  For output row r and column c, over the row's entries j in
 * ascending position from +0.0f: t = fl(t + fl(s_src[j] * X[j][c])); y = fl(s_dst[r] * t); y' = add ? fl(add[r][c] + y) : y;
 * out[r][c] = y'; sum (optional, in place) : sum[r][c] = fl(sum[r][c] + y').  An empty row gives +0.0 (or add unchanged).
 * X [n_src][d]; add, sum, out [n_dst][d].  out must not overlap X; out may BE add (each lane reads its own columns before it
 * writes them), no other overlap of add, sum and out with each other or with X. */
int ure_gcn_propagate(const int64_t *off, const int32_t *idx, int64_t n_dst, int64_t n_src, const float *s_src, const float *s_dst,
                      const float *X, int32_t d, const float *add, float *sum, float *out, void *stream);
/* out[i] = fl(X[i] * c) for n floats, n a multiple of 4 (the layer mean's 1 / (L + 1)); out may be X. */
int ure_gcn_scale(const float *X, int64_t n, float c, float *out, void *stream);
/* tag[k] = file_tag[pos[k]] for the nnz entries of the CSR (pos: an entry's file position; file_tag: the step of the epoch in
 * which every triple trains): once per epoch. */
int ure_gcn_gather_tags(const int32_t *file_tag, const int32_t *pos, int64_t nnz, int32_t *tag, void *stream);
/* The residual pass over the CSR entries k = 0 .. nnz - 1 (row[k], col[k]: the entry's user and item; rating[k]: its rating, in
 * CSR order).  An entry with tag[k] == step is in the batch: pred = the bytes ure_score gives ONE model (U, V) at (row[k],
 * col[k]) (csrc/score_dot.h), err[k] = fl(pred - rating[k]).  Every other entry gets err[k] = +0.0 (the gradient walks go by
 * the tag, not by this value).  pred_out (optional, [nnz]): pred, and +0.0 outside the batch. */
int ure_gcn_residual(const int32_t *row, const int32_t *col, const float *rating, const int32_t *tag, int64_t nnz, int32_t step,
                     const float *U, const float *V, int64_t n_user, int64_t n_item, int32_t d, float *err, float *pred_out, void *stream);
/* One masked walk.  For row r of this side and column c, over the row's entries k in ascending position that are in the batch
 * (tag[q] == step, q = map ? map[k] : k -- the entry's CSR position; map is NULL on the CSR side), from +0.0f:
 * g = fl(g + fl(fl(2 err[q]) * T[idx[k]][c])); G[r][c] = g, +0.0 in every byte for a row without an entry in the batch.
 * T [n_src][d] is the OTHER side's table.  row_loss (optional, float64 [n_dst]): the chain from 0.0 over the same entries of
 * (double)err[q] * (double)err[q].  Every row reads all its entries each step, although few are in the batch. */
int ure_gcn_grad(const int64_t *off, const int32_t *idx, const int32_t *map, const int32_t *tag, const float *err, int64_t n_dst,
                 int64_t n_src, int64_t nnz, int32_t step, const float *T, int32_t d, float *G, double *row_loss, void *stream);
/* The loss of a step from its rows' sums, in ure_epoch_sse_batch's order: lane t of 256 adds row_loss[t], row_loss[t + 256],
 * ... in ascending order from 0.0, the 256 lane sums are folded pairwise (w = 128 .. 1: lane t += lane t + w);
 * loss[0] = (first ? 0.0 : loss[0]) + that sum -- an epoch's steps are added in step order. */
int ure_gcn_step_loss(const double *row_loss, int64_t n, int32_t first, double *loss, void *stream);
/* torch.optim.SGD(momentum = mu, weight_decay = lam) on n floats (n a multiple of 4; both parameter tables in one call when they
 * are contiguous), in place: g0 = fl(g[i] * gscale) (the backward's 1 / (L + 1); 1.0f is exact); g' = fl(g0 + fl(lam * w));
 * m = first ? g' : fl(fl(mu * m) + g'); w = fl(w - fl(lr * m)).  first: the first step of the job (m is written, not read).
 * Zero columns with zero g stay exactly zero.  w, m and g must not overlap. */
int ure_gcn_sgd_step(float *w, float *m, const float *g, int64_t n, float gscale, float lr, float lam, float mu, int32_t first, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ULTRARE_GCN_H */

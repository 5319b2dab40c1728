/*
 * ultrare_nmf.h -- the NeuMF backbone (csrc/nmf.hip): part of the C ABI of libultrare_hip.so, included by ultrare_hip.h.
 * New symbols; URE_ABI_VERSION is unchanged, as for the other CSR entries.  The reference names the model (its SISA merge
 * handles user_mat_mf and user_mat_mlp) and has no source for it; the arithmetic is stated in numpy in ultrare_amd/nmf.py and
 * the kernels are held to it bit for bit.
 *
 * The model (He et al. 2017, as rating regression): GMF width k, MLP layers[0 .. m] = L0 .. Lm (n_layers = m + 1, 1 <= m <= 4),
 * e = L0 / 2; every width a power of two, k and L1 .. Lm in 4 .. 128, L0 in 8 .. 128.  Tables are held per side, GMF and MLP
 * columns in one row: U [n_user][k + e] = [pg | pm], V [n_item][k + e] = [qg | qm].  Every other parameter lives in ONE float
 * vector `dense` of ure_nmf_dense_size floats: W_0 [L1][L0] row-major, b_0 [L1], W_1, b_1, ..., h [k + Lm], c, and zeros up to
 * a multiple of 4 (so that ure_gcn_sgd_step updates tables and dense in one call when they are contiguous).
 *
 * Forward of a pair (u, i), every operation ONE float32 operation rounded on its own (no fma), every chain held by one lane in
 * ascending index from +0.0f:
 *   g[c]      = fl(pg[c] * qg[c])                                                  c < k
 *   a_0       = [pm ; qm]
 *   z         = fl(chain_i fl(W_j[o][i] * a_j[i]) + b_j[o]);  a_(j+1)[o] = z <= 0 ? +0.0 : z
 *   pred      = fl(chain(fl(h[c] * g[c]), c < k, then fl(h[k + c] * a_m[c]), c < Lm) + c)
 * Backward of sum err^2, err = fl(pred - rating), ge = fl(2 * err):
 *   dg[c]     = fl(ge * h[c]);  dpg[c] = fl(dg[c] * qg[c]);  dqg[c] = fl(dg[c] * pg[c])
 *   delta_m[o] = a_m[o] > 0 ? fl(ge * h[k + o]) : +0.0
 *   t[i]      = chain_o fl(W_j[o][i] * delta_(j+1)[o]);  delta_j[i] = a_j[i] > 0 ? t[i] : +0.0 (j >= 1);  [dpm ; dqm] = t (j = 0)
 *
 * A step's batch is named by RANK: rank[q] is the place of CSR entry q in the epoch's order (a host-made inverse permutation,
 * gathered with ure_gcn_gather_tags); entry q is in the batch iff lo <= rank[q] < lo + n_slots, and its SLOT is rank[q] - lo.
 * Per-entry intermediates live in buffers indexed by slot:
 *   err [n_slots], act [n_slots][A] = [g | a_0 | a_1 | .. | a_m] (A = k + L0 + .. + Lm), dlt [n_slots][Dw] = [delta_1 | .. |
 *   delta_m] (Dw = L1 + .. + Lm), emb [n_slots][2 (k + e)] = [dpg | dpm | dqg | dqm].
 *
 * The weights of a stack are staged once per workgroup in LDS; a stack that needs more than URE_NMF_LDS_BYTES there
 * (4 * (sum_j L_j (L_(j+1) + 1) + sum_j L_(j+1) + k + Lm + 1 + 4 (A + 256)) bytes) is refused by the argument check.
 * No floating-point atomics; nothing depends on the stream, the grid or the other entries.  n_user, n_item, nnz, n in
 * 1 .. 2^31 - 1; an index outside its table is read as the nearest valid one.  `layers` is a HOST array.  Argument checks come
 * before any HIP call.  Memory contract: DESIGN.md 4.20.  Nothing synchronises.
 */
#ifndef ULTRARE_NMF_H
#define ULTRARE_NMF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define URE_NMF_MAX_FC 4
#define URE_NMF_LDS_BYTES 61440
#define URE_NMF_CHUNK 256             /* slots of one weight-gradient chunk */

/* Floats of the dense vector (a multiple of 4), or -1 for a (k, layers) the kernels refuse. */
int64_t ure_nmf_dense_size(int32_t k, const int32_t *layers, int32_t n_layers);
/* The training pass over the CSR entries q = 0 .. nnz - 1 (row[q], col[q]: the entry's user and item; rating[q] in CSR order).
 * An entry of the batch runs forward and backward as stated above and writes err, act, dlt and emb of its slot (pred_out,
 * optional [n_slots]: pred).  Every other entry writes nothing; a slot no entry has stays untouched. */
int ure_nmf_forward_backward(const int32_t *row, const int32_t *col, const float *rating, const int32_t *rank, int64_t nnz, int32_t lo,
                             int32_t n_slots, const float *U, const float *V, int64_t n_user, int64_t n_item, const float *dense, int32_t k,
                             const int32_t *layers, int32_t n_layers, float *err, float *pred_out, float *act, float *dlt, float *emb,
                             void *stream);
/* Bytes of ure_nmf_weight_grad's scratch (the chunk partials), or -1 (also for n_slots outside 1 .. 2^31 - 1 - URE_NMF_CHUNK, which
 * ure_nmf_weight_grad refuses). */
int64_t ure_nmf_weight_grad_scratch(int32_t n_slots, int32_t k, const int32_t *layers, int32_t n_layers);
/* g_dense (laid out as dense) = the sums over the slots 0 .. n_slots - 1 of: gW_j[o][i]: fl(delta_(j+1)[o] * a_j[i]); gb_j[o]:
 * delta_(j+1)[o]; gh[c]: fl(fl(2 err) * g[c]) (c < k), fl(fl(2 err) * a_m[c - k]); gc: fl(2 err); the padding: +0.0.  Each sum
 * is a two-level chain: within a chunk of URE_NMF_CHUNK consecutive slots in ascending slot from +0.0f, the chunk sums then
 * added in ascending chunk order starting FROM the first.  blocks: the workgroups of the chunk launch (0: one per chunk); the
 * result does not depend on it. */
int ure_nmf_weight_grad(const float *err, const float *act, const float *dlt, int32_t n_slots, int32_t k, const int32_t *layers,
                        int32_t n_layers, float *g_dense, void *scratch, int64_t scratch_bytes, int32_t blocks, void *stream);
/* One masked walk over a side's rows.  For row r and column c < width, over the row's entries p in ascending position that are
 * in the batch (by rank[q], q = map ? map[p] : p -- the entry's CSR position; map is NULL on the CSR side), from +0.0f:
 * g = fl(g + E[slot][col0 + c]); G[r][c] = g, +0.0 in every byte for a row without an entry in the batch.  E [n_slots][ld];
 * G [n_rows][width]; ld, col0 and width multiples of 4, width <= 256.  row_loss (optional, float64 [n_rows], with err
 * [n_slots]): the chain from 0.0 over the same entries of (double)err[slot] * (double)err[slot] -- ure_gcn_grad's, so
 * ure_gcn_step_loss folds it. */
int ure_nmf_row_sum(const int64_t *off, const int32_t *map, const int32_t *rank, int64_t n_rows, int64_t nnz, int32_t lo, int32_t n_slots,
                    const float *E, int32_t ld, int32_t col0, int32_t width, const float *err, float *G, double *row_loss, void *stream);
/* The forward alone, for ONE model at the pairs (uid[j], iid[j]), j < n, under ure_score's protocol: acc = first ? 0 : pred[j];
 * acc = fl(acc + p) with p the bytes the training forward gives; on `last` acc = fl(acc / (float)n_models_total) and (sse given)
 * the squared errors against rating go to sse [URE_SCORE_PARTIALS] as ure_score lays them out; pred[j] = acc.  An ensemble is
 * one call per model, in list order.  The sse chain (nmf.sse_ref): W = min(ceil(n / 4), URE_SCORE_PARTIALS) workgroups of four
 * waves; wave w takes the pairs j = w, w + 4 W, ... in ascending order and runs sq = fmaf(er, er, sq) from +0.0f with
 * er = fl(acc - rating[j]); sse[b] = the float64 chain from 0.0 over the four waves 4 b .. 4 b + 3 of workgroup b, 0.0 behind. */
int ure_nmf_score(const float *U, const float *V, const float *dense, int32_t k, const int32_t *layers, int32_t n_layers, int64_t n_user,
                  int64_t n_item, int32_t n_models_total, int32_t first, int32_t last, const int32_t *uid, const int32_t *iid,
                  const float *rating, int64_t n, float *pred, double *sse, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ULTRARE_NMF_H */

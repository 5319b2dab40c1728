/*
 * ultrare_nmf_rank.h -- full-catalogue top-k and exact ranks under a NeuMF ensemble (csrc/nmf_rank.hip): part of the C ABI of
 * libultrare_hip.so, included by ultrare_hip.h.  New symbols; URE_ABI_VERSION is unchanged.  The contract is stated in numpy in
 * ultrare_amd/nmf.py (recommend_ref, rank_ref; prefix_ref and forward_from_prefix_ref for the kernel's evaluation order).
 *
 * score(u, i) = the ensemble mean of the NeuMF forward (ultrare_nmf.h) under ure_nmf_score's protocol: acc = +0.0f;
 * acc = fl(acc + pred_m(u, i)) for the models in list order; fl(acc / (float)n_models) -- the bytes a chain of ure_nmf_score
 * calls (first .. last) writes for the same pair.  All models of a call share (k, layers); model m is U_tables[m]
 * [n_user][k + e], V_tables[m] [n_item][k + e] and dense_vecs[m] [ure_nmf_dense_size] (device memory; the three pointer
 * arrays are HOST arrays, as `layers` is).  Any n_models >= 1.
 *
 * Everything else is ure_recommend_topk's / ure_rank_pairs' (ultrare_hip.h): the key order (score descending, NaN below -inf,
 * -0.0 == +0.0, then item id ascending), users [n_query] (an id outside [0, n_user) reads the nearest valid row), the
 * exclusion CSR (both or neither; rows sorted and unique), 1 <= top_k <= 128, padding (NaN, -1), targets in any order with
 * duplicates and empty rows, rank -1 for an excluded target, a target of rank r < top_k being item r of the top-k row,
 * n_targets = tgt_off[n_query] read on the device and bounded by the scratch, and the memory contract.  The
 * selection and counting kernels are the MF entries' own (csrc/rec_select.h, csrc/rank_count.h) with another scorer.
 *
 * Evaluation order.  One lane holds an item, a wave QW users of the workgroup's 4 QW.  The layer-0 chain of output o runs over
 * a_0 = [pm ; qm] in ascending i from +0.0f; its first e terms depend on (model, user, o) only, are summed once per tile and
 * start every item's chain.  The operations and their order are those of ultrare_nmf.h's forward, so are the bytes.  No fused
 * multiply-add, no floating-point atomics (the bucket flush of the rank counting adds integers); results do not depend on
 * the stream, the grid or how users are batched.
 *
 * LDS.  A workgroup of the tile kernels holds, in floats: the stack's image W = sum_j (L_j (L_(j+1) + 1) + L_(j+1)) + k + Lm + 1
 * (ultrare_nmf.h), the items' halves 65 e, the users' rows and prefixes 4 QW (k + L1), and -- stacks of two and more layers --
 * activation columns 4 QW (wa + wb) (64 >> p) with wa = max(L1, L3 where a fourth layer follows), wb = L2 where a third
 * follows, p = 0 .. 3 the halvings of the lanes a wave walks at a time:
 *   tile bytes = 16 ceil(4 (W + 65 e + 4 QW (k + L1 + (wa + wb) (64 >> p))) / 16)
 * plus the selection state 4 QW (12 (top_k + 64) + 272) (top-k) or the counting state 49152 + 48 QW (ranks).  The entries take
 * the first of (QW, p) = (4, 0), (2, 0), (1, 0), (1, 1), (1, 2), (1, 3) whose sum is at most URE_NMF_RANK_LDS_BYTES; a one-layer
 * stack always runs at (4, 0).  Every stack ure_nmf_dense_size admits fits at QW = 1.
 *
 * Argument checks come before any HIP call.  Nothing synchronises.
 */
#ifndef ULTRARE_NMF_RANK_H
#define ULTRARE_NMF_RANK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define URE_NMF_RANK_LDS_BYTES 163840

/* Bytes of ure_nmf_recommend_topk's scratch (the item splits' partial lists; 0 for one split), or -1 for arguments it refuses. */
int64_t ure_nmf_recommend_scratch(int64_t n_query, int32_t n_item, int32_t top_k, int32_t n_models, int32_t k, const int32_t *layers,
                                  int32_t n_layers);
/* scores / items [n_query][top_k]: the top_k non-excluded items of every query user by key, best first; (NaN, -1) behind the
 * eligible items. */
int ure_nmf_recommend_topk(const float *const *U_tables, const float *const *V_tables, const float *const *dense_vecs, int32_t n_models, int32_t k,
                           const int32_t *layers, int32_t n_layers, int64_t n_user, const int32_t *users, int64_t n_query, int32_t n_item,
                           const int64_t *excl_off, const int32_t *excl_items, int32_t top_k, float *scores, int32_t *items, void *scratch,
                           int64_t scratch_bytes, void *stream);
/* Bytes of ure_nmf_rank_pairs' scratch for n_targets = tgt_off[n_query] targets (24 each), or -1 for arguments it refuses. */
int64_t ure_nmf_rank_pairs_scratch(int64_t n_query, int64_t n_targets, int32_t n_item, int32_t n_models, int32_t k, const int32_t *layers,
                                   int32_t n_layers);
/* ranks [n_targets], in input order: the number of non-excluded items whose key beats the target's, -1 for an excluded target. */
int ure_nmf_rank_pairs(const float *const *U_tables, const float *const *V_tables, const float *const *dense_vecs, int32_t n_models, int32_t k,
                       const int32_t *layers, int32_t n_layers, int64_t n_user, const int32_t *users, int64_t n_query, int32_t n_item,
                       const int64_t *tgt_off, const int32_t *tgt_items, const int64_t *excl_off, const int32_t *excl_items, int32_t *ranks,
                       void *scratch, int64_t scratch_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ULTRARE_NMF_RANK_H */

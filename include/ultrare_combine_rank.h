/*
 * ultrare_combine_rank.h -- full-catalogue top-k and exact ranks under the learned shard combiner (csrc/mf_combine_rank.hip):
 * part of the C ABI of libultrare_hip.so, included by ultrare_hip.h.  New symbols; URE_ABI_VERSION is unchanged.  The contract is
 * stated in numpy in ultrare_amd/combine.py (weighted_scores_ref, recommend_ref, rank_ref).
 *
 * score_w(u, i) = the float ure_score_weighted (ultrare_hip.h, "Learned shard combiner") writes to pred for the pair, bit for
 * bit, for both links: p_s = model s's float32 score as ure_score gives it for that model alone (0.f + the dot: a dot of -0.0
 * becomes +0.0); z = b, then z = z + w[s] * (double)p_s for s = 0, 1, ... in float64, every product rounded (no fma);
 * mu = z (link 0) or 1 / (1 + exp(-z)) (link 1); the score is (float)mu.  (w, b) is the row W[group_of_user[u]] of W (device,
 * [n_groups][n_models + 1] doubles), row 0 when group_of_user (device int32 [n_user]) is NULL; a user whose entry is outside
 * [0, n_groups), or whose id is outside [0, n_user), takes w = 1 / n_models, b = 0 under link 0 and NaN under link 1.  Both
 * routes call one device function for mu (link_mean, csrc/score_dot.h).  Ranking is by this float, never by z: under link 1 many
 * items of a user may share (float)mu == 1.0f or a common tiny value, and such ties are broken by the item id.
 *
 * The arguments are ure_recommend_topk's / ure_rank_pairs' followed by link, W, n_groups, group_of_user, n_user as
 * ure_score_weighted takes them, and everything else is inherited from those two entries: the key order (score descending, NaN
 * below -inf, -0.0 == +0.0, then item id ascending), the exclusion CSR, padding (NaN, -1), duplicate and empty target rows, rank
 * -1 for an excluded target, a target of rank r < k being item r of the top-k row, n_targets = tgt_off[n_query] read on the
 * device and bounded by the scratch, and the memory contract.  The selection and counting kernels are the mean
 * route's own (csrc/rec_select.h, csrc/rank_count.h) with another scorer.  No floating-point atomics; results do not depend on
 * the stream, the grid or how users are batched.
 *
 * Limits, checked before any HIP call (the sizers return -1 for what the calls refuse): 1 <= n_models <=
 * URE_MAX_MODELS_PER_CALL (the combiner's limit, not the mean route's "any"), link 0 or 1, n_groups >= 1, W non-NULL, n_user >= 1
 * with a map, d a power of two in [4, 256], 1 <= k <= 128.
 *
 * LDS.  With QW = 8 users a wave (4 at d = 256) and QT = 4 QW a workgroup, the tile kernels hold
 *   the MF tile           4 (QT d + 64 (d + 4))          50,176 at d = 128; 82,944 at d = 256
 *   the weight rows       QT (33 * 8 + 4)                 8,576 at QT = 32;  4,288 at QT = 16  (33 doubles and a "no group" flag a user)
 *   the selection state   QT (12 (k + 64) + 272)         82,432 at QT = 32, k = 128; 41,216 at QT = 16
 *   or the counting state 49,152 + 12 QT                 49,536 at QT = 32; 49,344 at QT = 16
 * The largest sums are 141,184 bytes (top-k, d = 128, k = 128) and 136,576 (ranks, d = 256), within URE_COMBINE_RANK_LDS_BYTES:
 * nothing ure_recommend_topk serves inside the limits above is refused.
 *
 * Nothing synchronises.
 */
#ifndef ULTRARE_COMBINE_RANK_H
#define ULTRARE_COMBINE_RANK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define URE_COMBINE_RANK_LDS_BYTES 163840

/* Bytes of ure_recommend_topk_weighted's scratch (ure_recommend_scratch(n_query, n_item, k)), or -1 for arguments it refuses. */
int64_t ure_recommend_weighted_scratch(int64_t n_query, int32_t n_item, int32_t k, int32_t d, int32_t n_models, int32_t link, int32_t n_groups);
/* scores / items [n_query][k]: the k non-excluded items of every query user with the largest keys under score_w, best first;
 * (NaN, -1) behind the eligible items. */
int ure_recommend_topk_weighted(const float *const *U_tables, const float *const *V_tables, int32_t n_models, const int32_t *users, int64_t n_query,
                                int32_t n_item, int32_t d, const int64_t *excl_off, const int32_t *excl_items, int32_t k, float *scores,
                                int32_t *items, void *scratch, int64_t scratch_bytes, void *stream, int32_t link, const double *W, int32_t n_groups,
                                const int32_t *group_of_user, int32_t n_user);
/* Bytes of ure_rank_pairs_weighted's scratch for n_targets = tgt_off[n_query] targets (24 each), or -1 for arguments it refuses. */
int64_t ure_rank_pairs_weighted_scratch(int64_t n_query, int64_t n_targets, int32_t n_item, int32_t d, int32_t n_models, int32_t link,
                                        int32_t n_groups);
/* ranks [n_targets], in input order: the number of non-excluded items whose key under score_w beats the target's, -1 for an
 * excluded target. */
int ure_rank_pairs_weighted(const float *const *U_tables, const float *const *V_tables, int32_t n_models, const int32_t *users, int64_t n_query,
                            int32_t n_item, int32_t d, const int64_t *tgt_off, const int32_t *tgt_items, const int64_t *excl_off,
                            const int32_t *excl_items, int32_t *ranks, void *scratch, int64_t scratch_bytes, void *stream, int32_t link,
                            const double *W, int32_t n_groups, const int32_t *group_of_user, int32_t n_user);

#ifdef __cplusplus
}
#endif
#endif /* ULTRARE_COMBINE_RANK_H */

// mf_combine_rank.hip -- full-catalogue top-k and exact ranks under the learned shard combiner, for gfx950
// (include/ultrare_combine_rank.h; the contract in numpy is ultrare_amd/combine.py: weighted_scores_ref, recommend_ref, rank_ref).
//
// The selection of rec_select.h and the counting of rank_count.h, which are the MF mean route's own, with the third scorer
// policy (CombinedScorer, rec_score.h): per model the MF tile's staging and dot products, each lane carrying z in float64 for
// its item against its wave's QW users under the users' own weight rows (staged in LDS once per tile), link_mean (score_dot.h,
// the function ure_score_weighted calls) once per (user, item).  The scores are ure_score_weighted's bit for bit.
#include "rank_count.h"

namespace ure {
namespace {

// What both entries and both sizers refuse of the combiner's part and the row width.
inline bool combined_ok(int32_t n_models, int32_t d, int32_t link, int32_t n_groups)
{
    return n_models >= 1 && n_models <= URE_MAX_MODELS_PER_CALL && (link == 0 || link == 1) && n_groups >= 1 && pow2(d) && d >= 4 && d <= 256;
}

// The widest workgroup of the two kernels fits the CU: the header's sum.
static_assert(CombinedScorer<32>::tile_lds({}) + 32 * (kRecMaxK + kRecCand) * 12 + 32 * kRecItems * 4 + 32 * 16 <= URE_COMBINE_RANK_LDS_BYTES,
              "top-k at d = 128, top_k = 128");
static_assert(CombinedScorer<64>::tile_lds({}) + kRankLdsTargets * 12 + 16 * 12 <= URE_COMBINE_RANK_LDS_BYTES, "ranks at d = 256");

}  // namespace
}  // namespace ure

using namespace ure;

extern "C" {

int64_t ure_recommend_weighted_scratch(int64_t n_query, int32_t n_item, int32_t k, int32_t d, int32_t n_models, int32_t link, int32_t n_groups)
{
    if (!combined_ok(n_models, d, link, n_groups)) return -1;
    return rec_scratch_bytes(n_query, n_item, k);
}

int ure_recommend_topk_weighted(const float *const *U_tables, const float *const *V_tables, int32_t n_models, const int32_t *users, int64_t n_query,
                                int32_t n_item, int32_t d, const int64_t *excl_off, const int32_t *excl_items, int32_t k, float *scores,
                                int32_t *items, void *scratch, int64_t scratch_bytes, void *stream, int32_t link, const double *W, int32_t n_groups,
                                const int32_t *group_of_user, int32_t n_user)
{
    URE_ARG(U_tables && V_tables);
    URE_ARG(n_models >= 1 && n_models <= URE_MAX_MODELS_PER_CALL);
    URE_ARG(link == 0 || link == 1);
    URE_ARG(n_groups >= 1);
    URE_ARG(W);
    URE_ARG(!group_of_user || n_user >= 1);
    URE_ARG(users && n_query >= 1 && n_item >= 1);
    URE_ARG(pow2(d) && d >= 4 && d <= 256);
    URE_ARG(k >= 1 && k <= kRecMaxK);
    URE_ARG((excl_off == nullptr) == (excl_items == nullptr));
    URE_ARG(scores && items);
    for (int m = 0; m < n_models; ++m) URE_ARG(U_tables[m] && V_tables[m]);
    const int64_t need = rec_scratch_bytes(n_query, n_item, k);
    URE_ARG(scratch_bytes >= need && (need == 0 || scratch));

    hipStream_t st = static_cast<hipStream_t>(stream);
    const RecArgs A = rec_args(users, n_query, n_item, excl_off, excl_items, k, scores, items, scratch);
    const float **tab = nullptr;
    if (int rc = rec_upload_tables(U_tables, V_tables, n_models, st, &tab)) return rc;
    int rc = 0;
    dispatch_group_width(d / 4, [&](auto lpr) {
        using P = CombinedScorer<decltype(lpr)::value>;
        rc = launch_rec<P>(CombinedCtx{tab, n_models, link, W, n_groups, group_of_user, n_user}, A, st);
    });
    if (rc == 0) rc = launch_rec_merge(A, st, "ure_recommend_topk_weighted");
    URE_HIP(hipFreeAsync(tab, st));
    return rc;
}

int64_t ure_rank_pairs_weighted_scratch(int64_t n_query, int64_t n_targets, int32_t n_item, int32_t d, int32_t n_models, int32_t link,
                                        int32_t n_groups)
{
    if (!combined_ok(n_models, d, link, n_groups)) return -1;
    if (n_query < 1 || n_item < 1 || n_targets < 0 || n_targets > INT32_MAX) return -1;
    return n_targets * kRankBytes;
}

int ure_rank_pairs_weighted(const float *const *U_tables, const float *const *V_tables, int32_t n_models, const int32_t *users, int64_t n_query,
                            int32_t n_item, int32_t d, const int64_t *tgt_off, const int32_t *tgt_items, const int64_t *excl_off,
                            const int32_t *excl_items, int32_t *ranks, void *scratch, int64_t scratch_bytes, void *stream, int32_t link,
                            const double *W, int32_t n_groups, const int32_t *group_of_user, int32_t n_user)
{
    URE_ARG(U_tables && V_tables);
    URE_ARG(n_models >= 1 && n_models <= URE_MAX_MODELS_PER_CALL);
    URE_ARG(link == 0 || link == 1);
    URE_ARG(n_groups >= 1);
    URE_ARG(W);
    URE_ARG(!group_of_user || n_user >= 1);
    URE_ARG(users && n_query >= 1 && n_item >= 1);
    URE_ARG(pow2(d) && d >= 4 && d <= 256);
    URE_ARG(tgt_off && tgt_items && ranks);
    URE_ARG((excl_off == nullptr) == (excl_items == nullptr));
    URE_ARG(scratch_bytes >= 0 && (scratch_bytes == 0 || scratch));
    for (int m = 0; m < n_models; ++m) URE_ARG(U_tables[m] && V_tables[m]);
    // n_targets = tgt_off[n_query] lives on the device: the scratch bounds it, and the kernels do nothing beyond that bound
    const int64_t cap = std::min<int64_t>(scratch_bytes / kRankBytes, INT32_MAX);
    if (cap == 0) return 0;

    hipStream_t st = static_cast<hipStream_t>(stream);
    const RankArgs A = rank_args(users, n_query, n_item, tgt_off, tgt_items, excl_off, excl_items, ranks, scratch, cap);
    const float **tab = nullptr;
    if (int rc = rec_upload_tables(U_tables, V_tables, n_models, st, &tab)) return rc;
    int rc = 0;
    dispatch_group_width(d / 4, [&](auto lpr) {
        using P = CombinedScorer<decltype(lpr)::value>;
        rc = launch_rank<P>(CombinedCtx{tab, n_models, link, W, n_groups, group_of_user, n_user}, A, st);
    });
    URE_HIP(hipFreeAsync(tab, st));
    return rc;
}

}  // extern "C"

// mf_rank.hip -- exact full-catalogue ranks of (user, item) pairs under an MF ensemble, for gfx950: the passes of rank_count.h
// with the MF scorer of rec_score.h (the scores are ure_score's bit for bit).
#include "rank_count.h"

using namespace ure;

extern "C" {

int64_t ure_rank_pairs_scratch(int64_t n_query, int64_t n_targets, int32_t n_item, int32_t d)
{
    if (n_query < 1 || n_item < 1 || !(pow2(d) && d >= 4 && d <= 256) || n_targets < 0 || n_targets > INT32_MAX) return -1;
    return n_targets * kRankBytes;
}

int ure_rank_pairs(const float *const *U_tables, const float *const *V_tables, int32_t n_models, const int32_t *users, int64_t n_query,
                   int32_t n_item, int32_t d, const int64_t *tgt_off, const int32_t *tgt_items, const int64_t *excl_off,
                   const int32_t *excl_items, int32_t *ranks, void *scratch, int64_t scratch_bytes, void *stream)
{
    URE_ARG(U_tables && V_tables && n_models >= 1);
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
    dispatch_group_width(d / 4, [&](auto W) {
        using P = MfScorer<decltype(W)::value>;
        rc = launch_rank<P>(typename P::Ctx{tab, n_models}, A, st);
    });
    URE_HIP(hipFreeAsync(tab, st));
    return rc;
}

}  // extern "C"

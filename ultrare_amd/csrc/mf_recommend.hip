// mf_recommend.hip -- full-catalogue top-k recommendation from an MF ensemble for gfx950.
//
// The scores and the key order are those of rec_score.h (bit for bit ure_score's ensemble mean); the selection -- candidate
// buffer, merge by rank, split merge -- is rec_select.h's with the MF scorer (MfScorer: per model the users' U rows and 64
// items' V rows staged in LDS, each lane keeping the running sums of its item against its wave's QW users in registers).
//
#include "rec_select.h"

namespace ure {

struct RecTables {
    const float *U[URE_MAX_MODELS_PER_CALL];
    const float *V[URE_MAX_MODELS_PER_CALL];
};

// tab[m] = U_m, tab[S + m] = V_m for one chunk of models (the pointers travel as kernel arguments, so the
// caller's host array may go away at once)
__global__ void rec_tables_kernel(RecTables T, int n, int m0, int S, const float **tab)
{
    const int t = threadIdx.x;
    if (t < n) {
        tab[m0 + t] = T.U[t];
        tab[S + m0 + t] = T.V[t];
    }
}

int rec_upload_tables(const float *const *U_tables, const float *const *V_tables, int n_models, hipStream_t st, const float ***out)
{
    const float **tab = nullptr;
    URE_HIP(hipMallocAsync(reinterpret_cast<void **>(&tab), sizeof(float *) * 2 * (size_t)n_models, st));
    for (int m0 = 0; m0 < n_models; m0 += URE_MAX_MODELS_PER_CALL) {
        RecTables T;
        const int c = std::min(n_models - m0, URE_MAX_MODELS_PER_CALL);
        for (int j = 0; j < c; ++j) {
            T.U[j] = U_tables[m0 + j];
            T.V[j] = V_tables[m0 + j];
        }
        hipLaunchKernelGGL(rec_tables_kernel, dim3(1), dim3(kWave), 0, st, T, c, m0, n_models, tab);
    }
    *out = tab;
    return 0;
}

}  // namespace ure

using namespace ure;

extern "C" {

int64_t ure_recommend_scratch(int64_t n_query, int32_t n_item, int32_t k) { return rec_scratch_bytes(n_query, n_item, k); }

int ure_recommend_topk(const float *const *U_tables, const float *const *V_tables, int32_t n_models, const int32_t *users, int64_t n_query,
                       int32_t n_item, int32_t d, const int64_t *excl_off, const int32_t *excl_items, int32_t k, float *scores,
                       int32_t *items, void *scratch, int64_t scratch_bytes, void *stream)
{
    URE_ARG(U_tables && V_tables && n_models >= 1);
    URE_ARG(users && n_query >= 1 && n_item >= 1);
    URE_ARG(pow2(d) && d >= 4 && d <= 256);
    URE_ARG(k >= 1 && k <= kRecMaxK);
    URE_ARG((excl_off == nullptr) == (excl_items == nullptr));
    URE_ARG(scores && items);
    for (int m = 0; m < n_models; ++m) URE_ARG(U_tables[m] && V_tables[m]);
    const int64_t need = ure_recommend_scratch(n_query, n_item, k);
    URE_ARG(scratch_bytes >= need && (need == 0 || scratch));

    hipStream_t st = static_cast<hipStream_t>(stream);
    const RecArgs A = rec_args(users, n_query, n_item, excl_off, excl_items, k, scores, items, scratch);

    // the model table lives on the device for the call: any number of models in one pass
    const float **tab = nullptr;
    if (int rc = rec_upload_tables(U_tables, V_tables, n_models, st, &tab)) return rc;
    int rc = 0;
    dispatch_group_width(d / 4, [&](auto W) {
        using P = MfScorer<decltype(W)::value>;
        rc = launch_rec<P>(typename P::Ctx{tab, n_models}, A, st);
    });
    if (rc == 0) rc = launch_rec_merge(A, st, "ure_recommend_topk");
    URE_HIP(hipFreeAsync(tab, st));
    return rc;
}

}  // extern "C"

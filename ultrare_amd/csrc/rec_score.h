// rec_score.h -- the ensemble scoring shared by mf_recommend.hip (top-k) and mf_rank.hip (exact ranks).
//
// score(u, i) = (sum over models, in list order, of U_m[u] . V_m[i]) / S with every dot product in
// score_kernel's (mf_eval.hip) order: partial j = a.x*b.x + three fmaf over columns 4j .. 4j+3, the d/4
// partials added by group_sum's balanced tree over contiguous halves, the model results added into one
// float starting from 0.  The scores equal what ure_score writes for the same pairs, bit for bit, and a
// pair scored alone (rec_score_pair) equals the same pair scored inside a tile (rec_score_tile).
//
// Key order: score descending (NaN below -inf, -0.0 == +0.0), then item id ascending.  The 64-bit key
// (order_bits(score) << 32 | ~item) is larger for the better item and 0 only for padding (item -1, NaN).
#pragma once
#include "group_width.h"
#include "ure_internal.h"

namespace ure {

constexpr int kRecItems = 64;        // items per tile: one per lane, shared by the workgroup's 4 waves

// The model list on the device for one call: tab[m] = U_m, tab[S + m] = V_m (stream-ordered allocation; the
// caller frees it with hipFreeAsync on the same stream).  Defined in mf_recommend.hip.
int rec_upload_tables(const float *const *U_tables, const float *const *V_tables, int n_models, hipStream_t st, const float ***tab);

__device__ __forceinline__ uint32_t order_bits(float s)
{
    if (s != s) return 0u;                                  // NaN below every number
    uint32_t b = __float_as_uint(s);
    if ((b << 1) == 0u) b = 0u;                             // -0.0 == +0.0
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);      // -inf -> 0x007FFFFF > 0
}

__device__ __forceinline__ uint64_t rec_key(float s, int item)
{
    return ((uint64_t)order_bits(s) << 32) | (uint64_t)(~(uint32_t)item);
}

// Orders this wave's LDS accesses before and after (LDS operations of one wave complete in issue order).
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// out[t] = the tree sum over partials [J0, J0 + N) of user row t (u + t * D) against the item row v.
template <int D, int QW, int J0, int N>
__device__ __forceinline__ void rec_dot(float (&out)[QW], const float *v, const float *u)
{
    if constexpr (N == 1) {
        const float4 b = *reinterpret_cast<const float4 *>(v + J0 * 4);
#pragma unroll
        for (int t = 0; t < QW; ++t) {
            const float4 a = *reinterpret_cast<const float4 *>(u + t * D + J0 * 4);
            float p = a.x * b.x;
            p = fmaf(a.y, b.y, p);
            p = fmaf(a.z, b.z, p);
            p = fmaf(a.w, b.w, p);
            out[t] = p;
        }
    } else {
        float r[QW];
        rec_dot<D, QW, J0, N / 2>(out, v, u);
        rec_dot<D, QW, J0 + N / 2, N / 2>(r, v, u);
#pragma unroll
        for (int t = 0; t < QW; ++t) out[t] += r[t];
    }
}

// Scores one tile: s[t] = score(uid[w * QW + t], i0 + lane) for the wave's QW users of the workgroup's
// QT = kWavesPerBlock * QW (user rows q0 + r < n_query are staged, the rest read zeros; items in [i0, ie)).
// Per model the users' U rows go to Us [QT][D] and the tile's V rows to Vs [64][D + 4] (padded: conflict-free
// ds_read_b128 across lanes).  Workgroup-wide: every thread of the block calls it with the same arguments.
template <int LPR, int QW>
__device__ __forceinline__ void rec_score_tile(float (&s)[QW], const float *const *tab, int n_models, float *Us, float *Vs,
                                               const int32_t *uid, int64_t q0, int64_t n_query, int i0, int ie)
{
    constexpr int D = LPR * 4;
    constexpr int QT = kWavesPerBlock * QW;
    constexpr int VS = D + 4;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float n_s = (float)n_models;
    float acc[QW];
#pragma unroll
    for (int t = 0; t < QW; ++t) acc[t] = 0.f;
    for (int m = 0; m < n_models; ++m) {
        const float *Um = tab[m], *Vm = tab[n_models + m];
        __syncthreads();
        for (int f = tid; f < QT * LPR; f += kBlock) {
            const int r = f / LPR, c = f % LPR;
            const float4 x = q0 + r < n_query ? ldg_f4(Um + (size_t)uid[r] * D + c * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4 *>(Us + r * D + c * 4) = x;
        }
        for (int f = tid; f < kRecItems * LPR; f += kBlock) {
            const int r = f / LPR, c = f % LPR;
            const float4 x = i0 + r < ie ? ldg_f4(Vm + (size_t)(i0 + r) * D + c * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4 *>(Vs + r * VS + c * 4) = x;
        }
        __syncthreads();
        float p[QW];
        rec_dot<D, QW, 0, LPR>(p, Vs + lane * VS, Us + w * QW * D);
#pragma unroll
        for (int t = 0; t < QW; ++t) acc[t] += p[t];
    }
#pragma unroll
    for (int t = 0; t < QW; ++t) s[t] = acc[t] / n_s;       // score_kernel: acc / (float)n_total
}

// The score of one (user, item) pair, read straight from the tables: the same products, tree and model order.
template <int LPR>
__device__ __forceinline__ float rec_score_pair(const float *const *tab, int n_models, int user, int item)
{
    constexpr int D = LPR * 4;
    const float n_s = (float)n_models;
    float acc = 0.f;
    for (int m = 0; m < n_models; ++m) {
        float p[1];
        rec_dot<D, 1, 0, LPR>(p, tab[n_models + m] + (size_t)item * D, tab[m] + (size_t)user * D);
        acc += p[0];
    }
    return acc / n_s;
}

// The MF ensemble as a scorer policy of the selection (rec_select.h) and counting (rank_count.h) kernels: rec_score_tile over
// Us [QT][D] and Vs [64][D + 4] at the head of the workgroup's LDS, rec_score_pair straight from the tables.
template <int LPR>
struct MfScorer {
    static constexpr int QW = LPR * 4 >= 256 ? 4 : 8;
    static constexpr int D = LPR * 4;
    static constexpr int QT = kWavesPerBlock * QW;
    struct Ctx {
        const float *const *tab;     // [2 * S] device: U_0 .. U_{S-1}, V_0 .. V_{S-1}
        int n_models;
    };
    __host__ __device__ static constexpr int tile_lds(const Ctx &) { return (QT * D + kRecItems * (D + 4)) * 4; }
    __host__ __device__ static constexpr int pair_lds(const Ctx &) { return 0; }
    __device__ __forceinline__ static void tile(float (&s)[QW], const Ctx &C, char *lds, const int32_t *uid, int64_t q0, int64_t n_query, int i0,
                                                int ie)
    {
        float *Us = reinterpret_cast<float *>(lds);
        rec_score_tile<LPR, QW>(s, C.tab, C.n_models, Us, Us + QT * D, uid, q0, n_query, i0, ie);
    }
    __device__ __forceinline__ static float pair(const Ctx &C, char *, int user, int item) { return rec_score_pair<LPR>(C.tab, C.n_models, user, item); }
};

}  // namespace ure

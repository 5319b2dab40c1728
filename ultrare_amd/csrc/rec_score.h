// rec_score.h -- the ensemble scoring shared by mf_recommend.hip (top-k), mf_rank.hip (exact ranks) and mf_combine_rank.hip
// (both under the learned shard combiner: CombinedScorer, at the end).
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
#include "score_dot.h"

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

// One tile's per-model dot products: for every model m in list order, add(m, p) with p[t] = U_m[uid[w * QW + t]] . V_m[i0 + lane]
// for the wave's QW users of the workgroup's QT = kWavesPerBlock * QW (user rows q0 + r < n_query are staged, the rest read
// zeros; items in [i0, ie)).  Per model the users' U rows go to Us [QT][D] and the tile's V rows to Vs [64][D + 4] (padded:
// conflict-free ds_read_b128 across lanes).  Workgroup-wide: every thread of the block calls it with the same arguments.
template <int LPR, int QW, class Add>
__device__ __forceinline__ void rec_tile_models(const float *const *tab, int n_models, float *Us, float *Vs, const int32_t *uid, int64_t q0,
                                                int64_t n_query, int i0, int ie, Add add)
{
    constexpr int D = LPR * 4;
    constexpr int QT = kWavesPerBlock * QW;
    constexpr int VS = D + 4;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
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
        add(m, p);
    }
}

// Scores one tile: s[t] = score(uid[w * QW + t], i0 + lane), the mean over rec_tile_models' dot products.
template <int LPR, int QW>
__device__ __forceinline__ void rec_score_tile(float (&s)[QW], const float *const *tab, int n_models, float *Us, float *Vs,
                                               const int32_t *uid, int64_t q0, int64_t n_query, int i0, int ie)
{
    const float n_s = (float)n_models;
    float acc[QW];
#pragma unroll
    for (int t = 0; t < QW; ++t) acc[t] = 0.f;
    rec_tile_models<LPR, QW>(tab, n_models, Us, Vs, uid, q0, n_query, i0, ie, [&](int, const float(&p)[QW]) {
#pragma unroll
        for (int t = 0; t < QW; ++t) acc[t] += p[t];
    });
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

// The weighted ensemble (the learned shard combiner, mf_combine.hip) as the third scorer policy: the bytes ure_score_weighted
// writes to pred for the pair.  p_s = 0.f + the model's dot (score_kernel's running sum starts at zero: a dot of -0.0 becomes
// +0.0); z = b, then z = z + w[s] * (double)p_s for s = 0, 1, ... in float64, every product rounded (-ffp-contract=off);
// (float)link_mean(link, z).  The weight row is W[group_of_user[u]] (row 0 without a map); a user in no group takes w = 1 / S,
// b = 0 under link 0 and NaN under link 1.
// The tile is rec_tile_models' with, behind Us and Vs, the QT users' weight rows Ws [QT][kCwRow] doubles (row r: w[0 .. S - 1],
// then b; "no group" resolved while staging) and a flag per user for the NaN of link 1: a weight is one broadcast LDS read per
// (user, model), link_mean and the conversion run once per (user, item).
constexpr int kCwRow = URE_MAX_MODELS_PER_CALL + 1;

struct CombinedCtx {
    const float *const *tab;         // [2 * S] device: U_0 .. U_{S-1}, V_0 .. V_{S-1}
    int n_models;
    int link;
    const double *W;                 // [n_groups][S + 1] device
    int n_groups;
    const int32_t *group_of_user;    // [n_user] device, or nullptr: row 0
    int n_user;
};

// The weight row of `user`: its group, or -1 for a user in no group.
__device__ __forceinline__ int combined_group(const CombinedCtx &C, int user)
{
    int g = 0;
    if (C.group_of_user) g = (user >= 0 && user < C.n_user) ? C.group_of_user[user] : -1;
    return (g < 0 || g >= C.n_groups) ? -1 : g;
}

// link_mean behind a call.  Inlined QW times behind the model loop, the float64 exp put the whole tile kernel under another
// register budget: 286 spilled registers in rec_topk_kernel at d = 256, none this way (and one copy of the code, not QW).
__device__ __attribute__((noinline)) inline double link_mean_call(int link, double z) { return link_mean(link, z); }

template <int LPR>
struct CombinedScorer {
    static constexpr int QW = MfScorer<LPR>::QW;
    static constexpr int D = LPR * 4;
    static constexpr int QT = kWavesPerBlock * QW;
    static constexpr int kRows = (QT * D + kRecItems * (D + 4)) * 4;     // MfScorer's Us and Vs
    using Ctx = CombinedCtx;
    __host__ __device__ static constexpr int tile_lds(const Ctx &) { return kRows + QT * kCwRow * 8 + QT * 4; }
    __host__ __device__ static constexpr int pair_lds(const Ctx &) { return 0; }
    __device__ __forceinline__ static void tile(float (&s)[QW], const Ctx &C, char *lds, const int32_t *uid, int64_t q0, int64_t n_query, int i0,
                                                int ie)
    {
        float *Us = reinterpret_cast<float *>(lds);
        double *Ws = reinterpret_cast<double *>(lds + kRows);
        int32_t *none = reinterpret_cast<int32_t *>(Ws + QT * kCwRow);
        const int S = C.n_models, X = S + 1;
        const int tid = threadIdx.x, w = tid >> 6;
        const double w_mean = 1.0 / (double)S;
        __syncthreads();                                    // the tile before has read Ws
        for (int f = tid; f < QT * X; f += kBlock) {
            const int r = f / X, c = f % X;
            const int g = combined_group(C, uid[r]);        // (rows past n_query hold user 0)
            Ws[r * kCwRow + c] = g < 0 ? (c < S ? w_mean : 0.0) : C.W[(size_t)g * X + c];
            if (c == 0) none[r] = g < 0;
        }
        __syncthreads();
        // z starts from the bias here, not at m == 0 inside the model loop: that test had the compiler peel the loop's first trip,
        // and the two copies of the dot products spilled 800 registers at d = 128
        const double *wr = Ws + w * QW * kCwRow;
        double z[QW];
#pragma unroll
        for (int t = 0; t < QW; ++t) z[t] = wr[t * kCwRow + S];
        rec_tile_models<LPR, QW>(C.tab, S, Us, Us + QT * D, uid, q0, n_query, i0, ie, [&](int m, const float(&p)[QW]) {
#pragma unroll
            for (int t = 0; t < QW; ++t) {
                const float ps = 0.f + p[t];
                z[t] = z[t] + wr[t * kCwRow + m] * (double)ps;
            }
        });
#pragma unroll
        for (int t = 0; t < QW; ++t) {
            double mu = link_mean_call(C.link, z[t]);
            if (C.link != 0 && none[w * QW + t]) mu = __builtin_nan("");
            s[t] = (float)mu;
        }
    }
    __device__ __forceinline__ static float pair(const Ctx &C, char *, int user, int item)
    {
        const int S = C.n_models;
        const int g = combined_group(C, user);
        const bool outside = g < 0;
        const double *wr = C.W + (size_t)(outside ? 0 : g) * (S + 1);
        const double w_mean = 1.0 / (double)S;
        double z = outside ? 0.0 : wr[S];
        for (int m = 0; m < S; ++m) {
            float p[1];
            rec_dot<D, 1, 0, LPR>(p, C.tab[S + m] + (size_t)item * D, C.tab[m] + (size_t)user * D);
            const float ps = 0.f + p[0];
            // the weight is read before the test (row 0 is there for a user in no group): a load under the test is a branch in the
            // loop, and the row loads then took all 512 registers (40 - 51 spilled at d = 256)
            const double wv = wr[m];
            z = z + (outside ? w_mean : wv) * (double)ps;
        }
        double mu = link_mean(C.link, z);
        if (C.link != 0 && outside) mu = __builtin_nan("");
        return (float)mu;
    }
};

}  // namespace ure

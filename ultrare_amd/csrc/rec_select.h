// rec_select.h -- full-catalogue top-k selection from an ensemble, written once for every scorer (mf_recommend.hip: the MF dot
// products of rec_score.h; nmf_rank.hip: the NeuMF forward; mf_combine_rank.hip: the MF dot products under the shard combiner).
//
// One fused pass scores and selects; the score matrix never reaches HBM.  A workgroup owns a tile of
// QT = 4 * QW users (QW per wave) and streams the item tiles of its split: the scorer gives each lane the
// scores of its item against its wave's QW users in registers.  Per user the wave keeps a sorted top-k list
// and an unsorted candidate buffer in LDS: a scored item enters the buffer only if its key beats the current
// k-th key, and only such survivors pay for the exclusion test (binary search in the query row's sorted list).
// A full buffer is merged into the list by rank (keys are unique: the item id is part of the key), so the
// result does not depend on the order in which candidates arrive.  With several item splits per user tile each
// split writes its own sorted top-k; rec_merge_splits_kernel merges them split by split.
//
// A scorer policy P gives:
//   P::QW                                 users per wave
//   P::Ctx                                what a call passes to the scorer (trivially copyable: it travels as a kernel argument)
//   P::tile_lds(C)                        bytes of LDS the tile scorer stages (a multiple of 16, host and device)
//   P::tile(s, C, lds, uid, q0, n_query, i0, ie)
//                                         workgroup-wide: s[t] = score(uid[w * QW + t], i0 + lane) over all models
//   P::pair_lds(C), P::pair(C, lds, user, item)
//                                         one pair alone, the same bytes as the tile gives (rank_count.h)
#pragma once
#include "rec_score.h"

namespace ure {

constexpr int kRecCand = 64;         // candidate slots per user
constexpr int kRecMaxK = 128;
constexpr int kRecTargetBlocks = 1024;   // splits fill about 4 workgroups per CU at small n_query
constexpr int kRecMinSplitItems = 512;

// Merges nc candidates (ck / cs) into the sorted list (tk / ts, k entries, padding keys 0 at the end) by
// rank and returns the new k-th key.  Wave-wide; k + nc <= 192.
__device__ __forceinline__ uint64_t rec_merge_cand(uint64_t *tk, float *ts, const uint64_t *ck, const float *cs, int k, int nc, int lane)
{
    wave_lds_sync();
    const int E = k + nc;
    uint64_t ek[3];
    float es[3];
    int er[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int e = lane + 64 * a;
        ek[a] = 0;
        es[a] = 0.f;
        er[a] = 0;
        if (e < E) {
            ek[a] = e < k ? tk[e] : ck[e - k];
            es[a] = e < k ? ts[e] : cs[e - k];
        }
    }
    for (int j = 0; j < E; ++j) {
        const uint64_t x = j < k ? tk[j] : ck[j - k];
#pragma unroll
        for (int a = 0; a < 3; ++a) er[a] += x > ek[a];
    }
    wave_lds_sync();
    for (int e = lane; e < k; e += 64) {
        tk[e] = 0;
        ts[e] = __builtin_nanf("");
    }
    wave_lds_sync();
#pragma unroll
    for (int a = 0; a < 3; ++a)
        if (ek[a] != 0 && er[a] < k) {
            tk[er[a]] = ek[a];
            ts[er[a]] = es[a];
        }
    wave_lds_sync();
    return tk[k - 1];
}

struct RecArgs {
    const int32_t *users;
    int64_t n_query;
    int32_t n_item;
    const int64_t *excl_off;
    const int32_t *excl_items;
    int k;
    int splits;
    int span;                        // items per split (a multiple of kRecItems)
    float *scores;                   // splits == 1: the outputs
    int32_t *items;
    uint64_t *pkey;                  // splits > 1: [n_query][splits][k] partial lists
    float *pscore;
};

// A launch's argument: the scorer's part first (for the MF scorer the model table and count lead the kernel arguments).
template <class P>
struct RecCall {
    typename P::Ctx C;
    RecArgs A;
};

// LDS of the selection state behind the scorer's: lists, candidate buffers, the tile's scores, thresholds, counts, user ids.
inline size_t rec_select_lds(int QT, int k) { return (size_t)QT * (k + kRecCand) * 12 + (size_t)QT * kRecItems * 4 + (size_t)QT * 16; }

template <class P>
__global__ __launch_bounds__(kBlock) void rec_topk_kernel(RecCall<P> K)
{
    constexpr int QW = P::QW;
    constexpr int QT = kWavesPerBlock * QW;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const RecArgs &A = K.A;
    const int k = A.k;
    uint64_t *tk = reinterpret_cast<uint64_t *>(smem + P::tile_lds(K.C));          // [QT][k], behind the scorer's LDS
    uint64_t *ck = tk + QT * k;                                                    // [QT][C]
    float *ts = reinterpret_cast<float *>(ck + QT * kRecCand);                     // [QT][k]
    float *cs = ts + QT * k;                                                       // [QT][C]
    float *sc = cs + QT * kRecCand;                                                // [QT][64] scores of the tile
    uint64_t *thr = reinterpret_cast<uint64_t *>(sc + QT * kRecItems);             // [QT] k-th key of each list
    int32_t *cnt = reinterpret_cast<int32_t *>(thr + QT);                          // [QT] candidates held
    int32_t *uid = cnt + QT;                                                       // [QT]

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t q0 = (int64_t)blockIdx.x * QT;
    const int split = blockIdx.y;
    const int ib = (int)std::min<int64_t>((int64_t)split * A.span, A.n_item);
    const int ie = (int)std::min<int64_t>((int64_t)ib + A.span, A.n_item);

    if (tid < QT) uid[tid] = q0 + tid < A.n_query ? A.users[q0 + tid] : 0;
    for (int e = tid; e < QT * k; e += kBlock) {
        tk[e] = 0;
        ts[e] = __builtin_nanf("");
    }
    for (int r = tid; r < QT; r += kBlock) {
        thr[r] = 0;
        cnt[r] = 0;
    }
    __syncthreads();

    for (int i0 = ib; i0 < ie; i0 += kRecItems) {
        float sv[QW];
        P::tile(sv, K.C, smem, uid, q0, A.n_query, i0, ie);
#pragma unroll
        for (int t = 0; t < QW; ++t) sc[(w * QW + t) * kRecItems + lane] = sv[t];
        wave_lds_sync();

        // selection: wave w keeps the lists of its QW users (one user at a time: the state is wave-uniform, in LDS)
        const int item = i0 + lane;
#pragma unroll 1
        for (int t = 0; t < QW; ++t) {
            const int r = w * QW + t;
            const int64_t q = q0 + r;
            if (q >= A.n_query) break;                         // wave-uniform
            const float s = sc[r * kRecItems + lane];
            const uint64_t key = item < ie ? rec_key(s, item) : 0;
            uint64_t th = thr[r];
            int c = cnt[r];
            bool surv = key > th;
            if (surv && A.excl_off) {
                int64_t lo = A.excl_off[q], hi = A.excl_off[q + 1];
                const int64_t end = hi;
                while (lo < hi) {
                    const int64_t mid = (lo + hi) >> 1;
                    if (A.excl_items[mid] < item) lo = mid + 1;
                    else hi = mid;
                }
                if (lo < end && A.excl_items[lo] == item) surv = false;
            }
            uint64_t mask = __ballot(surv);
            int n = __popcll(mask);
            if (c + n > kRecCand) {
                th = rec_merge_cand(tk + r * k, ts + r * k, ck + r * kRecCand, cs + r * kRecCand, k, c, lane);
                c = 0;
                surv = surv && key > th;
                mask = __ballot(surv);
                n = __popcll(mask);
            }
            if (surv) {
                const int pos = c + __popcll(mask & ((1ull << lane) - 1ull));
                ck[r * kRecCand + pos] = key;
                cs[r * kRecCand + pos] = s;
            }
            wave_lds_sync();
            thr[r] = th;
            cnt[r] = c + n;
        }
    }

#pragma unroll 1
    for (int t = 0; t < QW; ++t) {
        const int r = w * QW + t;
        const int64_t q = q0 + r;
        if (q >= A.n_query) break;
        wave_lds_sync();
        if (cnt[r] > 0) rec_merge_cand(tk + r * k, ts + r * k, ck + r * kRecCand, cs + r * kRecCand, k, cnt[r], lane);
        wave_lds_sync();
        for (int e = lane; e < k; e += 64) {
            const uint64_t key = tk[r * k + e];
            const float s = ts[r * k + e];
            if (A.splits == 1) {
                A.scores[q * k + e] = s;
                A.items[q * k + e] = (int32_t)~(uint32_t)key;
            } else {
                const int64_t o = (q * A.splits + split) * k + e;
                A.pkey[o] = key;
                A.pscore[o] = s;
            }
        }
    }
}

// Number of keys in the sorted list a [k] (descending, padding 0 at the end) greater than x > 0.
__device__ __forceinline__ int rec_count_gt(const uint64_t *a, int k, uint64_t x)
{
    int lo = 0, hi = k;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] > x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// One wave per query row: the splits' sorted lists merged into the running list in split order.
static __global__ __launch_bounds__(kBlock) void rec_merge_splits_kernel(const uint64_t *__restrict__ pkey, const float *__restrict__ pscore,
                                                                         int64_t n_query, int splits, int k, float *__restrict__ scores,
                                                                         int32_t *__restrict__ items)
{
    __shared__ uint64_t sk[kWavesPerBlock][2][kRecMaxK];
    __shared__ float ss[kWavesPerBlock][2][kRecMaxK];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * kWavesPerBlock + w;
    if (q >= n_query) return;
    uint64_t *ak = sk[w][0], *bk = sk[w][1];
    float *as = ss[w][0], *bs = ss[w][1];
    const int64_t base = q * splits * k;
    for (int e = lane; e < k; e += 64) {
        ak[e] = pkey[base + e];
        as[e] = pscore[base + e];
    }
    for (int s = 1; s < splits; ++s) {
        for (int e = lane; e < k; e += 64) {
            bk[e] = pkey[base + (int64_t)s * k + e];
            bs[e] = pscore[base + (int64_t)s * k + e];
        }
        wave_lds_sync();
        uint64_t xk[2][2];
        float xs[2][2];
        int xr[2][2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int e = lane + 64 * h;
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                xk[h][g] = 0;
                xs[h][g] = 0.f;
                xr[h][g] = k;
            }
            if (e < k) {
                xk[h][0] = ak[e];
                xs[h][0] = as[e];
                if (xk[h][0]) xr[h][0] = e + rec_count_gt(bk, k, xk[h][0]);
                xk[h][1] = bk[e];
                xs[h][1] = bs[e];
                if (xk[h][1]) xr[h][1] = e + rec_count_gt(ak, k, xk[h][1]);
            }
        }
        wave_lds_sync();
        for (int e = lane; e < k; e += 64) {
            ak[e] = 0;
            as[e] = __builtin_nanf("");
        }
        wave_lds_sync();
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int g = 0; g < 2; ++g)
                if (xr[h][g] < k) {
                    ak[xr[h][g]] = xk[h][g];
                    as[xr[h][g]] = xs[h][g];
                }
        wave_lds_sync();
    }
    for (int e = lane; e < k; e += 64) {
        scores[q * k + e] = as[e];
        items[q * k + e] = (int32_t)~(uint32_t)ak[e];
    }
}

// Item splits per user tile: enough workgroups to fill the chip at small n_query, at least kRecMinSplitItems and
// 16 k items per split (a split's list is then at most 1/16 of the scores it replaces).  A function of (n_query,
// n_item, k) alone, so that the scratch sizers need no device.
static inline int rec_splits(int64_t n_query, int32_t n_item, int32_t k)
{
    const int64_t tiles = (n_query + 31) / 32;
    const int64_t by_items = std::max<int64_t>(1, n_item / std::max(kRecMinSplitItems, 16 * k));
    const int64_t want = std::max<int64_t>(1, (kRecTargetBlocks + tiles - 1) / tiles);
    return (int)std::min(want, by_items);
}

static inline int rec_span(int32_t n_item, int splits)
{
    const int64_t per = ((int64_t)n_item + splits - 1) / splits;
    return (int)((per + kRecItems - 1) / kRecItems * kRecItems);
}

// Bytes of the splits' partial lists (0: one split, the kernel writes the outputs itself), or -1 for sizes the entries refuse.
static inline int64_t rec_scratch_bytes(int64_t n_query, int32_t n_item, int32_t k)
{
    if (n_query < 1 || n_item < 1 || k < 1 || k > kRecMaxK) return -1;
    const int splits = rec_splits(n_query, n_item, k);
    return splits > 1 ? n_query * splits * k * (int64_t)(sizeof(uint64_t) + sizeof(float)) : 0;
}

// What every top-k entry fills of RecArgs from its arguments (the partial lists at `scratch`).
static inline RecArgs rec_args(const int32_t *users, int64_t n_query, int32_t n_item, const int64_t *excl_off, const int32_t *excl_items, int32_t k,
                               float *scores, int32_t *items, void *scratch)
{
    RecArgs A;
    A.users = users;
    A.n_query = n_query;
    A.n_item = n_item;
    A.excl_off = excl_off;
    A.excl_items = excl_items;
    A.k = k;
    A.splits = rec_splits(n_query, n_item, k);
    A.span = rec_span(n_item, A.splits);
    A.scores = scores;
    A.items = items;
    A.pkey = static_cast<uint64_t *>(scratch);
    A.pscore = A.splits > 1 ? reinterpret_cast<float *>(A.pkey + n_query * A.splits * k) : nullptr;
    return A;
}

// The selection launch of scorer P, and the merge of the splits behind it.
template <class P>
static int launch_rec(const typename P::Ctx &C, const RecArgs &A, hipStream_t st)
{
    constexpr int QT = kWavesPerBlock * P::QW;
    const size_t lds = (size_t)P::tile_lds(C) + rec_select_lds(QT, A.k);
    auto kern = rec_topk_kernel<P>;
    URE_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const unsigned tiles = (unsigned)((A.n_query + QT - 1) / QT);
    RecCall<P> K{C, A};
    hipLaunchKernelGGL(kern, dim3(tiles, (unsigned)A.splits), dim3(kBlock), lds, st, K);
    URE_HIP(hipGetLastError());
    return 0;
}

static inline int launch_rec_merge(const RecArgs &A, hipStream_t st, const char *who)
{
    if (A.splits <= 1) return 0;
    const unsigned blocks = (unsigned)((A.n_query + kWavesPerBlock - 1) / kWavesPerBlock);
    hipLaunchKernelGGL(rec_merge_splits_kernel, dim3(blocks), dim3(kBlock), 0, st, A.pkey, A.pscore, A.n_query, A.splits, A.k, A.scores, A.items);
    return hipGetLastError() == hipSuccess ? 0 : fail(-1, "%s: merge launch failed", who);
}

}  // namespace ure

// rank_count.h -- exact full-catalogue ranks of (user, item) pairs under an ensemble, written once for every scorer policy of
// rec_select.h (mf_rank.hip: the MF dot products; nmf_rank.hip: the NeuMF forward; mf_combine_rank.hip: the shard combiner).
//
// rank(q, t) = the number of items j of [0, n_item) outside query row q's exclusion list whose key
// rec_key(score(u, j), j) is greater than the target's key rec_key(score(u, t), t) (rec_score.h: the keys are unique).  An
// excluded target has rank -1.
//
// Counting by buckets: with a row's T target keys sorted descending, an item of key K counts for exactly the
// targets after position p(K) = #{targets with key >= K}, so it adds one to bucket p(K) and the rank of the target
// at sorted position j is the prefix sum of buckets 0 .. j.  The passes, all on `stream`:
//   rank_keys_kernel     a thread per target: its score alone (P::pair), its key, excluded or not.
//   rank_sort_kernel     a thread per target: its position in its row, by counting (duplicates by input order).
//   rank_excl_kernel     a wave per row: every excluded item scored alone and taken out of its bucket, so the
//                        stream needs no exclusion test (its streamed score is the same float).
//   rank_stream_kernel   rec_topk_kernel's tiles (P::tile): a workgroup owns QT users and an item split,
//                        scores every item and adds it to its bucket, found by binary search in the row's sorted
//                        keys.  Rows whose keys fit the workgroup's LDS budget count in LDS and flush their buckets
//                        with integer atomics; the rest search and count in global memory.  The score matrix never
//                        leaves registers.
//   rank_scan_kernel     a wave per row: buckets -> inclusive prefix sums, in place.
//   rank_gather_kernel   a thread per target: rank = the prefix sum at its sorted position (or -1).
// Every count is an integer, so the result does not depend on the order in which workgroups add to it.
#pragma once
#include "rec_select.h"

namespace ure {

constexpr int kRankLdsTargets = 4096;    // sorted keys (8 B) + buckets (4 B) per workgroup: 48 KB of LDS
constexpr int kRankTargetBlocks = 1024;
constexpr int kRankMinSplitItems = 512;
constexpr int kRankMaxFlatBlocks = 8192;  // grid-stride kernels over the targets
constexpr int64_t kRankBytes = 2 * sizeof(uint64_t) + 2 * sizeof(int32_t);   // scratch per target

// The row of entry i: the q with off[q] <= i < off[q + 1] (rows may be empty).
__device__ __forceinline__ int64_t rank_row_of(const int64_t *off, int64_t n_rows, int64_t i)
{
    int64_t lo = 0, hi = n_rows;                     // last q with off[q] <= i
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// #{j < n : a[j] >= x} of a descending array.
__device__ __forceinline__ int rank_count_ge(const uint64_t *a, int n, uint64_t x)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] >= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

struct RankArgs {
    const int32_t *users;
    int64_t n_query;
    int32_t n_item;
    int64_t cap;                     // targets the scratch holds (scratch_bytes / kRankBytes)
    const int64_t *tgt_off;
    const int32_t *tgt_items;
    const int64_t *excl_off;
    const int32_t *excl_items;
    int32_t *ranks;
    uint64_t *tkey;                  // [cap] keys in input order
    uint64_t *skey;                  // [cap] keys sorted descending within each row
    int32_t *spos;                   // [cap] sorted position of each target within its row
    int32_t *bucket;                 // [cap] bucket j of a row at its offset + j
    int splits;
    int span;
};

template <class P>
struct RankCall {
    typename P::Ctx C;
    RankArgs A;
};

// n_targets = tgt_off[n_query], known on the device only; 0 (nothing is done) when the scratch is too short for it.
__device__ __forceinline__ int64_t rank_targets(const RankArgs &A)
{
    const int64_t n = A.tgt_off[A.n_query];
    return n <= A.cap ? n : 0;
}

template <class P>
__device__ __forceinline__ void rank_key_one(const typename P::Ctx &C, const RankArgs &A, char *lds, int64_t i)
{
    const int64_t q = rank_row_of(A.tgt_off, A.n_query, i);
    const int item = A.tgt_items[i];
    A.tkey[i] = rec_key(P::pair(C, lds, A.users[q], item), item);
    bool excluded = false;
    if (A.excl_off) {
        int64_t lo = A.excl_off[q], hi = A.excl_off[q + 1];
        const int64_t end = hi;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (A.excl_items[mid] < item) lo = mid + 1;
            else hi = mid;
        }
        excluded = lo < end && A.excl_items[lo] == item;
    }
    A.ranks[i] = excluded ? -1 : 0;
    A.bucket[i] = 0;
}

template <class P>
__global__ __launch_bounds__(kBlock) void rank_keys_kernel(RankCall<P> K)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int64_t n_targets = rank_targets(K.A);
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_targets; i += (int64_t)gridDim.x * kBlock) rank_key_one<P>(K.C, K.A, smem, i);
}

__device__ __forceinline__ void rank_sort_one(const RankArgs &A, int64_t i)
{
    const int64_t q = rank_row_of(A.tgt_off, A.n_query, i);
    const int64_t b = A.tgt_off[q], e = A.tgt_off[q + 1];
    const uint64_t x = A.tkey[i];
    int pos = 0;
    for (int64_t j = b; j < e; ++j) {
        const uint64_t y = A.tkey[j];
        pos += y > x || (y == x && j < i);
    }
    A.spos[i] = pos;
    A.skey[b + pos] = x;
}

static __global__ __launch_bounds__(kBlock) void rank_sort_kernel(RankArgs A)
{
    const int64_t n_targets = rank_targets(A);
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_targets; i += (int64_t)gridDim.x * kBlock) rank_sort_one(A, i);
}

template <class P>
__global__ __launch_bounds__(kBlock) void rank_excl_kernel(RankCall<P> K)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const RankArgs &A = K.A;
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (q >= A.n_query || rank_targets(A) == 0) return;
    const int64_t b = A.tgt_off[q];
    const int T = (int)(A.tgt_off[q + 1] - b);
    if (T == 0) return;
    const int user = A.users[q];
    for (int64_t x = A.excl_off[q] + lane; x < A.excl_off[q + 1]; x += kWave) {
        const int item = A.excl_items[x];
        const int p = rank_count_ge(A.skey + b, T, rec_key(P::pair(K.C, smem, user, item), item));
        if (p < T) atomicSub(A.bucket + b + p, 1);
    }
}

// LDS of the counting state behind the scorer's: sorted keys, buckets, and per user its id, target count and LDS offset.
inline size_t rank_count_lds(int QT) { return (size_t)kRankLdsTargets * 12 + (size_t)QT * 12; }

template <class P>
__global__ __launch_bounds__(kBlock) void rank_stream_kernel(RankCall<P> K)
{
    constexpr int QW = P::QW;
    constexpr int QT = kWavesPerBlock * QW;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const RankArgs &A = K.A;
    uint64_t *lkey = reinterpret_cast<uint64_t *>(smem + P::tile_lds(K.C));        // [kRankLdsTargets], behind the scorer's LDS
    int32_t *lbkt = reinterpret_cast<int32_t *>(lkey + kRankLdsTargets);           // [kRankLdsTargets]
    int32_t *uid = lbkt + kRankLdsTargets;                                         // [QT]
    int32_t *rT = uid + QT;                                                        // [QT] targets of the row
    int32_t *lbase = rT + QT;                                                      // [QT] LDS offset of the row, -1: global

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t q0 = (int64_t)blockIdx.x * QT;
    const int ib = (int)std::min<int64_t>((int64_t)blockIdx.y * A.span, A.n_item);
    const int ie = (int)std::min<int64_t>((int64_t)ib + A.span, A.n_item);

    if (rank_targets(A) == 0) return;                    // block-uniform
    if (tid < QT) {
        const bool valid = q0 + tid < A.n_query;
        uid[tid] = valid ? A.users[q0 + tid] : 0;
        rT[tid] = valid ? (int)(A.tgt_off[q0 + tid + 1] - A.tgt_off[q0 + tid]) : 0;
    }
    __syncthreads();
    if (tid == 0) {
        int base = 0;
        for (int r = 0; r < QT; ++r) {
            const bool fits = rT[r] > 0 && base + rT[r] <= kRankLdsTargets;
            lbase[r] = fits ? base : -1;
            base += fits ? rT[r] : 0;
        }
    }
    __syncthreads();
    for (int r = 0; r < QT; ++r) {
        if (lbase[r] < 0) continue;                       // block-uniform
        const int64_t b = A.tgt_off[q0 + r];
        for (int e = tid; e < rT[r]; e += kBlock) {
            lkey[lbase[r] + e] = A.skey[b + e];
            lbkt[lbase[r] + e] = 0;
        }
    }
    // (the scorer's first barrier orders these stores before the first search)

    for (int i0 = ib; i0 < ie; i0 += kRecItems) {
        float sv[QW];
        P::tile(sv, K.C, smem, uid, q0, A.n_query, i0, ie);
        const int item = i0 + lane;
        if (item >= ie) continue;
#pragma unroll
        for (int t = 0; t < QW; ++t) {
            const int r = w * QW + t;
            const int T = rT[r];
            if (T == 0) continue;                         // also the rows past n_query
            const uint64_t key = rec_key(sv[t], item);
            if (lbase[r] >= 0) {
                const uint64_t *a = lkey + lbase[r];
                if (key < a[T - 1]) continue;            // below every target
                const int p = rank_count_ge(a, T, key);
                if (p < T) atomicAdd(lbkt + lbase[r] + p, 1);
            } else {
                const int64_t b = A.tgt_off[q0 + r];
                const uint64_t *a = A.skey + b;
                if (key < a[T - 1]) continue;
                const int p = rank_count_ge(a, T, key);
                if (p < T) atomicAdd(A.bucket + b + p, 1);
            }
        }
    }

    __syncthreads();
    for (int r = 0; r < QT; ++r) {
        if (lbase[r] < 0) continue;
        const int64_t b = A.tgt_off[q0 + r];
        for (int e = tid; e < rT[r]; e += kBlock) {
            const int c = lbkt[lbase[r] + e];
            if (c) atomicAdd(A.bucket + b + e, c);
        }
    }
}

static __global__ __launch_bounds__(kBlock) void rank_scan_kernel(RankArgs A)
{
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (q >= A.n_query || rank_targets(A) == 0) return;
    int32_t *bucket = A.bucket;
    const int64_t b = A.tgt_off[q], e = A.tgt_off[q + 1];
    int carry = 0;
    for (int64_t j0 = b; j0 < e; j0 += kWave) {
        const int64_t j = j0 + lane;
        int x = j < e ? bucket[j] : 0;
#pragma unroll
        for (int s = 1; s < kWave; s <<= 1) {
            const int y = __shfl_up(x, s);
            if (lane >= s) x += y;
        }
        x += carry;
        if (j < e) bucket[j] = x;
        carry = __shfl(x, kWave - 1);
    }
}

static __global__ __launch_bounds__(kBlock) void rank_gather_kernel(RankArgs A)
{
    const int64_t n_targets = rank_targets(A);
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_targets; i += (int64_t)gridDim.x * kBlock) {
        if (A.ranks[i] < 0) continue;
        const int64_t q = rank_row_of(A.tgt_off, A.n_query, i);
        A.ranks[i] = A.bucket[A.tgt_off[q] + A.spos[i]];
    }
}

// Item splits per user tile, as rec_splits without k: enough workgroups to fill the chip at small n_query, at least
// kRankMinSplitItems items per split.
static inline int rank_splits(int64_t n_query, int32_t n_item)
{
    const int64_t tiles = (n_query + 31) / 32;
    const int64_t by_items = std::max<int64_t>(1, n_item / kRankMinSplitItems);
    const int64_t want = std::max<int64_t>(1, (kRankTargetBlocks + tiles - 1) / tiles);
    return (int)std::min(want, by_items);
}

// What every rank entry fills of RankArgs from its arguments; the scratch holds `cap` targets.
static inline RankArgs rank_args(const int32_t *users, int64_t n_query, int32_t n_item, const int64_t *tgt_off, const int32_t *tgt_items,
                                 const int64_t *excl_off, const int32_t *excl_items, int32_t *ranks, void *scratch, int64_t cap)
{
    RankArgs A;
    A.users = users;
    A.n_query = n_query;
    A.n_item = n_item;
    A.cap = cap;
    A.tgt_off = tgt_off;
    A.tgt_items = tgt_items;
    A.excl_off = excl_off;
    A.excl_items = excl_items;
    A.ranks = ranks;
    A.tkey = static_cast<uint64_t *>(scratch);
    A.skey = A.tkey + cap;
    A.spos = reinterpret_cast<int32_t *>(A.skey + cap);
    A.bucket = A.spos + cap;
    A.splits = rank_splits(n_query, n_item);
    const int64_t per = ((int64_t)n_item + A.splits - 1) / A.splits;
    A.span = (int)((per + kRecItems - 1) / kRecItems * kRecItems);
    return A;
}

// The six passes with scorer P.
template <class P>
static int launch_rank(const typename P::Ctx &C, const RankArgs &A, hipStream_t st)
{
    constexpr int QT = kWavesPerBlock * P::QW;
    const unsigned tgt_blocks = (unsigned)std::min<int64_t>((A.cap + kBlock - 1) / kBlock, kRankMaxFlatBlocks);
    const unsigned row_blocks = (unsigned)((A.n_query + kWavesPerBlock - 1) / kWavesPerBlock);
    RankCall<P> K{C, A};
    const size_t pair_lds = (size_t)P::pair_lds(C);
    if (pair_lds > 65536) {
        URE_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(rank_keys_kernel<P>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pair_lds));
        URE_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(rank_excl_kernel<P>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pair_lds));
    }
    hipLaunchKernelGGL(rank_keys_kernel<P>, dim3(tgt_blocks), dim3(kBlock), pair_lds, st, K);
    hipLaunchKernelGGL(rank_sort_kernel, dim3(tgt_blocks), dim3(kBlock), 0, st, A);
    if (A.excl_off) hipLaunchKernelGGL(rank_excl_kernel<P>, dim3(row_blocks), dim3(kBlock), pair_lds, st, K);
    URE_HIP(hipGetLastError());
    const size_t lds = (size_t)P::tile_lds(C) + rank_count_lds(QT);
    auto kern = rank_stream_kernel<P>;
    URE_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const unsigned tiles = (unsigned)((A.n_query + QT - 1) / QT);
    hipLaunchKernelGGL(kern, dim3(tiles, (unsigned)A.splits), dim3(kBlock), lds, st, K);
    hipLaunchKernelGGL(rank_scan_kernel, dim3(row_blocks), dim3(kBlock), 0, st, A);
    hipLaunchKernelGGL(rank_gather_kernel, dim3(tgt_blocks), dim3(kBlock), 0, st, A);
    URE_HIP(hipGetLastError());
    return 0;
}

}  // namespace ure

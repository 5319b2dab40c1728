// csr_kmeans.hip -- k-means and balanced k-means (utils.py:354-418) on the sparse rating matrix: the cost and the centroid
// update read the ratings as CSR / CSC and never form the n_user x n_item array, and the balanced fill runs on the device
// (DESIGN.md 4.19).
//
//   ure_csr_kmeans_cost       dist[i][c] = ((-2 dot_ic) + esq_i) + csq_c          over the stored entries of row i, float32
//   ure_csr_kmeans_centroids  Ct[j][c]   = sum over members of x_ij * float32(1 / count_c)   over the stored entries of column j
//   ure_balanced_fill         label[u]   = the group ure_host_kmeans_assign gives user u
//
// The arithmetic is the dense route's (kmeans_cost_kernel / kmeans_centroid_kernel of ot.hip, scipy's csr order) restricted to
// the stored entries, stated in numpy in ultrare_amd/sparse_kmeans.py: float32 chains, sequential in ascending index from
// +0.0, one rounded multiply and one rounded add per term.  An entry that is not stored would add +-0 to a chain that starts
// at +0.0 and change no bit, so for finite centroids the results equal the dense route's bit for bit.  A chain is never split
// across lanes and nothing is accumulated with floating-point atomics.
//
// The lane layout and the two walks are csr_lanes.h's, shared with csr_group.hip: the centroids travel TRANSPOSED,
// Ct [n_item][k]; a lane owns one (row, centroid) or (item, cluster) pair, a group of G = pow2 >= min(k, 64) lanes shares the
// row (item) and hands its entries round with cross-lane reads; k > 64 loops over chunks of 64.
//
// The fill.  ure_host_kmeans_assign sorts the n k keys (order-preserving map of the float bits << 32 | flat index) and walks
// them, giving a user its first group with room.  That walk yields the one stable matching of the market in which users and
// groups both rank by the key, and deferred acceptance reaches the same matching in parallel rounds: every
// group keeps a threshold (UINT64_MAX at first); (a) every user picks the group with its smallest key <= the group's
// threshold; (b) every group with more than `capacity` choosers lowers its threshold to its capacity-th smallest chooser key
// (a radix select, one workgroup per group).  The first round that moves no threshold holds the answer.  Thresholds only
// decrease over a finite key set, so the loop ends; how many rounds it takes is recorded, not assumed.
#include "csr_lanes.h"

namespace ure {

constexpr int kCsqTile = 4096;       // floats of Ct staged per step of the squared-norm pass (16 KiB of LDS)
constexpr int kSelBlock = 1024;      // threads of a group's radix select
constexpr int64_t kFillHead = 4096;  // bytes of the fill workspace before the per-user keys: thresholds, counts, flag

// csq[c] = the sequential float32 sum of Ct[j][c]^2 over ALL items in ascending j from +0.0: k chains of n_item adds, made once
// per cost call.  One workgroup: all its threads stage a contiguous tile of Ct in LDS (the next tile travels in registers
// meanwhile), thread c < k then adds the tile's items to its chain.
__global__ __launch_bounds__(kBlock) void km_csq_kernel(const float *__restrict__ Ct, int64_t n_item, int k, float *__restrict__ csq)
{
    __shared__ float tile[kCsqTile];
    constexpr int kPer = kCsqTile / kBlock;
    const int items = kCsqTile / k;                        // whole items of a tile (>= 16)
    const int64_t total = n_item * k;
    const int64_t step = (int64_t)items * k;
    float next[kPer];
#pragma unroll
    for (int w = 0; w < kPer; ++w) {
        const int64_t t = (int64_t)w * kBlock + threadIdx.x;
        next[w] = t < step && t < total ? ldg(Ct + t) : 0.f;
    }
    float s = 0.f;
    for (int64_t base = 0; base < total; base += step) {
#pragma unroll
        for (int w = 0; w < kPer; ++w) tile[w * kBlock + threadIdx.x] = next[w];
        __syncthreads();
#pragma unroll
        for (int w = 0; w < kPer; ++w) {
            const int64_t t = (int64_t)w * kBlock + threadIdx.x;
            next[w] = t < step && base + step + t < total ? ldg(Ct + base + step + t) : 0.f;
        }
        if ((int)threadIdx.x < k) {
            const int m = (int)min<int64_t>(items, (total - base) / k);
#pragma unroll 8
            for (int t = 0; t < m; ++t) {                 // (unrolled: the LDS reads of eight terms travel together, the adds stay in order)
                const float v = tile[t * k + threadIdx.x];
                s = __fadd_rn(s, __fmul_rn(v, v));
            }
        }
        __syncthreads();
    }
    if ((int)threadIdx.x < k) stg(csq + threadIdx.x, s);
}

// The cost's arithmetic: float32 chains, one rounded multiply and one rounded add per term (the _rn intrinsics say so whatever
// the contraction flag of the build).
struct KmCost {
    using acc_t = float;
    using norm_t = float;
    static __device__ __forceinline__ int stride(int, int k) { return k; }          // Ct [n_item][k]: the stride is k itself
    static __device__ __forceinline__ float madd(float acc, float a, float b) { return __fadd_rn(acc, __fmul_rn(a, b)); }
    static __device__ __forceinline__ void store(float *dist, int c, int64_t i, int64_t, int k, float dot, float esq, const float *csq)
    {
        stg(dist + (size_t)i * k + c, __fadd_rn(__fadd_rn(__fmul_rn(-2.0f, dot), esq), ldg(csq + c)));   // dist[i][c]
    }
};

// The centroids' arithmetic: lane c adds x * inv_c, inv_c = float32(1 / count_c) read before the walk.
struct KmMean {
    using acc_t = float;
    struct prep_t {
        int cnt;
        float inv;
    };
    static __device__ __forceinline__ prep_t prepare(const int32_t *counts, int c, int k)
    {
        const int cnt = ldg(counts + min(c, k - 1));
        return {cnt, (float)(1.0 / (double)cnt)};          // (inf for a cluster without members: no entry is its, nothing is multiplied)
    }
    static __device__ __forceinline__ float add(float s, float x, prep_t p) { return __fadd_rn(s, __fmul_rn(x, p.inv)); }
    static __device__ __forceinline__ float finish(float s, prep_t p, const int32_t *, int) { return p.cnt > 0 ? s : 0.f; }
};

// ---- the fill ------------------------------------------------------------------------------------------------------------------
// The host's key: the order-preserving map of the float's bit pattern above the flat index (-0.0 before +0.0, NaN patterns by
// their bits).  n k < 2^32 keeps every flat index below 2^32 - 1, so no key equals UINT64_MAX.
__device__ __forceinline__ uint64_t fill_key(float d, uint32_t flat)
{
    uint32_t b = __float_as_uint(d);
    b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((uint64_t)b << 32) | (uint64_t)flat;
}

// capacity <= 0: numpy's argmin of a row -- the first minimum, and the first NaN wins.
__global__ __launch_bounds__(kBlock) void fill_argmin_kernel(const float *__restrict__ dist, int64_t n, int k, int32_t *__restrict__ label)
{
    const int64_t u = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (u >= n) return;
    const float *__restrict__ row = dist + u * k;
    float best_v = ldg(row);
    int best = 0;
    bool nan_seen = best_v != best_v;
    for (int c = 1; c < k && !nan_seen; ++c) {
        const float v = ldg(row + c);
        if (v != v) { best = c; nan_seen = true; }
        else if (v < best_v) { best = c; best_v = v; }
    }
    stg(label + u, (int32_t)best);
}

// Step (a): user u picks the group with its smallest key <= that group's threshold; cnt[g] counts the choosers of g.  Every
// user finds a group: a group turns users away only once `capacity` of them hold keys at or below its threshold, those stay
// with it, and capacity * k >= n.  (A user without one would keep group 0 with the key UINT64_MAX: nothing is read or
// written out of range.)
__global__ __launch_bounds__(kBlock) void fill_choose_kernel(const float *__restrict__ dist, int64_t n, int k, const uint64_t *__restrict__ thr,
                                                             int32_t *__restrict__ label, uint64_t *__restrict__ ckey, int32_t *__restrict__ cnt)
{
    __shared__ uint64_t s_thr[kCsrMaxK];
    __shared__ int s_cnt[kCsrMaxK];
    for (int c = threadIdx.x; c < k; c += kBlock) {
        s_thr[c] = ldg(thr + c);
        s_cnt[c] = 0;
    }
    __syncthreads();
    const int64_t u = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (u < n) {
        const float *__restrict__ row = dist + u * k;
        uint64_t best = UINT64_MAX;
        int bc = 0;
        for (int c = 0; c < k; ++c) {
            const uint64_t key = fill_key(ldg(row + c), (uint32_t)(u * k + c));
            if (key <= s_thr[c] && key < best) {
                best = key;
                bc = c;
            }
        }
        stg(label + u, (int32_t)bc);
        stg(ckey + u, best);
        atomicAdd(&s_cnt[bc], 1);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < k; c += kBlock)
        if (s_cnt[c]) atomicAdd(&cnt[c], s_cnt[c]);
}

// Step (b): group g = blockIdx.x with more than `capacity` choosers finds its capacity-th smallest chooser key by a radix
// select, eight bits at a time from the top (keys are distinct, so the eighth pass names one key), and takes it as its new
// threshold.  Integer atomics on the histogram: exact in any order.
__global__ __launch_bounds__(kSelBlock) void fill_select_kernel(const int32_t *__restrict__ label, const uint64_t *__restrict__ ckey, int64_t n,
                                                                const int32_t *__restrict__ cnt, int64_t capacity, uint64_t *__restrict__ thr,
                                                                int32_t *__restrict__ changed)
{
    const int g = blockIdx.x;
    if ((int64_t)ldg(cnt + g) <= capacity) return;         // the whole workgroup leaves
    __shared__ int hist[256];
    __shared__ uint64_t s_prefix;
    __shared__ int64_t s_rank;
    uint64_t prefix = 0;
    int64_t rank = capacity;                               // 1-based rank among the keys that share the prefix
    for (int shift = 56; shift >= 0; shift -= 8) {
        if (threadIdx.x < 256) hist[threadIdx.x] = 0;
        __syncthreads();
        for (int64_t u = threadIdx.x; u < n; u += kSelBlock) {
            if (ldg(label + u) != g) continue;
            const uint64_t key = ldg(ckey + u);
            if (shift == 56 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[(int)((key >> shift) & 255u)], 1);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int64_t r = rank;
            int d = 0;
            for (; d < 255; ++d) {
                if (r <= hist[d]) break;
                r -= hist[d];
            }
            s_prefix = (prefix << 8) | (uint64_t)d;
            s_rank = r;
        }
        __syncthreads();
        prefix = s_prefix;
        rank = s_rank;
    }
    if (threadIdx.x == 0) {
        stg(thr + g, prefix);
        atomicOr(changed, 1);
    }
}

}  // namespace ure

using namespace ure;

extern "C" {

int64_t ure_csr_kmeans_cost_scratch(int k)
{
    if (k < 1 || k > kCsrMaxK) return -1;
    return (int64_t)k * (int64_t)sizeof(float);
}

int ure_csr_kmeans_cost(const int64_t *row_off, const int32_t *col, const float *val, int64_t n, int64_t n_item, const float *Ct, int k,
                        float *dist_nk, void *workspace, int64_t workspace_bytes, void *stream)
{
    URE_ARG(row_off && col && val && Ct && dist_nk);
    URE_CSR_SIZES(n, n_item, k);
    URE_ARG(workspace != nullptr);
    URE_ARG(workspace_bytes >= ure_csr_kmeans_cost_scratch(k));
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *csq = static_cast<float *>(workspace);
    hipLaunchKernelGGL(km_csq_kernel, dim3(1), dim3(kBlock), 0, st, Ct, n_item, k, csq);
    const int G = group_width(k);
    const unsigned blocks = group_blocks(n, G);
    dispatch_group_width(G, [&](auto W) {
        hipLaunchKernelGGL((csr_row_walk<KmCost, decltype(W)::value>), dim3(blocks), dim3(kBlock), 0, st, row_off, col, val, n, n_item, Ct, k, k, csq, dist_nk);
    });
    URE_HIP(hipGetLastError());
    return 0;
}

int ure_csr_kmeans_centroids(const int64_t *col_off, const int32_t *row, const float *val, int64_t n_item, int64_t n, const int32_t *label, int k,
                             float *Ct, int32_t *counts, void *stream)
{
    URE_ARG(col_off && row && val && label && Ct && counts);
    URE_CSR_SIZES(n, n_item, k);
    hipStream_t st = static_cast<hipStream_t>(stream);
    URE_HIP(launch_counts(label, n, k, counts, st));
    const int G = group_width(k);
    const unsigned blocks = group_blocks(n_item, G);
    dispatch_group_width(G, [&](auto W) {
        hipLaunchKernelGGL((csr_col_walk<KmMean, decltype(W)::value>), dim3(blocks), dim3(kBlock), 0, st, col_off, row, val, label, n, n_item, k, counts, Ct, k);
    });
    URE_HIP(hipGetLastError());
    return 0;
}

int64_t ure_balanced_fill_scratch(int64_t n, int32_t k)
{
    if (n < 1 || n > INT32_MAX || k < 1 || k > kCsrMaxK || n * (int64_t)k >= ((int64_t)1 << 32)) return -1;
    return kFillHead + n * (int64_t)sizeof(uint64_t);
}

int ure_balanced_fill(const float *dist_nk, int64_t n, int32_t k, int64_t capacity, int32_t *label, int64_t *rounds_out, void *workspace,
                      int64_t workspace_bytes, void *stream)
{
    URE_ARG(dist_nk && label);
    URE_ARG(n >= 1 && n <= INT32_MAX);
    URE_ARG(k >= 1);
    URE_ARG(k <= kCsrMaxK);
    URE_ARG(n * (int64_t)k < ((int64_t)1 << 32));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned blocks = (unsigned)((n + kBlock - 1) / kBlock);
    if (capacity <= 0) {
        hipLaunchKernelGGL(fill_argmin_kernel, dim3(blocks), dim3(kBlock), 0, st, dist_nk, n, (int)k, label);
        URE_HIP(hipGetLastError());
        if (rounds_out) *rounds_out = 1;
        return 0;
    }
    if (capacity > n) capacity = n;                        // (no group can hold more than everyone)
    if (capacity * k < n) return ::ure::fail(-1, "ure_balanced_fill: capacity %lld x %d groups < %lld users", (long long)capacity, (int)k, (long long)n);
    URE_ARG(workspace != nullptr);
    URE_ARG(workspace_bytes >= ure_balanced_fill_scratch(n, k));
    char *ws = static_cast<char *>(workspace);
    uint64_t *thr = reinterpret_cast<uint64_t *>(ws);                                    // [256]
    int32_t *cnt = reinterpret_cast<int32_t *>(ws + kCsrMaxK * sizeof(uint64_t));        // [256], then the flag
    int32_t *changed = cnt + kCsrMaxK;
    uint64_t *ckey = reinterpret_cast<uint64_t *>(ws + kFillHead);                       // [n]
    URE_HIP(hipMemsetAsync(thr, 0xFF, kCsrMaxK * sizeof(uint64_t), st));
    const int64_t limit = n * (int64_t)k + 1;              // thresholds strictly decrease over n k keys: more rounds cannot happen
    for (int64_t round = 1; round <= limit; ++round) {
        URE_HIP(hipMemsetAsync(cnt, 0, (kCsrMaxK + 1) * sizeof(int32_t), st));
        hipLaunchKernelGGL(fill_choose_kernel, dim3(blocks), dim3(kBlock), 0, st, dist_nk, n, (int)k, thr, label, ckey, cnt);
        hipLaunchKernelGGL(fill_select_kernel, dim3((unsigned)k), dim3(kSelBlock), 0, st, label, ckey, n, cnt, capacity, thr, changed);
        URE_HIP(hipGetLastError());
        int32_t flag = 0;
        URE_HIP(hipMemcpyAsync(&flag, changed, sizeof(flag), hipMemcpyDeviceToHost, st));
        URE_HIP(hipStreamSynchronize(st));
        if (!flag) {
            if (rounds_out) *rounds_out = round;
            return 0;
        }
    }
    return ::ure::fail(-1, "ure_balanced_fill: no fixed point after %lld rounds (n=%lld k=%d)", (long long)limit, (long long)n, (int)k);
}

}  // extern "C"

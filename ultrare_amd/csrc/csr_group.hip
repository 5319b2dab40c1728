// csr_group.hip -- OT grouping on the sparse rating matrix: point-to-centroid cost and centroid update that read the
// ratings as CSR / CSC and never form the n_user x n_item array.
//
//   ure_csr_cost       dist[c][i] = float32(max((xx_i - 2 dot_ic) + cc_c, 0))   over the stored entries of row i
//   ure_csr_centroids  Ct[j][c]   = float32(S[c][j] / counts[c])                over the stored entries of column j
//
// The reference's own 'rating-ot' branch raises (utils.py:637 on a csr_matrix), so the arithmetic is this project's and is
// stated in numpy (ultrare_amd/sparse_group.py): float64 accumulators, every sum sequential in ascending index from +0.0,
// one rounding to float32 at the store.  A product of two float32 values is exact in float64, so the ORDER of the additions
// is the whole contract: no entry of a row or column is ever split across lanes that then add partial sums, and nothing is
// accumulated with floating-point atomics.  A value's bytes depend on its own row (column) and the centroids (labels) alone.
//
// Layout: the centroids travel TRANSPOSED, Ct [n_item][ldc] (ldc >= k): the k values of item j are one contiguous read -- a
// 128-byte line per stored entry at k = 32 -- and one contiguous store of the item's owner.  A lane owns one (row, centroid)
// pair (cost) or one (item, cluster) pair (centroids); a group of G = pow2 >= min(k, 64) lanes shares the row (item), 64 / G
// of them per wavefront; k > 64 loops over chunks of 64 centroids.  The (index, value) stream of a row is uniform across its
// group: the group loads G entries with one instruction and hands them round with cross-lane reads.
#include "csr_lanes.h"

namespace ure {

constexpr int kCcLanes = 256;        // lanes of the squared-norm reduction: the contract's, not a tuning knob

// cc[c] = |C_c|^2 in the contract's order: thread l adds Ct[j][c]^2 for j = l, l + 256, ... ascending, then thread 0 adds
// the 256 lane sums in ascending l.  One workgroup per centroid.
__global__ __launch_bounds__(kCcLanes) void csr_cc_kernel(const float *__restrict__ Ct, int64_t n_item, int ldc, double *__restrict__ cc)
{
    __shared__ double part[kCcLanes];
    const int c = blockIdx.x;
    double s = 0.0;
    for (int64_t j = threadIdx.x; j < n_item; j += kCcLanes) {
        const double v = (double)ldg(Ct + j * ldc + c);
        s = fma(v, v, s);
    }
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int l = 0; l < kCcLanes; ++l) t += part[l];
        cc[c] = t;
    }
}

// The cost's arithmetic: float64 fma chains (the walk converts each entry once), one rounding to float at the store.
struct OtCost {
    using acc_t = double;
    using norm_t = double;
    static __device__ __forceinline__ int stride(int ldc, int) { return ldc; }
    static __device__ __forceinline__ double madd(double acc, double a, double b) { return fma(a, b, acc); }
    static __device__ __forceinline__ void store(float *dist, int c, int64_t i, int64_t n, int, double dot, double xx, const double *cc)
    {
        const double v = (xx - 2.0 * dot) + ldg(cc + c);
        stg(dist + (size_t)c * n + i, (float)fmax(v, 0.0));                  // dist[c][i]
    }
};

// The centroids' arithmetic: the float64 sum of the members' entries, divided by the count (read after the walk) at the store.
struct OtMean {
    using acc_t = double;
    struct prep_t {};
    static __device__ __forceinline__ prep_t prepare(const int32_t *, int, int) { return {}; }
    static __device__ __forceinline__ double add(double s, double xd, prep_t) { return s + xd; }
    static __device__ __forceinline__ float finish(double s, prep_t, const int32_t *counts, int c)
    {
        const int cnt = ldg(counts + c);
        return cnt > 0 ? (float)(s / (double)cnt) : 0.f;
    }
};

}  // namespace ure

using namespace ure;

extern "C" {

int64_t ure_csr_cost_scratch(int k)
{
    if (k < 1 || k > kCsrMaxK) return -1;
    return (int64_t)k * (int64_t)sizeof(double);
}

int ure_csr_cost(const int64_t *row_off, const int32_t *col, const float *val, int64_t n, int64_t n_item, const float *Ct, int ldc, int k,
                 float *dist, void *scratch, int64_t scratch_bytes, void *stream)
{
    URE_ARG(row_off && col && val && Ct && dist);
    URE_CSR_SIZES(n, n_item, k);
    URE_ARG(ldc >= k);
    const int64_t need = ure_csr_cost_scratch(k);
    URE_ARG(scratch != nullptr);
    URE_ARG(scratch_bytes >= need);
    hipStream_t st = static_cast<hipStream_t>(stream);
    double *cc = static_cast<double *>(scratch);
    hipLaunchKernelGGL(csr_cc_kernel, dim3(k), dim3(kCcLanes), 0, st, Ct, n_item, ldc, cc);
    const int G = group_width(k);
    const unsigned blocks = group_blocks(n, G);
    dispatch_group_width(G, [&](auto W) {
        hipLaunchKernelGGL((csr_row_walk<OtCost, decltype(W)::value>), dim3(blocks), dim3(kBlock), 0, st, row_off, col, val, n, n_item, Ct, ldc, k, cc, dist);
    });
    URE_HIP(hipGetLastError());
    return 0;
}

int ure_csr_centroids(const int64_t *col_off, const int32_t *row, const float *val, const int32_t *label, int64_t n, int64_t n_item, int k,
                      float *Ct, int ldc, int32_t *counts, void *stream)
{
    URE_ARG(col_off && row && val && label && Ct && counts);
    URE_CSR_SIZES(n, n_item, k);
    URE_ARG(ldc >= k);
    hipStream_t st = static_cast<hipStream_t>(stream);
    URE_HIP(launch_counts(label, n, k, counts, st));
    const int G = group_width(k);
    const unsigned blocks = group_blocks(n_item, G);
    dispatch_group_width(G, [&](auto W) {
        hipLaunchKernelGGL((csr_col_walk<OtMean, decltype(W)::value>), dim3(blocks), dim3(kBlock), 0, st, col_off, row, val, label, n, n_item, k, counts, Ct, ldc);
    });
    URE_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"

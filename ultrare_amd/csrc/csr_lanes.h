// csr_lanes.h -- what the kernels that walk a CSR / CSC with a group of lanes share (csr_group.hip, csr_kmeans.hip): a lane
// owns one (row, centroid) or (item, cluster) pair, a group of G = pow2 >= min(k, 64) lanes shares the row (item), and the
// group hands the row's (index, value) stream round with cross-lane reads.
#pragma once
#include "ure_internal.h"

namespace ure {

constexpr int kCsrMaxK = 256;

// Lane `sub` of a group of G reads entry u of the G entries the group holds (one per lane).
template <int G, typename T>
__device__ __forceinline__ T group_read(T v, int u)
{
    return G == 1 ? v : __shfl(v, u, G);
}

inline int group_width(int k)
{
    int g = 1;
    while (g < k && g < kWave) g <<= 1;
    return g;
}

// counts[c] = members of cluster c (integer atomics: exact in any order).  counts is cleared by the caller.
static __global__ __launch_bounds__(kBlock) void csr_counts_kernel(const int32_t *__restrict__ label, int64_t n, int k, int32_t *__restrict__ counts)
{
    __shared__ int hist[kCsrMaxK];
    for (int c = threadIdx.x; c < k; c += kBlock) hist[c] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int l = ldg(label + i);
        if (l >= 0 && l < k) atomicAdd(&hist[l], 1);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < k; c += kBlock)
        if (hist[c]) atomicAdd(&counts[c], hist[c]);
}

}  // namespace ure

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

template <int G>
__global__ __launch_bounds__(kBlock) void csr_cost_kernel(const int64_t *__restrict__ row_off, const int32_t *__restrict__ col,
                                                          const float *__restrict__ val, int64_t n, int64_t n_item,
                                                          const float *__restrict__ Ct, int ldc, int k, const double *__restrict__ cc,
                                                          float *__restrict__ dist)
{
    constexpr int kRows = kBlock / G;                      // rows of a workgroup
    const int sub = threadIdx.x % G;
    const int64_t i = (int64_t)blockIdx.x * kRows + threadIdx.x / G;
    if (i >= n) return;                                    // whole groups leave together
    const int64_t b = ldg(row_off + i), e = ldg(row_off + i + 1);
    const unsigned last_item = (unsigned)(n_item - 1);
    for (int c0 = 0; c0 < k; c0 += G) {                    // one pass for k <= 64
        const int c = c0 + sub;
        const float *__restrict__ ct = Ct + min(c, k - 1);  // padding lanes read a valid column and store nothing
        double dot = 0.0, xx = 0.0;
        // (an index outside the catalogue never leaves Ct: the callers check their matrices, this keeps a bad one harmless)
        unsigned next_j = b + sub < e ? min((unsigned)ldg(col + b + sub), last_item) : 0u;
        float next_x = b + sub < e ? ldg(val + b + sub) : 0.f;
        for (int64_t p0 = b; p0 < e; p0 += G) {
            const unsigned mine_j = next_j;
            const float mine_x = next_x;
            const int64_t q = p0 + G + sub;                // the next tile's entries travel while this one is added
            next_j = q < e ? min((unsigned)ldg(col + q), last_item) : 0u;
            next_x = q < e ? ldg(val + q) : 0.f;
            const int m = (int)min<int64_t>(G, e - p0);
            if (m == G && G >= 4) {                        // a full tile: the G centroid values are requested four at a time
#pragma unroll
                for (int u = 0; u < G; u += 4) {
                    float cv[4], x[4];
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        const unsigned j = group_read<G>(mine_j, u + w);
                        x[w] = group_read<G>(mine_x, u + w);
                        cv[w] = ldg(ct + (size_t)j * ldc);
                    }
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        const double xd = (double)x[w];
                        dot = fma(xd, (double)cv[w], dot);
                        xx = fma(xd, xd, xx);
                    }
                }
            } else {
                for (int u = 0; u < m; ++u) {
                    const unsigned j = group_read<G>(mine_j, u);
                    const double xd = (double)group_read<G>(mine_x, u);
                    dot = fma(xd, (double)ldg(ct + (size_t)j * ldc), dot);
                    xx = fma(xd, xd, xx);
                }
            }
        }
        if (c < k) {
            const double v = (xx - 2.0 * dot) + ldg(cc + c);
            stg(dist + (size_t)c * n + i, (float)fmax(v, 0.0));
        }
    }
}

// Owner computes: the group that owns item j walks its column in ascending user id; lane c adds the value when the user's
// label is c.  The entry and its label are uniform across the group: lane `sub` fetches entry p0 + sub AND that user's
// label, so the dependent label reads of G entries are in flight together.
template <int G>
__global__ __launch_bounds__(kBlock) void csr_centroid_kernel(const int64_t *__restrict__ col_off, const int32_t *__restrict__ row,
                                                              const float *__restrict__ val, const int32_t *__restrict__ label, int64_t n,
                                                              int64_t n_item, int k, const int32_t *__restrict__ counts,
                                                              float *__restrict__ Ct, int ldc)
{
    constexpr int kItems = kBlock / G;
    const int sub = threadIdx.x % G;
    const int64_t j = (int64_t)blockIdx.x * kItems + threadIdx.x / G;
    if (j >= n_item) return;
    const int64_t b = ldg(col_off + j), e = ldg(col_off + j + 1);
    const unsigned last_user = (unsigned)(n - 1);
    for (int c0 = 0; c0 < k; c0 += G) {
        const int c = c0 + sub;
        double s = 0.0;
        int next_l = -1;
        float next_x = 0.f;
        if (b + sub < e) {
            next_l = ldg(label + min((unsigned)ldg(row + b + sub), last_user));
            next_x = ldg(val + b + sub);
        }
        for (int64_t p0 = b; p0 < e; p0 += G) {
            const int mine_l = next_l;
            const float mine_x = next_x;
            const int64_t q = p0 + G + sub;                // the next tile's entries and labels travel while this one is added
            if (q < e) {
                next_l = ldg(label + min((unsigned)ldg(row + q), last_user));
                next_x = ldg(val + q);
            }
            const int m = (int)min<int64_t>(G, e - p0);
            if (m == G) {
#pragma unroll
                for (int u = 0; u < G; ++u) {
                    const int l = group_read<G>(mine_l, u);
                    const double xd = (double)group_read<G>(mine_x, u);
                    if (l == c) s += xd;
                }
            } else {
                for (int u = 0; u < m; ++u) {
                    const int l = group_read<G>(mine_l, u);
                    const double xd = (double)group_read<G>(mine_x, u);
                    if (l == c) s += xd;
                }
            }
        }
        if (c < k) {
            const int cnt = ldg(counts + c);
            stg(Ct + (size_t)j * ldc + c, cnt > 0 ? (float)(s / (double)cnt) : 0.f);
        }
    }
}

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
    URE_ARG(n >= 1 && n <= INT32_MAX);
    URE_ARG(n_item >= 1 && n_item <= INT32_MAX);
    URE_ARG(k >= 1);
    URE_ARG(k <= kCsrMaxK);
    URE_ARG(ldc >= k);
    const int64_t need = ure_csr_cost_scratch(k);
    URE_ARG(scratch != nullptr);
    URE_ARG(scratch_bytes >= need);
    hipStream_t st = static_cast<hipStream_t>(stream);
    double *cc = static_cast<double *>(scratch);
    hipLaunchKernelGGL(csr_cc_kernel, dim3(k), dim3(kCcLanes), 0, st, Ct, n_item, ldc, cc);
    const int G = group_width(k);
    const unsigned blocks = (unsigned)((n + kBlock / G - 1) / (kBlock / G));
#define URE_CSR_COST(W) \
    case W: hipLaunchKernelGGL(csr_cost_kernel<W>, dim3(blocks), dim3(kBlock), 0, st, row_off, col, val, n, n_item, Ct, ldc, k, cc, dist); break
    switch (G) {
        URE_CSR_COST(1);
        URE_CSR_COST(2);
        URE_CSR_COST(4);
        URE_CSR_COST(8);
        URE_CSR_COST(16);
        URE_CSR_COST(32);
        URE_CSR_COST(64);
    }
#undef URE_CSR_COST
    URE_HIP(hipGetLastError());
    return 0;
}

int ure_csr_centroids(const int64_t *col_off, const int32_t *row, const float *val, const int32_t *label, int64_t n, int64_t n_item, int k,
                      float *Ct, int ldc, int32_t *counts, void *stream)
{
    URE_ARG(col_off && row && val && label && Ct && counts);
    URE_ARG(n >= 1 && n <= INT32_MAX);
    URE_ARG(n_item >= 1 && n_item <= INT32_MAX);
    URE_ARG(k >= 1);
    URE_ARG(k <= kCsrMaxK);
    URE_ARG(ldc >= k);
    hipStream_t st = static_cast<hipStream_t>(stream);
    URE_HIP(hipMemsetAsync(counts, 0, (size_t)k * sizeof(int32_t), st));
    const unsigned cblocks = (unsigned)std::min<int64_t>((n + kBlock - 1) / kBlock, 1024);
    hipLaunchKernelGGL(csr_counts_kernel, dim3(cblocks), dim3(kBlock), 0, st, label, n, k, counts);
    const int G = group_width(k);
    const unsigned blocks = (unsigned)((n_item + kBlock / G - 1) / (kBlock / G));
#define URE_CSR_CENT(W) \
    case W: hipLaunchKernelGGL(csr_centroid_kernel<W>, dim3(blocks), dim3(kBlock), 0, st, col_off, row, val, label, n, n_item, k, counts, Ct, ldc); break
    switch (G) {
        URE_CSR_CENT(1);
        URE_CSR_CENT(2);
        URE_CSR_CENT(4);
        URE_CSR_CENT(8);
        URE_CSR_CENT(16);
        URE_CSR_CENT(32);
        URE_CSR_CENT(64);
    }
#undef URE_CSR_CENT
    URE_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"

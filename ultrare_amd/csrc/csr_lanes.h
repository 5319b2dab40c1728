// csr_lanes.h -- what the kernels that walk a CSR / CSC with a group of lanes share (csr_group.hip, csr_kmeans.hip): a lane
// owns one (row, centroid) or (item, cluster) pair, a group of G = pow2 >= min(k, 64) lanes shares the row (item), and the
// group hands the row's (index, value) stream round with cross-lane reads.
//
// The two walks are written once, over <Arith, G>.  Arith is a file's statement of its arithmetic and holds what differs
// between the OT route and the k-means route, nothing else; the ORDER in which a chain receives its terms -- the part of the
// contract both share -- is the walk's: ascending index, never split across lanes.
#pragma once
#include "group_width.h"
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

// Workgroups that give every one of `owners` rows (items) a group of G lanes.
inline unsigned group_blocks(int64_t owners, int G)
{
    return (unsigned)((owners + kBlock / G - 1) / (kBlock / G));
}

// The size checks every entry of the family makes, reported with the entry's own file and line.
#define URE_CSR_SIZES(n, n_item, k)                  \
    do {                                             \
        URE_ARG(n >= 1 && n <= INT32_MAX);           \
        URE_ARG(n_item >= 1 && n_item <= INT32_MAX); \
        URE_ARG(k >= 1);                             \
        URE_ARG(k <= kCsrMaxK);                      \
    } while (0)

// The row walk, the cost kernel of both routes: one lane owns each (row, centroid) pair and feeds dot_ic = sum x_ij Ct[j][c]
// and xx_i = sum x_ij^2 the stored entries of row i in ascending order; k > 64 loops over chunks of G centroids.  Arith: acc_t
// (an entry is converted to it once), norm_t, stride(ldc, k) of Ct, madd(acc, a, b) -> acc + a b, store(dist, c, i, n, k, dot,
// xx, norm).  (The first eight arguments arrive in SGPRs and the walk's first loads depend on them: keep their order.)
template <typename Arith, int G>
__global__ __launch_bounds__(kBlock) void csr_row_walk(const int64_t *__restrict__ row_off, const int32_t *__restrict__ col,
                                                       const float *__restrict__ val, int64_t n, int64_t n_item, const float *__restrict__ Ct,
                                                       int ldc, int k, const typename Arith::norm_t *__restrict__ norm, float *__restrict__ dist)
{
    using acc_t = typename Arith::acc_t;
    constexpr int kRows = kBlock / G;                      // rows of a workgroup
    const int sub = threadIdx.x % G;
    const int64_t i = (int64_t)blockIdx.x * kRows + threadIdx.x / G;
    if (i >= n) return;                                    // whole groups leave together
    const int64_t b = ldg(row_off + i), e = ldg(row_off + i + 1);
    const unsigned last_item = (unsigned)(n_item - 1);
    const int ld = Arith::stride(ldc, k);
    for (int c0 = 0; c0 < k; c0 += G) {                    // one pass for k <= 64
        const int c = c0 + sub;
        const float *__restrict__ ct = Ct + min(c, k - 1);  // padding lanes read a valid column and store nothing
        acc_t dot = 0, xx = 0;
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
                        cv[w] = ldg(ct + (size_t)j * ld);
                    }
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        const acc_t xv = x[w];
                        dot = Arith::madd(dot, xv, cv[w]);
                        xx = Arith::madd(xx, xv, xv);
                    }
                }
            } else {
                for (int u = 0; u < m; ++u) {
                    const unsigned j = group_read<G>(mine_j, u);
                    const acc_t xv = group_read<G>(mine_x, u);
                    dot = Arith::madd(dot, xv, ldg(ct + (size_t)j * ld));
                    xx = Arith::madd(xx, xv, xv);
                }
            }
        }
        if (c < k) Arith::store(dist, c, i, n, k, dot, xx, norm);
    }
}

// The column walk, the centroid kernel of both routes, owner computes: the group that owns item j walks its column in ascending user id; lane c adds the entry
// when the user's label is c, and stores Ct[j][c].  The entry and its label are uniform across the group: lane `sub` fetches
// entry p0 + sub AND that user's label, so the dependent label reads of G entries are in flight together.  A long column
// stays with its one owner.  Arith: acc_t, prep_t prepare(counts, c, k) before the walk, add(s, x, prep) -> s, and
// finish(s, prep, counts, c) after it: the policy says on which side of the walk it reads its count.
template <typename Arith, int G>
__global__ __launch_bounds__(kBlock) void csr_col_walk(const int64_t *__restrict__ col_off, const int32_t *__restrict__ row,
                                                       const float *__restrict__ val, const int32_t *__restrict__ label, int64_t n,
                                                       int64_t n_item, int k, const int32_t *__restrict__ counts, float *__restrict__ Ct, int ldc)
{
    using acc_t = typename Arith::acc_t;
    constexpr int kItems = kBlock / G;
    const int sub = threadIdx.x % G;
    const int64_t j = (int64_t)blockIdx.x * kItems + threadIdx.x / G;
    if (j >= n_item) return;
    const int64_t b = ldg(col_off + j), e = ldg(col_off + j + 1);
    const unsigned last_user = (unsigned)(n - 1);
    for (int c0 = 0; c0 < k; c0 += G) {
        const int c = c0 + sub;
        const typename Arith::prep_t prep = Arith::prepare(counts, c, k);
        acc_t s = 0;
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
                    const acc_t xv = group_read<G>(mine_x, u);
                    if (l == c) s = Arith::add(s, xv, prep);
                }
            } else {
                for (int u = 0; u < m; ++u) {
                    const int l = group_read<G>(mine_l, u);
                    const acc_t xv = group_read<G>(mine_x, u);
                    if (l == c) s = Arith::add(s, xv, prep);
                }
            }
        }
        if (c < k) stg(Ct + (size_t)j * ldc + c, Arith::finish(s, prep, counts, c));
    }
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

// counts[0 .. k) cleared, then filled from the n labels.
inline hipError_t launch_counts(const int32_t *label, int64_t n, int k, int32_t *counts, hipStream_t st)
{
    const hipError_t e = hipMemsetAsync(counts, 0, (size_t)k * sizeof(int32_t), st);
    if (e != hipSuccess) return e;
    const unsigned blocks = (unsigned)std::min<int64_t>((n + kBlock - 1) / kBlock, 1024);
    hipLaunchKernelGGL(csr_counts_kernel, dim3(blocks), dim3(kBlock), 0, st, label, n, k, counts);
    return hipSuccess;
}

}  // namespace ure

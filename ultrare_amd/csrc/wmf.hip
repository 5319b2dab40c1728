// wmf.hip -- the two device calls of weighted matrix factorisation for implicit feedback (Hu, Koren, Volinsky 2008) for gfx950:
// ure_gram, the Gram matrix of a whole fixed table, and ure_wridge_rows, ure_ridge_rows with a confidence weight per entry and
// that Gram matrix added to every system.  A half sweep of implicit ALS is one call of each.  Replaces nothing of
// the reference, which has no implicit-feedback trainer.
//
// The contract (wmf.py: gram_ref, wridge_rows_ref).
//   ure_gram   G0[a][b] = sum_i F[i][a] F[i][b], a <= b < k, in float64 as a two-level chain: within a chunk of 256 consecutive rows
//              the sum runs in ascending row order from 0.0; the chunk sums are added in ascending chunk order, starting from the
//              first.  A product of two float32 values is exact in float64, so every step rounds once and numpy reproduces the
//              BYTES.  The output is the packed upper triangle, row-major, k (k + 1) / 2 doubles.
//   ure_wridge_rows   for segment s with entries j in CSR order, n_s of them, f_j = (double)F[idx[j]][0:k]:
//              G = G0 + sum_j wg_j f_j f_j^T + (l2 + l2_n n_s) I,  b = sum_j wb_j f_j,  x = G^-1 b by the stages of ridge_solve.h.
//              The term for (a, b) is fma(wg_j f_a, f_b, acc) with wg_j f_a exact in double; G0 joins where the register blocks go
//              to the packed triangle: acc + G0[a][b], then + ridge on the diagonal.  G0 == NULL adds nothing (not even 0.0), so
//              with wg = 1 and wb = val the bytes are ure_ridge_rows's.  Empty segments, failures and status: as ure_ridge_rows.
//
// gram_chunk_kernel   one workgroup per chunk (a strided walk over chunks let the compiler keep the 64 store predicates of d = 128 in
//                     scalar registers across it, and spill them): the chunk's rows come through LDS in the ridge
//                     kernel's tiles and register blocks (ridge_solve.h); the blocks go to LDS as the packed triangle and from there
//                     to the chunk's partial triangle in scratch.
// gram_fold_kernel    one thread per entry of the triangle adds the partials in chunk order.
// No floating-point atomics: the bytes depend on (F, n, k) alone -- not on the stream or on how the workgroups are scheduled.
#include "ridge_solve.h"
#include "ultrare_wmf.h"

namespace ure {

constexpr int kGramChunk = URE_GRAM_CHUNK;

static_assert(kGramChunk % RrShape<4>::T == 0 && kGramChunk % RrShape<128>::T == 0, "a chunk is a whole number of tiles");

template <int D>
__global__ __launch_bounds__(kBlock) void gram_chunk_kernel(const float *__restrict__ F, int64_t n, int k, int64_t chunks,
                                                            double *__restrict__ part)
{
    using S = RrShape<D>;
    constexpr int TB = S::TB, T = S::T, Q = D / 4;
    extern __shared__ __attribute__((aligned(16))) char gr_lds[];
    double *tile = reinterpret_cast<double *>(gr_lds);      // S::MAIN doubles: the tile, later the packed triangle
    const int tid = threadIdx.x;
    const int tri = k * (k + 1) / 2;
    bool is_g, is_b;
    int bi, bj;
    rr_owner<D>(tid, is_g, is_b, bi, bj);

    const int64_t c = blockIdx.x;                          // one workgroup per chunk: nothing is carried from chunk to chunk
    if (c >= chunks) return;
    const int64_t r0 = c * kGramChunk, r1 = min<int64_t>(n, r0 + kGramChunk);
    double acc[TB][TB];
#pragma unroll
    for (int a = 0; a < TB; ++a)
#pragma unroll
        for (int b = 0; b < TB; ++b) acc[a][b] = 0.0;
    for (int64_t t0 = r0; t0 < r1; t0 += T) {
        const int cnt = (int)min<int64_t>(T, r1 - t0);
        __syncthreads();                               // the tile before this one has been read
        for (int q = tid; q < cnt * Q; q += kBlock) {
            const int t = q / Q, col = (q % Q) * 4;
            rr_stage4<D>(F, t0 + t, col, k, tile + t * D + col);
        }
        __syncthreads();
        if (is_g) {
            for (int t = 0; t < cnt; ++t) {
                const double *row = tile + t * D;
                double fa[TB], fb[TB];
#pragma unroll
                for (int a = 0; a < TB; ++a) {
                    fa[a] = row[bi * TB + a];
                    fb[a] = row[bj * TB + a];
                }
#pragma unroll
                for (int a = 0; a < TB; ++a)
#pragma unroll
                    for (int b = 0; b < TB; ++b) acc[a][b] = fma(fa[a], fb[b], acc[a][b]);
            }
        }
    }
    __syncthreads();                                   // the last tile has been read
    if (is_g) {                                        // the blocks to LDS as the packed triangle, as the ridge kernels place them ...
#pragma unroll
        for (int a = 0; a < TB; ++a)
#pragma unroll
            for (int b = 0; b < TB; ++b) {
                const int row = bi * TB + a, col = bj * TB + b;
                if (col >= row && col < k) tile[tri_row(row, k) + col - row] = acc[a][b];
            }
    }
    __syncthreads();
    double *P = part + (size_t)c * tri;                // ... and from there to the chunk's partial in whole lines
    for (int e = tid; e < tri; e += kBlock) P[e] = tile[e];
}

__global__ __launch_bounds__(kBlock) void gram_fold_kernel(const double *__restrict__ part, int64_t chunks, int tri, double *__restrict__ G0)
{
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= tri) return;
    double acc = part[e];
    for (int64_t c = 1; c < chunks; ++c) acc = acc + part[(size_t)c * tri + e];
    G0[e] = acc;
}

template <int D>
__global__ __launch_bounds__(kBlock) void wridge_rows_kernel(const float *__restrict__ F, int64_t n_fixed, int k,
                                                             const int64_t *__restrict__ off, const int32_t *__restrict__ idx,
                                                             const float *__restrict__ wg, const float *__restrict__ wb, int64_t m,
                                                             const int32_t *__restrict__ order, const double *__restrict__ G0,
                                                             double l2, double l2_n, float *__restrict__ X, int32_t *__restrict__ status)
{
    using S = RrShape<D>;
    constexpr int TB = S::TB, T = S::T, Q = D / 4;
    extern __shared__ __attribute__((aligned(16))) char wr_lds[];
    double *tile = reinterpret_cast<double *>(wr_lds);
    double *rt = tile + S::MAIN, *ys = rt + T, *bs = ys + D, *dg = bs + D, *gt = dg + D;     // RrShape's layout, then T weights
    __shared__ int bad;

    const int tid = threadIdx.x;
    const int64_t s = order ? (int64_t)order[blockIdx.x] : (int64_t)blockIdx.x;
    if (s < 0 || s >= m) return;
    const int64_t j0 = off[s], j1 = off[s + 1];
    float *xrow = X + (size_t)s * D;
    if (j1 <= j0) {
        for (int c = tid; c < D; c += kBlock) xrow[c] = 0.f;
        return;
    }

    bool is_g, is_b;
    int bi, bj;
    rr_owner<D>(tid, is_g, is_b, bi, bj);
    double acc[TB][TB];
#pragma unroll
    for (int a = 0; a < TB; ++a)
#pragma unroll
        for (int b = 0; b < TB; ++b) acc[a][b] = 0.0;
    if (tid == 0) bad = 0;

    // ---- accumulate: ridge_rows_kernel's, with the entry's confidence on the left factor and wb in the place of the rating
    for (int64_t t0 = j0; t0 < j1; t0 += T) {
        const int cnt = (int)min<int64_t>(T, j1 - t0);
        __syncthreads();                                   // the tile before this one has been read
        for (int q = tid; q < cnt * Q; q += kBlock) {
            const int t = q / Q, c = (q % Q) * 4;
            const int64_t i = idx[t0 + t];
            double *dst = tile + t * D + c;
            if (i >= 0 && i < n_fixed) {
                rr_stage4<D>(F, i, c, k, dst);
            } else {
                dst[0] = dst[1] = dst[2] = dst[3] = 0.0;
                bad = 1;
            }
        }
        if (tid < cnt) {
            rt[tid] = (double)wb[t0 + tid];
            gt[tid] = (double)wg[t0 + tid];
        }
        __syncthreads();
        if (is_g) {
            for (int t = 0; t < cnt; ++t) {
                const double *row = tile + t * D;
                const double w = gt[t];
                double fa[TB], fb[TB];
#pragma unroll
                for (int a = 0; a < TB; ++a) {
                    fa[a] = w * row[bi * TB + a];          // exact: two float32 values
                    fb[a] = row[bj * TB + a];
                }
#pragma unroll
                for (int a = 0; a < TB; ++a)
#pragma unroll
                    for (int b = 0; b < TB; ++b) acc[a][b] = fma(fa[a], fb[b], acc[a][b]);
            }
        } else if (is_b) {
            for (int t = 0; t < cnt; ++t) {
                const double r = rt[t];
                const double *row = tile + t * D + bi * TB;
#pragma unroll
                for (int b = 0; b < TB; ++b) acc[0][b] = fma(r, row[b], acc[0][b]);
            }
        }
    }
    __syncthreads();

    // ---- the packed upper triangle of G (k x k) over the tile: the blocks, the fixed table's Gram matrix, the ridge; b beside it
    const double ridge = l2 + l2_n * (double)(j1 - j0);
    double *G = tile;
    if (is_g) {
#pragma unroll
        for (int a = 0; a < TB; ++a)
#pragma unroll
            for (int b = 0; b < TB; ++b) {
                const int row = bi * TB + a, col = bj * TB + b;
                if (col >= row && col < k) {
                    const int e = tri_row(row, k) + col - row;
                    const double g = G0 ? acc[a][b] + G0[e] : acc[a][b];
                    G[e] = row == col ? g + ridge : g;
                }
            }
    } else if (is_b) {
#pragma unroll
        for (int b = 0; b < TB; ++b) bs[bi * TB + b] = acc[0][b];
    }
    __syncthreads();

    // ---- factor, solve, store (ridge_solve.h)
    rr_factor_solve_store<D>(G, bs, ys, dg, k, bad != 0, xrow, status, s);
}

template <int D>
static int launch_gram(const float *F, int64_t n, int k, double *G0, double *part, hipStream_t st)
{
    const int64_t chunks = (n + kGramChunk - 1) / kGramChunk;
    const int tri = k * (k + 1) / 2;
    const size_t lds = (size_t)RrShape<D>::MAIN * sizeof(double);
    auto kern = gram_chunk_kernel<D>;
    URE_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)chunks), dim3(kBlock), lds, st, F, n, k, chunks, part);
    URE_HIP(hipGetLastError());
    hipLaunchKernelGGL(gram_fold_kernel, dim3((unsigned)((tri + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, part, chunks, tri, G0);
    URE_HIP(hipGetLastError());
    return 0;
}

template <int D>
static int launch_wridge(const float *F, int64_t n_fixed, int k, const int64_t *off, const int32_t *idx, const float *wg, const float *wb,
                         int64_t m, const int32_t *order, const double *G0, double l2, double l2_n, float *X, int32_t *status, hipStream_t st)
{
    const size_t lds = (size_t)(RrShape<D>::DOUBLES + RrShape<D>::T) * sizeof(double);
    auto kern = wridge_rows_kernel<D>;
    URE_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)m), dim3(kBlock), lds, st, F, n_fixed, k, off, idx, wg, wb, m, order, G0, l2, l2_n, X, status);
    URE_HIP(hipGetLastError());
    return 0;
}

}  // namespace ure

using namespace ure;

extern "C" {

int64_t ure_gram_scratch(int64_t n, int k)
{
    if (n < 1 || n > INT32_MAX || k < 1 || k > kRrMaxD) return -1;
    const int64_t chunks = (n + kGramChunk - 1) / kGramChunk;
    return chunks * (int64_t)(k * (k + 1) / 2) * (int64_t)sizeof(double);
}

int ure_gram(const float *F, int64_t n, int d, int k, double *G0, void *scratch, int64_t scratch_bytes, void *stream)
{
    URE_ARG(F && G0);
    URE_ARG(n >= 1 && n <= INT32_MAX);
    URE_ARG(k >= 1 && k <= d);
    URE_ARG(pow2(d) && d >= 4 && d <= kRrMaxD);
    const int64_t need = ure_gram_scratch(n, k);
    URE_ARG(need > 0 && scratch && scratch_bytes >= need);
    hipStream_t st = static_cast<hipStream_t>(stream);
    double *part = static_cast<double *>(scratch);
#define URE_GR(W) return launch_gram<W>(F, n, k, G0, part, st)
    switch (d) {
        case 4: URE_GR(4);
        case 8: URE_GR(8);
        case 16: URE_GR(16);
        case 32: URE_GR(32);
        case 64: URE_GR(64);
        case 128: URE_GR(128);
    }
#undef URE_GR
    return fail(-1, "ure_gram: unsupported d=%d", d);
}

int64_t ure_wridge_rows_scratch(int64_t m, int k)
{
    if (m < 0 || k < 1 || k > kRrMaxD) return -1;
    return 0;                                          // G never leaves the chip
}

int ure_wridge_rows(const float *F, int64_t n_fixed, int d, int k, const int64_t *off, const int32_t *idx, const float *wg, const float *wb,
                    int64_t m, const int32_t *order, const double *G0, double l2, double l2_n, float *X, int32_t *status, void *scratch,
                    int64_t scratch_bytes, void *stream)
{
    URE_ARG(F && off && idx && wg && wb && X && status);
    URE_ARG(n_fixed >= 1);
    URE_ARG(k >= 1 && k <= d);
    URE_ARG(pow2(d) && d >= 4 && d <= kRrMaxD);
    URE_ARG(m >= 0 && m <= INT32_MAX);
    URE_ARG(l2 >= 0.0 && l2 <= DBL_MAX);
    URE_ARG(l2_n >= 0.0 && l2_n <= DBL_MAX);
    const int64_t need = ure_wridge_rows_scratch(m, k);
    URE_ARG(need >= 0 && scratch_bytes >= need && (need == 0 || scratch));
    hipStream_t st = static_cast<hipStream_t>(stream);
    URE_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), st));
    URE_HIP(hipMemsetAsync(status + 1, 0xFF, sizeof(int32_t), st));
    if (m == 0) return 0;
#define URE_WR(W) return launch_wridge<W>(F, n_fixed, k, off, idx, wg, wb, m, order, G0, l2, l2_n, X, status, st)
    switch (d) {
        case 4: URE_WR(4);
        case 8: URE_WR(8);
        case 16: URE_WR(16);
        case 32: URE_WR(32);
        case 64: URE_WR(64);
        case 128: URE_WR(128);
    }
#undef URE_WR
    return fail(-1, "ure_wridge_rows: unsupported d=%d", d);
}

}  // extern "C"

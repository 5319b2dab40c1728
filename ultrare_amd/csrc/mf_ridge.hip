// mf_ridge.hip -- many small ridge systems for gfx950 (ure_ridge_rows): each segment of a CSR gathers rows of a FIXED table,
// accumulates its normal equations and solves them, all by one workgroup, in float64.  Fold-in of new users and the two
// halves of an ALS sweep are this one call.  Replaces nothing of the reference, which has no fold-in.
//
// The contract (ridge.py: ridge_rows_ref), for segment s with entries j = off[s] .. off[s + 1] - 1, n_s of them:
//   f_j = (double)F[idx[j]][0:k], r_j = (double)val[j]
//   G = sum_j f_j f_j^T + (l2 + l2_n n_s) I,  b = sum_j r_j f_j,  x = G^-1 b by Cholesky (G = R^T R) and two substitutions,
//   all in float64; x is rounded to float32 once, at the store.  Columns k .. d - 1 of X are written as zero.
//   An empty segment gives the zero row.  A pivot that is not positive and finite (or an index outside the table, or a
//   solution that is not finite) fills the row's k columns with NaN and counts in status = { failed segments, smallest
//   failed segment index (-1: none) }, kept with integer atomics.
//
// ridge_rows_kernel, one workgroup per segment (segment order[blockIdx.x], so that the host can hand out the longest first):
//   accumulate  the segment's rows come through LDS in tiles of T rows (as doubles, columns >= k zeroed).  G lives in
//               REGISTERS: thread t < NB (NB + 1) / 2 owns a TB x TB block of the upper triangle (TB = d / 16: 64 doubles at
//               d = 128) and the next NB threads own TB entries of b each; every sum takes the segment's entries in CSR order.
//               A product of two float32 values is exact in float64, so fma and multiply-add round alike here.
//   factor      the blocks go to LDS as the packed upper triangle (over the tile's space: 66,048 bytes at k = 128), the ridge
//               joins the diagonal, and a right-looking Cholesky runs there: per column one row scaling and one trailing update
//               spread over the 256 threads (2 barriers).
//   solve       thread c < k carries entry c of the right-hand side in a register through R^T y = b and R x = y, column by
//               column (1 barrier per column each).
// The shape, the staging of a tile and the factor / solve / store stages are ridge_solve.h's, shared with wmf.hip.
// No floating-point atomics and no sum that crosses workgroups: a row's bytes depend on its own segment alone -- not on the
// stream, on `order`, or on what else is in the call.
#include "ridge_solve.h"

namespace ure {

template <int D>
__global__ __launch_bounds__(kBlock) void ridge_rows_kernel(const float *__restrict__ F, int64_t n_fixed, int k,
                                                            const int64_t *__restrict__ off, const int32_t *__restrict__ idx,
                                                            const float *__restrict__ val, int64_t m, const int32_t *__restrict__ order,
                                                            double l2, double l2_n, float *__restrict__ X, int32_t *__restrict__ status)
{
    using S = RrShape<D>;
    constexpr int TB = S::TB, T = S::T, Q = D / 4;
    extern __shared__ __attribute__((aligned(16))) char rr_lds[];
    double *tile = reinterpret_cast<double *>(rr_lds);
    double *rt = tile + S::MAIN, *ys = rt + T, *bs = ys + D, *dg = bs + D;
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

    // the block this thread owns: row-major over the upper triangle of NB x NB blocks, then the NB blocks of b
    bool is_g, is_b;
    int bi, bj;
    rr_owner<D>(tid, is_g, is_b, bi, bj);
    double acc[TB][TB];
#pragma unroll
    for (int a = 0; a < TB; ++a)
#pragma unroll
        for (int b = 0; b < TB; ++b) acc[a][b] = 0.0;
    if (tid == 0) bad = 0;

    // ---- accumulate
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
        if (tid < cnt) rt[tid] = (double)val[t0 + tid];
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

    // ---- the packed upper triangle of G (k x k) over the tile, b beside it
    const double ridge = l2 + l2_n * (double)(j1 - j0);
    double *G = tile;
    if (is_g) {
#pragma unroll
        for (int a = 0; a < TB; ++a)
#pragma unroll
            for (int b = 0; b < TB; ++b) {
                const int row = bi * TB + a, col = bj * TB + b;
                if (col >= row && col < k) G[tri_row(row, k) + col - row] = row == col ? acc[a][b] + ridge : acc[a][b];
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
static int launch_ridge(const float *F, int64_t n_fixed, int k, const int64_t *off, const int32_t *idx, const float *val, int64_t m,
                        const int32_t *order, double l2, double l2_n, float *X, int32_t *status, hipStream_t st)
{
    const size_t lds = (size_t)RrShape<D>::DOUBLES * sizeof(double);
    auto kern = ridge_rows_kernel<D>;
    URE_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)m), dim3(kBlock), lds, st, F, n_fixed, k, off, idx, val, m, order, l2, l2_n, X, status);
    URE_HIP(hipGetLastError());
    return 0;
}

}  // namespace ure

using namespace ure;

extern "C" {

int64_t ure_ridge_rows_scratch(int64_t m, int k)
{
    if (m < 0 || k < 1 || k > kRrMaxD) return -1;
    return 0;                                          // G never leaves the chip
}

int ure_ridge_rows(const float *F, int64_t n_fixed, int d, int k, const int64_t *off, const int32_t *idx, const float *val, int64_t m,
                   const int32_t *order, double l2, double l2_n, float *X, int32_t *status, void *scratch, int64_t scratch_bytes,
                   void *stream)
{
    URE_ARG(F && off && idx && val && X && status);
    URE_ARG(n_fixed >= 1);
    URE_ARG(k >= 1 && k <= d);
    URE_ARG(pow2(d) && d >= 4 && d <= kRrMaxD);
    URE_ARG(m >= 0 && m <= INT32_MAX);
    URE_ARG(l2 >= 0.0 && l2 <= DBL_MAX);
    URE_ARG(l2_n >= 0.0 && l2_n <= DBL_MAX);
    const int64_t need = ure_ridge_rows_scratch(m, k);
    URE_ARG(need >= 0 && scratch_bytes >= need && (need == 0 || scratch));
    hipStream_t st = static_cast<hipStream_t>(stream);
    URE_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), st));
    URE_HIP(hipMemsetAsync(status + 1, 0xFF, sizeof(int32_t), st));
    if (m == 0) return 0;
#define URE_RR(W) return launch_ridge<W>(F, n_fixed, k, off, idx, val, m, order, l2, l2_n, X, status, st)
    switch (d) {
        case 4: URE_RR(4);
        case 8: URE_RR(8);
        case 16: URE_RR(16);
        case 32: URE_RR(32);
        case 64: URE_RR(64);
        case 128: URE_RR(128);
    }
#undef URE_RR
    return fail(-1, "ure_ridge_rows: unsupported d=%d", d);
}

}  // extern "C"

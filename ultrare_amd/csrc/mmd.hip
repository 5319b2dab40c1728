// mmd.hip -- attribute unlearning losses on selected rows of a float32 table, for gfx950.
//
// The reference's rbk / mmd_loss / buildLap (utils.py:223-279) compare the embeddings of two user groups S (the first n1
// selected rows) and T (the other n2).  With L_ij = |x_i - x_j|^2 over the m = n1 + n2 selected rows,
//   K_ij = sum_q exp(-L_ij / bw_q),   bw_q = bw / kernel_mul^(kernel_num / 2) * kernel_mul^q,   q = 0 .. kernel_num - 1,
//   loss = mean(K_SS) + mean(K_TT) - mean(K_ST) - mean(K_TS),
//   g_i  = sum_j c_ij w_ij (x_i - x_j),   w_ij = sum_q (-2 / bw_q) exp(-L_ij / bw_q),
//   c_ij = 2 / n1^2 (both in S), 2 / n2^2 (both in T), -2 / (n1 n2) (otherwise);  no gradient through bw.
// K is an implicit m x m matrix that is never written (ure_mmd_matrix apart, which is what rbk returns): workgroup
// (blockIdx.x, blockIdx.y) owns a tile of kMmdTile selected rows and walks the columns of split blockIdx.y a tile at a
// time, the features of both staged feature-major in LDS.
//   L     direct difference form, one fmaf per feature j = 0 .. d - 1 in order into one float32 accumulator (as
//         pair_tile of pair_dist.hip): L_ij == L_ji bit for bit, L_ii == 0.
//   K, w  one expf per bandwidth (the accurate one: no fast-math intrinsic), q in order; every K_ij goes straight into
//         a float64 accumulator of its block (SS, TT, ST, TS).
//   g     c_ij w_ij is parked in LDS; thread (ty, tx) owns rows ty + 16 i and features tx + 16 q and folds the tile's
//         64 columns in order, fmaf(c w, x_i - x_j, .), into float32 partial sums -- at most 64 terms long -- which it
//         then adds to float64 accumulators.
// Partial results go to scratch and are combined in a fixed order (split order; the four sums in a fixed tree): no
// floating-point atomics, the same arguments give the same bytes on any stream.  Unselected rows and the padding columns
// d .. ld - 1 are never read.
//
// The bandwidth's closed form and the u2u (Laplacian) loss share attr_colsum_kernel: per group and column the float64
// sums of (x - s) and (x - s)^2, s = the first selected row (both are invariant under a common shift; a shift inside the
// data keeps the closed form free of cancellation).
#include "mmd_tile.h"

namespace ure {

template <int DQ, bool GRAD>
__global__ __launch_bounds__(kBlock) void mmd_kernel(const float *__restrict__ X, int64_t ld, int d, const int32_t *__restrict__ rows, int m,
                                                     int n1, double kernel_mul, int kn, const double *__restrict__ bandwidth, float c_ss,
                                                     float c_tt, float c_x, int span, double *__restrict__ part_sums,
                                                     double *__restrict__ part_grad)
{
    extern __shared__ float mmd_lds[];
    mmd_tile_body<DQ, GRAD>(mmd_lds, X, ld, d, rows, m, n1, kernel_mul, kn, bandwidth, c_ss, c_tt, c_x, span, (int64_t)m * d, part_sums, part_grad);
}

// One workgroup: sums[k] = sum of the n_part partial sums, thread t taking t, t + 256, ... and the threads a fixed tree.
__global__ __launch_bounds__(kBlock) void mmd_sums_kernel(const double *__restrict__ part_sums, int64_t n_part, double *__restrict__ sums)
{
    __shared__ double red[kBlock][4];
    const double v = mmd_sums_fold(red, part_sums, n_part);
    if (threadIdx.x < 4) sums[threadIdx.x] = v;
}

// grad[e] = (float) of the splits' float64 partials of entry e added in split order.
__global__ __launch_bounds__(kBlock) void mmd_grad_combine_kernel(const double *__restrict__ part_grad, int splits, int64_t md, float *__restrict__ grad)
{
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < md; e += (int64_t)gridDim.x * kBlock) grad[e] = mmd_grad_entry(part_grad, splits, md, e);
}

// K [m x m] float32 itself, a tile per workgroup (rbk's return value; small m only).
__global__ __launch_bounds__(kBlock) void mmd_matrix_kernel(const float *__restrict__ X, int64_t ld, int d, int F, const int32_t *__restrict__ rows,
                                                            int64_t m, double kernel_mul, int kn, const double *__restrict__ bandwidth,
                                                            float *__restrict__ Kout)
{
    extern __shared__ float mmd_lds[];
    float *xr = mmd_lds, *xc = xr + F * kMmdLd, *ninv = xc + F * kMmdLd;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int64_t row0 = (int64_t)blockIdx.x * kMmdTile, c0 = (int64_t)blockIdx.y * kMmdTile;
    mmd_bandwidths(ninv, bandwidth, kernel_mul, kn);
    mmd_stage(xr, X, ld, d, F, rows, row0, m);
    mmd_stage(xc, X, ld, d, F, rows, c0, m);
    __syncthreads();
    float K[4][4], W[4][4];
    mmd_pair(xr, xc, d, ninv, kn, ty, tx, K, W);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t gi = row0 + ty + 16 * i, gj = c0 + tx + 16 * j;
            if (gi < m && gj < m) Kout[gi * m + gj] = K[i][j];
        }
}

// ---- column sums (the bodies are mmd_tile.h's) -------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void attr_colsum_kernel(const float *__restrict__ X, int64_t ld, int d, int slots, const int32_t *__restrict__ rows,
                                                             int64_t m, int64_t n1, int64_t per, double *__restrict__ partial)
{
    attr_colsum_body(X, ld, d, slots, rows, m, n1, per, partial);
}

__global__ __launch_bounds__(kMmdMaxD) void attr_stats_kernel(const float *__restrict__ X, int64_t ld, int d, const int32_t *__restrict__ rows, int64_t m,
                                                              int64_t n1, const double *__restrict__ partial, int blocks, double *__restrict__ stats,
                                                              double *__restrict__ bw_out, double *__restrict__ u2u_out)
{
    double bw = 0.0, u2u = 0.0;
    attr_stats_body(X, ld, d, rows, m, n1, partial, blocks, stats, bw, u2u);
    if (threadIdx.x == 0) {
        if (bw_out) *bw_out = bw;
        if (u2u_out) *u2u_out = u2u;
    }
}

__global__ __launch_bounds__(kBlock) void u2u_grad_kernel(const float *__restrict__ X, int64_t ld, int d, const int32_t *__restrict__ rows, int64_t m,
                                                          int64_t n1, const double *__restrict__ stats, float *__restrict__ grad)
{
    const double dn1 = (double)n1, dn2 = (double)(m - n1);
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < m * d; e += (int64_t)gridDim.x * kBlock)
        grad[e] = u2u_grad_entry(X, ld, rows, e / d, (int)(e % d), n1, dn1, dn2, stats);
}

static int check_rows(const float *X, int64_t ld, int d, const int32_t *rows, int64_t n1, int64_t n2)
{
    URE_ARG(X && rows);
    URE_ARG(n1 >= 1 && n2 >= 1 && n1 <= INT32_MAX && n2 <= INT32_MAX);
    URE_ARG(mmd_shape_ok(n1 + n2, d));
    URE_ARG(ld >= d);
    return 0;
}

static int launch_stats(const float *X, int64_t ld, int d, const int32_t *rows, int64_t m, int64_t n1, char *scratch, const MmdPlan &p,
                        double *bw_out, double *u2u_out, hipStream_t st)
{
    int slots = 1;
    while (slots < d) slots <<= 1;
    double *stats = reinterpret_cast<double *>(scratch), *partial = reinterpret_cast<double *>(scratch + p.off_partial);
    const int64_t per = (m + p.colsum_blocks - 1) / p.colsum_blocks;
    attr_colsum_kernel<<<p.colsum_blocks, kBlock, 0, st>>>(X, ld, d, slots, rows, m, n1, per, partial);
    URE_HIP(hipGetLastError());
    attr_stats_kernel<<<1, kMmdMaxD, 0, st>>>(X, ld, d, rows, m, n1, partial, p.colsum_blocks, stats, bw_out, u2u_out);
    URE_HIP(hipGetLastError());
    return 0;
}

template <int DQ, bool GRAD>
static int launch_mmd(const float *X, int64_t ld, int d, const int32_t *rows, int64_t m, int64_t n1, double kernel_mul, int kn, const double *bandwidth,
                      const MmdPlan &p, double *part_sums, double *part_grad, hipStream_t st)
{
    const size_t lds = mmd_lds_bytes(16 * DQ, true);
    auto kern = mmd_kernel<DQ, GRAD>;
    URE_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const double dn1 = (double)n1, dn2 = (double)(m - n1);
    hipLaunchKernelGGL(kern, dim3((unsigned)p.row_tiles, (unsigned)p.splits), dim3(kBlock), lds, st, X, ld, d, rows, (int)m, (int)n1, kernel_mul, kn, bandwidth,
                       (float)(2.0 / (dn1 * dn1)), (float)(2.0 / (dn2 * dn2)), (float)(-2.0 / (dn1 * dn2)), (int)p.span, part_sums, part_grad);
    URE_HIP(hipGetLastError());
    return 0;
}

}  // namespace ure

using namespace ure;

extern "C" {

int64_t ure_mmd_scratch(int64_t m, int32_t d)
{
    if (!mmd_shape_ok(m, d)) return -1;
    return mmd_plan(m, d).bytes;
}

int32_t ure_mmd_splits(int64_t m, int32_t d)
{
    if (!mmd_shape_ok(m, d)) return -1;
    return mmd_plan(m, d).splits;
}

int ure_mmd_bandwidth(const float *X, int64_t ld, int32_t d, const int32_t *rows, int64_t n1, int64_t n2, double *bandwidth, void *scratch,
                      int64_t scratch_bytes, void *stream)
{
    if (int rc = check_rows(X, ld, d, rows, n1, n2)) return rc;
    URE_ARG(bandwidth);
    const MmdPlan p = mmd_plan(n1 + n2, d);
    URE_ARG(scratch && scratch_bytes >= p.bytes);
    return launch_stats(X, ld, d, rows, n1 + n2, n1, static_cast<char *>(scratch), p, bandwidth, nullptr, static_cast<hipStream_t>(stream));
}

int ure_u2u_loss_grad(const float *X, int64_t ld, int32_t d, const int32_t *rows, int64_t n1, int64_t n2, double *value, float *grad, void *scratch,
                      int64_t scratch_bytes, void *stream)
{
    if (int rc = check_rows(X, ld, d, rows, n1, n2)) return rc;
    URE_ARG(value);
    const int64_t m = n1 + n2;
    const MmdPlan p = mmd_plan(m, d);
    URE_ARG(scratch && scratch_bytes >= p.bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = launch_stats(X, ld, d, rows, m, n1, static_cast<char *>(scratch), p, nullptr, value, st)) return rc;
    if (grad) {
        const unsigned blocks = (unsigned)std::min<int64_t>((m * d + kBlock - 1) / kBlock, 4096);
        u2u_grad_kernel<<<blocks, kBlock, 0, st>>>(X, ld, d, rows, m, n1, static_cast<const double *>(scratch), grad);
        URE_HIP(hipGetLastError());
    }
    return 0;
}

int ure_mmd_loss_grad(const float *X, int64_t ld, int32_t d, const int32_t *rows, int64_t n1, int64_t n2, double kernel_mul, int32_t kernel_num,
                      const double *bandwidth, double *sums, float *grad, void *scratch, int64_t scratch_bytes, void *stream)
{
    if (int rc = check_rows(X, ld, d, rows, n1, n2)) return rc;
    URE_ARG(kernel_mul > 0.0 && kernel_mul <= 1.79769313486231570e308);
    URE_ARG(kernel_num >= 1 && kernel_num <= kMmdMaxKernels);
    URE_ARG(bandwidth && sums);
    const int64_t m = n1 + n2;
    const MmdPlan p = mmd_plan(m, d);
    URE_ARG(scratch && scratch_bytes >= p.bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    char *base = static_cast<char *>(scratch);
    double *part_sums = reinterpret_cast<double *>(base + p.off_sums), *part_grad = reinterpret_cast<double *>(base + p.off_grad);
    int rc;
#define URE_MMD(DQ) rc = grad ? launch_mmd<DQ, true>(X, ld, d, rows, m, n1, kernel_mul, kernel_num, bandwidth, p, part_sums, part_grad, st) \
                              : launch_mmd<DQ, false>(X, ld, d, rows, m, n1, kernel_mul, kernel_num, bandwidth, p, part_sums, part_grad, st)
    if (d <= 16) URE_MMD(1);
    else if (d <= 32) URE_MMD(2);
    else if (d <= 64) URE_MMD(4);
    else URE_MMD(8);
#undef URE_MMD
    if (rc) return rc;
    mmd_sums_kernel<<<1, kBlock, 0, st>>>(part_sums, p.row_tiles * p.splits, sums);
    URE_HIP(hipGetLastError());
    if (grad) {
        const unsigned blocks = (unsigned)std::min<int64_t>((m * d + kBlock - 1) / kBlock, 4096);
        mmd_grad_combine_kernel<<<blocks, kBlock, 0, st>>>(part_grad, p.splits, m * d, grad);
        URE_HIP(hipGetLastError());
    }
    return 0;
}

int ure_mmd_matrix(const float *X, int64_t ld, int32_t d, const int32_t *rows, int64_t m, double kernel_mul, int32_t kernel_num,
                   const double *bandwidth, float *K, void *stream)
{
    URE_ARG(X && rows && bandwidth && K);
    URE_ARG(m >= 1 && m <= 8192);
    URE_ARG(d >= 1 && d <= kMmdMaxD && ld >= d);
    URE_ARG(kernel_mul > 0.0 && kernel_mul <= 1.79769313486231570e308);
    URE_ARG(kernel_num >= 1 && kernel_num <= kMmdMaxKernels);
    const int F = (d + 15) / 16 * 16;
    const size_t lds = mmd_lds_bytes(F, false);
    URE_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(mmd_matrix_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const unsigned tiles = (unsigned)((m + kMmdTile - 1) / kMmdTile);
    mmd_matrix_kernel<<<dim3(tiles, tiles), kBlock, lds, static_cast<hipStream_t>(stream)>>>(X, ld, d, F, rows, m, kernel_mul, kernel_num, bandwidth, K);
    URE_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"

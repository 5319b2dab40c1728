// attr_train.hip -- in-training attribute unlearning for gfx950 (include/ultrare_attr_train.h): the per-batch MMD ('d2d')
// or Laplacian ('u2u') term of the reference's training loop (utils.py:46-111) on the batch's distinct users of two attribute groups.
// The rows of a step and their counts (n1, n2) change every step and live in device memory; a training job reads nothing back.
//
//   masks    once per epoch: per user a bitset over the epoch's steps.  A wave owns a user and walks its CSR row once per 256 steps
//            (8 words held in registers, an OR butterfly over the wave): no atomics, rows of any length, every word written.
//   select   per step: an ordered compaction of the users whose bit is set, group 1 and then group 2, each in ascending id.  A
//            workgroup owns kSelChunk consecutive users; launch 1 counts both groups per workgroup, launch 2 adds the counts of the
//            workgroups in front of it (integers: any order gives the same sum) and scans its own users.  The place of a user in the
//            output is a function of the flags alone.
//   losses   mmd.hip's tile arithmetic (mmd_tile.h) with grids and scratch planned from the capacities (cap1, cap2) and m, n1 and the
//            coefficients read / derived from `counts` on the device; tiles past m contribute exact zeros, gradient rows at or
//            beyond m are written +0.0.  A step without both groups, or with a bandwidth that is not positive and finite, is not
//            valid: its outputs are +0.0 and the accumulator keeps its bytes.
//   hand-off G[rows[i]] += eta grad[i] for the selected rows of a valid step.
#include "mmd_tile.h"

namespace ure {

constexpr int kSelPerThread = 8;
constexpr int kSelChunk = kBlock * kSelPerThread;     // users per workgroup of the selection
constexpr int kMaskWords = 8;                         // words (256 steps) a wave gathers per walk of a row

__device__ __forceinline__ uint32_t wave_or(uint32_t v)
{
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) v |= (uint32_t)__shfl_xor((int)v, o, kWave);
    return v;
}

// A wave per user.
__global__ __launch_bounds__(kBlock) void attr_masks_kernel(const int64_t *__restrict__ off, const int32_t *__restrict__ tag, const int8_t *__restrict__ group,
                                                            int64_t n_user, int64_t nnz, int steps, int words, uint32_t *__restrict__ masks)
{
    const int lane = threadIdx.x & (kWave - 1);
    for (int64_t u = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave; u < n_user; u += (int64_t)gridDim.x * kWavesPerBlock) {
        const bool member = ldg(group + u) != 0;
        const int64_t b = max((int64_t)0, min(nnz, ldg(off + u))), e = max(b, min(nnz, ldg(off + u + 1)));
        for (int w0 = 0; w0 < words; w0 += kMaskWords) {
            uint32_t bits[kMaskWords];
#pragma unroll
            for (int k = 0; k < kMaskWords; ++k) bits[k] = 0u;
            if (member) {
                for (int64_t p = b + lane; p < e; p += kWave) {
                    const int t = ldg(tag + p);
                    const int w = (t >> 5) - w0;
                    if (t >= 0 && t < steps && w >= 0 && w < kMaskWords) {
#pragma unroll
                        for (int k = 0; k < kMaskWords; ++k)
                            if (k == w) bits[k] |= 1u << (t & 31);
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < kMaskWords; ++k) {
                const uint32_t v = wave_or(bits[k]);
                if (lane == 0 && w0 + k < words) masks[u * words + w0 + k] = v;
            }
        }
    }
}

// 1, 2 or 0: the group of user u if its bit of the step is set.
__device__ __forceinline__ int sel_flag(const uint32_t *__restrict__ masks, const int8_t *__restrict__ group, int64_t u, int64_t n_user, int words, int word,
                                        uint32_t bit)
{
    if (u >= n_user) return 0;
    const int g = ldg(group + u);
    if (g != 1 && g != 2) return 0;
    return (ldg(masks + u * words + word) & bit) ? g : 0;
}

// block_counts [blocks][2]
__global__ __launch_bounds__(kBlock) void attr_sel_count_kernel(const uint32_t *__restrict__ masks, const int8_t *__restrict__ group, int64_t n_user, int words,
                                                                int step, int32_t *__restrict__ block_counts)
{
    __shared__ int red[kWavesPerBlock][2];
    const int tid = threadIdx.x, word = step >> 5;
    const uint32_t bit = 1u << (step & 31);
    const int64_t u0 = (int64_t)blockIdx.x * kSelChunk + (int64_t)tid * kSelPerThread;
    int c1 = 0, c2 = 0;
#pragma unroll
    for (int k = 0; k < kSelPerThread; ++k) {
        const int f = sel_flag(masks, group, u0 + k, n_user, words, word, bit);
        c1 += f == 1;
        c2 += f == 2;
    }
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        c1 += __shfl_xor(c1, o, kWave);
        c2 += __shfl_xor(c2, o, kWave);
    }
    if ((tid & (kWave - 1)) == 0) {
        red[tid / kWave][0] = c1;
        red[tid / kWave][1] = c2;
    }
    __syncthreads();
    if (tid < 2) {
        int v = 0;
        for (int w = 0; w < kWavesPerBlock; ++w) v += red[w][tid];
        block_counts[(int64_t)blockIdx.x * 2 + tid] = v;
    }
}

__global__ __launch_bounds__(kBlock) void attr_sel_scatter_kernel(const uint32_t *__restrict__ masks, const int8_t *__restrict__ group, int64_t n_user,
                                                                  int words, int step, const int32_t *__restrict__ block_counts, int64_t cap1,
                                                                  int64_t cap2, int32_t *__restrict__ rows, int32_t *__restrict__ counts)
{
    __shared__ int64_t tot[kBlock][4];            // per thread: group 1 and 2 in front of this workgroup, group 1 and 2 in all
    __shared__ int scan[2][kBlock];
    const int tid = threadIdx.x, word = step >> 5;
    const uint32_t bit = 1u << (step & 31);
    int64_t before1 = 0, before2 = 0, all1 = 0, all2 = 0;
    for (int64_t b = tid; b < (int64_t)gridDim.x; b += kBlock) {
        const int a1 = block_counts[b * 2], a2 = block_counts[b * 2 + 1];
        all1 += a1;
        all2 += a2;
        if (b < (int64_t)blockIdx.x) {
            before1 += a1;
            before2 += a2;
        }
    }
    tot[tid][0] = before1;
    tot[tid][1] = before2;
    tot[tid][2] = all1;
    tot[tid][3] = all2;
    __syncthreads();
    for (int o = kBlock / 2; o > 0; o >>= 1) {
        if (tid < o)
#pragma unroll
            for (int k = 0; k < 4; ++k) tot[tid][k] += tot[tid + o][k];
        __syncthreads();
    }
    before1 = tot[0][0];
    before2 = tot[0][1];
    const int64_t n1 = min(tot[0][2], cap1), n2 = min(tot[0][3], cap2);
    // this workgroup's users: flags, then an inclusive scan of the threads' counts
    const int64_t u0 = (int64_t)blockIdx.x * kSelChunk + (int64_t)tid * kSelPerThread;
    int flag[kSelPerThread], c1 = 0, c2 = 0;
#pragma unroll
    for (int k = 0; k < kSelPerThread; ++k) {
        flag[k] = sel_flag(masks, group, u0 + k, n_user, words, word, bit);
        c1 += flag[k] == 1;
        c2 += flag[k] == 2;
    }
    scan[0][tid] = c1;
    scan[1][tid] = c2;
    __syncthreads();
    for (int o = 1; o < kBlock; o <<= 1) {
        const int a1 = tid >= o ? scan[0][tid - o] : 0, a2 = tid >= o ? scan[1][tid - o] : 0;
        __syncthreads();
        scan[0][tid] += a1;
        scan[1][tid] += a2;
        __syncthreads();
    }
    int64_t at1 = before1 + scan[0][tid] - c1, at2 = before2 + scan[1][tid] - c2;
#pragma unroll
    for (int k = 0; k < kSelPerThread; ++k) {
        if (flag[k] == 1) {
            if (at1 < n1) rows[at1] = (int32_t)(u0 + k);
            ++at1;
        } else if (flag[k] == 2) {
            if (at2 < n2) rows[n1 + at2] = (int32_t)(u0 + k);
            ++at2;
        }
    }
    // what lies behind the selected rows, and the counts
    const int64_t cap = cap1 + cap2;
    for (int64_t i = n1 + n2 + (int64_t)blockIdx.x * kBlock + tid; i < cap; i += (int64_t)gridDim.x * kBlock) rows[i] = -1;
    if (blockIdx.x == 0 && tid < 2) counts[tid] = (int32_t)(tid == 0 ? n1 : n2);
}

// ---- the losses at device counts ------------------------------------------------------------------------------------------------
struct StepCounts {
    int64_t m, n1;
};
__device__ __forceinline__ StepCounts step_counts(const int32_t *__restrict__ counts, int64_t cap1, int64_t cap2)
{
    const int64_t n1 = max((int64_t)0, min((int64_t)ldg(counts), cap1)), n2 = max((int64_t)0, min((int64_t)ldg(counts + 1), cap2));
    return {n1 + n2, n1};
}

__global__ __launch_bounds__(kBlock) void attr_colsum_dev_kernel(const float *__restrict__ X, int64_t ld, int d, int slots, const int32_t *__restrict__ rows,
                                                                 const int32_t *__restrict__ counts, int64_t cap1, int64_t cap2,
                                                                 double *__restrict__ partial)
{
    const StepCounts c = step_counts(counts, cap1, cap2);
    if (c.m < 1) return;                                   // (attr_stats_dev_kernel reads no partial then)
    attr_colsum_body(X, ld, d, slots, rows, c.m, c.n1, (c.m + gridDim.x - 1) / gridDim.x, partial);
}

// mmd: 1 the bandwidth decides validity (the MMD), 0 the counts alone (u2u).  fix_sigma > 0 stands for the bandwidth.
__global__ __launch_bounds__(kMmdMaxD) void attr_stats_dev_kernel(const float *__restrict__ X, int64_t ld, int d, const int32_t *__restrict__ rows,
                                                                  const int32_t *__restrict__ counts, int64_t cap1, int64_t cap2,
                                                                  const double *__restrict__ partial, int blocks, int mmd, double fix_sigma,
                                                                  double *__restrict__ stats, double *__restrict__ bw_out, double *__restrict__ u2u_out,
                                                                  int32_t *__restrict__ valid)
{
    const StepCounts c = step_counts(counts, cap1, cap2);
    double bw = 0.0, u2u = 0.0;
    if (c.m >= 1) attr_stats_body(X, ld, d, rows, c.m, c.n1, partial, blocks, stats, bw, u2u);      // (uniform: every thread or none)
    if (threadIdx.x == 0) {
        const bool both = c.n1 >= 1 && c.m - c.n1 >= 1;
        if (c.m < 2) bw = 0.0;
        if (fix_sigma > 0.0) bw = fix_sigma;
        const bool ok = both && (!mmd || (bw > 0.0 && bw <= 1.79769313486231570e308));
        if (!ok) u2u = 0.0;
        stats[0] = bw;
        stats[1] = u2u;
        if (bw_out) *bw_out = bw;
        if (u2u_out) *u2u_out = u2u;
        *valid = ok ? 1 : 0;
    }
}

template <int DQ>
__global__ __launch_bounds__(kBlock) void mmd_dev_kernel(const float *__restrict__ X, int64_t ld, int d, const int32_t *__restrict__ rows,
                                                         const int32_t *__restrict__ counts, int64_t cap1, int64_t cap2,
                                                         const int32_t *__restrict__ valid, double kernel_mul, int kn, const double *__restrict__ bandwidth,
                                                         int span, double *__restrict__ part_sums, double *__restrict__ part_grad)
{
    extern __shared__ float mmd_lds[];
    if (ldg(valid) == 0) return;                           // (the fold and the combine read no partial then)
    const StepCounts c = step_counts(counts, cap1, cap2);
    if ((int64_t)blockIdx.x * kMmdTile >= c.m) {           // a row tile past m: exact zeros
        if (threadIdx.x < 4) part_sums[((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * 4 + threadIdx.x] = 0.0;
        return;
    }
    const double dn1 = (double)c.n1, dn2 = (double)(c.m - c.n1);
    mmd_tile_body<DQ, true>(mmd_lds, X, ld, d, rows, (int)c.m, (int)c.n1, kernel_mul, kn, bandwidth, (float)(2.0 / (dn1 * dn1)), (float)(2.0 / (dn2 * dn2)),
                            (float)(-2.0 / (dn1 * dn2)), span, (cap1 + cap2) * d, part_sums, part_grad);
}

// One workgroup: the four sums, the loss into the accumulator (valid) or the skip counted (not).
__global__ __launch_bounds__(kBlock) void mmd_sums_dev_kernel(const double *__restrict__ part_sums, int64_t n_part, const int32_t *__restrict__ counts,
                                                              int64_t cap1, int64_t cap2, const int32_t *__restrict__ valid, double *__restrict__ sums,
                                                              double *__restrict__ acc, int32_t *__restrict__ skipped)
{
    __shared__ double red[kBlock][4];
    const bool ok = ldg(valid) != 0;
    const double v = ok ? mmd_sums_fold(red, part_sums, n_part) : 0.0;
    if (threadIdx.x < 4) sums[threadIdx.x] = v;
    if (threadIdx.x == 0) {
        if (ok && acc) {
            const StepCounts c = step_counts(counts, cap1, cap2);
            const double n1 = (double)c.n1, n2 = (double)(c.m - c.n1);
            *acc += red[0][0] / (n1 * n1) + red[0][1] / (n2 * n2) - red[0][2] / (n1 * n2) - red[0][3] / (n1 * n2);
        }
        if (!ok && skipped) *skipped += 1;
    }
}

__global__ __launch_bounds__(kBlock) void mmd_grad_combine_dev_kernel(const double *__restrict__ part_grad, int splits, int64_t cap, int d,
                                                                      const int32_t *__restrict__ counts, int64_t cap1, int64_t cap2,
                                                                      const int32_t *__restrict__ valid, float *__restrict__ grad)
{
    const int64_t live = ldg(valid) ? step_counts(counts, cap1, cap2).m * d : 0;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < cap * d; e += (int64_t)gridDim.x * kBlock)
        grad[e] = e < live ? mmd_grad_entry(part_grad, splits, cap * d, e) : 0.f;
}

__global__ __launch_bounds__(kBlock) void u2u_grad_dev_kernel(const float *__restrict__ X, int64_t ld, int d, const int32_t *__restrict__ rows, int64_t cap,
                                                              const int32_t *__restrict__ counts, int64_t cap1, int64_t cap2,
                                                              const int32_t *__restrict__ valid, const double *__restrict__ stats, float *__restrict__ grad,
                                                              double *__restrict__ acc, int32_t *__restrict__ skipped)
{
    const StepCounts c = step_counts(counts, cap1, cap2);
    const bool ok = ldg(valid) != 0;
    const int64_t live = ok ? c.m * d : 0;
    const double dn1 = (double)c.n1, dn2 = (double)(c.m - c.n1);
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < cap * d; e += (int64_t)gridDim.x * kBlock)
        grad[e] = e < live ? u2u_grad_entry(X, ld, rows, e / d, (int)(e % d), c.n1, dn1, dn2, stats) : 0.f;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (ok && acc) *acc += stats[1];
        if (!ok && skipped) *skipped += 1;
    }
}

__global__ __launch_bounds__(kBlock) void attr_add_grad_kernel(float *__restrict__ G, int64_t ldg_, int64_t n_rows, int d, const int32_t *__restrict__ rows,
                                                               const int32_t *__restrict__ counts, int64_t cap, const int32_t *__restrict__ valid,
                                                               const float *__restrict__ grad, float eta)
{
    if (ldg(valid) == 0) return;
    const int64_t m = min(cap, max((int64_t)0, (int64_t)ldg(counts)) + max((int64_t)0, (int64_t)ldg(counts + 1)));
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < m * d; e += (int64_t)gridDim.x * kBlock) {
        const int64_t i = e / d;
        const int f = (int)(e % d);
        const int64_t r = ldg(rows + i);
        if (r < 0 || r >= n_rows) continue;
        float *g = G + r * ldg_ + f;
        *g = __fadd_rn(*g, __fmul_rn(eta, ldg(grad + e)));
    }
}

static int check_step_rows(const float *X, int64_t ld, int d, const int32_t *rows, const int32_t *counts, int64_t cap1, int64_t cap2)
{
    URE_ARG(X && rows && counts);
    URE_ARG(cap1 >= 1 && cap2 >= 1 && cap1 <= INT32_MAX && cap2 <= INT32_MAX);
    URE_ARG(mmd_shape_ok(cap1 + cap2, d));
    URE_ARG(ld >= d);
    return 0;
}

static int launch_stats_dev(const float *X, int64_t ld, int d, const int32_t *rows, const int32_t *counts, int64_t cap1, int64_t cap2, int mmd,
                            double fix_sigma, char *scratch, const MmdPlan &p, double *bw_out, double *u2u_out, int32_t *valid, hipStream_t st)
{
    int slots = 1;
    while (slots < d) slots <<= 1;
    double *stats = reinterpret_cast<double *>(scratch), *partial = reinterpret_cast<double *>(scratch + p.off_partial);
    attr_colsum_dev_kernel<<<p.colsum_blocks, kBlock, 0, st>>>(X, ld, d, slots, rows, counts, cap1, cap2, partial);
    URE_HIP(hipGetLastError());
    attr_stats_dev_kernel<<<1, kMmdMaxD, 0, st>>>(X, ld, d, rows, counts, cap1, cap2, partial, p.colsum_blocks, mmd, fix_sigma, stats, bw_out, u2u_out, valid);
    URE_HIP(hipGetLastError());
    return 0;
}

template <int DQ>
static int launch_mmd_dev(const float *X, int64_t ld, int d, const int32_t *rows, const int32_t *counts, int64_t cap1, int64_t cap2, const int32_t *valid,
                          double kernel_mul, int kn, const double *bandwidth, const MmdPlan &p, double *part_sums, double *part_grad, hipStream_t st)
{
    const size_t lds = mmd_lds_bytes(16 * DQ, true);
    auto kern = mmd_dev_kernel<DQ>;
    URE_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)p.row_tiles, (unsigned)p.splits), dim3(kBlock), lds, st, X, ld, d, rows, counts, cap1, cap2, valid, kernel_mul, kn,
                       bandwidth, (int)p.span, part_sums, part_grad);
    URE_HIP(hipGetLastError());
    return 0;
}

static bool finite_or_unset(double v) { return v == v && v <= 1.79769313486231570e308 && v >= -1.79769313486231570e308; }

}  // namespace ure

using namespace ure;

extern "C" {

int ure_attr_step_masks(const int64_t *off, const int32_t *tag, const int8_t *group, int64_t n_user, int64_t nnz, int32_t steps, uint32_t *masks,
                        void *stream)
{
    URE_ARG(off && tag && group && masks);
    URE_ARG(n_user >= 1 && n_user <= INT32_MAX && nnz >= 1 && nnz <= INT32_MAX && steps >= 1);
    const int words = (steps + 31) / 32;
    const unsigned blocks = (unsigned)std::min<int64_t>((n_user + kWavesPerBlock - 1) / kWavesPerBlock, 65536);
    attr_masks_kernel<<<blocks, kBlock, 0, static_cast<hipStream_t>(stream)>>>(off, tag, group, n_user, nnz, steps, words, masks);
    URE_HIP(hipGetLastError());
    return 0;
}

int64_t ure_attr_select_scratch(int64_t n_user)
{
    if (n_user < 1 || n_user > INT32_MAX) return -1;
    return (n_user + kSelChunk - 1) / kSelChunk * 2 * (int64_t)sizeof(int32_t);
}

int ure_attr_select(const uint32_t *masks, const int8_t *group, int64_t n_user, int32_t steps, int32_t step, int64_t cap1, int64_t cap2, int32_t *rows,
                    int32_t *counts, void *scratch, int64_t scratch_bytes, void *stream)
{
    URE_ARG(masks && group && rows && counts);
    URE_ARG(n_user >= 1 && n_user <= INT32_MAX && steps >= 1 && step >= 0 && step < steps);
    URE_ARG(cap1 >= 1 && cap2 >= 1 && cap1 + cap2 <= INT32_MAX);
    URE_ARG(scratch && scratch_bytes >= ure_attr_select_scratch(n_user));
    const int words = (steps + 31) / 32;
    const unsigned blocks = (unsigned)((n_user + kSelChunk - 1) / kSelChunk);
    hipStream_t st = static_cast<hipStream_t>(stream);
    int32_t *block_counts = static_cast<int32_t *>(scratch);
    attr_sel_count_kernel<<<blocks, kBlock, 0, st>>>(masks, group, n_user, words, step, block_counts);
    URE_HIP(hipGetLastError());
    attr_sel_scatter_kernel<<<blocks, kBlock, 0, st>>>(masks, group, n_user, words, step, block_counts, cap1, cap2, rows, counts);
    URE_HIP(hipGetLastError());
    return 0;
}

int64_t ure_attr_scratch(int64_t cap, int32_t d)
{
    if (!mmd_shape_ok(cap, d)) return -1;
    return mmd_plan(cap, d).bytes;
}

int ure_attr_bandwidth(const float *X, int64_t ld, int32_t d, const int32_t *rows, const int32_t *counts, int64_t cap1, int64_t cap2, double fix_sigma,
                       double *bandwidth, int32_t *valid, void *scratch, int64_t scratch_bytes, void *stream)
{
    if (int rc = check_step_rows(X, ld, d, rows, counts, cap1, cap2)) return rc;
    URE_ARG(bandwidth && valid && finite_or_unset(fix_sigma));
    const MmdPlan p = mmd_plan(cap1 + cap2, d);
    URE_ARG(scratch && scratch_bytes >= p.bytes);
    return launch_stats_dev(X, ld, d, rows, counts, cap1, cap2, 1, fix_sigma, static_cast<char *>(scratch), p, bandwidth, nullptr, valid,
                            static_cast<hipStream_t>(stream));
}

int ure_attr_mmd_loss_grad(const float *X, int64_t ld, int32_t d, const int32_t *rows, const int32_t *counts, int64_t cap1, int64_t cap2,
                           double kernel_mul, int32_t kernel_num, double fix_sigma, double *bandwidth, double *sums, float *grad, int32_t *valid,
                           double *acc, int32_t *skipped, void *scratch, int64_t scratch_bytes, void *stream)
{
    if (int rc = check_step_rows(X, ld, d, rows, counts, cap1, cap2)) return rc;
    URE_ARG(kernel_mul > 0.0 && kernel_mul <= 1.79769313486231570e308);
    URE_ARG(kernel_num >= 1 && kernel_num <= kMmdMaxKernels);
    URE_ARG(sums && grad && valid && finite_or_unset(fix_sigma));
    const int64_t cap = cap1 + cap2;
    const MmdPlan p = mmd_plan(cap, d);
    URE_ARG(scratch && scratch_bytes >= p.bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    char *base = static_cast<char *>(scratch);
    if (int rc = launch_stats_dev(X, ld, d, rows, counts, cap1, cap2, 1, fix_sigma, base, p, bandwidth, nullptr, valid, st)) return rc;
    const double *bw = reinterpret_cast<const double *>(base);                 // stats[0]
    double *part_sums = reinterpret_cast<double *>(base + p.off_sums), *part_grad = reinterpret_cast<double *>(base + p.off_grad);
    int rc;
#define URE_MMD(DQ) rc = launch_mmd_dev<DQ>(X, ld, d, rows, counts, cap1, cap2, valid, kernel_mul, kernel_num, bw, p, part_sums, part_grad, st)
    if (d <= 16) URE_MMD(1);
    else if (d <= 32) URE_MMD(2);
    else if (d <= 64) URE_MMD(4);
    else URE_MMD(8);
#undef URE_MMD
    if (rc) return rc;
    mmd_sums_dev_kernel<<<1, kBlock, 0, st>>>(part_sums, p.row_tiles * p.splits, counts, cap1, cap2, valid, sums, acc, skipped);
    URE_HIP(hipGetLastError());
    const unsigned blocks = (unsigned)std::min<int64_t>((cap * d + kBlock - 1) / kBlock, 4096);
    mmd_grad_combine_dev_kernel<<<blocks, kBlock, 0, st>>>(part_grad, p.splits, cap, d, counts, cap1, cap2, valid, grad);
    URE_HIP(hipGetLastError());
    return 0;
}

int ure_attr_u2u_loss_grad(const float *X, int64_t ld, int32_t d, const int32_t *rows, const int32_t *counts, int64_t cap1, int64_t cap2, double *value,
                           float *grad, int32_t *valid, double *acc, int32_t *skipped, void *scratch, int64_t scratch_bytes, void *stream)
{
    if (int rc = check_step_rows(X, ld, d, rows, counts, cap1, cap2)) return rc;
    URE_ARG(value && grad && valid);
    const int64_t cap = cap1 + cap2;
    const MmdPlan p = mmd_plan(cap, d);
    URE_ARG(scratch && scratch_bytes >= p.bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = launch_stats_dev(X, ld, d, rows, counts, cap1, cap2, 0, 0.0, static_cast<char *>(scratch), p, nullptr, value, valid, st)) return rc;
    const unsigned blocks = (unsigned)std::min<int64_t>((cap * d + kBlock - 1) / kBlock, 4096);
    u2u_grad_dev_kernel<<<blocks, kBlock, 0, st>>>(X, ld, d, rows, cap, counts, cap1, cap2, valid, static_cast<const double *>(scratch), grad, acc, skipped);
    URE_HIP(hipGetLastError());
    return 0;
}

int ure_attr_add_grad(float *G, int64_t ldg, int64_t n_rows, int32_t d, const int32_t *rows, const int32_t *counts, int64_t cap, const int32_t *valid,
                      const float *grad, float eta, void *stream)
{
    URE_ARG(G && rows && counts && valid && grad);
    URE_ARG(d >= 1 && d <= kMmdMaxD && ldg >= d && n_rows >= 1 && n_rows <= INT32_MAX && cap >= 1 && cap <= INT32_MAX);
    URE_ARG(eta == eta && eta <= 3.402823466e38f && eta >= -3.402823466e38f);
    const unsigned blocks = (unsigned)std::min<int64_t>((cap * d + kBlock - 1) / kBlock, 4096);
    attr_add_grad_kernel<<<blocks, kBlock, 0, static_cast<hipStream_t>(stream)>>>(G, ldg, n_rows, d, rows, counts, cap, valid, grad, eta);
    URE_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"

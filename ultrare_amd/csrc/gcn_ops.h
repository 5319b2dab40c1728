// gcn_ops.h -- what the kernels over a shard's graph share (gcn.hip, bpr.hip, nmf.hip, influence.hip): the float4 operations of a
// lane's four columns, every one a rounded float32 operation of its own (__fmul_rn / __fadd_rn: never contracted), the fold of
// 256 float64 lane sums, and the host-side checks and grid sizes of their entries.  The masked row walk is row_walk.h's, the
// lane-group coordinates and the dot are csr_lanes.h's and score_dot.h's.
#pragma once
#include "row_walk.h"
#include "score_dot.h"

namespace ure {

__device__ __forceinline__ float4 f4_zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
// acc + s * v, the product and the sum rounded separately
__device__ __forceinline__ float4 f4_mul_add(float4 acc, float s, float4 v)
{
    acc.x = __fadd_rn(acc.x, __fmul_rn(s, v.x));
    acc.y = __fadd_rn(acc.y, __fmul_rn(s, v.y));
    acc.z = __fadd_rn(acc.z, __fmul_rn(s, v.z));
    acc.w = __fadd_rn(acc.w, __fmul_rn(s, v.w));
    return acc;
}
__device__ __forceinline__ float4 f4_scale(float s, float4 v)
{
    return make_float4(__fmul_rn(s, v.x), __fmul_rn(s, v.y), __fmul_rn(s, v.z), __fmul_rn(s, v.w));
}
__device__ __forceinline__ float4 f4_add(float4 a, float4 b)
{
    return make_float4(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y), __fadd_rn(a.z, b.z), __fadd_rn(a.w, b.w));
}
__device__ __forceinline__ float4 f4_sub(float4 a, float4 b)
{
    return make_float4(__fsub_rn(a.x, b.x), __fsub_rn(a.y, b.y), __fsub_rn(a.z, b.z), __fsub_rn(a.w, b.w));
}

// The sums of the 256 threads of a workgroup -> one value, in epoch_sse_kernel's order (job_io.hip): thread t += thread t + w for
// w = 128, 64 .. 1.  Every thread calls it with the workgroup's part[256] of LDS and receives the sum.
__device__ __forceinline__ double fold_256(double acc, double *part)
{
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] = __dadd_rn(part[threadIdx.x], part[threadIdx.x + w]);
        __syncthreads();
    }
    return part[0];
}

inline unsigned stream_blocks(int64_t items)
{
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + kBlock - 1) / kBlock, 4096));
}

// [a, a + na) and [b, b + nb) bytes share no byte
inline bool apart(const void *a, int64_t na, const void *b, int64_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x + (uintptr_t)na <= y || y + (uintptr_t)nb <= x;
}

inline bool width_ok(int d) { return d >= 4 && d <= 256 && pow2(d); }

}  // namespace ure

#define URE_GCN_SIZES(n_dst, n_src, d)               \
    do {                                             \
        URE_ARG(n_dst >= 1 && n_dst <= INT32_MAX);   \
        URE_ARG(n_src >= 1 && n_src <= INT32_MAX);   \
        URE_ARG(width_ok(d));                        \
    } while (0)

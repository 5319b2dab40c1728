// score_dot.h -- the scaffold of the ensemble-scoring kernels (mf_eval.hip, mf_combine.hip): the LPR = d / 4 lanes of a group hold
// one float4 each of a user row and an item row; the lane's four products are one fmaf chain and the lanes are added by the
// group's xor butterfly (group_sum), so every lane of the group ends with the score.  Here, once: the lane-group coordinates
// (PairLanes), the dot (pair_dot), the combiner's link (link_mean, which rec_score.h's weighted scorer calls too), the
// squared-error partials ure_eval_reduce and the host read (sq_partials), and on the host
// the model list, the grid size and the width dispatch (group_width.h).
// NOT here: the gather of four models' rows, which score_kernel, combine_stats_kernel and score_weighted_kernel each spell out.
// As one inlined function it changed their loops' code (the row offset scaled to bytes ahead of the loop, the blocks laid out
// in another order) and measured 1-2 % slower in score_kernel and combine_stats_kernel.
#pragma once
#include <algorithm>
#include <cmath>

#include "group_width.h"
#include "ure_internal.h"

namespace ure {

struct TableList {
    const float *U[URE_MAX_MODELS_PER_CALL];
    const float *V[URE_MAX_MODELS_PER_CALL];
};

// The model list of one call, checked: 0, or the failure of an entry that lacks a table.
inline int fill_tables(TableList &T, const float *const *U_tables, const float *const *V_tables, int n_models)
{
    for (int m = 0; m < n_models; ++m) {
        URE_ARG(U_tables[m] && V_tables[m]);
        T.U[m] = U_tables[m];
        T.V[m] = V_tables[m];
    }
    return 0;
}

// Workgroups for n pairs, a pair per lane group and G groups per wave, at least one and at most `cap`.
inline unsigned pair_blocks(int64_t n, int G, int64_t cap)
{
    const int64_t waves = (n + G - 1) / G;
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((waves + kWavesPerBlock - 1) / kWavesPerBlock, cap));
}

// Where a thread stands in a kernel that gives every pair a group of LPR lanes: lane `sub` of group `grp` of its wave, which is
// wave `wave_id` of the grid's `n_waves`.
template <int LPR>
struct PairLanes {
    static constexpr int D = LPR * 4;            // row width
    static constexpr int G = kWave / LPR;        // pairs of a wave
    const int lane = threadIdx.x & 63;
    const int sub = lane & (LPR - 1), grp = lane / LPR;
    const int64_t wave_id = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * kBlock) >> 6;
};

template <int LPR>
__device__ __forceinline__ float pair_dot(const float4 a, const float4 b)
{
    float p = a.x * b.x;
    p = fmaf(a.y, b.y, p);
    p = fmaf(a.z, b.z, p);
    p = fmaf(a.w, b.w, p);
    return group_sum<LPR>(p);
}

// The mean of the combiner's generalised linear model (mf_combine.hip) at z: link 0 the identity, link 1 the logistic function.
// Here, once, for ure_combine_stats, ure_score_weighted and the weighted scorer of rec_score.h: their floats agree bit for bit
// because they are this function's.
__device__ __forceinline__ double link_mean(int link, double z) { return link == 0 ? z : 1.0 / (1.0 + exp(-z)); }

// The squared errors of a launch, sq per thread, as sse[URE_SCORE_PARTIALS]: one partial per workgroup -- its waves' butterfly
// sums added in double, in order -- and zeros behind the last workgroup's.  No atomics: thousands of waves adding to ONE address
// serialise at ~12 ns each (measured: 69 us for score_kernel); the partials are summed in a fixed order by ure_eval_reduce or by
// the host.  Workgroup-wide: every thread of the block calls it.
__device__ __forceinline__ void sq_partials(float sq, double *__restrict__ sse)
{
    __shared__ float part[kWavesPerBlock];
    sq = wave_sum(sq);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sq;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < kWavesPerBlock; ++k) t += (double)part[k];
        sse[blockIdx.x] = t;
    }
    for (int t = gridDim.x + threadIdx.x; blockIdx.x == 0 && t < URE_SCORE_PARTIALS; t += kBlock) sse[t] = 0.0;
}

}  // namespace ure

// score_dot.h -- one model's score of one (user, item) pair as ure_score forms it, shared by mf_eval.hip (score_kernel) and
// mf_combine.hip: the LPR lanes of a group hold one float4 each of the two rows; the lane's four products are one fmaf chain
// and the lanes are added by the group's xor butterfly (group_sum).  Every lane of the group ends with the score.
#pragma once
#include "ure_internal.h"

namespace ure {

struct TableList {
    const float *U[URE_MAX_MODELS_PER_CALL];
    const float *V[URE_MAX_MODELS_PER_CALL];
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

}  // namespace ure

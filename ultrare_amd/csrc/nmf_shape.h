// nmf_shape.h -- the shape code of the NeuMF kernels, shared by nmf.hip (training and pair scoring) and nmf_rank.hip (catalogue
// sweeps): where everything of a (k, layers) lies, the argument check of a stack, and the staging of a stack's weights in LDS.
#pragma once
#include "gcn_ops.h"

namespace ure {

constexpr int kFc = URE_NMF_MAX_FC;
constexpr int kMaxW = 128;                       // the widest layer

// Where everything of a (k, layers) lies: in the dense vector, in the LDS image of the weights and in a slot's rows.
struct NmfShape {
    int k, e, m, wd;                             // wd = k + e: a table row
    int L[kFc + 1];
    int w_at[kFc], b_at[kFc], h_at, c_at, n_real, n_dense;       // the dense vector (n_dense: padded to a multiple of 4)
    int lw_at[kFc], lb_at[kFc], lh_at, lc_at, lds_w;             // the LDS image (floats)
    int a_at[kFc + 1], A;                        // a_j within an act row (behind g)
    int d_at[kFc + 1], Dw;                       // delta_j (j = 1 .. m) within a dlt row
    int lds_bytes;
};

inline bool width_in(int v, int lo) { return v >= lo && v <= kMaxW && pow2(v); }

// false for a (k, layers) outside the header's limits or beyond the LDS budget
inline bool fill_shape(NmfShape &S, int k, const int32_t *layers, int n_layers)
{
    if (!layers || n_layers < 2 || n_layers > kFc + 1 || !width_in(k, 4) || !width_in(layers[0], 8)) return false;
    for (int j = 1; j < n_layers; ++j)
        if (!width_in(layers[j], 4)) return false;
    S.k = k, S.m = n_layers - 1, S.e = layers[0] / 2, S.wd = k + S.e;
    for (int j = 0; j <= kFc; ++j) S.L[j] = j < n_layers ? layers[j] : 0;
    int at = 0, lat = 0, a = k, d = 0;
    for (int j = 0; j < S.m; ++j) {
        S.w_at[j] = at, at += S.L[j + 1] * S.L[j];
        S.b_at[j] = at, at += S.L[j + 1];
        S.lw_at[j] = lat, lat += S.L[j] * (S.L[j + 1] + 1);
        S.lb_at[j] = lat, lat += S.L[j + 1];
    }
    for (int j = S.m; j < kFc; ++j) S.w_at[j] = S.b_at[j] = S.lw_at[j] = S.lb_at[j] = 0;
    S.h_at = at, at += k + S.L[S.m];
    S.c_at = at, at += 1;
    S.n_real = at, S.n_dense = (at + 3) / 4 * 4;
    S.lh_at = lat, lat += k + S.L[S.m];
    S.lc_at = lat, lat += 1;
    S.lds_w = lat;
    for (int j = 0; j <= kFc; ++j) {
        S.a_at[j] = a, a += S.L[j];
        S.d_at[j] = j >= 1 ? d : 0;
        if (j >= 1) d += S.L[j];
    }
    S.A = a, S.Dw = d;
    S.lds_bytes = 4 * (S.lds_w + kWavesPerBlock * (S.A + 2 * kMaxW));
    return S.lds_bytes <= URE_NMF_LDS_BYTES;
}

// The lanes of ONE wave have written LDS that other lanes of it read next.
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// dense -> the LDS image; workgroup-wide, ends with a barrier
__device__ __forceinline__ void stage_weights(const NmfShape &S, const float *__restrict__ dense, float *__restrict__ wl)
{
    for (int j = 0; j < S.m; ++j) {
        const int Lin = S.L[j], Lout = S.L[j + 1];
        for (int t = threadIdx.x; t < Lin * Lout; t += kBlock) wl[S.lw_at[j] + (t % Lin) * (Lout + 1) + t / Lin] = ldg(dense + S.w_at[j] + t);
        for (int t = threadIdx.x; t < Lout; t += kBlock) wl[S.lb_at[j] + t] = ldg(dense + S.b_at[j] + t);
    }
    for (int t = threadIdx.x; t < S.k + S.L[S.m] + 1; t += kBlock) wl[S.lh_at + t] = ldg(dense + S.h_at + t);       // (h, then c)
    __syncthreads();
}

}  // namespace ure

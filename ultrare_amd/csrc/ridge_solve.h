// ridge_solve.h -- what the batched ridge kernels share (mf_ridge.hip: ure_ridge_rows; wmf.hip: ure_wridge_rows, ure_gram): the
// shape of a workgroup's LDS and register blocks, the staging of one tile of table rows as doubles, the thread-to-block map, and
// the factor / solve / store stages, written once.  A system's bytes are a function of the packed triangle and the right-hand
// side these stages are handed, whichever kernel accumulated them.
#pragma once
#include "ure_internal.h"

#include <cfloat>
#include <cmath>

namespace ure {

constexpr int kRrMaxD = 128;             // a padded 256 would need a 257 KiB triangle: refused

template <int D>
struct RrShape {
    static constexpr int TB = D >= 16 ? D / 16 : 1;                 // edge of a thread's register block of G
    static constexpr int NB = D / TB;                               // blocks per side: 16, or D below 16
    static constexpr int NTRI = NB * (NB + 1) / 2;                  // threads that own a block (136 of 256 at D >= 16)
    static constexpr int T = D <= 32 ? 64 : 2048 / D;               // rows per tile: at most 16 KiB of doubles
    static constexpr int TRI = D * (D + 1) / 2;
    static constexpr int MAIN = T * D > TRI ? T * D : TRI;          // the tile, later the packed triangle
    static constexpr int DOUBLES = MAIN + T + 3 * D;                // + ratings | y, x | b | sqrt of the pivots
};

__device__ __forceinline__ int tri_row(int a, int k) { return a * k - a * (a - 1) / 2; }     // index of (a, a); (a, b) is + b - a

// The block thread `tid` owns: row-major over the upper triangle of NB x NB blocks (is_g), then the NB blocks of b (is_b).
template <int D>
__device__ __forceinline__ void rr_owner(int tid, bool &is_g, bool &is_b, int &bi, int &bj)
{
    constexpr int NB = RrShape<D>::NB, NTRI = RrShape<D>::NTRI;
    is_g = tid < NTRI;
    is_b = tid >= NTRI && tid < NTRI + NB;
    bi = bj = 0;
    if (is_g) {
        int r = tid;
        while (r >= NB - bi) { r -= NB - bi; ++bi; }
        bj = bi + r;
    } else if (is_b) {
        bi = bj = tid - NTRI;
    }
}

// Four columns of table row i (c .. c + 3) into the tile as doubles, columns >= k zeroed.
template <int D>
__device__ __forceinline__ void rr_stage4(const float *__restrict__ F, int64_t i, int c, int k, double *dst)
{
    const float4 v = ldg_f4(F + (size_t)i * D + c);
    dst[0] = c + 0 < k ? (double)v.x : 0.0;
    dst[1] = c + 1 < k ? (double)v.y : 0.0;
    dst[2] = c + 2 < k ? (double)v.z : 0.0;
    dst[3] = c + 3 < k ? (double)v.w : 0.0;
}

// factor, solve and store of one system by the whole workgroup.  G: the packed upper triangle (k x k) in LDS, the ridge on its
// diagonal already; bs: the right-hand side; ys, dg: k doubles each.  Every thread has passed a barrier since G and bs were
// written.  failed: the segment is spoilt already (uniform over the workgroup).
//   factor  G = R^T R, R over G's upper triangle (the diagonal of R in dg; G's own diagonal keeps the pivots)
//   solve   R^T y = b forwards, R x = y backwards; thread c carries entry c
//   store   x rounded to float32 once; columns k .. D - 1 zero; a failed system: NaN in its k columns and the status words
template <int D>
__device__ __forceinline__ void rr_factor_solve_store(double *G, const double *bs, double *ys, double *dg, int k, bool failed,
                                                      float *__restrict__ xrow, int32_t *__restrict__ status, int64_t s)
{
    const int tid = threadIdx.x;
    for (int j = 0; j < k && !failed; ++j) {
        const int rj = tri_row(j, k);
        const double p = G[rj];                            // every thread reads the same word: the branch is uniform
        if (!(p > 0.0 && p <= DBL_MAX)) {
            failed = true;
            break;
        }
        const double sq = sqrt(p);
        if (tid == 0) dg[j] = sq;
        for (int b = j + 1 + tid; b < k; b += kBlock) G[rj + b - j] = G[rj + b - j] / sq;
        __syncthreads();
        for (int a = j + 1 + (tid >> 4); a < k; a += kBlock / 16) {
            const double ra = G[rj + a - j];
            double *ga = G + tri_row(a, k) - a;
            for (int b = a + (tid & 15); b < k; b += 16) ga[b] = fma(-ra, G[rj + b - j], ga[b]);
        }
        __syncthreads();
    }

    double v = 0.0;
    if (!failed) {
        if (tid < k) v = bs[tid];
        for (int j = 0; j < k; ++j) {
            if (tid == j) ys[j] = v / dg[j];
            __syncthreads();
            if (tid > j && tid < k) v = fma(-G[tri_row(j, k) + tid - j], ys[j], v);
        }
        if (tid < k) v = ys[tid];                          // (its own store)
        for (int j = k - 1; j >= 0; --j) {
            if (tid == j) ys[j] = v / dg[j];
            __syncthreads();
            if (tid < j) v = fma(-G[tri_row(tid, k) + j - tid], ys[j], v);
        }
        v = tid < k ? ys[tid] : 0.0;
    }
    if (__syncthreads_or(tid < k && !(fabs(v) <= DBL_MAX))) failed = true;
    for (int c = tid; c < D; c += kBlock) xrow[c] = c >= k ? 0.f : failed ? __builtin_nanf("") : (float)ys[c];
    if (failed && tid == 0) {
        atomicAdd(status, 1);
        atomicMin(reinterpret_cast<unsigned *>(status) + 1, (unsigned)s);
    }
}

}  // namespace ure

// mmd_tile.h -- the tile arithmetic of the attribute losses, shared by mmd.hip (counts on the host: the post-training fine-tune,
// DESIGN 4.18) and attr_train.hip (counts in device memory: the per-batch term of training).  What a kernel of either
// file computes for given (m, n1, coefficients, span, strides) is written ONCE here; the kernels differ in where those values come
// from.  The arithmetic itself is described at the head of mmd.hip.
#pragma once
#include "ure_internal.h"

#include <cmath>

namespace ure {

constexpr int kMmdTile = 64;                 // rows and columns of a tile
constexpr int kMmdLd = kMmdTile + 1;         // LDS stride of staged features (feature-major) and of the tile of c w
constexpr int kMmdMaxD = 128;
constexpr int kMmdMaxKernels = 16;
constexpr int kMmdMaxSplits = 16;            // scratch: at most 16 m d float64 gradient partials
constexpr int kMmdTargetBlocks = 1024;       // workgroups the column split aims for
constexpr int kColsumMaxBlocks = 128;
constexpr int kColsumRows = 256;             // selected rows per workgroup of attr_colsum_kernel, at least
// stats (float64, in scratch): bandwidth, u2u value, then per column the shift s, sum_S (x - s), sum_T (x - s)
constexpr int kStatsShift = 2, kStatsVS = kStatsShift + kMmdMaxD, kStatsVT = kStatsVS + kMmdMaxD, kStatsLen = kStatsVT + kMmdMaxD;
constexpr int kColsumPartial = 4 * kMmdMaxD; // per workgroup: vS, vT, qS, qT per column

struct MmdPlan {
    int splits;          // column splits (blockIdx.y)
    int64_t span;        // columns per split, a multiple of kMmdTile
    int64_t row_tiles;
    int colsum_blocks;
    int64_t off_partial, off_sums, off_grad, bytes;   // scratch layout (bytes)
};

// The layout is a function of (m, d) alone.
inline MmdPlan mmd_plan(int64_t m, int d)
{
    MmdPlan p;
    p.row_tiles = (m + kMmdTile - 1) / kMmdTile;
    int64_t s = (kMmdTargetBlocks + p.row_tiles - 1) / p.row_tiles;
    s = std::max<int64_t>(1, std::min<int64_t>({s, p.row_tiles, (int64_t)kMmdMaxSplits}));
    const int64_t per = (p.row_tiles + s - 1) / s;
    p.splits = (int)((p.row_tiles + per - 1) / per);
    p.span = per * kMmdTile;
    p.colsum_blocks = (int)std::max<int64_t>(1, std::min<int64_t>(kColsumMaxBlocks, m / kColsumRows));
    p.off_partial = (int64_t)kStatsLen * 8;
    p.off_sums = p.off_partial + (int64_t)p.colsum_blocks * kColsumPartial * 8;
    p.off_grad = p.off_sums + p.row_tiles * p.splits * 4 * 8;
    p.bytes = p.off_grad + (int64_t)p.splits * m * d * 8;
    return p;
}

// (m + a tile stays inside int32: the kernels index the selected rows with int)
inline bool mmd_shape_ok(int64_t m, int d) { return m >= 2 && m <= INT32_MAX - kMmdTile && d >= 1 && d <= kMmdMaxD; }

inline size_t mmd_lds_bytes(int F, bool with_tile) { return ((size_t)2 * F * kMmdLd + (with_tile ? kMmdTile * kMmdLd : 0) + 2 * kMmdMaxKernels) * sizeof(float); }

// kMmdTile selected rows base .. base + 63 (those below `limit`; the others and the features d .. F - 1 as zeros) into
// dst, feature-major.  Every thread of the workgroup calls it.
__device__ __forceinline__ void mmd_stage(float *dst, const float *__restrict__ X, int64_t ld, int d, int F, const int32_t *__restrict__ rows,
                                          int64_t base, int64_t limit)
{
    for (int e = threadIdx.x; e < kMmdTile * F; e += kBlock) {
        const int r = e / F, f = e % F;
        float v = 0.f;
        if (base + r < limit && f < d) v = ldg(X + (int64_t)ldg(rows + base + r) * ld + f);
        dst[f * kMmdLd + r] = v;
    }
}

// -1 / bw_q and -2 / bw_q as float32 (NaN for a bandwidth that is not positive and finite) into ninv[0 .. 2 kn).
__device__ __forceinline__ void mmd_bandwidths(float *ninv, const double *__restrict__ bandwidth, double kernel_mul, int kn)
{
    const int q = threadIdx.x;
    if (q < kn) {
        const double bw = ldg(bandwidth);
        double den = 1.0, bq;
        for (int i = 0; i < kn / 2; ++i) den *= kernel_mul;
        bq = bw / den;
        for (int i = 0; i < q; ++i) bq *= kernel_mul;
        const float v = (bw > 0.0 && bw <= 1.79769313486231570e308) ? (float)(-1.0 / bq) : __builtin_nanf("");
        ninv[q] = v;
        ninv[kn + q] = __fadd_rn(v, v);
    }
}

// Thread (ty, tx)'s 4 x 4 entries (rows ty + 16 i, columns tx + 16 j) of K and w from the staged features.
__device__ __forceinline__ void mmd_pair(const float *xr, const float *xc, int d, const float *ninv, int kn, int ty, int tx, float (&K)[4][4],
                                         float (&W)[4][4])
{
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int kk = 0; kk < d; ++kk) {
        float a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            a[i] = xr[kk * kMmdLd + ty + 16 * i];
            b[i] = xc[kk * kMmdLd + tx + 16 * i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float s = __fsub_rn(a[i], b[j]);
                acc[i][j] = fmaf(s, s, acc[i][j]);
            }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) K[i][j] = W[i][j] = 0.f;
    for (int q = 0; q < kn; ++q) {
        const float ni = ninv[q], ni2 = ninv[kn + q];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float e = expf(__fmul_rn(acc[i][j], ni));
                K[i][j] = __fadd_rn(K[i][j], e);
                W[i][j] = fmaf(ni2, e, W[i][j]);
                __builtin_amdgcn_sched_barrier(0);          // (expf's range selects, left to float free, pile up in SGPRs and spill)
            }
    }
}

__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

// What workgroup (blockIdx.x, blockIdx.y) of an MMD launch does: the row tile blockIdx.x against the columns of split
// blockIdx.y.  DQ = ceil(d / 16): features per thread of the gradient product.  part_sums [row tile][split][4] (SS, TT, ST, TS),
// part_grad [split][grad_stride] float64, row i of a split at i d.  mmd_lds: 2 F kMmdLd + kMmdTile kMmdLd + 2 kMmdMaxKernels floats.
template <int DQ, bool GRAD>
__device__ __forceinline__ void mmd_tile_body(float *mmd_lds, const float *__restrict__ X, int64_t ld, int d, const int32_t *__restrict__ rows, int m,
                                              int n1, double kernel_mul, int kn, const double *__restrict__ bandwidth, float c_ss, float c_tt,
                                              float c_x, int span, int64_t grad_stride, double *__restrict__ part_sums,
                                              double *__restrict__ part_grad)
{
    constexpr int F = 16 * DQ;
    float *xr = mmd_lds, *xc = xr + F * kMmdLd, *wt = xc + F * kMmdLd, *ninv = wt + kMmdTile * kMmdLd;
    __shared__ double red[kWavesPerBlock][4];
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int row0 = (int)blockIdx.x * kMmdTile;
    const int c_begin = (int)blockIdx.y * span, c_end = (int)min((int64_t)m, (int64_t)c_begin + span);
    mmd_bandwidths(ninv, bandwidth, kernel_mul, kn);
    mmd_stage(xr, X, ld, d, F, rows, row0, m);
    __syncthreads();
    float xi[4][DQ];
    double gacc[4][DQ];
    if (GRAD) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int q = 0; q < DQ; ++q) {
                xi[i][q] = xr[(tx + 16 * q) * kMmdLd + ty + 16 * i];
                gacc[i][q] = 0.0;
            }
    }
    double s_ss = 0.0, s_tt = 0.0, s_st = 0.0, s_ts = 0.0;
    for (int c0 = c_begin; c0 < c_end; c0 += kMmdTile) {
        __syncthreads();                                   // the tile before is read
        mmd_stage(xc, X, ld, d, F, rows, c0, c_end);
        __syncthreads();
        float K[4][4], W[4][4];
        mmd_pair(xr, xc, d, ninv, kn, ty, tx, K, W);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int gi = row0 + ty + 16 * i;
            const bool row_s = gi < n1;
            double a_s = 0.0, a_t = 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int gj = c0 + tx + 16 * j;
                const bool in = gi < m && gj < c_end, col_s = gj < n1;
                if (in) {
                    if (col_s) a_s += (double)K[i][j];
                    else a_t += (double)K[i][j];
                }
                if (GRAD) {
                    const float c = row_s == col_s ? (row_s ? c_ss : c_tt) : c_x;
                    wt[(ty + 16 * i) * kMmdLd + tx + 16 * j] = in ? __fmul_rn(c, W[i][j]) : 0.f;
                }
            }
            if (row_s) {
                s_ss += a_s;
                s_st += a_t;
            } else {
                s_ts += a_s;
                s_tt += a_t;
            }
        }
        if (GRAD) {
            __syncthreads();
            float g[4][DQ];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int q = 0; q < DQ; ++q) g[i][q] = 0.f;
            for (int j = 0; j < kMmdTile; ++j) {
                float w4[4], xj[DQ];
#pragma unroll
                for (int i = 0; i < 4; ++i) w4[i] = wt[(ty + 16 * i) * kMmdLd + j];
#pragma unroll
                for (int q = 0; q < DQ; ++q) xj[q] = xc[(tx + 16 * q) * kMmdLd + j];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int q = 0; q < DQ; ++q) g[i][q] = fmaf(w4[i], __fsub_rn(xi[i][q], xj[q]), g[i][q]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int q = 0; q < DQ; ++q) gacc[i][q] += (double)g[i][q];
        }
    }
    if (GRAD) {
        double *out = part_grad + (int64_t)blockIdx.y * grad_stride;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int gi = row0 + ty + 16 * i;
#pragma unroll
            for (int q = 0; q < DQ; ++q) {
                const int f = tx + 16 * q;
                if (gi < m && f < d) out[(int64_t)gi * d + f] = gacc[i][q];
            }
        }
    }
    // the four sums of the workgroup: an xor butterfly inside each wave, then the waves in order
    s_ss = wave_sum_f64(s_ss);
    s_tt = wave_sum_f64(s_tt);
    s_st = wave_sum_f64(s_st);
    s_ts = wave_sum_f64(s_ts);
    if ((tid & (kWave - 1)) == 0) {
        red[tid / kWave][0] = s_ss;
        red[tid / kWave][1] = s_tt;
        red[tid / kWave][2] = s_st;
        red[tid / kWave][3] = s_ts;
    }
    __syncthreads();
    if (tid < 4) {
        double v = red[0][tid];
        for (int w = 1; w < kWavesPerBlock; ++w) v += red[w][tid];
        part_sums[((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * 4 + tid] = v;
    }
}

// One workgroup of kBlock threads: -> in thread k < 4 the sum of the n_part partial sums [.][k], thread t taking t, t + 256, ...
// and the threads a fixed tree (the value is meaningful in the threads 0 .. 3 only).  red: kBlock x 4 float64 of LDS.
__device__ __forceinline__ double mmd_sums_fold(double (*red)[4], const double *__restrict__ part_sums, int64_t n_part)
{
    const int tid = threadIdx.x;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t p = tid; p < n_part; p += kBlock)
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] += part_sums[p * 4 + k];
#pragma unroll
    for (int k = 0; k < 4; ++k) red[tid][k] = v[k];
    __syncthreads();
    for (int o = kBlock / 2; o > 0; o >>= 1) {
        if (tid < o)
#pragma unroll
            for (int k = 0; k < 4; ++k) red[tid][k] += red[tid + o][k];
        __syncthreads();
    }
    return red[0][tid & 3];
}

// The float32 gradient entry e: the splits' float64 partials (split s at s * stride) added in split order.
__device__ __forceinline__ float mmd_grad_entry(const double *__restrict__ part_grad, int splits, int64_t stride, int64_t e)
{
    double v = part_grad[e];
    for (int s = 1; s < splits; ++s) v += part_grad[(int64_t)s * stride + e];
    return (float)v;
}

// ---- column sums -----------------------------------------------------------------------------------------------------
// Workgroup b takes the selected rows [b per, (b + 1) per), cut into 256 / slots contiguous pieces (slots = the power
// of two >= d); thread (c, f) = (tid / slots, tid % slots) walks piece c in row order for column f.  With t = x - s:
// partial[b][0 .. 3][f] = sum_S t, sum_T t, sum_S t^2, sum_T t^2, the pieces added in order.  m >= 1.
__device__ __forceinline__ void attr_colsum_body(const float *__restrict__ X, int64_t ld, int d, int slots, const int32_t *__restrict__ rows, int64_t m,
                                                 int64_t n1, int64_t per, double *__restrict__ partial)
{
    __shared__ double red[4][kBlock];
    const int tid = threadIdx.x, f = tid % slots, c = tid / slots, pieces = kBlock / slots;
    const int64_t b0 = min(m, (int64_t)blockIdx.x * per), b1 = min(m, b0 + per);
    const int64_t piece = (b1 - b0 + pieces - 1) / pieces;
    const int64_t i0 = min(b1, b0 + c * piece), i1 = min(b1, i0 + piece);
    double v_s = 0.0, v_t = 0.0, q_s = 0.0, q_t = 0.0;
    if (f < d) {
        const double s = (double)ldg(X + (int64_t)ldg(rows) * ld + f);
        for (int64_t i = i0; i < i1; ++i) {
            const double t = (double)ldg(X + (int64_t)ldg(rows + i) * ld + f) - s;
            if (i < n1) {
                v_s += t;
                q_s += t * t;
            } else {
                v_t += t;
                q_t += t * t;
            }
        }
    }
    red[0][tid] = v_s;
    red[1][tid] = v_t;
    red[2][tid] = q_s;
    red[3][tid] = q_t;
    __syncthreads();
    if (tid < slots && tid < d) {
        for (int k = 0; k < 4; ++k) {
            double v = red[k][tid];
            for (int p = 1; p < pieces; ++p) v += red[k][p * slots + tid];
            partial[((int64_t)blockIdx.x * 4 + k) * kMmdMaxD + tid] = v;
        }
    }
}

// One workgroup of kMmdMaxD threads: the workgroups' partials added in order per column, then thread 0 adds the columns
// in order and returns (in thread 0 only) bandwidth = (2 m sum |t_i|^2 - 2 |sum t_i|^2) / (m^2 - m) and
// u2u = n2 sum_S |t|^2 + n1 sum_T |t|^2 - 2 vS . vT; both are also left in stats[0], stats[1].  m >= 1.
__device__ __forceinline__ void attr_stats_body(const float *__restrict__ X, int64_t ld, int d, const int32_t *__restrict__ rows, int64_t m, int64_t n1,
                                                const double *__restrict__ partial, int blocks, double *__restrict__ stats, double &bw_out,
                                                double &u2u_out)
{
    __shared__ double col[4][kMmdMaxD];
    const int f = threadIdx.x;
    if (f < d) {
        for (int k = 0; k < 4; ++k) {
            double v = partial[(int64_t)k * kMmdMaxD + f];
            for (int b = 1; b < blocks; ++b) v += partial[((int64_t)b * 4 + k) * kMmdMaxD + f];
            col[k][f] = v;
        }
        stats[kStatsShift + f] = (double)ldg(X + (int64_t)ldg(rows) * ld + f);
        stats[kStatsVS + f] = col[0][f];
        stats[kStatsVT + f] = col[1][f];
    }
    __syncthreads();
    if (f == 0) {
        double q_s = 0.0, q_t = 0.0, vv = 0.0, dot = 0.0;
        for (int j = 0; j < d; ++j) {
            q_s += col[2][j];
            q_t += col[3][j];
            const double v = col[0][j] + col[1][j];
            vv += v * v;
            dot += col[0][j] * col[1][j];
        }
        const double dm = (double)m, dn1 = (double)n1, dn2 = (double)(m - n1);
        const double bw = (2.0 * dm * (q_s + q_t) - 2.0 * vv) / (dm * dm - dm);
        const double u2u = dn2 * q_s + dn1 * q_t - 2.0 * dot;
        stats[0] = bw;
        stats[1] = u2u;
        bw_out = bw;
        u2u_out = u2u;
    }
}

// The u2u gradient entry (i, f): 2 (n2 (x_if - s_f) - vT_f) for i in S, 2 (n1 (x_if - s_f) - vS_f) for i in T, in float64,
// rounded once.
__device__ __forceinline__ float u2u_grad_entry(const float *__restrict__ X, int64_t ld, const int32_t *__restrict__ rows, int64_t i, int f, int64_t n1,
                                                double dn1, double dn2, const double *__restrict__ stats)
{
    const double t = (double)ldg(X + (int64_t)ldg(rows + i) * ld + f) - stats[kStatsShift + f];
    return (float)(i < n1 ? 2.0 * (dn2 * t - stats[kStatsVT + f]) : 2.0 * (dn1 * t - stats[kStatsVS + f]));
}

}  // namespace ure

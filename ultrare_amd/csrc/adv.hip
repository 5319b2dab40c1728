// adv.hip -- the gradient of the attribute probe's loss with respect to its input rows, for gfx950 (the arithmetic is
// stated in numpy in ultrare_amd/adv_unlearn.py, the entry in include/ultrare_adv.h).  The probe is attack.hip's: one hidden layer
// of H relu units (H = 0: ONE linear unit whose output is the logit), one parameter set per cross-validation fold, and a position
// is served by the fold that held it out.
//   adv_input_grad_kernel  workgroup = up to kAdvRun = 256 consecutive entries of ONE fold's group of the plan (perm / fold_off), so
//                          the fold's packed parameters are staged in LDS once and no lane waits on a position another fold serves.
//                          The run is walked kAdvTile = 32 positions at a time: rows standardised into LDS, the forward chains on a
//                          16 x 16 thread grid (2 rows x 2 units per pass), the logit / p / coef of a row on one lane each, the
//                          deltas written over the activations, and the d backward chains on an 8 x 32 grid (4 rows per thread,
//                          consecutive columns on consecutive lanes).
// ONE image of W1 is held, transposed, with the ODD row stride HP = He | 1: W1T[c * HP + h].  The forward reads it with consecutive
// units on consecutive lanes (stride 1), the backward with consecutive columns on consecutive lanes (stride HP): ds_read_b32 banks
// are (a / 4) % 32 per 32-lane half, and an odd stride puts the 32 columns of a half on 32 different banks, so neither read
// conflicts and the second, row-major image (64 KiB more at H = d = 128: 166 KiB, over a CU's 160) is not needed.
// The shared definitions of attack.hip (the shape, the float64 sigmoid) are COPIED here, not moved to a header: attack.hip is not
// touched and its kernels keep their machine code.  No floating-point atomics, no float32 operation contracted.
#include "ure_internal.h"

namespace ure {

constexpr int kAdvMaxD = URE_ATTACK_MAX_D, kAdvMaxH = URE_ATTACK_MAX_H, kAdvMaxFolds = URE_ATTACK_MAX_FOLDS;
constexpr int kAdvRun = URE_ADV_RUN, kAdvTile = 32;
static_assert(kAdvRun % kAdvTile == 0 && kBlock == 256 && kAdvTile == 32, "the thread grids below are 16 x 16 and 8 x 32 on tiles of 32 rows");

__host__ __device__ inline int adv_hp(int He) { return He | 1; }
__host__ __device__ inline int adv_odd(int v) { return v | 1; }      // the row strides of zs and rs: odd, as HP is (one lane per row walks them)
// LDS in floats: W1T | b1 | w2 | b2 (4) | mean | inv | zs [tile][ZS] | rs [tile][RS] | coef [tile] | pos, row, bad int [tile] each
__host__ __device__ inline int adv_lds_floats(int d, int He)
{
    return d * adv_hp(He) + 2 * He + 4 + 2 * d + kAdvTile * adv_odd(d + 1) + kAdvTile * adv_odd(He + 1) + 4 * kAdvTile;
}

// attack.hip's atk_sigmoid: the float64 sigmoid of the float32 logit rounded once.  noinline: one copy of the float64 exp, outside
// the kernel's register budget.
__device__ __noinline__ float adv_sigmoid(float t) { return (float)(1.0 / (1.0 + exp(-(double)t))); }

__global__ __launch_bounds__(kBlock) void adv_input_grad_kernel(const float *__restrict__ X, int64_t ld, const int32_t *__restrict__ rows,
                                                                const int32_t *__restrict__ fold_of, int m, int n1, int folds, int d, int H,
                                                                const float *__restrict__ stats, const float *__restrict__ params,
                                                                const float *__restrict__ fw, float target0, float target1,
                                                                const int32_t *__restrict__ perm, const int32_t *__restrict__ fold_off,
                                                                float *__restrict__ grad, float *__restrict__ p_out)
{
    extern __shared__ float adv_lds[];
    const int tid = threadIdx.x;
    const int He = H > 0 ? H : 1, HP = adv_hp(He), ZS = adv_odd(d + 1), RS = adv_odd(He + 1);
    const bool linear = H == 0;
    const float nan = __builtin_nanf("");

    // the run of this workgroup: entries [k0, k1) of group g (uniform)
    int g = 0, lo = 0, hi = m, b = blockIdx.x;
    if (fold_of) {
        bool found = false;
        for (g = 0; g <= folds; ++g) {
            lo = min(max(ldg(fold_off + g), 0), m);
            hi = min(max(ldg(fold_off + g + 1), lo), m);
            const int runs = (hi - lo + kAdvRun - 1) / kAdvRun;
            if (b < runs) {
                found = true;
                break;
            }
            b -= runs;
        }
        if (!found) return;
    } else if ((int64_t)b * kAdvRun >= m) {
        return;
    }
    const int k0 = lo + b * kAdvRun, k1 = min(hi, k0 + kAdvRun);

    if (g == folds) {       // positions no fold serves: NaN rows (fold_of given, so g counts up to folds)
        for (int k = k0 + (tid >> 5); k < k1; k += kBlock / 32) {
            const int pos = ldg(perm + k);
            if (pos < 0 || pos >= m) continue;
            for (int c = tid & 31; c < d; c += 32) grad[(int64_t)pos * d + c] = nan;
            if (p_out && (tid & 31) == 0) p_out[pos] = nan;
        }
        return;
    }

    const int f = g;
    float *W1T = adv_lds;                                        // [d][HP]
    float *b1 = W1T + d * HP, *w2 = b1 + He, *b2 = w2 + He;     // b2: 4 floats
    float *mean = b2 + 4, *inv = mean + d;
    float *zs = inv + d;                                         // [kAdvTile][ZS]
    float *rs = zs + kAdvTile * ZS;                              // [kAdvTile][RS]: activations, then deltas
    float *coef = rs + kAdvTile * RS;                            // [kAdvTile]
    int *posr = reinterpret_cast<int *>(coef + kAdvTile), *rowr = posr + kAdvTile, *badr = rowr + kAdvTile;
    const int P = linear ? d + 1 : He * d + 2 * He + 1, at_b1 = He * d, at_w2 = at_b1 + He, at_b2 = at_w2 + He;
    const float *w = params + (int64_t)f * P;

    for (int e = tid; e < He * d; e += kBlock) W1T[(e % d) * HP + e / d] = ldg(w + e);
    for (int h = tid; h < He; h += kBlock) {
        b1[h] = ldg(w + at_b1 + h);
        w2[h] = linear ? 1.0f : ldg(w + at_w2 + h);
    }
    if (tid == 0) b2[0] = linear ? 0.0f : ldg(w + at_b2);
    for (int c = tid; c < d; c += kBlock) {
        mean[c] = ldg(stats + ((int64_t)f * 2 + 0) * d + c);
        inv[c] = ldg(stats + ((int64_t)f * 2 + 1) * d + c);
    }
    const float wc0 = ldg(fw + 4 * f), wc1 = ldg(fw + 4 * f + 1);
    const int ty = tid >> 4, tx = tid & 15;         // the forward's grid
    const int ry = tid >> 5, cx = tid & 31;         // the backward's

#pragma unroll 1
    for (int t0 = k0; t0 < k1; t0 += kAdvTile) {
        // 0. the tile's positions
        if (tid < kAdvTile) {
            const int k = t0 + tid;
            int pos = -1;
            if (k < k1) {
                pos = perm && fold_of ? ldg(perm + k) : k;
                if (pos < 0 || pos >= m) pos = -1;
            }
            posr[tid] = pos;
            rowr[tid] = pos >= 0 ? ldg(rows + pos) : 0;
            badr[tid] = pos >= 0 && fold_of ? ldg(fold_of + pos) != f : 0;
        }
        __syncthreads();        // (also: the staged parameters, and the tile before this one is done with)
        // 1. the rows, standardised
#pragma unroll 1
        for (int e = tid; e < kAdvTile * d; e += kBlock) {
            const int r = e / d, c = e - r * d;
            float z = 0.0f;
            if (posr[r] >= 0) z = (ldg(X + (int64_t)rowr[r] * ld + c) - mean[c]) * inv[c];
            zs[r * ZS + c] = z;
        }
        __syncthreads();
        // 2. forward: rows ty and ty + 16, units tx + 32 j and tx + 32 j + 16
        {
            const float *z0 = zs + ty * ZS, *z1 = zs + (ty + 16) * ZS;
#pragma unroll 1
            for (int ha = tx; ha < He; ha += 32) {
                const int hb = min(ha + 16, He - 1);
                float a0 = 0.0f, a1 = 0.0f, c0 = 0.0f, c1 = 0.0f;
#pragma unroll 4
                for (int c = 0; c < d; ++c) {
                    const float x0 = z0[c], x1 = z1[c], wa = W1T[c * HP + ha], wb = W1T[c * HP + hb];
                    a0 = a0 + wa * x0;
                    a1 = a1 + wa * x1;
                    c0 = c0 + wb * x0;
                    c1 = c1 + wb * x1;
                }
                a0 = a0 + b1[ha], a1 = a1 + b1[ha];
                rs[ty * RS + ha] = linear ? a0 : (a0 <= 0.0f ? 0.0f : a0);
                rs[(ty + 16) * RS + ha] = linear ? a1 : (a1 <= 0.0f ? 0.0f : a1);
                if (ha + 16 < He) {
                    c0 = c0 + b1[hb], c1 = c1 + b1[hb];
                    rs[ty * RS + hb] = linear ? c0 : (c0 <= 0.0f ? 0.0f : c0);
                    rs[(ty + 16) * RS + hb] = linear ? c1 : (c1 <= 0.0f ? 0.0f : c1);
                }
            }
        }
        __syncthreads();
        // 3. one lane per row: the logit, p and coef
        if (tid < kAdvTile) {
            const int pos = posr[tid];
            const float *r = rs + tid * RS;
            float t = r[0];
            if (!linear) {
                t = 0.0f;
#pragma unroll 4
                for (int h = 0; h < He; ++h) t = t + w2[h] * r[h];
                t = t + b2[0];
            }
            float cf = 0.0f;
            if (pos >= 0) {
                const bool cls1 = pos < n1;
                const float p = adv_sigmoid(t);
                cf = (cls1 ? wc1 : wc0) * (p - (cls1 ? target1 : target0));
                if (p_out) p_out[pos] = badr[tid] ? nan : p;
            }
            coef[tid] = cf;
        }
        __syncthreads();
        // 4. the deltas, over the activations
#pragma unroll 1
        for (int e = tid; e < kAdvTile * He; e += kBlock) {
            const int r = e / He, h = e - r * He;
            const float v = rs[r * RS + h], cf = coef[r];
            rs[r * RS + h] = linear ? cf : (v > 0.0f ? cf * w2[h] : 0.0f);
        }
        __syncthreads();
        // 5. the backward chains: rows ry + 8 i, columns cx + 32 j
        {
            const float *d0 = rs + ry * RS, *d1 = d0 + 8 * RS, *d2 = d1 + 8 * RS, *d3 = d2 + 8 * RS;
#pragma unroll 1
            for (int c = cx; c < d; c += 32) {
                const float *wcol = W1T + c * HP;
                float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
#pragma unroll 4
                for (int h = 0; h < He; ++h) {
                    const float wv = wcol[h];
                    s0 = s0 + d0[h] * wv;
                    s1 = s1 + d1[h] * wv;
                    s2 = s2 + d2[h] * wv;
                    s3 = s3 + d3[h] * wv;
                }
                const float iv = inv[c];
                const float out[4] = {s0 * iv, s1 * iv, s2 * iv, s3 * iv};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int r = ry + 8 * i, pos = posr[r];
                    if (pos >= 0) grad[(int64_t)pos * d + c] = badr[r] ? nan : out[i];
                }
            }
        }
        __syncthreads();
    }
}

}  // namespace ure

using namespace ure;

extern "C" {

int ure_adv_input_grad(const float *X, int64_t ld, int32_t d, const int32_t *rows, const int32_t *fold_of, int64_t m, int64_t n1, int32_t folds, int32_t H,
                       const float *stats, const float *params, const float *fw, float target0, float target1, float *grad, float *p_out,
                       const int32_t *perm, const int32_t *fold_off, void *stream)
{
    URE_ARG(X && rows && stats && params && fw && grad);
    URE_ARG(d >= 1 && d <= kAdvMaxD && H >= 0 && H <= kAdvMaxH && folds >= 1 && folds <= kAdvMaxFolds && m >= 1 && m <= URE_ATTACK_MAX_ROWS);
    URE_ARG(ld >= d && n1 >= 0 && n1 <= m);
    URE_ARG(target0 - target0 == 0.0f && target1 - target1 == 0.0f);      // finite: neither NaN nor an infinity
    URE_ARG(!fold_of || (perm && fold_off));
    const int He = H > 0 ? H : 1;
    const size_t lds = 4 * (size_t)adv_lds_floats(d, He);
    // a group's runs: ceil(n_g / run) <= n_g / run + 1 over folds + 1 groups
    const int64_t blocks = (m + kAdvRun - 1) / kAdvRun + (fold_of ? folds + 1 : 0);
    URE_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(adv_input_grad_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(adv_input_grad_kernel, dim3((unsigned)blocks), dim3(kBlock), lds, static_cast<hipStream_t>(stream), X, ld, rows, fold_of, (int)m,
                       (int)n1, (int)folds, (int)d, (int)H, stats, params, fw, target0, target1, perm, fold_off, grad, p_out);
    URE_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"

// adv.hip -- the gradient of the attribute probe's loss with respect to its input rows, for gfx950 (the arithmetic is
// stated in numpy in ultrare_amd/adv_unlearn.py, the entry in include/ultrare_adv.h).  The probe is probe.h's, and a position is
// served by the fold that held it out.
//   adv_input_grad_kernel  workgroup = up to kAdvRun = 256 consecutive entries of ONE fold's group of the plan (perm / fold_off), so
//                          the fold's packed parameters are staged in LDS once and no lane waits on a position another fold serves.
//                          The run is walked kTile = 32 positions at a time: probe.h's standardisation, forward (2 rows x 2 units
//                          per pass) and logit, then p / coef of a row on one lane each, the deltas written over the activations,
//                          and the d backward chains on an 8 x 32 grid (4 rows per thread, consecutive columns on consecutive lanes).
// ONE image of W1 is held, transposed, and probe.h's layout is taken with ODD row strides (HP = He | 1): W1T[c * HP + h].  The
// forward reads it with consecutive units on consecutive lanes (stride 1), the backward with consecutive columns on consecutive
// lanes (stride HP): ds_read_b32 banks are (a / 4) % 32 per 32-lane half, and an odd stride puts the 32 columns of a half on 32
// different banks, so neither read conflicts and the second, row-major image (64 KiB more at H = d = 128: 166 KiB, over a CU's 160)
// is not needed.  The row strides of zs and rs are odd as HP is: one lane per row walks them.
// No floating-point atomics, no float32 operation contracted.
#include "probe.h"

namespace ure {

constexpr int kAdvRun = URE_ADV_RUN, kTile = kProbeTile;
static_assert(kAdvRun % kTile == 0 && kBlock == 256 && kTile == 32, "the backward's thread grid is 8 x 32 on tiles of 32 rows");

// LDS: probe.h's layout with odd strides, then pos, row, bad int [tile] each
static size_t adv_lds_bytes(int d, int He) { return 4 * ((size_t)probe_lds(d, He, 1).floats + 3 * kTile); }

__global__ __launch_bounds__(kBlock) void adv_input_grad_kernel(const float *__restrict__ X, int64_t ld, const int32_t *__restrict__ rows,
                                                                const int32_t *__restrict__ fold_of, int m, int n1, int folds, int d, int H,
                                                                const float *__restrict__ stats, const float *__restrict__ params,
                                                                const float *__restrict__ fw, float target0, float target1,
                                                                const int32_t *__restrict__ perm, const int32_t *__restrict__ fold_off,
                                                                float *__restrict__ grad, float *__restrict__ p_out)
{
    extern __shared__ float adv_lds[];
    const int tid = threadIdx.x;
    const AtkShape s = atk_shape(d, H);
    const int He = s.He;
    const bool linear = s.linear;
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
    const ProbeLds L = probe_lds(d, He, 1, adv_lds);             // rs: activations, then deltas
    int *posr = reinterpret_cast<int *>(adv_lds + L.floats), *rowr = posr + kTile, *badr = rowr + kTile;
    probe_stage(L, s, params + (int64_t)f * s.P, stats + (int64_t)f * 2 * d);
    const float wc0 = ldg(fw + 4 * f), wc1 = ldg(fw + 4 * f + 1);
    const int ry = tid >> 5, cx = tid & 31;         // the backward's grid

#pragma unroll 1
    for (int t0 = k0; t0 < k1; t0 += kTile) {
        // 0. the tile's positions
        if (tid < kTile) {
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
        probe_standardize(L, d, X, ld, [&](int r, int &row) { return posr[r] >= 0 && (row = rowr[r], true); });
        __syncthreads();
        // 2. forward: rows ty and ty + 16, units h0 + tx and h0 + tx + 16 a pass
#pragma unroll 1
        for (int h0 = 0; h0 < He; h0 += 32) probe_forward<2>(L, s, h0);
        __syncthreads();
        // 3. one lane per row: the logit, p and coef
        if (tid < kTile) {
            const int pos = posr[tid];
            const float t = probe_logit(L, s, tid);
            float cf = 0.0f;
            if (pos >= 0) {
                const bool cls1 = pos < n1;
                const float p = probe_sigmoid(t);
                cf = (cls1 ? wc1 : wc0) * (p - (cls1 ? target1 : target0));
                if (p_out) p_out[pos] = badr[tid] ? nan : p;
            }
            L.coef[tid] = cf;
        }
        __syncthreads();
        // 4. the deltas, over the activations
#pragma unroll 1
        for (int e = tid; e < kTile * He; e += kBlock) {
            const int r = e / He, h = e - r * He;
            const float v = L.rs[r * L.RS + h], cf = L.coef[r];
            L.rs[r * L.RS + h] = linear ? cf : (v > 0.0f ? cf * L.w2[h] : 0.0f);
        }
        __syncthreads();
        // 5. the backward chains: rows ry + 8 i, columns cx + 32 j
        {
            const float *d0 = L.rs + ry * L.RS, *d1 = d0 + 8 * L.RS, *d2 = d1 + 8 * L.RS, *d3 = d2 + 8 * L.RS;
#pragma unroll 1
            for (int c = cx; c < d; c += 32) {
                const float *wcol = L.W1T + c * L.HP;
                float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
#pragma unroll 4
                for (int h = 0; h < He; ++h) {
                    const float wv = wcol[h];
                    s0 = s0 + d0[h] * wv;
                    s1 = s1 + d1[h] * wv;
                    s2 = s2 + d2[h] * wv;
                    s3 = s3 + d3[h] * wv;
                }
                const float iv = L.inv[c];
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
    URE_ARG(probe_shape_ok(m, d, H, folds, 1, 1, URE_ATTACK_MAX_ROWS));
    URE_ARG(ld >= d && n1 >= 0 && n1 <= m);
    URE_ARG(target0 - target0 == 0.0f && target1 - target1 == 0.0f);      // finite: neither NaN nor an infinity
    URE_ARG(!fold_of || (perm && fold_off));
    const size_t lds = adv_lds_bytes(d, atk_shape(d, H).He);
    // a group's runs: ceil(n_g / run) <= n_g / run + 1 over folds + 1 groups
    const int64_t blocks = (m + kAdvRun - 1) / kAdvRun + (fold_of ? folds + 1 : 0);
    URE_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(adv_input_grad_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(adv_input_grad_kernel, dim3((unsigned)blocks), dim3(kBlock), lds, static_cast<hipStream_t>(stream), X, ld, rows, fold_of, (int)m,
                       (int)n1, (int)folds, (int)d, (int)H, stats, params, fw, target0, target1, perm, fold_off, grad, p_out);
    URE_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"

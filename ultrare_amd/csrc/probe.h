// probe.h -- the attribute probe, shared by attack.hip (which trains and scores it) and adv.hip (which differentiates
// it with respect to its input rows).  One hidden layer of H relu units (H = 0: logistic regression, run as ONE linear
// hidden unit whose output is the logit), one packed parameter set [W1 H x d | b1 | w2 | b2] per cross-validation fold, rows
// standardised by the fold's (mean, 1 / std), p the float64 sigmoid of the float32 logit.  What a kernel of either file computes
// for a tile of kProbeTile = 32 rows up to the logit is written ONCE here, so the two agree bit for bit by construction; the
// arithmetic is stated in numpy in ultrare_amd/attack.py (forward_ref).  Chains start from +0.0 and round every multiply and add on
// its own (-ffp-contract=off).
#pragma once
#include "ure_internal.h"

namespace ure {

constexpr int kProbeMaxD = URE_ATTACK_MAX_D, kProbeMaxH = URE_ATTACK_MAX_H, kProbeMaxFolds = URE_ATTACK_MAX_FOLDS;
constexpr int kProbeTile = 32;
static_assert(kBlock == 256 && kProbeTile == 32, "probe_forward's thread grid is 16 x 16 on a tile of 32 rows");

// (the name is attack.hip's, where it came from: it is part of the kernels' symbols)
struct AtkShape {
    int d, H, He, linear;       // He = max(H, 1) hidden units as the kernels run them
    int P, at_b1, at_w2, at_b2;
};

__host__ __device__ inline AtkShape atk_shape(int d, int H)
{
    AtkShape s;
    s.d = d, s.H = H, s.He = H > 0 ? H : 1, s.linear = H == 0;
    s.at_b1 = s.He * d, s.at_w2 = s.at_b1 + s.He, s.at_b2 = s.at_w2 + s.He;
    s.P = H > 0 ? s.at_b2 + 1 : d + 1;
    return s;
}

// the limits of every entry that takes a probe; what an entry needs at least (training: two folds, a row per fold) and takes at most is its own
inline bool probe_shape_ok(int64_t m, int d, int H, int folds, int min_folds, int64_t min_m, int64_t max_m)
{
    return d >= 1 && d <= kProbeMaxD && H >= 0 && H <= kProbeMaxH && folds >= min_folds && folds <= kProbeMaxFolds && m >= min_m && m <= max_m;
}

__host__ __device__ inline bool atk_is_weight(const AtkShape &s, int e) { return e < s.at_b1 || (!s.linear && e >= s.at_w2 && e < s.at_b2); }

// The LDS of a workgroup that runs the probe on one fold, in floats from `base`:
//   W1T [d][HP] | b1 [He] | w2 [He] | b2 (4) | mean [d] | inv [d] | zs [tile][ZS] | rs [tile][RS] | coef [tile]
// W1 is held transposed (the lanes of a forward read consecutive hidden units).  The row strides are data: odd = 0 gives the plain
// He, d + 1, He + 1; odd = 1 makes each of them odd (a walk with the row stride between lanes then meets 32 banks).
// A kernel keeps what else it needs in front of `base` or behind `floats`.
struct ProbeLds {
    int HP, ZS, RS, floats;
    float *W1T, *b1, *w2, *b2, *mean, *inv, *zs, *rs, *coef;
};

__host__ __device__ inline ProbeLds probe_lds(int d, int He, int odd, float *base = nullptr)      // (no base: for `floats` alone)
{
    ProbeLds L;
    L.HP = He | odd, L.ZS = (d + 1) | odd, L.RS = (He + 1) | odd;
    int at = 0;
    L.W1T = base + at, at += d * L.HP;
    L.b1 = base + at, at += He;
    L.w2 = base + at, at += He;
    L.b2 = base + at, at += 4;
    L.mean = base + at, at += d;
    L.inv = base + at, at += d;
    L.zs = base + at, at += kProbeTile * L.ZS;
    L.rs = base + at, at += kProbeTile * L.RS;
    L.coef = base + at, at += kProbeTile;
    L.floats = at;
    return L;
}

// one fold's packed parameters w and statistics (mean [d] | inv [d]) into LDS; the linear probe gets w2 = 1, b2 = 0
__device__ __forceinline__ void probe_stage(const ProbeLds &L, const AtkShape &s, const float *__restrict__ w, const float *__restrict__ stats)
{
    const int tid = threadIdx.x, d = s.d, He = s.He;
    for (int e = tid; e < He * d; e += kBlock) L.W1T[(e % d) * L.HP + e / d] = ldg(w + e);
    for (int h = tid; h < He; h += kBlock) {
        L.b1[h] = ldg(w + s.at_b1 + h);
        L.w2[h] = s.linear ? 1.0f : ldg(w + s.at_w2 + h);
    }
    if (tid == 0) L.b2[0] = s.linear ? 0.0f : ldg(w + s.at_b2);
    for (int c = tid; c < d; c += kBlock) {
        L.mean[c] = ldg(stats + c);
        L.inv[c] = ldg(stats + d + c);
    }
}

// zs[r][c] = (x[c] - mean[c]) * inv[c] for the tile's 32 slots of the table X; live(r, row) says whether slot r holds a position and,
// if it does, sets its row of X.  A dead slot gets +0.0, which leave a chain that started from +0.0 as it was.  (`row` starts at 0 for
// the compiler's sake: left undefined, or with one callable that returns a row or -1, attack_train_kernel<2, 1> and <2, 2> are
// allotted 5 - 6 fewer VGPRs and their forward loops wait on every LDS read in turn)
template <class Live>
__device__ __forceinline__ void probe_standardize(const ProbeLds &L, int d, const float *X, int64_t ld, Live live)
{
#pragma unroll 1
    for (int e = threadIdx.x; e < kProbeTile * d; e += kBlock) {
        const int r = e / d, c = e - r * d;
        int row = 0;
        float z = 0.0f;
        if (live(r, row)) z = (ldg(X + (int64_t)row * ld + c) - L.mean[c]) * L.inv[c];
        L.zs[r * L.ZS + c] = z;
    }
}

// forward on the 16 x 16 thread grid: thread (ty, tx) computes rows ty and ty + 16 of the tile and the units h0 + tx + 16 j, j < HQ,
// into rs.  (Clamped copies of the unit index LDS; a unit at or beyond He is never stored.)
template <int HQ>
__device__ __forceinline__ void probe_forward(const ProbeLds &L, const AtkShape &s, int h0)
{
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15, d = s.d, He = s.He;
    int hf[HQ];
    float t0[HQ], t1[HQ];
#pragma unroll
    for (int j = 0; j < HQ; ++j) hf[j] = min(h0 + tx + 16 * j, He - 1), t0[j] = 0.0f, t1[j] = 0.0f;
    const float *z0 = L.zs + ty * L.ZS, *z1 = L.zs + (ty + 16) * L.ZS;
#pragma unroll 4
    for (int c = 0; c < d; ++c) {
        const float a0 = z0[c], a1 = z1[c];
#pragma unroll
        for (int j = 0; j < HQ; ++j) {
            const float wv = L.W1T[c * L.HP + hf[j]];
            t0[j] = t0[j] + wv * a0;
            t1[j] = t1[j] + wv * a1;
        }
    }
#pragma unroll
    for (int j = 0; j < HQ; ++j)
        if (h0 + tx + 16 * j < He) {
            const float b = L.b1[hf[j]], a0 = t0[j] + b, a1 = t1[j] + b;
            L.rs[ty * L.RS + hf[j]] = s.linear ? a0 : (a0 <= 0.0f ? 0.0f : a0);
            L.rs[(ty + 16) * L.RS + hf[j]] = s.linear ? a1 : (a1 <= 0.0f ? 0.0f : a1);
        }
}

// the logit of the tile's row `r` from its activations in rs (one lane per row)
__device__ __forceinline__ float probe_logit(const ProbeLds &L, const AtkShape &s, int r)
{
    const float *a = L.rs + r * L.RS;
    if (s.linear) return a[0];
    float t = 0.0f;
#pragma unroll 4
    for (int h = 0; h < s.He; ++h) t = t + L.w2[h] * a[h];
    return t + L.b2[0];
}

// p = 1 / (1 + exp(-t)) evaluated in float64 and rounded to float32 ONCE: the correctly rounded sigmoid of the float32 logit (but for
// the last bit of the float64 exp), so the contract's numpy line gives the same float32.  noinline: one copy of the float64 exp,
// outside the calling kernel's register budget (inlined it cost attack_train_kernel<> 100 - 180 VGPRs per instantiation).
__device__ __noinline__ float probe_sigmoid(float t) { return (float)(1.0 / (1.0 + exp(-(double)t))); }

// tree over the 256 threads of a workgroup: red[t] += red[t + w], w = 128 .. 1 (lightgcn.fold_256's fold), with a trailing barrier so
// that `red` can be reused at once
template <class T>
__device__ __forceinline__ T block_fold(T *red, T v)
{
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if (t < w) red[t] = red[t] + red[t + w];
        __syncthreads();
    }
    const T out = red[0];
    __syncthreads();
    return out;
}

}  // namespace ure

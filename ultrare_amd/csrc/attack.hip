// attack.hip -- the attribute-inference attacker on selected rows of a float32 table, for gfx950 (the arithmetic is
// stated in numpy in ultrare_amd/attack.py, the entries in include/ultrare_attack.h).
//
// The probe of probe.h is trained by full-batch Adam to tell the first n1 selected rows from the rest, one parameter set per
// cross-validation fold.
//   attack_train_kernel   workgroup (chunk, fold) owns kChunk = 256 consecutive positions.  The fold's packed parameters are staged
//                         in LDS once, then the chunk is walked kTile = 32 positions at a time: probe.h's standardisation,
//                         forward (2 rows x HQ units per thread) and logit, then p / coef / loss of a row on one lane each, and the
//                         gradient chains continued in registers (thread (ty, tx) owns units ty + 16 i and columns tx + 16 j).
//                         A position the fold holds out (and the tail behind m) has coef = +0.0: its terms are zeros, which
//                         leave a chain that started from +0.0 as it was.  The chunk's sums go to scratch.
//   attack_update_kernel  thread = one parameter of one fold: the chunk sums added in chunk order, then Adam.  Its workgroup 0 also
//                         folds the epoch's loss.
// No floating-point atomics, no float32 operation contracted (-ffp-contract=off), one float64 exp per row for p.
//
// The AUC is the exact count of (positive, negative) pairs with s_p > s_n and s_p == s_n: auc_tile_kernel holds one positive per
// lane and walks the negatives through LDS, kAucNeg at a time; integer partial counts per workgroup, summed by auc_sum_kernel.
#include "probe.h"

namespace ure {

constexpr int kChunk = URE_ATTACK_CHUNK, kTile = kProbeTile;
constexpr int kAucPos = URE_AUC_TILE_POS, kAucNeg = URE_AUC_TILE_NEG, kAucMaxSplit = 128;
static_assert(kChunk == kBlock && kAucPos == kBlock && kChunk % kTile == 0, "one thread per position of a chunk");

// training and its statistics want two folds and a row per fold
static bool atk_shape_ok(int64_t m, int d, int H, int folds) { return probe_shape_ok(m, d, H, folds, 2, folds, URE_ATTACK_MAX_ROWS); }

// scratch of ure_attack_train: [part_loss double folds x chunks | l2sum double folds | part_grad float folds x chunks x P | mom | var float folds x P]
struct AtkPlan {
    int64_t chunks, off_l2, off_grad, off_mom, off_var, bytes;
};

static AtkPlan atk_plan(int64_t m, const AtkShape &s, int folds)
{
    AtkPlan p;
    p.chunks = (m + kChunk - 1) / kChunk;
    p.off_l2 = 8 * folds * p.chunks;
    p.off_grad = p.off_l2 + 8 * folds;
    p.off_mom = p.off_grad + 4 * folds * p.chunks * s.P;
    p.off_var = p.off_mom + 4 * (int64_t)folds * s.P;
    p.bytes = (p.off_var + 4 * (int64_t)folds * s.P + 7) / 8 * 8;
    return p;
}

// LDS of the training kernel: kBlock + kTile doubles (the fold's tree, the tile's row losses) in front of probe.h's layout, plain strides
static size_t atk_lds_bytes(int d, int He) { return 8 * (kBlock + kTile) + 4 * (size_t)probe_lds(d, He, 0).floats; }

// (noinline: one copy of the float64 exp / log1p, outside the training kernel's register budget)
__device__ __noinline__ double atk_softplus(double v) { return fmax(v, 0.0) + log1p(exp(-fabs(v))); }

// ---- statistics: workgroup = one column, every fold at once ------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void attack_stats_kernel(const float *__restrict__ X, int64_t ld, const int32_t *__restrict__ rows,
                                                              const int32_t *__restrict__ fold_of, int64_t m, int folds, int d, float *__restrict__ stats)
{
    __shared__ double red[kBlock];
    __shared__ double mean_s[kProbeMaxFolds];
    __shared__ int ntrain[kProbeMaxFolds];
    const int t = threadIdx.x, c = blockIdx.x;
    if (t < kProbeMaxFolds) ntrain[t] = 0;
    __syncthreads();
    double acc[kProbeMaxFolds];
    int cnt[kProbeMaxFolds];
#pragma unroll
    for (int f = 0; f < kProbeMaxFolds; ++f) acc[f] = 0.0, cnt[f] = 0;
    for (int64_t i = t; i < m; i += kBlock) {
        const double x = (double)ldg(X + (int64_t)ldg(rows + i) * ld + c);
        const int fo = ldg(fold_of + i);
#pragma unroll
        for (int f = 0; f < kProbeMaxFolds; ++f) {
            acc[f] = acc[f] + (fo != f ? x : 0.0);
            cnt[f] += fo != f;
        }
    }
#pragma unroll
    for (int f = 0; f < kProbeMaxFolds; ++f) {
        if (f < folds) {                  // (uniform)
            atomicAdd(&ntrain[f], cnt[f]);
            const double s = block_fold(red, acc[f]);
            if (t == 0) mean_s[f] = s / (double)ntrain[f];
        }
    }
    __syncthreads();
    double mean[kProbeMaxFolds];
#pragma unroll
    for (int f = 0; f < kProbeMaxFolds; ++f) mean[f] = f < folds ? mean_s[f] : 0.0, acc[f] = 0.0;
    for (int64_t i = t; i < m; i += kBlock) {
        const double x = (double)ldg(X + (int64_t)ldg(rows + i) * ld + c);
        const int fo = ldg(fold_of + i);
#pragma unroll
        for (int f = 0; f < kProbeMaxFolds; ++f) {
            const double dv = x - mean[f];
            acc[f] = acc[f] + (fo != f ? dv * dv : 0.0);
        }
    }
#pragma unroll
    for (int f = 0; f < kProbeMaxFolds; ++f) {
        if (f < folds) {
            const double var = block_fold(red, acc[f]) / (double)ntrain[f];
            if (t == 0) {
                stats[((int64_t)f * 2 + 0) * d + c] = (float)mean[f];
                stats[((int64_t)f * 2 + 1) * d + c] = var > 0.0 ? (float)(1.0 / sqrt(var)) : 0.0f;
            }
        }
    }
}

// ---- training: one chunk of one fold ---------------------------------------------------------------------------------------------
template <int HQ, int DQ>
__global__ __launch_bounds__(kBlock) void attack_train_kernel(const float *__restrict__ X, int64_t ld, const int32_t *__restrict__ rows,
                                                              const int32_t *__restrict__ fold_of, int m, int n1, AtkShape s,
                                                              const float *__restrict__ stats, const float *__restrict__ fw,
                                                              const float *__restrict__ win, int chunks, double *__restrict__ part_loss,
                                                              double *__restrict__ l2sum, float *__restrict__ part_grad)
{
    extern __shared__ double atk_lds[];
    const int d = s.d, He = s.He;
    double *red = atk_lds, *rloss = red + kBlock;
    const ProbeLds L = probe_lds(d, He, 0, reinterpret_cast<float *>(rloss + kTile));
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int f = blockIdx.y, chunk = blockIdx.x;

    probe_stage(L, s, win + (int64_t)f * s.P, stats + (int64_t)f * 2 * d);
    __syncthreads();

    if (chunk == 0) {       // l2sum[f]: the 256-lane fold over the packed index of float64 w^2, the biases adding nothing
        double sq = 0.0;
        for (int e = tid; e < s.P; e += kBlock)
            if (atk_is_weight(s, e)) {
                const double v = (double)(e < s.at_b1 ? L.W1T[(e % d) * L.HP + e / d] : L.w2[e - s.at_w2]);
                sq = sq + v * v;
            }
        const double tot = block_fold(red, sq);
        if (tid == 0) l2sum[f] = tot;
    }

    const float wc0 = ldg(fw + 4 * f), wc1 = ldg(fw + 4 * f + 1);
    // the units and columns this thread owns in the gradient (clamped copies index LDS; what lies outside is never stored)
    int hh[HQ], cc[DQ];
    float w2r[HQ];
#pragma unroll
    for (int i = 0; i < HQ; ++i) hh[i] = min(ty + 16 * i, He - 1), w2r[i] = L.w2[hh[i]];
#pragma unroll
    for (int j = 0; j < DQ; ++j) cc[j] = min(tx + 16 * j, d - 1);

    float acc[HQ][DQ], gb1[HQ], gw2[HQ], gb2 = 0.0f;
#pragma unroll
    for (int i = 0; i < HQ; ++i) {
        gb1[i] = 0.0f, gw2[i] = 0.0f;
#pragma unroll
        for (int j = 0; j < DQ; ++j) acc[i][j] = 0.0f;
    }
    double closs = 0.0;

    const int base = chunk * kChunk;
#pragma unroll 1
    for (int p0 = base; p0 < base + kChunk && p0 < m; p0 += kTile) {
        // 1. the tile's rows, standardised (the tail behind m: dead slots)
        probe_standardize(L, d, X, ld, [&](int r, int &row) { return p0 + r < m && (row = ldg(rows + p0 + r), true); });
        __syncthreads();
        // 2. forward: rows ty and ty + 16, units tx + 16 j
        probe_forward<HQ>(L, s, 0);
        __syncthreads();
        // 3. one lane per row: the logit, p, coef and the row's loss
        if (tid < kTile) {
            const int i = p0 + tid;
            const float t = probe_logit(L, s, tid);
            float cf = 0.0f;
            double lo = 0.0;
            if (i < m && ldg(fold_of + i) != f) {
                const bool pos = i < n1;
                const float wc = pos ? wc1 : wc0;
                cf = wc * (probe_sigmoid(t) - (pos ? 1.0f : 0.0f));
                const double sgn = pos ? -(double)t : (double)t;
                lo = (double)wc * atk_softplus(sgn);
            }
            L.coef[tid] = cf;
            rloss[tid] = lo;
        }
        __syncthreads();
        // 4. the gradient chains go on over the tile's rows, in order
        if (tid == 0)
            for (int r = 0; r < kTile; ++r) closs = closs + rloss[r];
#pragma unroll 2
        for (int r = 0; r < kTile; ++r) {
            const float cf = L.coef[r];
            float dl[HQ];
#pragma unroll
            for (int i = 0; i < HQ; ++i) {
                const float rv = L.rs[r * L.RS + hh[i]];
                dl[i] = s.linear ? cf : (rv > 0.0f ? cf * w2r[i] : 0.0f);
                if (tx == 0) {
                    gb1[i] = gb1[i] + dl[i];
                    gw2[i] = gw2[i] + cf * rv;
                }
            }
            if (tid == 0) gb2 = gb2 + cf;
#pragma unroll
            for (int j = 0; j < DQ; ++j) {
                const float z = L.zs[r * L.ZS + cc[j]];
#pragma unroll
                for (int i = 0; i < HQ; ++i) acc[i][j] = acc[i][j] + dl[i] * z;
            }
        }
        __syncthreads();
    }

    float *out = part_grad + ((int64_t)f * chunks + chunk) * s.P;
#pragma unroll
    for (int i = 0; i < HQ; ++i) {
        const int h = ty + 16 * i;
        if (h < He) {
#pragma unroll
            for (int j = 0; j < DQ; ++j)
                if (tx + 16 * j < d) out[h * d + tx + 16 * j] = acc[i][j];
            if (tx == 0) {
                out[s.at_b1 + h] = gb1[i];
                if (!s.linear) out[s.at_w2 + h] = gw2[i];
            }
        }
    }
    if (tid == 0) {
        if (!s.linear) out[s.at_b2] = gb2;
        part_loss[(int64_t)f * chunks + chunk] = closs;
    }
}

// ---- update: one parameter per thread ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void attack_update_kernel(AtkShape s, int chunks, const float *__restrict__ part_grad,
                                                               const double *__restrict__ part_loss, const double *__restrict__ l2sum,
                                                               const float *__restrict__ fw, const float *__restrict__ sc, int epoch, int epochs,
                                                               float beta1, float beta2, float eps, float l2, const float *win,
                                                               float *wout, float *__restrict__ mom, float *__restrict__ var,
                                                               double *__restrict__ loss)
{
    __shared__ double red[kBlock];
    const int f = blockIdx.y, e = blockIdx.x * kBlock + threadIdx.x;
    const float m_train = ldg(fw + 4 * f + 2);
    if (blockIdx.x == 0) {
        double v = 0.0;
        for (int j = threadIdx.x; j < chunks; j += kBlock) v = v + ldg(part_loss + (int64_t)f * chunks + j);
        const double tot = block_fold(red, v);
        if (threadIdx.x == 0) loss[(int64_t)f * epochs + epoch] = tot / (double)m_train + 0.5 * (double)l2 * ldg(l2sum + f);
    }
    if (e >= s.P) return;
    const float *pg = part_grad + (int64_t)f * chunks * s.P + e;
    float g = ldg(pg);
    for (int j = 1; j < chunks; ++j) g = g + ldg(pg + (int64_t)j * s.P);
    const int64_t at = (int64_t)f * s.P + e;
    const float w = ldg(win + at);
    const float m0 = epoch == 0 ? 0.0f : mom[at], v0 = epoch == 0 ? 0.0f : var[at];
    const float s1 = ldg(sc + 2 * epoch), s2 = ldg(sc + 2 * epoch + 1);
    g = g / m_train;
    g = g + (atk_is_weight(s, e) ? l2 : 0.0f) * w;
    const float c1 = 1.0f - beta1, c2 = 1.0f - beta2;
    const float m1 = m0 + c1 * (g - m0);
    const float v1 = beta2 * v0 + (c2 * g) * g;
    const float den = sqrtf(v1) / s2 + eps;
    wout[at] = w - s1 * (m1 / den);
    mom[at] = m1;
    var[at] = v1;
}

// ---- scoring: one wave per row --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void attack_score_kernel(const float *__restrict__ X, int64_t ld, const int32_t *__restrict__ rows,
                                                              const int32_t *__restrict__ fold_of, int64_t m, int folds, AtkShape s,
                                                              const float *__restrict__ stats, const float *__restrict__ params, float *__restrict__ scores)
{
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int d = s.d, He = s.He;
    for (int64_t i = (int64_t)blockIdx.x * kWavesPerBlock + wv; i < m; i += (int64_t)gridDim.x * kWavesPerBlock) {      // (uniform per wave)
        const int f = fold_of ? ldg(fold_of + i) : 0;
        if (f < 0 || f >= folds) {
            if (lane == 0) scores[i] = __builtin_nanf("");
            continue;
        }
        const float *w = params + (int64_t)f * s.P, *mean = stats + (int64_t)f * 2 * d, *inv = mean + d;
        const float *x = X + (int64_t)ldg(rows + i) * ld;
        float r[2] = {0.0f, 0.0f};              // the units lane and lane + 64
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int h = lane + kWave * k;
            if (h < He) {
                float t = 0.0f;
                for (int c = 0; c < d; ++c) {
                    const float z = (ldg(x + c) - ldg(mean + c)) * ldg(inv + c);
                    t = t + ldg(w + h * d + c) * z;
                }
                const float a = t + ldg(w + s.at_b1 + h);
                r[k] = s.linear ? a : (a <= 0.0f ? 0.0f : a);
            }
        }
        float t = __shfl(r[0], 0, kWave);
        if (!s.linear) {        // every lane walks the chain over the units (the wave's lanes hold them)
            t = 0.0f;
            for (int h = 0; h < He; ++h) {
                const float rv = h < kWave ? __shfl(r[0], h, kWave) : __shfl(r[1], h - kWave, kWave);
                t = t + ldg(w + s.at_w2 + h) * rv;
            }
            t = t + ldg(w + s.at_b2);
        }
        if (lane == 0) scores[i] = probe_sigmoid(t);
    }
}

// ---- pair counts ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void auc_tile_kernel(const float *__restrict__ scores, const int32_t *__restrict__ pos, int64_t n1,
                                                          const int32_t *__restrict__ neg, int64_t n2, int64_t neg_tiles, int64_t *__restrict__ part,
                                                          int32_t *__restrict__ flags)
{
    __shared__ float sn[kAucNeg];
    __shared__ int64_t red[kBlock];
    __shared__ int nan_s;
    const int t = threadIdx.x;
    if (t == 0) nan_s = 0;
    const int64_t ip = (int64_t)blockIdx.x * kAucPos + t;
    const bool have = ip < n1;
    const float sp = have ? ldg(scores + ldg(pos + ip)) : __builtin_nanf("");     // a NaN counts for nothing
    bool bad = have && sp != sp;
    int64_t gt = 0, eq = 0;
    for (int64_t tile = blockIdx.y; tile < neg_tiles; tile += gridDim.y) {
        __syncthreads();
        for (int k = t; k < kAucNeg; k += kBlock) {
            const int64_t in = tile * kAucNeg + k;
            float v = __builtin_nanf("");
            if (in < n2) {
                v = ldg(scores + ldg(neg + in));
                bad |= v != v;
            }
            sn[k] = v;
        }
        __syncthreads();
        int g32 = 0, e32 = 0;
#pragma unroll 8
        for (int k = 0; k < kAucNeg; ++k) {
            const float v = sn[k];
            g32 += sp > v;
            e32 += sp == v;
        }
        gt += g32, eq += e32;
    }
    if (bad) atomicOr(&nan_s, 1);
    const int64_t G = block_fold(red, gt), E = block_fold(red, eq);
    if (t == 0) {
        const int64_t blk = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
        part[2 * blk] = G, part[2 * blk + 1] = E;
        flags[blk] = nan_s;
    }
}

__global__ __launch_bounds__(kBlock) void auc_sum_kernel(const int64_t *__restrict__ part, const int32_t *__restrict__ flags, int64_t n_part,
                                                         int64_t *__restrict__ counts, int32_t *__restrict__ nan_flag)
{
    __shared__ int64_t red[kBlock];
    int64_t g = 0, e = 0, b = 0;
    for (int64_t k = threadIdx.x; k < n_part; k += kBlock) g += ldg(part + 2 * k), e += ldg(part + 2 * k + 1), b |= ldg(flags + k) != 0;
    const int64_t G = block_fold(red, g), E = block_fold(red, e), B = block_fold(red, b);
    if (threadIdx.x == 0) counts[0] = G, counts[1] = E, *nan_flag = B != 0;
}

__global__ __launch_bounds__(kBlock) void confusion_kernel(const float *__restrict__ scores, const int32_t *__restrict__ pos, int64_t n1,
                                                           const int32_t *__restrict__ neg, int64_t n2, float thr, int64_t *__restrict__ counts)
{
    __shared__ int64_t red[kBlock];
    int64_t tp = 0, fp = 0;
    for (int64_t k = threadIdx.x; k < n1; k += kBlock) tp += ldg(scores + ldg(pos + k)) > thr;
    for (int64_t k = threadIdx.x; k < n2; k += kBlock) fp += ldg(scores + ldg(neg + k)) > thr;
    const int64_t TP = block_fold(red, tp), FP = block_fold(red, fp);
    if (threadIdx.x == 0) counts[0] = TP, counts[1] = n1 - TP, counts[2] = n2 - FP, counts[3] = FP;
}

struct AucPlan {
    int64_t pos_tiles, neg_tiles, split, n_part, off_flags, bytes;
};

static AucPlan auc_plan(int64_t n1, int64_t n2)
{
    AucPlan p;
    p.pos_tiles = (n1 + kAucPos - 1) / kAucPos;
    p.neg_tiles = (n2 + kAucNeg - 1) / kAucNeg;
    p.split = std::min<int64_t>(p.neg_tiles, kAucMaxSplit);
    p.n_part = p.pos_tiles * p.split;
    p.off_flags = 16 * p.n_part;
    p.bytes = (p.off_flags + 4 * p.n_part + 7) / 8 * 8;
    return p;
}

static bool auc_shape_ok(int64_t n1, int64_t n2) { return n1 >= 1 && n2 >= 1 && n1 <= INT32_MAX && n2 <= INT32_MAX; }

template <int HQ, int DQ>
static int launch_train(const float *X, int64_t ld, const int32_t *rows, const int32_t *fold_of, int64_t m, int64_t n1, int folds, const AtkShape &s,
                        const float *stats, const float *fw, const float *win, const AtkPlan &p, double *part_loss, double *l2sum, float *part_grad,
                        bool first, hipStream_t st)
{
    const size_t lds = atk_lds_bytes(s.d, s.He);
    auto kern = attack_train_kernel<HQ, DQ>;
    if (first) URE_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));     // once per call, not per epoch
    hipLaunchKernelGGL(kern, dim3((unsigned)p.chunks, (unsigned)folds), dim3(kBlock), lds, st, X, ld, rows, fold_of, (int)m, (int)n1, s, stats, fw, win,
                       (int)p.chunks, part_loss, l2sum, part_grad);
    URE_HIP(hipGetLastError());
    return 0;
}

static int quarter(int v) { return v <= 16 ? 1 : v <= 32 ? 2 : v <= 64 ? 4 : 8; }

}  // namespace ure

using namespace ure;

extern "C" {

int64_t ure_attack_scratch(int64_t m, int32_t d, int32_t H, int32_t folds)
{
    if (!atk_shape_ok(m, d, H, folds)) return -1;
    return atk_plan(m, atk_shape(d, H), folds).bytes;
}

int ure_attack_standardize(const float *X, int64_t ld, int32_t d, const int32_t *rows, const int32_t *fold_of, int64_t m, int32_t folds, float *stats,
                           void *stream)
{
    URE_ARG(X && rows && fold_of && stats);
    URE_ARG(atk_shape_ok(m, d, 0, folds));
    URE_ARG(ld >= d);
    attack_stats_kernel<<<d, kBlock, 0, static_cast<hipStream_t>(stream)>>>(X, ld, rows, fold_of, m, folds, d, stats);
    URE_HIP(hipGetLastError());
    return 0;
}

int ure_attack_train(const float *X, int64_t ld, int32_t d, const int32_t *rows, const int32_t *fold_of, int64_t m, int64_t n1, int32_t folds, int32_t H,
                     const float *stats, const float *fw, const float *sc, int32_t epochs, float beta1, float beta2, float eps, float l2,
                     const float *params0, float *params, double *loss, void *scratch, int64_t scratch_bytes, void *stream)
{
    URE_ARG(X && rows && fold_of && stats && fw && sc && params0 && params && loss);
    URE_ARG(atk_shape_ok(m, d, H, folds));
    URE_ARG(ld >= d && n1 >= 1 && n1 < m && epochs >= 1);
    URE_ARG(beta1 >= 0.0f && beta1 < 1.0f && beta2 >= 0.0f && beta2 < 1.0f && eps > 0.0f && l2 >= 0.0f);
    const AtkShape s = atk_shape(d, H);
    const AtkPlan p = atk_plan(m, s, folds);
    URE_ARG(scratch && scratch_bytes >= p.bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    char *base = static_cast<char *>(scratch);
    double *part_loss = reinterpret_cast<double *>(base), *l2sum = reinterpret_cast<double *>(base + p.off_l2);
    float *part_grad = reinterpret_cast<float *>(base + p.off_grad), *mom = reinterpret_cast<float *>(base + p.off_mom),
          *var = reinterpret_cast<float *>(base + p.off_var);
    const int hq = quarter(s.He), dq = quarter(d);
    const dim3 ugrid((unsigned)((s.P + kBlock - 1) / kBlock), (unsigned)folds);
    for (int e = 0; e < epochs; ++e) {
        const float *win = e == 0 ? params0 : params;
        int rc = -1;
#define URE_ATK(HQ, DQ) \
    if (hq == HQ && dq == DQ) rc = launch_train<HQ, DQ>(X, ld, rows, fold_of, m, n1, folds, s, stats, fw, win, p, part_loss, l2sum, part_grad, e == 0, st)
        URE_ATK(1, 1); URE_ATK(1, 2); URE_ATK(1, 4); URE_ATK(1, 8);
        URE_ATK(2, 1); URE_ATK(2, 2); URE_ATK(2, 4); URE_ATK(2, 8);
        URE_ATK(4, 1); URE_ATK(4, 2); URE_ATK(4, 4); URE_ATK(4, 8);
        URE_ATK(8, 1); URE_ATK(8, 2); URE_ATK(8, 4); URE_ATK(8, 8);
#undef URE_ATK
        if (rc) return rc;
        attack_update_kernel<<<ugrid, kBlock, 0, st>>>(s, (int)p.chunks, part_grad, part_loss, l2sum, fw, sc, e, epochs, beta1, beta2, eps, l2, win, params,
                                                       mom, var, loss);
        URE_HIP(hipGetLastError());
    }
    return 0;
}

int ure_attack_score(const float *X, int64_t ld, int32_t d, const int32_t *rows, const int32_t *fold_of, int64_t m, int32_t folds, int32_t H,
                     const float *stats, const float *params, float *scores, void *stream)
{
    URE_ARG(X && rows && stats && params && scores);
    URE_ARG(probe_shape_ok(m, d, H, folds, 1, 1, INT32_MAX));
    URE_ARG(ld >= d);
    const unsigned blocks = (unsigned)std::min<int64_t>((m + kWavesPerBlock - 1) / kWavesPerBlock, 8192);
    attack_score_kernel<<<blocks, kBlock, 0, static_cast<hipStream_t>(stream)>>>(X, ld, rows, fold_of, m, folds, atk_shape(d, H), stats, params, scores);
    URE_HIP(hipGetLastError());
    return 0;
}

int64_t ure_auc_scratch(int64_t n1, int64_t n2)
{
    if (!auc_shape_ok(n1, n2)) return -1;
    return auc_plan(n1, n2).bytes;
}

int ure_auc_counts(const float *scores, const int32_t *pos, int64_t n1, const int32_t *neg, int64_t n2, int64_t *counts, int32_t *nan_flag, void *scratch,
                   int64_t scratch_bytes, void *stream)
{
    URE_ARG(scores && pos && neg && counts && nan_flag);
    URE_ARG(auc_shape_ok(n1, n2));
    const AucPlan p = auc_plan(n1, n2);
    URE_ARG(scratch && scratch_bytes >= p.bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    int64_t *part = static_cast<int64_t *>(scratch);
    int32_t *flags = reinterpret_cast<int32_t *>(static_cast<char *>(scratch) + p.off_flags);
    auc_tile_kernel<<<dim3((unsigned)p.pos_tiles, (unsigned)p.split), kBlock, 0, st>>>(scores, pos, n1, neg, n2, p.neg_tiles, part, flags);
    URE_HIP(hipGetLastError());
    auc_sum_kernel<<<1, kBlock, 0, st>>>(part, flags, p.n_part, counts, nan_flag);
    URE_HIP(hipGetLastError());
    return 0;
}

int ure_confusion_counts(const float *scores, const int32_t *pos, int64_t n1, const int32_t *neg, int64_t n2, float thr, int64_t *counts, void *stream)
{
    URE_ARG(scores && pos && neg && counts);
    URE_ARG(auc_shape_ok(n1, n2));
    URE_ARG(thr == thr);
    confusion_kernel<<<1, kBlock, 0, static_cast<hipStream_t>(stream)>>>(scores, pos, n1, neg, n2, thr, counts);
    URE_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"

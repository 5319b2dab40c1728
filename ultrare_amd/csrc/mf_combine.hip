// mf_combine.hip -- the learned shard combiner for gfx950: the sufficient statistics of a generalised linear model over the S
// shard scores of every training pair in ONE pass (ure_combine_stats), and the scoring of pairs with fitted weights
// (ure_score_weighted).  Replaces nothing of the reference: method/utils.py:140-145 takes the plain mean of the shard scores;
// this is the opt-in alternative.  The Newton solve of at most 33 unknowns stays on the host.
//
// The contract, all in float64 unless said otherwise, for a pair j = (u, i, r):
//   p[j,s]  model s's float32 score, bit for bit ure_score's for that model alone (score_dot.h), x[j] = (p[j,0..S-1], 1)
//   z[j]    b + sum_s w[s] * (double)p[j,s], accumulated in the order b, s = 0, 1, ...  NOT contracted: every product is
//           rounded before it is added (the library is built with -ffp-contract=off), in both kernels of this file
//   link 0  mu = z, h = 1, loss = (mu - r)^2 / 2           link 1  mu = 1 / (1 + exp(-z)), h = mu (1 - mu),
//                                                                   loss = max(z, 0) + log1p(exp(-|z|)) - r z
//   stats   out = { n, sum loss, g = sum (mu - r) x  [S + 1], H = sum h x x^T  upper triangle, row-major [(S+1)(S+2)/2] }
//
// ure_combine_stats is two launches:
//   combine_stats_kernel   a workgroup takes tiles of kCbTile pairs (tile t of workgroup b: b + t * gridDim.x).  Phase A: the
//                          four waves gather the rows and leave the tile's x in LDS (the n x S score matrix is never written
//                          to memory: 2.9 GB at 22.5 M pairs x 32 models).  Phase B: one thread per pair forms z, mu, h and
//                          the loss.  Phase C: every thread OWNS up to kCbOwn of the 1 + (S+1) + (S+1)(S+2)/2 sums (595 at
//                          S = 32) in registers and walks the tile in pair order.  The workgroup's sums go to scratch.
//   combine_reduce_kernel  one workgroup per sum adds the workgroups' partials: thread t those of workgroups t, t + 256, ...
//                          in turn, then a fixed tree.
// No floating-point atomics; the order of every addition depends on (n, S) alone, so two calls give the same bytes.
#include "score_dot.h"

#include <cmath>

namespace ure {

constexpr int kCbTile = 64;              // pairs per tile: x takes 64 * 33 * 8 = 16.5 KiB of LDS at S = 32
constexpr int kCbMaxBlocks = 2048;       // workgroups (= partial vectors in scratch)
constexpr int kCbMaxX = URE_MAX_MODELS_PER_CALL + 1;
constexpr int kCbOwn = 3;                // sums per thread: 595 <= 3 * 256

static inline int64_t cb_len(int S) { return 2 + (int64_t)(S + 1) + (int64_t)(S + 1) * (S + 2) / 2; }
static inline int64_t cb_blocks(int64_t n) { return std::min<int64_t>((n + kCbTile - 1) / kCbTile, kCbMaxBlocks); }

template <int LPR>
__global__ __launch_bounds__(kBlock) void combine_stats_kernel(TableList T, int S, const int32_t *__restrict__ uid,
                                                               const int32_t *__restrict__ iid, const float *__restrict__ rating,
                                                               int64_t n, int link, const double *__restrict__ w,
                                                               double *__restrict__ partial, int len)
{
    constexpr int D = LPR * 4;
    constexpr int G = kWave / LPR;
    __shared__ double xs[kCbTile * kCbMaxX];
    __shared__ double cs[3 * kCbTile];            // per pair: loss | mu - r | h
    __shared__ double ws[kCbMaxX];
    const int X = S + 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = lane & (LPR - 1), grp = lane / LPR;

    // the sums this thread owns: e = 1 the loss, e = 2 .. S + 2 the gradient, then H's upper triangle row by row; each is
    // sum over pairs of (c * x[a]) * x[b] with c = loss | mu - r | h and x[S] = 1
    int ea[kCbOwn], eb[kCbOwn], ec[kCbOwn];
    double acc[kCbOwn];
    int n_own = 0;
#pragma unroll
    for (int k = 0; k < kCbOwn; ++k) {
        const int e = 1 + tid + k * kBlock;
        acc[k] = 0.0;
        ea[k] = eb[k] = S;
        ec[k] = 0;
        if (e < len) n_own = k + 1;
        if (e >= 2 && e < 2 + X) {
            ec[k] = 1;
            ea[k] = e - 2;
        } else if (e >= 2 + X && e < len) {
            int r = e - 2 - X, a = 0;
            while (r >= X - a) { r -= X - a; ++a; }
            ec[k] = 2;
            ea[k] = a;
            eb[k] = a + r;
        }
    }
    if (tid < X) ws[tid] = w[tid];

    const int64_t n_tiles = (n + kCbTile - 1) / kCbTile;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t j0 = tile * kCbTile;
        const int cnt = (int)min<int64_t>(kCbTile, n - j0);
        // ---- phase A: the tile's scores (a wave's trip count does not depend on the lane: the butterfly needs every lane)
        for (int t = wave * G + grp; t < kCbTile; t += kWavesPerBlock * G) {
            const bool act = t < cnt;
            const int u = act ? uid[j0 + t] : 0, i = act ? iid[j0 + t] : 0;
            for (int m0 = 0; m0 < S; m0 += 4) {
                float4 a[4], b[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    a[k] = make_float4(0.f, 0.f, 0.f, 0.f);
                    b[k] = a[k];
                    if (m0 + k < S) {
                        a[k] = *reinterpret_cast<const float4 *>(T.U[m0 + k] + (size_t)u * D + sub * 4);
                        b[k] = *reinterpret_cast<const float4 *>(T.V[m0 + k] + (size_t)i * D + sub * 4);
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float p = 0.f;                          // ure_score with first = 1: the running sum starts at zero
                    p += pair_dot<LPR>(a[k], b[k]);
                    if (sub == 0 && m0 + k < S) xs[t * X + m0 + k] = (double)p;
                }
            }
            if (sub == 0) xs[t * X + S] = 1.0;
        }
        __syncthreads();
        // ---- phase B: one thread per pair
        if (tid < cnt) {
            const double *x = xs + tid * X;
            double z = ws[S];
            for (int s = 0; s < S; ++s) z = z + ws[s] * x[s];
            const double r = (double)rating[j0 + tid];
            const double mu = link_mean(link, z);
            double h = 1.0, loss;
            if (link == 0) {
                loss = (mu - r) * (mu - r) * 0.5;
            } else {
                h = mu * (1.0 - mu);
                loss = fmax(z, 0.0) + log1p(exp(-fabs(z))) - r * z;
            }
            cs[tid] = loss;
            cs[kCbTile + tid] = mu - r;
            cs[2 * kCbTile + tid] = h;
        }
        __syncthreads();
        // ---- phase C: every sum takes the tile's pairs in order
        if (n_own > 0) {
            for (int t = 0; t < cnt; ++t) {
                const double *x = xs + t * X;
#pragma unroll
                for (int k = 0; k < kCbOwn; ++k)
                    if (k < n_own) acc[k] += (cs[ec[k] * kCbTile + t] * x[ea[k]]) * x[eb[k]];
            }
        }
        __syncthreads();
    }
    double *mine = partial + (size_t)blockIdx.x * len;
#pragma unroll
    for (int k = 0; k < kCbOwn; ++k)
        if (k < n_own) mine[1 + tid + k * kBlock] = acc[k];
}

// out[e] = the sum over the B workgroups of partial[b][e], e = blockIdx.x + 1; out[0] = n.
__global__ __launch_bounds__(kBlock) void combine_reduce_kernel(const double *__restrict__ partial, int B, int len, int64_t n,
                                                                double *__restrict__ out)
{
    __shared__ double s[kBlock];
    const int e = blockIdx.x + 1;
    double a = 0.0;
    for (int b = threadIdx.x; b < B; b += kBlock) a += partial[(size_t)b * len + e];
    s[threadIdx.x] = a;
    __syncthreads();
#pragma unroll
    for (int o = kBlock / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[e] = s[0];
        if (e == 1) out[0] = (double)n;
    }
}

// pred[j] = (float)link(z[j]) with the weight row of the user's group, and squared-error partials laid out as ure_score's (one
// per workgroup, at most URE_SCORE_PARTIALS, the rest zeroed), so ure_eval_users / ure_eval_reduce run on the result unchanged.
// (z carried in registers beside the dot by every lane group, score_kernel's loop: 71-73 ms at 22.5 M pairs x 32 models, d = 128,
// where this form takes 48 and score_kernel's mean 62-64.)
template <int LPR>
__global__ __launch_bounds__(kBlock) void score_weighted_kernel(TableList T, int S, const int32_t *__restrict__ uid,
                                                                const int32_t *__restrict__ iid, const float *__restrict__ rating,
                                                                int64_t n, int link, const double *__restrict__ W, int n_groups,
                                                                const int32_t *__restrict__ group_of_user, int n_user,
                                                                float *__restrict__ pred, double *__restrict__ sse)
{
    constexpr int D = LPR * 4;
    constexpr int G = kWave / LPR;
    // combine_stats_kernel's phases A and B: the tile's float32 scores through LDS, then one thread per pair carries z
    __shared__ float ps[kCbTile * kCbMaxX];       // row stride S + 1
    const int X = S + 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = lane & (LPR - 1), grp = lane / LPR;
    const double w_mean = 1.0 / (double)S;
    float sq = 0.f;
    const int64_t n_tiles = (n + kCbTile - 1) / kCbTile;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t j0 = tile * kCbTile;
        const int cnt = (int)min<int64_t>(kCbTile, n - j0);
        for (int t = wave * G + grp; t < kCbTile; t += kWavesPerBlock * G) {
            const bool act = t < cnt;
            const int u = act ? uid[j0 + t] : 0, i = act ? iid[j0 + t] : 0;
            for (int m0 = 0; m0 < S; m0 += 4) {
                float4 a[4], b[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    a[k] = make_float4(0.f, 0.f, 0.f, 0.f);
                    b[k] = a[k];
                    if (m0 + k < S) {
                        a[k] = *reinterpret_cast<const float4 *>(T.U[m0 + k] + (size_t)u * D + sub * 4);
                        b[k] = *reinterpret_cast<const float4 *>(T.V[m0 + k] + (size_t)i * D + sub * 4);
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float p = 0.f;
                    p += pair_dot<LPR>(a[k], b[k]);
                    if (sub == 0 && m0 + k < S) ps[t * X + m0 + k] = p;
                }
            }
        }
        __syncthreads();
        if (tid < cnt) {
            const int64_t j = j0 + tid;
            const int u = uid[j];
            int g = 0;
            if (group_of_user) g = (u >= 0 && u < n_user) ? group_of_user[u] : -1;
            const bool outside = g < 0 || g >= n_groups;     // in no group: the mean ensemble (link 0)
            const double *wr = W + (size_t)(outside ? 0 : g) * X;
            const float *x = ps + tid * X;
            double z = outside ? 0.0 : wr[S];
            for (int s = 0; s < S; ++s) z = z + (outside ? w_mean : wr[s]) * (double)x[s];
            double mu = link_mean(link, z);
            if (link != 0 && outside) mu = __builtin_nan("");    // (the host refuses such a map before the launch)
            const float out = (float)mu;
            if (sse) {
                const float e = out - rating[j];
                sq = fmaf(e, e, sq);
            }
            pred[j] = out;
        }
        __syncthreads();
    }
    if (sse) sq_partials(sq, sse);
}

}  // namespace ure

using namespace ure;

extern "C" {

int64_t ure_combine_stats_len(int n_models)
{
    if (n_models < 1 || n_models > URE_MAX_MODELS_PER_CALL) return -1;
    return cb_len(n_models);
}

int64_t ure_combine_stats_scratch(int64_t n, int n_models)
{
    if (n < 1 || n_models < 1 || n_models > URE_MAX_MODELS_PER_CALL) return -1;
    return cb_blocks(n) * cb_len(n_models) * (int64_t)sizeof(double);
}

int ure_combine_stats(const float *const *U_tables, const float *const *V_tables, int n_models, const int32_t *uid, const int32_t *iid,
                      const float *rating, int64_t n, int d, int link, const double *w, double *out, void *scratch, int64_t scratch_bytes,
                      void *stream)
{
    URE_ARG(U_tables && V_tables);
    URE_ARG(n_models >= 1 && n_models <= URE_MAX_MODELS_PER_CALL);
    URE_ARG(uid && iid && rating);
    URE_ARG(n >= 1);
    URE_ARG(pow2(d) && d >= 4 && d <= 256);
    URE_ARG(link == 0 || link == 1);
    URE_ARG(w && out && scratch);
    URE_ARG(scratch_bytes >= ure_combine_stats_scratch(n, n_models));
    TableList T;
    if (int rc = fill_tables(T, U_tables, V_tables, n_models)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int len = (int)cb_len(n_models);
    const unsigned blocks = (unsigned)cb_blocks(n);
    double *partial = static_cast<double *>(scratch);
    const bool known = dispatch_group_width(d / 4, [&](auto W) {
        hipLaunchKernelGGL(combine_stats_kernel<decltype(W)::value>, dim3(blocks), dim3(kBlock), 0, st, T, n_models, uid, iid, rating, n, link, w,
                           partial, len);
    });
    if (!known) return fail(-1, "ure_combine_stats: unsupported d=%d", d);
    hipLaunchKernelGGL(combine_reduce_kernel, dim3((unsigned)(len - 1)), dim3(kBlock), 0, st, (const double *)partial, (int)blocks, len, n, out);
    URE_HIP(hipGetLastError());
    return 0;
}

int ure_score_weighted(const float *const *U_tables, const float *const *V_tables, int n_models, const int32_t *uid, const int32_t *iid,
                       const float *rating, int64_t n, int d, int link, const double *W, int n_groups, const int32_t *group_of_user,
                       int32_t n_user, float *pred, double *sse, void *stream)
{
    URE_ARG(U_tables && V_tables);
    URE_ARG(n_models >= 1 && n_models <= URE_MAX_MODELS_PER_CALL);
    URE_ARG(uid && iid && pred && (!sse || rating));
    URE_ARG(n >= 1);
    URE_ARG(pow2(d) && d >= 4 && d <= 256);
    URE_ARG(link == 0 || link == 1);
    URE_ARG(W);
    URE_ARG(n_groups >= 1);
    URE_ARG(!group_of_user || n_user >= 1);
    TableList T;
    if (int rc = fill_tables(T, U_tables, V_tables, n_models)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned blocks = (unsigned)std::min<int64_t>((n + kCbTile - 1) / kCbTile, URE_SCORE_PARTIALS);
    const bool known = dispatch_group_width(d / 4, [&](auto lpr) {
        hipLaunchKernelGGL(score_weighted_kernel<decltype(lpr)::value>, dim3(blocks), dim3(kBlock), 0, st, T, n_models, uid, iid, rating, n, link,
                           W, n_groups, group_of_user, n_user, pred, sse);
    });
    if (!known) return fail(-1, "ure_score_weighted: unsupported d=%d", d);
    URE_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"

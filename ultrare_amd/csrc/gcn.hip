// gcn.hip -- the LightGCN backbone (include/ultrare_gcn.h; the contract is ultrare_amd/lightgcn.py): propagation over a shard's
// CSR / CSC, the masked loss-gradient walks, the residual pass and the SGD update.
//
// One shape serves the propagate and the two gradient walks: a group of G = d / 4 lanes owns an output row and holds its d
// columns as one float4 per lane (1 lane at d = 4, a whole wavefront at d = 256); the row's entries are fetched a tile of G at
// a time, one per lane, and handed round with group_read (csr_lanes.h); the chain of a (row, column) is one lane's, in
// ascending entry position.  Every float operation is a rounded one of its own (gcn_ops.h).  The gradient walk's loop, its row
// ownership and its order are row_walk.h's; gcn_grad_kernel states what a fetch reads and what a term adds.  The propagate keeps
// a loop of its own (the next tile's entries travel while this one is added, four rows in flight).
#include "gcn_ops.h"

namespace ure {
namespace {

// out[r] = [add[r] +] s_dst[r] * sum_j s_src[j] X[j] over row r's entries.  Lane `sub` fetches entry p0 + sub AND that
// neighbour's s, so the dependent reads of a tile are in flight together, and the next tile's travel while this one is added;
// a full tile requests four neighbour rows at a time (csr_row_walk's shape).  Groups narrower than four lanes (d = 4, 8) read
// their indices themselves, four entries at a time, so that they too have four rows in flight.
template <int G>
__global__ __launch_bounds__(kBlock) void gcn_propagate_kernel(const int64_t *__restrict__ off, const int32_t *__restrict__ idx, int64_t n_dst,
                                                               int64_t n_src, const float *__restrict__ s_src, const float *__restrict__ s_dst,
                                                               const float *__restrict__ X, const float *add, float *sum, float *out)
{
    constexpr int kRows = kBlock / G, D = 4 * G;
    const int sub = threadIdx.x % G;
    const int64_t r = (int64_t)blockIdx.x * kRows + threadIdx.x / G;
    if (r >= n_dst) return;                                // whole groups leave together
    const int64_t b = ldg(off + r), e = ldg(off + r + 1);
    const unsigned last = (unsigned)(n_src - 1);
    const float *__restrict__ x = X + 4 * sub;
    float4 t = f4_zero();
    if (G >= 4) {
        unsigned next_j = 0u;
        float next_s = 0.f;
        if (b + sub < e) {
            next_j = min((unsigned)ldg(idx + b + sub), last);
            next_s = ldg(s_src + next_j);
        }
        for (int64_t p0 = b; p0 < e; p0 += G) {
            const unsigned mine_j = next_j;
            const float mine_s = next_s;
            const int64_t q = p0 + G + sub;
            if (q < e) {
                next_j = min((unsigned)ldg(idx + q), last);
                next_s = ldg(s_src + next_j);
            }
            const int m = (int)min<int64_t>(G, e - p0);
            if (m == G) {
#pragma unroll
                for (int u = 0; u < G; u += 4) {
                    float4 xv[4];
                    float sv[4];
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        const unsigned j = group_read<G>(mine_j, u + w);
                        sv[w] = group_read<G>(mine_s, u + w);
                        xv[w] = ldg_f4(x + (size_t)j * D);
                    }
#pragma unroll
                    for (int w = 0; w < 4; ++w) t = f4_mul_add(t, sv[w], xv[w]);
                }
            } else {
                for (int u = 0; u < m; ++u) {
                    const unsigned j = group_read<G>(mine_j, u);
                    const float sv = group_read<G>(mine_s, u);
                    t = f4_mul_add(t, sv, ldg_f4(x + (size_t)j * D));
                }
            }
        }
    } else {
        for (int64_t p0 = b; p0 < e; p0 += 4) {
            const int m = (int)min<int64_t>(4, e - p0);
            float4 xv[4];
            float sv[4];
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                if (w < m) {
                    const unsigned j = min((unsigned)ldg(idx + p0 + w), last);
                    sv[w] = ldg(s_src + j);
                    xv[w] = ldg_f4(x + (size_t)j * D);
                }
            }
#pragma unroll
            for (int w = 0; w < 4; ++w)
                if (w < m) t = f4_mul_add(t, sv[w], xv[w]);
        }
    }
    const size_t at = (size_t)r * D + 4 * sub;
    float4 y = f4_scale(ldg(s_dst + r), t);
    if (add) y = f4_add(ldg_f4(add + at), y);              // (out may be add: read before the store below)
    stg_f4(out + at, y);
    if (sum) stg_f4(sum + at, f4_add(ldg_f4(sum + at), y));
}

// G[r] = sum over row r's entries in the batch of (2 err) T[idx].  A fetch reads the entry's tag and -- for an entry of the
// batch -- its residual and its index, so only an entry of the batch costs a row of T.  The row's float64 loss chain rides along
// in every lane (lane 0 stores it).
template <int G, bool MAPPED>
__global__ __launch_bounds__(kBlock) void gcn_grad_kernel(const int64_t *__restrict__ off, const int32_t *__restrict__ idx, const int32_t *__restrict__ map,
                                                          const int32_t *__restrict__ tag, const float *__restrict__ err, int64_t n_dst, int64_t n_src,
                                                          int64_t nnz, int step, const float *__restrict__ T, float *__restrict__ Gout,
                                                          double *__restrict__ row_loss)
{
    constexpr int D = 4 * G;
    const RowLanes<G> L;
    if (L.past(n_dst)) return;
    const unsigned last = (unsigned)(n_src - 1), last_pos = (unsigned)(nnz - 1);
    const float *__restrict__ x = T + 4 * L.sub;
    float4 g = f4_zero();
    double loss = 0.0;
    struct Entry { unsigned j; float e; bool in; };
    tile_walk<G>(
        ldg(off + L.r), ldg(off + L.r + 1), L.sub,
        [&](int64_t k, bool inside) {
            Entry mine{0u, 0.f, false};
            if (inside) {
                const unsigned q = entry_pos<MAPPED>(map, k, last_pos);
                mine.in = ldg(tag + q) == step;
                if (mine.in) {
                    mine.e = ldg(err + q);
                    mine.j = min((unsigned)ldg(idx + k), last);
                }
            }
            return mine;
        },
        [&](const Entry &mine, int u) {
            if (!group_read<G>((int)mine.in, u)) return;
            const unsigned j = group_read<G>(mine.j, u);
            const float ee = group_read<G>(mine.e, u);
            g = f4_mul_add(g, __fmul_rn(2.f, ee), ldg_f4(x + (size_t)j * D));
            loss += (double)ee * (double)ee;
        });
    stg_f4(Gout + (size_t)L.r * D + 4 * L.sub, g);
    if (row_loss && L.sub == 0) stg(row_loss + L.r, loss);
}

// The residual pass: a group of LPR = d / 4 lanes per CSR entry, the dot of score_dot.h.  Every lane of a wave takes part in
// every dot (an entry outside the batch, or past the end, multiplies zeros), so the butterfly never meets an idle lane.
template <int LPR>
__global__ __launch_bounds__(kBlock) void gcn_residual_kernel(const int32_t *__restrict__ row, const int32_t *__restrict__ col,
                                                              const float *__restrict__ rating, const int32_t *__restrict__ tag, int64_t nnz, int step,
                                                              const float *__restrict__ U, const float *__restrict__ V, int64_t n_user, int64_t n_item,
                                                              float *__restrict__ err, float *__restrict__ pred_out)
{
    const PairLanes<LPR> L;
    const unsigned last_u = (unsigned)(n_user - 1), last_i = (unsigned)(n_item - 1);
    for (int64_t base = L.wave_id * L.G; base < nnz; base += L.n_waves * L.G) {
        const int64_t k = base + L.grp;
        const bool in = k < nnz && ldg(tag + k) == step;
        float4 a = f4_zero(), c = f4_zero();
        if (in) {
            a = ldg_f4(U + (size_t)min((unsigned)ldg(row + k), last_u) * L.D + 4 * L.sub);
            c = ldg_f4(V + (size_t)min((unsigned)ldg(col + k), last_i) * L.D + 4 * L.sub);
        }
        const float pred = pair_dot<LPR>(a, c);
        if (k < nnz && L.sub == 0) {
            stg(err + k, in ? __fsub_rn(pred, ldg(rating + k)) : 0.f);
            if (pred_out) stg(pred_out + k, in ? pred : 0.f);
        }
    }
}

__global__ __launch_bounds__(kBlock) void gcn_gather_tags_kernel(const int32_t *__restrict__ file_tag, const int32_t *__restrict__ pos, int64_t nnz,
                                                                 int32_t *__restrict__ tag)
{
    const unsigned last = (unsigned)(nnz - 1);
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < nnz; k += (int64_t)gridDim.x * kBlock)
        stg(tag + k, ldg(file_tag + min((unsigned)ldg(pos + k), last)));
}

__global__ __launch_bounds__(kBlock) void gcn_scale_kernel(const float *X, int64_t n4, float c, float *out)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kBlock)
        stg_f4(out + 4 * i, f4_scale(c, ldg_f4(X + 4 * i)));
}

__device__ __forceinline__ float sgd_one(float &w, float m, float g, float gscale, float lr, float lam, float mu, bool first)
{
    const float g1 = __fadd_rn(__fmul_rn(g, gscale), __fmul_rn(lam, w));
    m = first ? g1 : __fadd_rn(__fmul_rn(mu, m), g1);
    w = __fsub_rn(w, __fmul_rn(lr, m));
    return m;
}

__global__ __launch_bounds__(kBlock) void gcn_sgd_kernel(float *__restrict__ w, float *__restrict__ m, const float *__restrict__ g, int64_t n4,
                                                         float gscale, float lr, float lam, float mu, int first)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kBlock) {
        float4 wv = ldg_f4(w + 4 * i), mv = first ? f4_zero() : ldg_f4(m + 4 * i);
        const float4 gv = ldg_f4(g + 4 * i);
        mv.x = sgd_one(wv.x, mv.x, gv.x, gscale, lr, lam, mu, first);
        mv.y = sgd_one(wv.y, mv.y, gv.y, gscale, lr, lam, mu, first);
        mv.z = sgd_one(wv.z, mv.z, gv.z, gscale, lr, lam, mu, first);
        mv.w = sgd_one(wv.w, mv.w, gv.w, gscale, lr, lam, mu, first);
        stg_f4(w + 4 * i, wv);
        stg_f4(m + 4 * i, mv);
    }
}

// epoch_sse_kernel's order (job_io.hip) over float64 row sums, one workgroup.
__global__ __launch_bounds__(256) void gcn_step_loss_kernel(const double *__restrict__ row_loss, int64_t n, int first, double *loss)
{
    __shared__ double part[256];
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) acc += ldg(row_loss + i);
    const double s = fold_256(acc, part);
    if (threadIdx.x == 0) loss[0] = (first ? 0.0 : loss[0]) + s;
}

}  // namespace
}  // namespace ure

using namespace ure;

extern "C" int ure_gcn_propagate(const int64_t *off, const int32_t *idx, int64_t n_dst, int64_t n_src, const float *s_src, const float *s_dst,
                                 const float *X, int32_t d, const float *add, float *sum, float *out, void *stream)
{
    URE_GCN_SIZES(n_dst, n_src, d);
    URE_ARG(off && idx && s_src && s_dst && X && out);
    const int64_t nb_dst = n_dst * d * 4, nb_src = n_src * d * 4;
    URE_ARG(apart(out, nb_dst, X, nb_src));
    URE_ARG(!add || add == out || apart(add, nb_dst, out, nb_dst));
    URE_ARG(!sum || (apart(sum, nb_dst, out, nb_dst) && apart(sum, nb_dst, X, nb_src) && (!add || apart(sum, nb_dst, add, nb_dst))));
    hipStream_t st = (hipStream_t)stream;
    dispatch_group_width(d / 4, [&](auto w) {
        constexpr int G = decltype(w)::value;
        hipLaunchKernelGGL(gcn_propagate_kernel<G>, dim3(group_blocks(n_dst, G)), dim3(kBlock), 0, st, off, idx, n_dst, n_src, s_src, s_dst, X, add,
                           sum, out);
    });
    URE_HIP(hipGetLastError());
    return 0;
}

extern "C" int ure_gcn_scale(const float *X, int64_t n, float c, float *out, void *stream)
{
    URE_ARG(X && out && n >= 4 && n % 4 == 0);
    URE_ARG(X == out || apart(X, n * 4, out, n * 4));
    hipLaunchKernelGGL(gcn_scale_kernel, dim3(stream_blocks(n / 4)), dim3(kBlock), 0, (hipStream_t)stream, X, n / 4, c, out);
    URE_HIP(hipGetLastError());
    return 0;
}

extern "C" int ure_gcn_gather_tags(const int32_t *file_tag, const int32_t *pos, int64_t nnz, int32_t *tag, void *stream)
{
    URE_ARG(file_tag && pos && tag && nnz >= 1 && nnz <= INT32_MAX);
    URE_ARG(apart(tag, nnz * 4, file_tag, nnz * 4) && apart(tag, nnz * 4, pos, nnz * 4));
    hipLaunchKernelGGL(gcn_gather_tags_kernel, dim3(stream_blocks(nnz)), dim3(kBlock), 0, (hipStream_t)stream, file_tag, pos, nnz, tag);
    URE_HIP(hipGetLastError());
    return 0;
}

extern "C" int ure_gcn_residual(const int32_t *row, const int32_t *col, const float *rating, const int32_t *tag, int64_t nnz, int32_t step,
                                const float *U, const float *V, int64_t n_user, int64_t n_item, int32_t d, float *err, float *pred_out, void *stream)
{
    URE_GCN_SIZES(n_user, n_item, d);
    URE_ARG(row && col && rating && tag && U && V && err);
    URE_ARG(nnz >= 1 && nnz <= INT32_MAX && step >= 0);
    hipStream_t st = (hipStream_t)stream;
    dispatch_group_width(d / 4, [&](auto w) {
        constexpr int LPR = decltype(w)::value;
        hipLaunchKernelGGL(gcn_residual_kernel<LPR>, dim3(pair_blocks(nnz, kWave / LPR, 4096)), dim3(kBlock), 0, st, row, col, rating, tag, nnz,
                           (int)step, U, V, n_user, n_item, err, pred_out);
    });
    URE_HIP(hipGetLastError());
    return 0;
}

extern "C" int ure_gcn_grad(const int64_t *off, const int32_t *idx, const int32_t *map, const int32_t *tag, const float *err, int64_t n_dst,
                            int64_t n_src, int64_t nnz, int32_t step, const float *T, int32_t d, float *G_out, double *row_loss, void *stream)
{
    URE_GCN_SIZES(n_dst, n_src, d);
    URE_ARG(off && idx && tag && err && T && G_out);
    URE_ARG(nnz >= 1 && nnz <= INT32_MAX && step >= 0);
    URE_ARG(apart(G_out, n_dst * d * 4, T, n_src * d * 4));
    hipStream_t st = (hipStream_t)stream;
    dispatch_group_width(d / 4, [&](auto w) {
        constexpr int G = decltype(w)::value;
        launch_by_map(map, gcn_grad_kernel<G, true>, gcn_grad_kernel<G, false>, n_dst, G, st, off, idx, map, tag, err, n_dst, n_src, nnz, (int)step, T,
                      G_out, row_loss);
    });
    URE_HIP(hipGetLastError());
    return 0;
}

extern "C" int ure_gcn_step_loss(const double *row_loss, int64_t n, int32_t first, double *loss, void *stream)
{
    URE_ARG(row_loss && loss && n >= 1 && n <= INT32_MAX);
    URE_ARG(apart(loss, 8, row_loss, n * 8));
    hipLaunchKernelGGL(gcn_step_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, row_loss, n, (int)first, loss);
    URE_HIP(hipGetLastError());
    return 0;
}

extern "C" int ure_gcn_sgd_step(float *w, float *m, const float *g, int64_t n, float gscale, float lr, float lam, float mu, int32_t first,
                                void *stream)
{
    URE_ARG(w && m && g && n >= 4 && n % 4 == 0);
    URE_ARG(apart(w, n * 4, m, n * 4) && apart(w, n * 4, g, n * 4) && apart(m, n * 4, g, n * 4));
    hipLaunchKernelGGL(gcn_sgd_kernel, dim3(stream_blocks(n / 4)), dim3(kBlock), 0, (hipStream_t)stream, w, m, g, n / 4, gscale, lr, lam, mu,
                       (int)first);
    URE_HIP(hipGetLastError());
    return 0;
}

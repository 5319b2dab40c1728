// nmf.hip -- the NeuMF backbone (include/ultrare_nmf.h; the contract is ultrare_amd/nmf.py): the per-sample forward and backward
// through GMF, MLP and head, the weight-gradient sums over a step's slots, the masked row sums of the embedding gradients (the
// walk is row_walk.h's; nmf_row_sum_kernel states what a fetch reads and what a term adds) and the scoring pass.
//
// The MLP runs on the VALU (f32 MFMA issues at the vector rate on gfx950 and its summation order cannot be stated).  One
// wavefront owns a sample: lane o holds the chain of output o of a layer (forward) or of input i (backward), the activations
// of the sample sit in the wave's own piece of LDS and are read as broadcasts.  The weights of the stack are staged once per
// workgroup in LDS, layer j as Wt[i][o] with a row pitch of L_(j+1) + 1 floats: the forward's lanes read consecutive o of one
// i, the backward's lanes consecutive i of one o at an odd pitch -- neither collides on a bank.  Every float operation is a
// rounded one of its own (gcn_ops.h).
#include "nmf_shape.h"

namespace ure {
namespace {

// The forward of one pair by one wave: av [A] receives [g | a_0 | .. | a_m]; every lane returns pred.
__device__ __forceinline__ float nmf_forward(const NmfShape &S, const float *wl, float *av, const float *__restrict__ urow,
                                             const float *__restrict__ vrow, int lane)
{
    const int k = S.k, e = S.e;
    for (int c = lane; c < k; c += kWave) av[c] = __fmul_rn(ldg(urow + c), ldg(vrow + c));
    for (int c = lane; c < e; c += kWave) {
        av[k + c] = ldg(urow + k + c);
        av[k + e + c] = ldg(vrow + k + c);
    }
    wave_sync();
    for (int j = 0; j < S.m; ++j) {
        const int Lin = S.L[j], Lout = S.L[j + 1], ld = Lout + 1;
        const float *w = wl + S.lw_at[j], *b = wl + S.lb_at[j], *a = av + S.a_at[j];
        float *an = av + S.a_at[j + 1];
        for (int o = lane; o < Lout; o += kWave) {
            float t = 0.f;
            for (int i = 0; i < Lin; ++i) t = __fadd_rn(t, __fmul_rn(w[i * ld + o], a[i]));
            const float z = __fadd_rn(t, b[o]);
            an[o] = z <= 0.f ? 0.f : z;
        }
        wave_sync();
    }
    float pred = 0.f;
    if (lane == 0) {
        const float *h = wl + S.lh_at, *am = av + S.a_at[S.m];
        float t = 0.f;
        for (int c = 0; c < k; ++c) t = __fadd_rn(t, __fmul_rn(h[c], av[c]));
        for (int c = 0; c < S.L[S.m]; ++c) t = __fadd_rn(t, __fmul_rn(h[k + c], am[c]));
        pred = __fadd_rn(t, wl[S.lc_at]);
    }
    return __shfl(pred, 0, kWave);
}

// A workgroup takes kBlock consecutive CSR entries at a time, lists those of the batch, and its four waves go through the list.
__global__ __launch_bounds__(kBlock) void nmf_fwd_bwd_kernel(NmfShape S, const int32_t *__restrict__ row, const int32_t *__restrict__ col,
                                                             const float *__restrict__ rating, const int32_t *__restrict__ rank, int64_t nnz, int lo,
                                                             int n_slots, const float *__restrict__ U, const float *__restrict__ V, int64_t n_user,
                                                             int64_t n_item, const float *__restrict__ dense, float *__restrict__ err,
                                                             float *__restrict__ pred_out, float *__restrict__ act, float *__restrict__ dlt,
                                                             float *__restrict__ emb)
{
    extern __shared__ float lds[];
    __shared__ int list[kBlock], slot_of[kBlock];
    __shared__ int n_list;
    stage_weights(S, dense, lds);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float *av = lds + S.lds_w + wave * (S.A + 2 * kMaxW), *dv = av + S.A;
    const float *h = lds + S.lh_at;
    const int k = S.k, e = S.e, wd = S.wd, m = S.m;
    const unsigned last_u = (unsigned)(n_user - 1), last_i = (unsigned)(n_item - 1);
    for (int64_t base = (int64_t)blockIdx.x * kBlock; base < nnz; base += (int64_t)gridDim.x * kBlock) {       // uniform across the workgroup
        if (threadIdx.x == 0) n_list = 0;
        __syncthreads();
        const int64_t mine = base + threadIdx.x;
        if (mine < nnz) {
            const int64_t r = (int64_t)ldg(rank + mine) - lo;
            if (r >= 0 && r < n_slots) {
                const int at = atomicAdd(&n_list, 1);          // (the order of the list plays no part: a sample's bytes are its own)
                list[at] = (int)threadIdx.x;
                slot_of[at] = (int)r;
            }
        }
        __syncthreads();
        const int n = n_list;
        for (int t = wave; t < n; t += kWavesPerBlock) {
            const int64_t q = base + list[t];
            const size_t slot = (size_t)slot_of[t];
            const float *urow = U + (size_t)min((unsigned)ldg(row + q), last_u) * wd;
            const float *vrow = V + (size_t)min((unsigned)ldg(col + q), last_i) * wd;
            const float pred = nmf_forward(S, lds, av, urow, vrow, lane);
            const float er = __fsub_rn(pred, ldg(rating + q)), ge = __fmul_rn(2.f, er);
            if (lane == 0) {
                stg(err + slot, er);
                if (pred_out) stg(pred_out + slot, pred);
            }
            float *arow = act + slot * S.A, *drow = dlt + slot * S.Dw, *erow = emb + slot * 2 * wd;
            for (int c = lane; c < S.A; c += kWave) stg(arow + c, av[c]);
            for (int c = lane; c < k; c += kWave) {
                const float dg = __fmul_rn(ge, h[c]);
                stg(erow + c, __fmul_rn(dg, ldg(vrow + c)));
                stg(erow + wd + c, __fmul_rn(dg, ldg(urow + c)));
            }
            int cur = 0;
            {
                const float *am = av + S.a_at[m];
                for (int o = lane; o < S.L[m]; o += kWave) {
                    const float d = am[o] > 0.f ? __fmul_rn(ge, h[k + o]) : 0.f;
                    dv[o] = d;
                    stg(drow + S.d_at[m] + o, d);
                }
            }
            wave_sync();
            for (int j = m - 1; j >= 0; --j) {
                const int Lin = S.L[j], Lout = S.L[j + 1], ld = Lout + 1;
                const float *w = lds + S.lw_at[j], *din = dv + cur * kMaxW, *aj = av + S.a_at[j];
                float *dout = dv + (cur ^ 1) * kMaxW;
                for (int i = lane; i < Lin; i += kWave) {
                    float s = 0.f;
                    for (int o = 0; o < Lout; ++o) s = __fadd_rn(s, __fmul_rn(w[i * ld + o], din[o]));
                    if (j > 0) {
                        const float d = aj[i] > 0.f ? s : 0.f;
                        dout[i] = d;
                        stg(drow + S.d_at[j] + i, d);
                    } else {
                        stg(erow + (i < e ? k + i : wd + k + (i - e)), s);
                    }
                }
                wave_sync();
                cur ^= 1;
            }
        }
        __syncthreads();                                       // the list is rewritten next
    }
}

// One wave per pair; ure_score's protocol round the forward (score_kernel, mf_eval.hip).
__global__ __launch_bounds__(kBlock) void nmf_score_kernel(NmfShape S, const float *__restrict__ U, const float *__restrict__ V,
                                                           const float *__restrict__ dense, int64_t n_user, int64_t n_item, int n_total, int first,
                                                           int last, const int32_t *__restrict__ uid, const int32_t *__restrict__ iid,
                                                           const float *__restrict__ rating, int64_t n, float *__restrict__ pred,
                                                           double *__restrict__ sse)
{
    extern __shared__ float lds[];
    stage_weights(S, dense, lds);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float *av = lds + S.lds_w + wave * (S.A + 2 * kMaxW);
    const unsigned last_u = (unsigned)(n_user - 1), last_i = (unsigned)(n_item - 1);
    const int64_t n_waves = (int64_t)gridDim.x * kWavesPerBlock;
    float sq = 0.f;
    for (int64_t j = (int64_t)blockIdx.x * kWavesPerBlock + wave; j < n; j += n_waves) {
        const float *urow = U + (size_t)min((unsigned)ldg(uid + j), last_u) * S.wd;
        const float *vrow = V + (size_t)min((unsigned)ldg(iid + j), last_i) * S.wd;
        const float p = nmf_forward(S, lds, av, urow, vrow, lane);
        if (lane == 0) {
            float acc = first ? 0.f : pred[j];
            acc = __fadd_rn(acc, p);
            if (last) {
                acc = __fdiv_rn(acc, (float)n_total);
                if (sse) {
                    const float er = acc - rating[j];
                    sq = fmaf(er, er, sq);
                }
            }
            pred[j] = acc;
        }
    }
    if (last && sse) sq_partials(sq, sse);
}

// The chunk partials: part[chunk][p] for every float p of the dense vector, a chain over the chunk's slots in ascending order.
// Thread p (blockIdx.y tiles the vector) walks the slots; consecutive p read consecutive a_j[i] of a slot and one delta.
__global__ __launch_bounds__(kBlock) void nmf_wgrad_part_kernel(NmfShape S, const float *__restrict__ err, const float *__restrict__ act,
                                                                const float *__restrict__ dlt, int n_slots, int n_chunks, float *__restrict__ part)
{
    for (int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const int s0 = chunk * URE_NMF_CHUNK, s1 = min(s0 + URE_NMF_CHUNK, n_slots);
        const int p = blockIdx.y * kBlock + threadIdx.x;
        if (p < S.n_dense) {
            // mode 0: delta * a; 1: delta; 2: (2 err) * a; 3: 2 err; 4: the padding
            int mode = 4, xc = 0, yc = 0;
            if (p < S.h_at) {
                int j = 0;
                while (j + 1 < S.m && p >= S.w_at[j + 1]) ++j;
                if (p < S.b_at[j]) {
                    const int r = p - S.w_at[j];
                    mode = 0, xc = S.d_at[j + 1] + r / S.L[j], yc = S.a_at[j] + r % S.L[j];
                } else {
                    mode = 1, xc = S.d_at[j + 1] + (p - S.b_at[j]);
                }
            } else if (p < S.c_at) {
                const int c = p - S.h_at;
                mode = 2, yc = c < S.k ? c : S.a_at[S.m] + (c - S.k);
            } else if (p == S.c_at) {
                mode = 3;
            }
            float t = 0.f;
            if (mode == 0)
                for (int s = s0; s < s1; ++s) t = __fadd_rn(t, __fmul_rn(ldg(dlt + (size_t)s * S.Dw + xc), ldg(act + (size_t)s * S.A + yc)));
            else if (mode == 1)
                for (int s = s0; s < s1; ++s) t = __fadd_rn(t, ldg(dlt + (size_t)s * S.Dw + xc));
            else if (mode == 2)
                for (int s = s0; s < s1; ++s) t = __fadd_rn(t, __fmul_rn(__fmul_rn(2.f, ldg(err + s)), ldg(act + (size_t)s * S.A + yc)));
            else if (mode == 3)
                for (int s = s0; s < s1; ++s) t = __fadd_rn(t, __fmul_rn(2.f, ldg(err + s)));
            stg(part + (size_t)chunk * S.n_dense + p, t);
        }
    }
}

__global__ __launch_bounds__(kBlock) void nmf_wgrad_sum_kernel(const float *__restrict__ part, int n_dense, int n_chunks, float *__restrict__ out)
{
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_dense) return;
    float t = ldg(part + p);
    for (int c = 1; c < n_chunks; ++c) t = __fadd_rn(t, ldg(part + (size_t)c * n_dense + p));
    stg(out + p, t);
}

// The masked row sums (row_walk.h's walk): the batch is named by rank and the term is a slot's row.  A fetch reads the entry's
// slot and -- for an entry of the batch -- its residual; an entry outside the batch has slot -1.  The group is the power of two
// that covers width / 4 lanes; lanes beyond the width idle.
template <int G, bool MAPPED>
__global__ __launch_bounds__(kBlock) void nmf_row_sum_kernel(const int64_t *__restrict__ off, const int32_t *__restrict__ map,
                                                             const int32_t *__restrict__ rank, int64_t n_rows, int64_t nnz, int lo, int n_slots,
                                                             const float *__restrict__ E, int ld, int col0, int width, const float *__restrict__ err,
                                                             float *__restrict__ Gout, double *__restrict__ row_loss)
{
    const RowLanes<G> L;
    if (L.past(n_rows)) return;
    const unsigned last_pos = (unsigned)(nnz - 1);
    const bool live = 4 * L.sub < width;
    const float *__restrict__ x = E + col0 + 4 * (live ? L.sub : 0);
    float4 g = f4_zero();
    double loss = 0.0;
    struct Entry { int slot; float e; };
    tile_walk<G>(
        ldg(off + L.r), ldg(off + L.r + 1), L.sub,
        [&](int64_t p, bool inside) {
            Entry mine{-1, 0.f};
            if (inside) {
                const int64_t s = (int64_t)ldg(rank + entry_pos<MAPPED>(map, p, last_pos)) - lo;
                if (s >= 0 && s < n_slots) {
                    mine.slot = (int)s;
                    if (row_loss) mine.e = ldg(err + s);
                }
            }
            return mine;
        },
        [&](const Entry &mine, int u) {
            const int slot = group_read<G>(mine.slot, u);
            if (slot < 0) return;
            const float ee = group_read<G>(mine.e, u);
            g = f4_add(g, ldg_f4(x + (size_t)slot * ld));
            loss += (double)ee * (double)ee;
        });
    if (live) stg_f4(Gout + (size_t)L.r * width + 4 * L.sub, g);
    if (row_loss && L.sub == 0) stg(row_loss + L.r, loss);
}

}  // namespace
}  // namespace ure

using namespace ure;

// A slot count whose last chunk's end, s0 + URE_NMF_CHUNK, still fits an int; the chunks of it (the sum in 64 bits).
static inline bool slots_ok(int32_t n_slots) { return n_slots >= 1 && n_slots <= INT32_MAX - URE_NMF_CHUNK; }
static inline int64_t wgrad_chunks(int32_t n_slots) { return ((int64_t)n_slots + URE_NMF_CHUNK - 1) / URE_NMF_CHUNK; }

#define URE_NMF_SHAPE(S, k, layers, n_layers) \
    NmfShape S;                               \
    URE_ARG(fill_shape(S, k, layers, n_layers))

extern "C" int64_t ure_nmf_dense_size(int32_t k, const int32_t *layers, int32_t n_layers)
{
    NmfShape S;
    return fill_shape(S, k, layers, n_layers) ? S.n_dense : -1;
}

extern "C" int ure_nmf_forward_backward(const int32_t *row, const int32_t *col, const float *rating, const int32_t *rank, int64_t nnz, int32_t lo,
                                        int32_t n_slots, const float *U, const float *V, int64_t n_user, int64_t n_item, const float *dense,
                                        int32_t k, const int32_t *layers, int32_t n_layers, float *err, float *pred_out, float *act, float *dlt,
                                        float *emb, void *stream)
{
    URE_NMF_SHAPE(S, k, layers, n_layers);
    URE_ARG(row && col && rating && rank && U && V && dense && err && act && dlt && emb);
    URE_ARG(nnz >= 1 && nnz <= INT32_MAX && n_user >= 1 && n_user <= INT32_MAX && n_item >= 1 && n_item <= INT32_MAX);
    URE_ARG(lo >= 0 && n_slots >= 1 && (int64_t)lo + n_slots <= nnz);
    const unsigned blocks = (unsigned)std::min<int64_t>((nnz + kBlock - 1) / kBlock, 2048);
    hipLaunchKernelGGL(nmf_fwd_bwd_kernel, dim3(blocks), dim3(kBlock), (size_t)S.lds_bytes, (hipStream_t)stream, S, row, col, rating, rank, nnz,
                       (int)lo, (int)n_slots, U, V, n_user, n_item, dense, err, pred_out, act, dlt, emb);
    URE_HIP(hipGetLastError());
    return 0;
}

extern "C" int64_t ure_nmf_weight_grad_scratch(int32_t n_slots, int32_t k, const int32_t *layers, int32_t n_layers)
{
    NmfShape S;
    if (!slots_ok(n_slots) || !fill_shape(S, k, layers, n_layers)) return -1;
    return wgrad_chunks(n_slots) * S.n_dense * 4;
}

extern "C" int ure_nmf_weight_grad(const float *err, const float *act, const float *dlt, int32_t n_slots, int32_t k, const int32_t *layers,
                                   int32_t n_layers, float *g_dense, void *scratch, int64_t scratch_bytes, int32_t blocks, void *stream)
{
    URE_NMF_SHAPE(S, k, layers, n_layers);
    URE_ARG(err && act && dlt && g_dense && scratch);
    URE_ARG(slots_ok(n_slots) && blocks >= 0);
    const int n_chunks = (int)wgrad_chunks(n_slots);
    URE_ARG(scratch_bytes >= (int64_t)n_chunks * S.n_dense * 4);
    URE_ARG(apart(g_dense, (int64_t)S.n_dense * 4, scratch, scratch_bytes));
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)(blocks ? std::min<int>(blocks, n_chunks) : n_chunks);
    hipLaunchKernelGGL(nmf_wgrad_part_kernel, dim3(grid, (S.n_dense + kBlock - 1) / kBlock), dim3(kBlock), 0, st, S, err, act, dlt, (int)n_slots, n_chunks, (float *)scratch);
    hipLaunchKernelGGL(nmf_wgrad_sum_kernel, dim3((S.n_dense + kBlock - 1) / kBlock), dim3(kBlock), 0, st, (const float *)scratch, S.n_dense, n_chunks,
                       g_dense);
    URE_HIP(hipGetLastError());
    return 0;
}

extern "C" int ure_nmf_row_sum(const int64_t *off, const int32_t *map, const int32_t *rank, int64_t n_rows, int64_t nnz, int32_t lo, int32_t n_slots,
                               const float *E, int32_t ld, int32_t col0, int32_t width, const float *err, float *G_out, double *row_loss, void *stream)
{
    URE_ARG(off && rank && E && G_out);
    URE_ARG(n_rows >= 1 && n_rows <= INT32_MAX && nnz >= 1 && nnz <= INT32_MAX);
    URE_ARG(lo >= 0 && n_slots >= 1 && (int64_t)lo + n_slots <= nnz);
    URE_ARG(width >= 4 && width <= 256 && width % 4 == 0 && col0 >= 0 && col0 % 4 == 0 && ld % 4 == 0 && col0 + width <= ld);
    URE_ARG(!row_loss || err);
    URE_ARG(apart(G_out, n_rows * width * 4, E, (int64_t)n_slots * ld * 4));
    hipStream_t st = (hipStream_t)stream;
    dispatch_group_width(group_width(width / 4), [&](auto w) {
        constexpr int G = decltype(w)::value;
        launch_by_map(map, nmf_row_sum_kernel<G, true>, nmf_row_sum_kernel<G, false>, n_rows, G, st, off, map, rank, n_rows, nnz, (int)lo, (int)n_slots, E,
                      (int)ld, (int)col0, (int)width, err, G_out, row_loss);
    });
    URE_HIP(hipGetLastError());
    return 0;
}

extern "C" int ure_nmf_score(const float *U, const float *V, const float *dense, int32_t k, const int32_t *layers, int32_t n_layers, int64_t n_user,
                             int64_t n_item, int32_t n_models_total, int32_t first, int32_t last, const int32_t *uid, const int32_t *iid,
                             const float *rating, int64_t n, float *pred, double *sse, void *stream)
{
    URE_NMF_SHAPE(S, k, layers, n_layers);
    URE_ARG(U && V && dense && uid && iid && pred);
    URE_ARG(n >= 1 && n <= INT32_MAX && n_user >= 1 && n_user <= INT32_MAX && n_item >= 1 && n_item <= INT32_MAX);
    URE_ARG(n_models_total >= 1 && (!sse || rating));
    const unsigned blocks = (unsigned)std::min<int64_t>((n + kWavesPerBlock - 1) / kWavesPerBlock, URE_SCORE_PARTIALS);
    hipLaunchKernelGGL(nmf_score_kernel, dim3(blocks), dim3(kBlock), (size_t)S.lds_bytes, (hipStream_t)stream, S, U, V, dense, n_user, n_item,
                       (int)n_models_total, (int)first, (int)last, uid, iid, rating, n, pred, sse);
    URE_HIP(hipGetLastError());
    return 0;
}

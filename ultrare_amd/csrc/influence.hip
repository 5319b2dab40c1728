// influence.hip -- Newton-step (influence) unlearning of an MF shard (include/ultrare_influence.h; the contract is
// ultrare_amd/influence.py): the coefficient pass, the Hessian-vector / gradient walk over a shard's CSR / CSC, the fixed-order
// dot and the conjugate-gradient vector operations, whose scalars never leave the device.
//
// The walk is row_walk.h's: a group of G = d / 4 lanes owns an output row, the chain of a (row, column) is one lane's, in
// ascending entry position.  inf_walk_kernel's own: the d columns as four float64 accumulators per lane, what a fetch reads,
// the early store of an inactive or empty row, the row end held inside nnz.  The 256-lane fold of the dot is gcn_ops.h's.  Every
// operation is a rounded float64 operation of its own (__dmul_rn / __dadd_rn and -ffp-contract=off: never contracted).
#include "gcn_ops.h"

namespace ure {
namespace {

typedef double ure_d2 __attribute__((ext_vector_type(2)));
struct d4 {
    double x, y, z, w;
};
__device__ __forceinline__ d4 ldg_d4(const double *p)
{
    const ure_d2 a = *(const ure_d2 URE_AS1 *)p, b = *(const ure_d2 URE_AS1 *)(p + 2);
    return d4{a.x, a.y, b.x, b.y};
}
__device__ __forceinline__ void stg_d4(double *p, d4 v)
{
    ure_d2 a, b;
    a.x = v.x, a.y = v.y, b.x = v.z, b.y = v.w;
    *(ure_d2 URE_AS1 *)p = a;
    *(ure_d2 URE_AS1 *)(p + 2) = b;
}
__device__ __forceinline__ d4 widen(float4 v) { return d4{(double)v.x, (double)v.y, (double)v.z, (double)v.w}; }
// acc + s * v, the product and the sum rounded separately
__device__ __forceinline__ d4 d4_mul_add(d4 acc, double s, d4 v)
{
    acc.x = __dadd_rn(acc.x, __dmul_rn(s, v.x));
    acc.y = __dadd_rn(acc.y, __dmul_rn(s, v.y));
    acc.z = __dadd_rn(acc.z, __dmul_rn(s, v.z));
    acc.w = __dadd_rn(acc.w, __dmul_rn(s, v.w));
    return acc;
}
// p = a_0 b_0 (first) or p + a_0 b_0, then + a_1 b_1, + a_2 b_2, + a_3 b_3
template <bool FIRST>
__device__ __forceinline__ double lane_chain(double p, d4 a, d4 b)
{
    p = FIRST ? __dmul_rn(a.x, b.x) : __dadd_rn(p, __dmul_rn(a.x, b.x));
    p = __dadd_rn(p, __dmul_rn(a.y, b.y));
    p = __dadd_rn(p, __dmul_rn(a.z, b.z));
    return __dadd_rn(p, __dmul_rn(a.w, b.w));
}
// The balanced tree of adjacent pairs over the LPR lanes of a group as an xor butterfly (a + b == b + a bit for bit): every lane
// ends with the sum.
template <int LPR>
__device__ __forceinline__ double group_sum_f64(double v)
{
#pragma unroll
    for (int o = 1; o < LPR; o <<= 1) v = __dadd_rn(v, __shfl_xor(v, o, kWave));
    return v;
}

// A group of LPR = d / 4 lanes per CSR entry, gcn_residual_kernel's shape.  Every lane of a wave takes part in every dot (a group
// past the end works on the last entry and stores nothing), so the butterfly never meets an idle lane.
template <int LPR, bool DIR>
__global__ __launch_bounds__(kBlock) void inf_coef_kernel(const int32_t *__restrict__ row, const int32_t *__restrict__ col,
                                                          const float *__restrict__ rating, int64_t nnz, const float *__restrict__ U,
                                                          const float *__restrict__ V, const double *__restrict__ P, const double *__restrict__ Q,
                                                          int64_t n_user, int64_t n_item, double *__restrict__ out)
{
    const PairLanes<LPR> L;
    const unsigned last_u = (unsigned)(n_user - 1), last_i = (unsigned)(n_item - 1);
    for (int64_t base = L.wave_id * L.G; base < nnz; base += L.n_waves * L.G) {
        const int64_t k = base + L.grp;
        const int64_t kk = min<int64_t>(k, nnz - 1);
        const size_t au = (size_t)min((unsigned)ldg(row + kk), last_u) * L.D + 4 * L.sub;
        const size_t ai = (size_t)min((unsigned)ldg(col + kk), last_i) * L.D + 4 * L.sub;
        const d4 u = widen(ldg_f4(U + au)), v = widen(ldg_f4(V + ai));
        double p;
        if (DIR) {
            p = lane_chain<true>(0.0, ldg_d4(P + au), v);
            p = lane_chain<false>(p, u, ldg_d4(Q + ai));
        } else {
            p = lane_chain<true>(0.0, u, v);
        }
        p = group_sum_f64<LPR>(p);
        if (k < nnz && L.sub == 0) stg(out + k, DIR ? p : __dsub_rn(p, (double)ldg(rating + k)));
    }
}

// out[r] = 2 (sum over row r's entries of a[q] T[idx] [+ b[q] D[idx]]) + reg2 X[r].  A fetch reads the entry's coefficients and
// its index; every entry of the row counts.  An inactive or empty row stores zeros and reads no entry.
template <int G, bool MAPPED, bool SECOND>
__global__ __launch_bounds__(kBlock) void inf_walk_kernel(const int64_t *__restrict__ off, const int32_t *__restrict__ idx, const int32_t *__restrict__ map,
                                                          const double *__restrict__ a, const float *__restrict__ T, const double *__restrict__ b,
                                                          const double *__restrict__ Dir, double reg2, const double *__restrict__ X,
                                                          const uint8_t *__restrict__ active, int64_t n_dst, int64_t n_src, int64_t nnz,
                                                          double *__restrict__ out)
{
    constexpr int D = 4 * G;
    const RowLanes<G> L;
    if (L.past(n_dst)) return;
    const size_t at = (size_t)L.r * D + 4 * L.sub;
    int64_t p_begin = 0, p_end = 0;
    if (!active || ldg(active + L.r)) {
        p_begin = ldg(off + L.r);
        p_end = min<int64_t>(ldg(off + L.r + 1), nnz);
    }
    d4 acc = d4{0.0, 0.0, 0.0, 0.0};
    if (p_begin >= p_end) {
        stg_d4(out + at, acc);
        return;
    }
    const unsigned last = (unsigned)(n_src - 1), last_pos = (unsigned)(nnz - 1);
    const float *__restrict__ t = T + 4 * L.sub;
    const double *__restrict__ dd = SECOND ? Dir + 4 * L.sub : nullptr;
    struct Entry { unsigned j; double a, b; };
    tile_walk<G>(
        p_begin, p_end, L.sub,
        [&](int64_t k, bool inside) {
            Entry mine{0u, 0.0, 0.0};
            if (inside) {
                const unsigned q = entry_pos<MAPPED>(map, k, last_pos);
                mine.a = ldg(a + q);
                if (SECOND) mine.b = ldg(b + q);
                mine.j = min((unsigned)ldg(idx + k), last);
            }
            return mine;
        },
        [&](const Entry &mine, int u) {
            const unsigned j = group_read<G>(mine.j, u);
            acc = d4_mul_add(acc, group_read<G>(mine.a, u), widen(ldg_f4(t + (size_t)j * D)));
            if (SECOND) acc = d4_mul_add(acc, group_read<G>(mine.b, u), ldg_d4(dd + (size_t)j * D));
        });
    const d4 x = ldg_d4(X + at);
    d4 y;
    y.x = __dadd_rn(__dmul_rn(2.0, acc.x), __dmul_rn(reg2, x.x));
    y.y = __dadd_rn(__dmul_rn(2.0, acc.y), __dmul_rn(reg2, x.y));
    y.z = __dadd_rn(__dmul_rn(2.0, acc.z), __dmul_rn(reg2, x.z));
    y.w = __dadd_rn(__dmul_rn(2.0, acc.w), __dmul_rn(reg2, x.w));
    stg_d4(out + at, y);
}

constexpr int kDotChunk = 4096;                            // influence.DOT_CHUNK: 16 values per lane

__global__ __launch_bounds__(256) void inf_dot_chunk_kernel(const double *x, const double *y, int64_t n, double *__restrict__ partial)
{
    __shared__ double part[256];
    const int64_t base = (int64_t)blockIdx.x * kDotChunk + threadIdx.x;
    double acc = 0.0;
#pragma unroll 4
    for (int j = 0; j < kDotChunk / 256; ++j) {
        const int64_t i = base + (int64_t)j * 256;
        if (i < n) acc = __dadd_rn(acc, __dmul_rn(ldg(x + i), ldg(y + i)));
    }
    const double s = fold_256(acc, part);
    if (threadIdx.x == 0) stg(partial + blockIdx.x, s);
}

__global__ __launch_bounds__(256) void inf_dot_fold_kernel(const double *__restrict__ partial, int64_t n, double *out)
{
    __shared__ double part[256];
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) acc = __dadd_rn(acc, ldg(partial + i));
    const double s = fold_256(acc, part);
    if (threadIdx.x == 0) stg(out, s);
}

enum { kRr = 0, kPap = 1, kRrNew = 2, kThresh = 3, kFlag = 4, kAlpha = 5, kBeta = 6 };

__global__ void inf_cg_start_kernel(double *state, double tol)
{
    if (threadIdx.x || blockIdx.x) return;
    const double rr = state[kRr], thresh = __dmul_rn(__dmul_rn(tol, tol), rr);
    state[kThresh] = thresh;
    state[kFlag] = rr <= thresh ? 1.0 : 0.0;
    state[kPap] = state[kRrNew] = state[kAlpha] = state[kBeta] = state[7] = 0.0;
}

__global__ __launch_bounds__(kBlock) void inf_cg_xr_kernel(const double *__restrict__ state, double *__restrict__ x, double *__restrict__ r,
                                                           const double *__restrict__ p, const double *__restrict__ Ap, int64_t n)
{
    const double pAp = ldg(state + kPap);
    if (ldg(state + kFlag) != 0.0 || !(pAp > 0.0)) return;
    const double alpha = __ddiv_rn(ldg(state + kRr), pAp);
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        stg(x + i, __dadd_rn(ldg(x + i), __dmul_rn(alpha, ldg(p + i))));
        stg(r + i, __dsub_rn(ldg(r + i), __dmul_rn(alpha, ldg(Ap + i))));
    }
}

__global__ void inf_cg_beta_kernel(double *state, double *log_rr, int32_t *log_flag, int64_t it)
{
    if (threadIdx.x || blockIdx.x) return;
    double flag = state[kFlag];
    if (flag == 0.0) {
        const double pAp = state[kPap], rr = state[kRr];
        if (!(pAp > 0.0)) {
            flag = 2.0;
        } else {
            const double rr_new = state[kRrNew];
            state[kAlpha] = __ddiv_rn(rr, pAp);
            state[kBeta] = __ddiv_rn(rr_new, rr);
            state[kRr] = rr_new;
            if (rr_new <= state[kThresh]) flag = 1.0;
        }
        state[kFlag] = flag;
    }
    log_rr[it] = state[kRr];
    log_flag[it] = (int32_t)flag;
}

__global__ __launch_bounds__(kBlock) void inf_cg_p_kernel(const double *__restrict__ state, double *__restrict__ p, const double *__restrict__ r, int64_t n)
{
    if (ldg(state + kFlag) != 0.0) return;
    const double beta = ldg(state + kBeta);
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
        stg(p + i, __dadd_rn(ldg(r + i), __dmul_rn(beta, ldg(p + i))));
}

inline int64_t dot_chunks(int64_t n) { return (n + kDotChunk - 1) / kDotChunk; }

}  // namespace
}  // namespace ure

using namespace ure;

extern "C" int ure_inf_coef(const int32_t *row, const int32_t *col, const float *rating, int64_t nnz, const float *U, const float *V, const double *P,
                            const double *Q, int64_t n_user, int64_t n_item, int32_t d, double *out, void *stream)
{
    URE_GCN_SIZES(n_user, n_item, d);
    URE_ARG(row && col && rating && U && V && out);
    URE_ARG((P == nullptr) == (Q == nullptr));
    URE_ARG(nnz >= 1 && nnz <= INT32_MAX);
    URE_ARG(apart(out, nnz * 8, U, n_user * d * 4) && apart(out, nnz * 8, V, n_item * d * 4) && apart(out, nnz * 8, rating, nnz * 4));
    URE_ARG(apart(out, nnz * 8, row, nnz * 4) && apart(out, nnz * 8, col, nnz * 4));
    URE_ARG(!P || (apart(out, nnz * 8, P, n_user * d * 8) && apart(out, nnz * 8, Q, n_item * d * 8)));
    hipStream_t st = (hipStream_t)stream;
    dispatch_group_width(d / 4, [&](auto w) {
        constexpr int LPR = decltype(w)::value;
        const dim3 grid(pair_blocks(nnz, kWave / LPR, 4096));
        if (P)
            hipLaunchKernelGGL((inf_coef_kernel<LPR, true>), grid, dim3(kBlock), 0, st, row, col, rating, nnz, U, V, P, Q, n_user, n_item, out);
        else
            hipLaunchKernelGGL((inf_coef_kernel<LPR, false>), grid, dim3(kBlock), 0, st, row, col, rating, nnz, U, V, P, Q, n_user, n_item, out);
    });
    URE_HIP(hipGetLastError());
    return 0;
}

extern "C" int ure_inf_walk(const int64_t *off, const int32_t *idx, const int32_t *map, const double *a, const float *T, const double *b,
                            const double *D, double reg, const double *X, const uint8_t *active, int64_t n_dst, int64_t n_src, int64_t nnz, int32_t d,
                            double *out, void *stream)
{
    URE_GCN_SIZES(n_dst, n_src, d);
    URE_ARG(off && idx && a && T && X && out);
    URE_ARG((b == nullptr) == (D == nullptr));
    URE_ARG(nnz >= 1 && nnz <= INT32_MAX);
    URE_ARG(reg >= 0.0 && reg <= 1.7e308);
    const int64_t nb = n_dst * d * 8;
    URE_ARG(apart(out, nb, X, nb) && apart(out, nb, T, n_src * d * 4) && apart(out, nb, a, nnz * 8));
    URE_ARG(!b || (apart(out, nb, b, nnz * 8) && apart(out, nb, D, n_src * d * 8)));
    URE_ARG(apart(out, nb, off, (n_dst + 1) * 8) && apart(out, nb, idx, nnz * 4));
    URE_ARG(!map || apart(out, nb, map, nnz * 4));
    URE_ARG(!active || apart(out, nb, active, n_dst));
    hipStream_t st = (hipStream_t)stream;
    const double reg2 = 2.0 * reg;
    dispatch_group_width(d / 4, [&](auto w) {
        constexpr int G = decltype(w)::value;
        if (b)
            launch_by_map(map, inf_walk_kernel<G, true, true>, inf_walk_kernel<G, false, true>, n_dst, G, st, off, idx, map, a, T, b, D, reg2, X, active,
                          n_dst, n_src, nnz, out);
        else
            launch_by_map(map, inf_walk_kernel<G, true, false>, inf_walk_kernel<G, false, false>, n_dst, G, st, off, idx, map, a, T, b, D, reg2, X, active,
                          n_dst, n_src, nnz, out);
    });
    URE_HIP(hipGetLastError());
    return 0;
}

extern "C" int64_t ure_inf_dot_scratch(int64_t n) { return n < 1 ? 0 : dot_chunks(n) * 8; }

extern "C" int ure_inf_dot(const double *x, const double *y, int64_t n, void *scratch, int64_t scratch_bytes, double *out, void *stream)
{
    URE_ARG(x && y && out && scratch);
    URE_ARG(n >= 1 && dot_chunks(n) <= INT32_MAX);
    URE_ARG(scratch_bytes >= ure_inf_dot_scratch(n));
    const int64_t ns = dot_chunks(n) * 8;
    URE_ARG(apart(scratch, ns, x, n * 8) && apart(scratch, ns, y, n * 8) && apart(scratch, ns, out, 8));
    URE_ARG(apart(out, 8, x, n * 8) && apart(out, 8, y, n * 8));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(inf_dot_chunk_kernel, dim3((unsigned)dot_chunks(n)), dim3(256), 0, st, x, y, n, (double *)scratch);
    hipLaunchKernelGGL(inf_dot_fold_kernel, dim3(1), dim3(256), 0, st, (const double *)scratch, dot_chunks(n), out);
    URE_HIP(hipGetLastError());
    return 0;
}

extern "C" int ure_inf_cg_start(double *state, double tol, void *stream)
{
    URE_ARG(state && tol > 0.0 && tol < 1.0);
    hipLaunchKernelGGL(inf_cg_start_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state, tol);
    URE_HIP(hipGetLastError());
    return 0;
}

extern "C" int ure_inf_cg_xr(const double *state, double *x, double *r, const double *p, const double *Ap, int64_t n, void *stream)
{
    URE_ARG(state && x && r && p && Ap && n >= 1 && n <= (int64_t)1 << 40);
    const int64_t nb = n * 8;
    URE_ARG(apart(x, nb, r, nb) && apart(x, nb, p, nb) && apart(x, nb, Ap, nb) && apart(r, nb, p, nb) && apart(r, nb, Ap, nb));
    URE_ARG(apart(state, 64, x, nb) && apart(state, 64, r, nb));
    hipLaunchKernelGGL(inf_cg_xr_kernel, dim3(stream_blocks(n)), dim3(kBlock), 0, (hipStream_t)stream, state, x, r, p, Ap, n);
    URE_HIP(hipGetLastError());
    return 0;
}

extern "C" int ure_inf_cg_beta(double *state, double *log_rr, int32_t *log_flag, int64_t it, int64_t n_log, void *stream)
{
    URE_ARG(state && log_rr && log_flag && n_log >= 1 && n_log <= INT32_MAX && it >= 0 && it < n_log);
    URE_ARG(apart(state, 64, log_rr, n_log * 8) && apart(state, 64, log_flag, n_log * 4) && apart(log_rr, n_log * 8, log_flag, n_log * 4));
    hipLaunchKernelGGL(inf_cg_beta_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state, log_rr, log_flag, it);
    URE_HIP(hipGetLastError());
    return 0;
}

extern "C" int ure_inf_cg_p(const double *state, double *p, const double *r, int64_t n, void *stream)
{
    URE_ARG(state && p && r && n >= 1 && n <= (int64_t)1 << 40);
    URE_ARG(apart(p, n * 8, r, n * 8) && apart(state, 64, p, n * 8));
    hipLaunchKernelGGL(inf_cg_p_kernel, dim3(stream_blocks(n)), dim3(kBlock), 0, (hipStream_t)stream, state, p, r, n);
    URE_HIP(hipGetLastError());
    return 0;
}

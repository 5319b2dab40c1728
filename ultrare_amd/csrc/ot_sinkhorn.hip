// ot_sinkhorn.hip -- entropic (log-domain Sinkhorn) OT between n points and k clusters, solved on the device.
//
// The contract is POT's ot.bregman.sinkhorn_log with uniform marginals, restated in numpy in the tests
// (tests/test_gpu_sinkhorn.py::sinkhorn_contract).  With Mr = -M / reg, M = dist^T [n, k] (ure_ot_cost's [k][n] matrix,
// read transposed), loga = log(1/n), logb = log(1/k), u = v = 0, for ii = 0 .. num_iter_max - 1:
//     v  = logb - LSE_i(Mr_ij + u_i)        u = loga - LSE_j(Mr_ij + v_j)
//     ii % 10 == 0: err = || colsum(u, v) - exp(logb) ||_2 ; err < stop_thr: stop (iters = ii + 1)
// label_i = first argmax_j (Mr_ij + v_j).  Everything is float64 except the costs themselves.
//
// One iteration is two launches on the stream:
//   sk_pass_kernel     one point per thread: u_i from the row LSE of Mr_ij + v_j (online max / sum), then, with the
//                      workgroup's 256 new u in LDS, per-column partials (max, sum exp(. - max)) of Mr_ij + u_i over
//                      the workgroup's points, wave = column.  The matrix is read twice; the second read is of the
//                      tile the first one just brought on chip.
//   sk_combine_kernel  one workgroup per column merges the partials of all workgroups in a fixed order into the next v.
// and at check iterations a third, sk_check_kernel (one workgroup), forms err from v_ii and v_ii+1 in closed form:
// colsum_j(u_ii, v_ii) = exp(logb_j + v_ii,j - v_ii+1,j), so colsum_j - exp(logb_j) = exp(logb_j) expm1(v_ii,j - v_ii+1,j).
// v lives in two buffers by the parity of ii, so that after a stop at ii both u_ii and v_ii are still there.  A device
// word records the stop; every later launch of the batch the host has queued returns at once.  No float atomics and a
// fixed reduction order everywhere: two calls give the same bits.  The [n, k] plan is never formed.
#include "ure_internal.h"

#include <cmath>

namespace ure {

constexpr int kSinkhornMaxK = 1024;
constexpr int kSkPts = kBlock;          // points per workgroup of the pass and label kernels

struct sk_state {
    int32_t stop;                       // 0: running; ii + 1: err < stop_thr at check iteration ii
    int32_t bad;                        // a non-finite err was met
    double err;                         // the last err computed
};

__device__ __forceinline__ double wave_max(double x)
{
    for (int o = 32; o > 0; o >>= 1) x = fmax(x, __shfl_xor(x, o, kWave));
    return x;
}

__device__ __forceinline__ double wave_sum(double x)
{
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, kWave);
    return x;
}

// init != 0: only the column partials of Mr_ij + 0 (the first v); otherwise iteration ii: u from v_in, then the partials.
__global__ __launch_bounds__(kBlock) void sk_pass_kernel(const float *__restrict__ dist, int64_t n, int k, double inv_reg, double loga,
                                                         const double *__restrict__ v_in, double *__restrict__ u,
                                                         double *__restrict__ pm, double *__restrict__ ps, const sk_state *__restrict__ st,
                                                         int init)
{
    if (st->stop) return;
    __shared__ double sv[kSinkhornMaxK];
    __shared__ double su[kSkPts];
    const int64_t i0 = (int64_t)blockIdx.x * kSkPts;
    const int rows = (int)min<int64_t>(kSkPts, n - i0);
    const int64_t B = gridDim.x;
    if (init) {
        su[threadIdx.x] = 0.0;
    } else {
        for (int j = threadIdx.x; j < k; j += kBlock) sv[j] = v_in[j];
        __syncthreads();
        if ((int)threadIdx.x < rows) {
            const int64_t i = i0 + threadIdx.x;
            double m = -INFINITY, s = 0.0;
            for (int j = 0; j < k; ++j) {
                const double x = -(double)dist[(size_t)j * n + i] * inv_reg + sv[j];
                const double t = exp(-fabs(x - m));          // one exp either way: rescale the sum or add the new term
                if (x > m) { s = s * t + 1.0; m = x; }
                else s += t;
            }
            const double ui = loga - (m + log(s));
            u[i] = ui;
            su[threadIdx.x] = ui;
        }
    }
    __syncthreads();
    // column partials: wave w takes columns w, w + 4, ...; lane l the points l, l + 64, l + 128, l + 192 of the tile
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    constexpr int R = kSkPts / kWave;
    for (int j = wave; j < k; j += kWavesPerBlock) {
        double y[R];
        double m = -INFINITY;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int p = lane + r * kWave;
            y[r] = p < rows ? -(double)dist[(size_t)j * n + i0 + p] * inv_reg + su[p] : -INFINITY;
            m = fmax(m, y[r]);
        }
        m = wave_max(m);                                      // finite: point 0 of the tile is always there
        double s = 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) s += exp(y[r] - m);
        s = wave_sum(s);
        if (lane == 0) {
            pm[(size_t)j * B + blockIdx.x] = m;
            ps[(size_t)j * B + blockIdx.x] = s;
        }
    }
}

// Block-wide reductions in a fixed tree order (every thread gets the result).
template <bool IsMax>
__device__ __forceinline__ double block_reduce(double x, double *red)
{
    x = IsMax ? wave_max(x) : wave_sum(x);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    double r = red[0];
    for (int w = 1; w < kWavesPerBlock; ++w) r = IsMax ? fmax(r, red[w]) : r + red[w];
    __syncthreads();
    return r;
}

// One workgroup per column j: v_out[j] = logb - LSE over the B workgroups' partials.
__global__ __launch_bounds__(kBlock) void sk_combine_kernel(const double *__restrict__ pm, const double *__restrict__ ps, int64_t B,
                                                            double logb, double *__restrict__ v_out, const sk_state *__restrict__ st)
{
    if (st->stop) return;
    __shared__ double red[kWavesPerBlock];
    const int j = blockIdx.x;
    const double *m_j = pm + (size_t)j * B, *s_j = ps + (size_t)j * B;
    double m = -INFINITY;
    for (int64_t b = threadIdx.x; b < B; b += kBlock) m = fmax(m, m_j[b]);
    m = block_reduce<true>(m, red);
    double s = 0.0;
    for (int64_t b = threadIdx.x; b < B; b += kBlock) s += s_j[b] * exp(m_j[b] - m);
    s = block_reduce<false>(s, red);
    if (threadIdx.x == 0) v_out[j] = logb - (m + log(s));
}

// Check iteration ii (one workgroup): err from v_ii and v_ii+1; the stop word when err < stop_thr.
__global__ __launch_bounds__(kBlock) void sk_check_kernel(const double *__restrict__ v_ii, const double *__restrict__ v_next, int k, double eb,
                                                          double stop_thr, int ii, sk_state *__restrict__ st)
{
    if (st->stop) return;
    __shared__ double red[kWavesPerBlock];
    double q = 0.0;
    for (int j = threadIdx.x; j < k; j += kBlock) {
        const double e = eb * expm1(v_ii[j] - v_next[j]);
        q += e * e;
    }
    q = block_reduce<false>(q, red);
    if (threadIdx.x == 0) {
        const double err = sqrt(q);
        st->err = err;
        if (!isfinite(err)) st->bad = 1;
        if (err < stop_thr || !isfinite(err)) st->stop = ii + 1;
    }
}

// label_i = first argmax_j (Mr_ij + v_j); cost_min_i = min_j M_ij (fp32, exact in any order).
__global__ __launch_bounds__(kBlock) void sk_label_kernel(const float *__restrict__ dist, int64_t n, int k, double inv_reg,
                                                          const double *__restrict__ v, int32_t *__restrict__ label, float *__restrict__ cost_min)
{
    __shared__ double sv[kSinkhornMaxK];
    for (int j = threadIdx.x; j < k; j += kBlock) sv[j] = v[j];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * kSkPts + threadIdx.x;
    if (i >= n) return;
    double best = -INFINITY;
    float cmin = INFINITY;
    int arg = 0;
    for (int j = 0; j < k; ++j) {
        const float c = dist[(size_t)j * n + i];
        const double x = -(double)c * inv_reg + sv[j];
        if (x > best) { best = x; arg = j; }
        cmin = c < cmin ? c : cmin;
    }
    label[i] = arg;
    if (cost_min) cost_min[i] = cmin;
}

struct sk_layout {
    int64_t B, off_state, off_v, off_u, off_pm, off_ps, total;
};

static inline int64_t sk_align(int64_t x) { return (x + 255) & ~(int64_t)255; }

static sk_layout sk_plan(int64_t n, int k)
{
    sk_layout L;
    L.B = (n + kSkPts - 1) / kSkPts;
    L.off_state = 0;
    L.off_v = sk_align((int64_t)sizeof(sk_state));
    L.off_u = L.off_v + sk_align(2 * (int64_t)k * 8);
    L.off_pm = L.off_u + sk_align(n * 8);
    L.off_ps = L.off_pm + sk_align(L.B * k * 8);
    L.total = L.off_ps + sk_align(L.B * k * 8);
    return L;
}

}  // namespace ure

using namespace ure;

extern "C" {

int64_t ure_ot_sinkhorn_scratch(int64_t n, int k)
{
    if (n < 1 || n > INT32_MAX || k < 1 || k > kSinkhornMaxK) return -1;
    return sk_plan(n, k).total;
}

int ure_ot_sinkhorn(const float *dist, int64_t n, int k, double reg, int num_iter_max, double stop_thr, double *u, double *v, int32_t *label,
                    float *cost_min, void *scratch, int64_t scratch_bytes, int32_t *iters, double *err, void *stream)
{
    URE_ARG(dist && v && label && scratch && iters && err);
    URE_ARG(n >= 1 && n <= INT32_MAX);
    URE_ARG(k >= 1 && k <= kSinkhornMaxK);
    URE_ARG(reg > 0 && std::isfinite(reg));
    URE_ARG(num_iter_max >= 1);
    URE_ARG(stop_thr >= 0);
    URE_ARG(scratch_bytes >= ure_ot_sinkhorn_scratch(n, k));
    const sk_layout P = sk_plan(n, k);
    char *base = static_cast<char *>(scratch);
    sk_state *dst = reinterpret_cast<sk_state *>(base + P.off_state);
    double *vbuf[2] = {reinterpret_cast<double *>(base + P.off_v), reinterpret_cast<double *>(base + P.off_v) + k};
    double *ud = u ? u : reinterpret_cast<double *>(base + P.off_u);
    double *pm = reinterpret_cast<double *>(base + P.off_pm), *ps = reinterpret_cast<double *>(base + P.off_ps);
    const double inv_reg = 1.0 / reg, loga = std::log(1.0 / (double)n), logb = std::log(1.0 / (double)k), eb = std::exp(logb);
    const unsigned blocks = (unsigned)P.B;
    hipStream_t s = static_cast<hipStream_t>(stream);

    URE_HIP(hipMemsetAsync(dst, 0, sizeof(sk_state), s));
    hipLaunchKernelGGL(sk_pass_kernel, dim3(blocks), dim3(kBlock), 0, s, dist, n, k, inv_reg, loga, (const double *)nullptr, ud, pm, ps,
                       (const sk_state *)dst, 1);
    hipLaunchKernelGGL(sk_combine_kernel, dim3(k), dim3(kBlock), 0, s, (const double *)pm, (const double *)ps, P.B, logb, vbuf[0],
                       (const sk_state *)dst);
    URE_HIP(hipGetLastError());
    // batches of 10, 20, 40, 80, 160, 160, ... iterations between host reads of the stop word; the launches a batch holds
    // beyond the stop return at once
    sk_state host{};
    int ii = 0;
    for (int batch = 10; ii < num_iter_max; batch = std::min(2 * batch, 160)) {
        const int end = std::min(num_iter_max, ii + batch);
        for (; ii < end; ++ii) {
            hipLaunchKernelGGL(sk_pass_kernel, dim3(blocks), dim3(kBlock), 0, s, dist, n, k, inv_reg, loga, (const double *)vbuf[ii & 1], ud, pm,
                               ps, (const sk_state *)dst, 0);
            hipLaunchKernelGGL(sk_combine_kernel, dim3(k), dim3(kBlock), 0, s, (const double *)pm, (const double *)ps, P.B, logb,
                               vbuf[(ii + 1) & 1], (const sk_state *)dst);
            if (ii % 10 == 0)
                hipLaunchKernelGGL(sk_check_kernel, dim3(1), dim3(kBlock), 0, s, (const double *)vbuf[ii & 1], (const double *)vbuf[(ii + 1) & 1], k,
                                   eb, stop_thr, ii, dst);
        }
        URE_HIP(hipGetLastError());
        URE_HIP(hipMemcpyAsync(&host, dst, sizeof(sk_state), hipMemcpyDeviceToHost, s));
        URE_HIP(hipStreamSynchronize(s));
        if (host.stop) break;
    }
    if (host.bad) return fail(-2, "ure_ot_sinkhorn: the marginal error is not finite (%g) at iteration %d: reg = %g too small for the costs?",
                              host.err, host.stop - 1, reg);
    const int last = host.stop ? host.stop - 1 : num_iter_max - 1;
    const double *vf = vbuf[last & 1];
    hipLaunchKernelGGL(sk_label_kernel, dim3(blocks), dim3(kBlock), 0, s, dist, n, k, inv_reg, vf, label, cost_min);
    URE_HIP(hipGetLastError());
    URE_HIP(hipMemcpyAsync(v, vf, (size_t)k * sizeof(double), hipMemcpyDeviceToDevice, s));
    URE_HIP(hipStreamSynchronize(s));
    *iters = host.stop ? host.stop : num_iter_max;
    *err = host.err;
    return 0;
}

}  // extern "C"

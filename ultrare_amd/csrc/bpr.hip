// bpr.hip -- BPR training with device-side negative sampling (include/ultrare_bpr.h; the contract is ultrare_amd/bpr.py): the
// per-epoch negative draw and the index of the entries by their negative item, and per step the coefficient pass and the two
// gradient walks that stand where gcn.hip's residual pass and masked walks stand in an MSE step.
//
// The walks are row_walk.h's: a group of G = d / 4 lanes owns an output row, the chain of a (row, column) is one lane's, in
// ascending entry position, never split; theirs is what a fetch reads (the negative beside the item, the loss term of the entry's
// own x) and what a term adds.  Every float operation is a rounded one of its own (gcn_ops.h).  The index is a stable
// LSD radix sort of (negative item, CSR position) with 8-bit digits: per pass a histogram of every tile of kSortTile entries, one
// scan of the (digit, tile) counts and a scatter that ranks a tile's entries in order.  Integer atomics only in the histograms.
#include "gcn_ops.h"

namespace ure {
namespace {

constexpr int kSortRounds = 4;
constexpr int kSortTile = kBlock * kSortRounds;     // entries of a workgroup; entry `round * kBlock + thread` of its tile is a thread's
constexpr int kDigits = 256;
static_assert(kDigits == kBlock, "a thread of the sort kernels owns one digit");

__device__ __forceinline__ uint64_t mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// neg[q]: the r-th item user u has none of, r drawn from (key, epoch, file position).  #{t : c[t] - t <= r} by binary search: the
// keys c[t] - t of a row of distinct ascending items do not decrease.
__global__ __launch_bounds__(kBlock) void bpr_sample_kernel(const int64_t *__restrict__ off_d, const int32_t *__restrict__ col_d,
                                                            const int32_t *__restrict__ row_u, const int32_t *__restrict__ pos, int64_t nnz,
                                                            int64_t n_user, int64_t n_item, int64_t nnz_d, uint64_t key, uint64_t epoch,
                                                            int32_t *__restrict__ neg)
{
    const unsigned last_u = (unsigned)(n_user - 1);
    for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < nnz; q += (int64_t)gridDim.x * kBlock) {
        const unsigned u = min((unsigned)ldg(row_u + q), last_u);
        const uint64_t p = (uint64_t)(unsigned)ldg(pos + q);
        // (a distinct-item CSR that is not one -- offsets out of order or past its end -- reads inside col_d all the same)
        const int64_t b = min(max(ldg(off_d + u), (int64_t)0), nnz_d), e = min(max(ldg(off_d + u + 1), b), nnz_d);
        const int64_t m = max(n_item - (e - b), (int64_t)0);
        const uint64_t z = mix64(key + 0x9E3779B97F4A7C15ull * (1ull + (epoch << 32) + p));
        const int64_t r = (int64_t)(((z >> 32) * (uint64_t)m) >> 32);
        int64_t lo = b, hi = e;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)ldg(col_d + mid) - (mid - b) <= r)
                lo = mid + 1;
            else
                hi = mid;
        }
        stg(neg + q, (int32_t)min(r + (lo - b), n_item - 1));
    }
}

// The key of entry i in a pass: pass 0 reads the negatives themselves (clamped to the catalogue), later passes the keys the
// pass before wrote.
__device__ __forceinline__ unsigned sort_key(const int32_t *__restrict__ keys, int64_t i, unsigned last_item)
{
    return min((unsigned)ldg(keys + i), last_item);
}

// counts[digit * tiles + tile] = entries of the tile with that digit.  Every word of counts is written.
__global__ __launch_bounds__(kBlock) void bpr_sort_hist_kernel(const int32_t *__restrict__ keys, int64_t nnz, unsigned last_item, int shift,
                                                               int64_t tiles, int32_t *__restrict__ counts)
{
    __shared__ int hist[kDigits];
    hist[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kSortTile;
#pragma unroll
    for (int r = 0; r < kSortRounds; ++r) {
        const int64_t i = base + r * kBlock + threadIdx.x;
        if (i < nnz) atomicAdd(&hist[(sort_key(keys, i, last_item) >> shift) & (kDigits - 1)], 1);      // (integers: exact in any order)
    }
    __syncthreads();
    stg(counts + (int64_t)threadIdx.x * tiles + blockIdx.x, (int32_t)hist[threadIdx.x]);
}

// The exclusive scan of counts [kDigits * tiles] in place, one workgroup: thread t owns digit t's row of `tiles` words.
__global__ __launch_bounds__(kDigits) void bpr_sort_scan_kernel(int32_t *__restrict__ counts, int64_t tiles)
{
    __shared__ int part[kDigits];
    int32_t *__restrict__ mine = counts + (int64_t)threadIdx.x * tiles;
    int sum = 0;
    for (int64_t i = 0; i < tiles; ++i) sum += ldg(mine + i);
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int o = 1; o < kDigits; o <<= 1) {
        const int t = (int)threadIdx.x >= o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += t;
        __syncthreads();
    }
    int run = part[threadIdx.x] - sum;
    for (int64_t i = 0; i < tiles; ++i) {
        const int c = ldg(mine + i);
        stg(mine + i, (int32_t)run);
        run += c;
    }
}

// One pass's scatter.  A tile's entries are ranked in their order (round, wave, lane): the lanes of a wave that hold one digit
// find each other with eight ballots, the waves of a round are ordered through wave_cnt, the rounds through running.
__global__ __launch_bounds__(kBlock) void bpr_sort_scatter_kernel(const int32_t *__restrict__ keys, const int32_t *__restrict__ vals, int64_t nnz,
                                                                  unsigned last_item, int shift, int64_t tiles, const int32_t *__restrict__ counts,
                                                                  int32_t *__restrict__ keys_out, int32_t *__restrict__ vals_out)
{
    __shared__ int gbase[kDigits], running[kDigits], wave_cnt[kWavesPerBlock][kDigits];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    gbase[threadIdx.x] = ldg(counts + (int64_t)threadIdx.x * tiles + blockIdx.x);
    running[threadIdx.x] = 0;
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; ++w) wave_cnt[w][threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kSortTile;
    for (int r = 0; r < kSortRounds; ++r) {
        const int64_t i = base + r * kBlock + threadIdx.x;
        const bool valid = i < nnz;
        const unsigned key = valid ? sort_key(keys, i, last_item) : 0u;
        const int val = valid ? (vals ? ldg(vals + i) : (int32_t)i) : 0;
        const int digit = (int)((key >> shift) & (kDigits - 1));
        uint64_t peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (digit >> b) & 1;
            const uint64_t has = __ballot(bit);
            peers &= bit ? has : ~has;
        }
        const int below = __popcll(peers & ((1ull << lane) - 1ull));
        if (valid && below == 0) wave_cnt[wave][digit] = __popcll(peers);
        __syncthreads();
        if (valid) {
            int at = running[digit] + below;
            for (int w = 0; w < wave; ++w) at += wave_cnt[w][digit];
            const int64_t dst = (int64_t)gbase[digit] + at;
            if (dst >= 0 && dst < nnz) {                   // (always, for counts this call made from the same keys)
                stg(keys_out + dst, (int32_t)key);
                stg(vals_out + dst, (int32_t)val);
            }
        }
        __syncthreads();
        int s = 0;
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; ++w) {
            s += wave_cnt[w][threadIdx.x];
            wave_cnt[w][threadIdx.x] = 0;
        }
        running[threadIdx.x] += s;
        __syncthreads();
    }
}

// off_n[i] = the first sorted position whose key is >= i (i = 0 .. n_item), usr_n[t] = row_u[map_n[t]].
__global__ __launch_bounds__(kBlock) void bpr_index_finish_kernel(const int32_t *__restrict__ sorted_keys, const int32_t *__restrict__ map_n,
                                                                  const int32_t *__restrict__ row_u, int64_t nnz, int64_t n_item,
                                                                  int64_t *__restrict__ off_n, int32_t *__restrict__ usr_n)
{
    const unsigned last_pos = (unsigned)(nnz - 1);
    const int64_t n = max(nnz, n_item + 1);
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < n; t += (int64_t)gridDim.x * kBlock) {
        if (t < nnz) stg(usr_n + t, ldg(row_u + min((unsigned)ldg(map_n + t), last_pos)));
        if (t <= n_item) {
            int64_t lo = 0, hi = nnz;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if ((int64_t)ldg(sorted_keys + mid) < t)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            stg(off_n + t, lo);
        }
    }
}

__device__ __forceinline__ double bpr_loss_term(float x)
{
    const double xd = (double)x;
    return fmax(-xd, 0.0) + log1p(exp(-fabs(xd)));
}

// The coefficient pass: gcn_residual_kernel's shape, two dots that share the user row.
template <int LPR>
__global__ __launch_bounds__(kBlock) void bpr_coef_kernel(const int32_t *__restrict__ row, const int32_t *__restrict__ col, const int32_t *__restrict__ neg,
                                                          const int32_t *__restrict__ tag, int64_t nnz, int step, const float *__restrict__ U,
                                                          const float *__restrict__ V, int64_t n_user, int64_t n_item, float *__restrict__ w_out,
                                                          float *__restrict__ x_out, float *__restrict__ pos_out, float *__restrict__ neg_out)
{
    const PairLanes<LPR> L;
    const unsigned last_u = (unsigned)(n_user - 1), last_i = (unsigned)(n_item - 1);
    for (int64_t base = L.wave_id * L.G; base < nnz; base += L.n_waves * L.G) {
        const int64_t k = base + L.grp;
        const bool in = k < nnz && ldg(tag + k) == step;
        float4 a = f4_zero(), c = f4_zero(), n = f4_zero();
        if (in) {
            a = ldg_f4(U + (size_t)min((unsigned)ldg(row + k), last_u) * L.D + 4 * L.sub);
            c = ldg_f4(V + (size_t)min((unsigned)ldg(col + k), last_i) * L.D + 4 * L.sub);
            n = ldg_f4(V + (size_t)min((unsigned)ldg(neg + k), last_i) * L.D + 4 * L.sub);
        }
        const float sp = pair_dot<LPR>(a, c), sn = pair_dot<LPR>(a, n);
        if (k < nnz && L.sub == 0) {
            const float x = __fsub_rn(sp, sn);
            stg(x_out + k, in ? x : 0.f);
            stg(w_out + k, in ? (float)(-1.0 / (1.0 + exp((double)x))) : 0.f);
            if (pos_out) stg(pos_out + k, in ? sp : 0.f);
            if (neg_out) stg(neg_out + k, in ? sn : 0.f);
        }
    }
}

// G_u[r] = sum over user r's entries in the batch of w (V[item] - V[negative]), the negative fetched beside the item.  The fetch
// also turns its own entry's x into the loss term, so a tile's terms cost one evaluation each; the row's float64 chain receives
// them in entry order in every lane (lane 0 stores it).
template <int G>
__global__ __launch_bounds__(kBlock) void bpr_grad_user_kernel(const int64_t *__restrict__ off, const int32_t *__restrict__ col, const int32_t *__restrict__ neg,
                                                               const int32_t *__restrict__ tag, const float *__restrict__ w, const float *__restrict__ x,
                                                               int64_t n_user, int64_t n_item, int step, const float *__restrict__ V,
                                                               float *__restrict__ Gout, double *__restrict__ row_loss)
{
    constexpr int D = 4 * G;
    const RowLanes<G> L;
    if (L.past(n_user)) return;
    const unsigned last = (unsigned)(n_item - 1);
    const float *__restrict__ v = V + 4 * L.sub;
    float4 g = f4_zero();
    double loss = 0.0;
    struct Entry { unsigned j, n; float w; double t; bool in; };
    tile_walk<G>(
        ldg(off + L.r), ldg(off + L.r + 1), L.sub,
        [&](int64_t k, bool inside) {
            Entry mine{0u, 0u, 0.f, 0.0, false};
            if (inside) {
                mine.in = ldg(tag + k) == step;
                if (mine.in) {
                    mine.w = ldg(w + k);
                    mine.t = bpr_loss_term(ldg(x + k));
                    mine.j = min((unsigned)ldg(col + k), last);
                    mine.n = min((unsigned)ldg(neg + k), last);
                }
            }
            return mine;
        },
        [&](const Entry &mine, int u) {
            if (!group_read<G>((int)mine.in, u)) return;
            const unsigned j = group_read<G>(mine.j, u), n = group_read<G>(mine.n, u);
            const float ww = group_read<G>(mine.w, u);
            g = f4_add(g, f4_scale(ww, f4_sub(ldg_f4(v + (size_t)j * D), ldg_f4(v + (size_t)n * D))));
            loss += group_read<G>(mine.t, u);
        });
    stg_f4(Gout + (size_t)L.r * D + 4 * L.sub, g);
    if (row_loss && L.sub == 0) stg(row_loss + L.r, loss);
}

// One part of an item's chain: the entries [b, e) of `idx` (their users) and `map` (their CSR positions), those of the batch
// added as coefficient * U[user], coefficient = w or fl(-w).
template <int G, bool NEGATE>
__device__ __forceinline__ float4 bpr_item_part(float4 g, int64_t b, int64_t e, int sub, const int32_t *__restrict__ idx, const int32_t *__restrict__ map,
                                                const int32_t *__restrict__ tag, const float *__restrict__ w, unsigned last_user, unsigned last_pos,
                                                int step, const float *__restrict__ x)
{
    struct Entry { unsigned j; float w; bool in; };
    tile_walk<G>(
        b, e, sub,
        [&](int64_t k, bool inside) {
            Entry mine{0u, 0.f, false};
            if (inside) {
                const unsigned q = entry_pos<true>(map, k, last_pos);
                mine.in = ldg(tag + q) == step;
                if (mine.in) {
                    mine.w = NEGATE ? -ldg(w + q) : ldg(w + q);
                    mine.j = min((unsigned)ldg(idx + k), last_user);
                }
            }
            return mine;
        },
        [&](const Entry &mine, int u) {
            if (!group_read<G>((int)mine.in, u)) return;
            const unsigned j = group_read<G>(mine.j, u);
            g = f4_mul_add(g, group_read<G>(mine.w, u), ldg_f4(x + (size_t)j * (4 * G)));
        });
    return g;
}

// G_i[r]: item r's CSC row (through to_csr), then -- in the same accumulator -- its row of the negative index.
template <int G>
__global__ __launch_bounds__(kBlock) void bpr_grad_item_kernel(const int64_t *__restrict__ off_i, const int32_t *__restrict__ row, const int32_t *__restrict__ to_csr,
                                                               const int64_t *__restrict__ off_n, const int32_t *__restrict__ map_n,
                                                               const int32_t *__restrict__ usr_n, const int32_t *__restrict__ tag,
                                                               const float *__restrict__ w, int64_t n_item, int64_t n_user, int64_t nnz, int step,
                                                               const float *__restrict__ U, float *__restrict__ Gout)
{
    const RowLanes<G> L;
    if (L.past(n_item)) return;
    const unsigned last_user = (unsigned)(n_user - 1), last_pos = (unsigned)(nnz - 1);
    const float *__restrict__ x = U + 4 * L.sub;
    // (offsets are read as they are in gcn.hip; the negative index's are clamped to its arrays, which this library made)
    float4 g = bpr_item_part<G, false>(f4_zero(), ldg(off_i + L.r), ldg(off_i + L.r + 1), L.sub, row, to_csr, tag, w, last_user, last_pos, step, x);
    const int64_t nb = min(max(ldg(off_n + L.r), (int64_t)0), nnz), ne = min(max(ldg(off_n + L.r + 1), nb), nnz);
    g = bpr_item_part<G, true>(g, nb, ne, L.sub, usr_n, map_n, tag, w, last_user, last_pos, step, x);
    stg_f4(Gout + (size_t)L.r * (4 * G) + 4 * L.sub, g);
}

inline int64_t align256(int64_t bytes) { return (bytes + 255) / 256 * 256; }
inline int64_t sort_tiles(int64_t nnz) { return (nnz + kSortTile - 1) / kSortTile; }
inline int sort_passes(int64_t n_item)
{
    int p = 1;
    while (p < 4 && ((int64_t)1 << (8 * p)) < n_item) ++p;
    return p;
}

}  // namespace
}  // namespace ure

using namespace ure;

extern "C" int ure_bpr_sample(const int64_t *off_d, const int32_t *col_d, int64_t nnz_d, const int32_t *row_u, const int32_t *pos, int64_t nnz,
                              int64_t n_user, int64_t n_item, uint64_t key, int32_t epoch, int32_t *neg, void *stream)
{
    URE_ARG(off_d && col_d && row_u && pos && neg);
    URE_ARG(nnz >= 1 && nnz <= INT32_MAX && nnz_d >= 1 && nnz_d <= nnz && epoch >= 0);
    URE_ARG(n_user >= 1 && n_user <= INT32_MAX && n_item >= 1 && n_item <= INT32_MAX);
    URE_ARG(apart(neg, nnz * 4, row_u, nnz * 4) && apart(neg, nnz * 4, pos, nnz * 4) && apart(neg, nnz * 4, col_d, nnz_d * 4) &&
            apart(neg, nnz * 4, off_d, (n_user + 1) * 8));
    hipLaunchKernelGGL(bpr_sample_kernel, dim3(stream_blocks(nnz)), dim3(kBlock), 0, (hipStream_t)stream, off_d, col_d, row_u, pos, nnz, n_user, n_item,
                       nnz_d, key, (uint64_t)epoch, neg);
    URE_HIP(hipGetLastError());
    return 0;
}

extern "C" int64_t ure_bpr_index_scratch(int64_t nnz, int64_t n_item)
{
    if (nnz <= 0 || nnz > INT32_MAX || n_item <= 0 || n_item > INT32_MAX) return 0;
    return 3 * align256(nnz * 4) + align256(sort_tiles(nnz) * kDigits * 4);
}

extern "C" int ure_bpr_index(const int32_t *neg, const int32_t *row_u, int64_t nnz, int64_t n_item, int64_t *off_n, int32_t *map_n, int32_t *usr_n,
                             void *scratch, int64_t scratch_bytes, void *stream)
{
    URE_ARG(neg && row_u && off_n && map_n && usr_n && scratch);
    URE_ARG(nnz >= 1 && nnz <= INT32_MAX && n_item >= 1 && n_item <= INT32_MAX);
    URE_ARG(scratch_bytes >= ure_bpr_index_scratch(nnz, n_item) && (uintptr_t)scratch % 4 == 0);
    const int64_t nb = nnz * 4, nb_off = (n_item + 1) * 8;
    URE_ARG(apart(map_n, nb, usr_n, nb) && apart(map_n, nb, off_n, nb_off) && apart(usr_n, nb, off_n, nb_off));
    for (const void *out : {(const void *)map_n, (const void *)usr_n})
        URE_ARG(apart(out, nb, neg, nb) && apart(out, nb, row_u, nb) && apart(out, nb, scratch, scratch_bytes));
    URE_ARG(apart(off_n, nb_off, neg, nb) && apart(off_n, nb_off, row_u, nb) && apart(off_n, nb_off, scratch, scratch_bytes));
    URE_ARG(apart(scratch, scratch_bytes, neg, nb) && apart(scratch, scratch_bytes, row_u, nb));
    hipStream_t st = (hipStream_t)stream;
    char *base = (char *)scratch;
    int32_t *key_buf[2] = {(int32_t *)base, (int32_t *)(base + align256(nb))};
    int32_t *val_buf = (int32_t *)(base + 2 * align256(nb)), *counts = (int32_t *)(base + 3 * align256(nb));
    const int64_t tiles = sort_tiles(nnz);
    const int passes = sort_passes(n_item);
    const unsigned last_item = (unsigned)(n_item - 1);
    const int32_t *src_key = neg, *src_val = nullptr;       // (pass 0: the values are the positions themselves)
    for (int p = 0; p < passes; ++p) {
        int32_t *dst_key = key_buf[p & 1], *dst_val = (passes - 1 - p) % 2 == 0 ? map_n : val_buf;
        hipLaunchKernelGGL(bpr_sort_hist_kernel, dim3((unsigned)tiles), dim3(kBlock), 0, st, src_key, nnz, last_item, 8 * p, tiles, counts);
        hipLaunchKernelGGL(bpr_sort_scan_kernel, dim3(1), dim3(kDigits), 0, st, counts, tiles);
        hipLaunchKernelGGL(bpr_sort_scatter_kernel, dim3((unsigned)tiles), dim3(kBlock), 0, st, src_key, src_val, nnz, last_item, 8 * p, tiles, counts,
                           dst_key, dst_val);
        src_key = dst_key;
        src_val = dst_val;
    }
    hipLaunchKernelGGL(bpr_index_finish_kernel, dim3(stream_blocks(std::max(nnz, n_item + 1))), dim3(kBlock), 0, st, src_key, map_n, row_u, nnz, n_item,
                       off_n, usr_n);
    URE_HIP(hipGetLastError());
    return 0;
}

extern "C" int ure_bpr_coef(const int32_t *row, const int32_t *col, const int32_t *neg, const int32_t *tag, int64_t nnz, int32_t step, const float *U,
                            const float *V, int64_t n_user, int64_t n_item, int32_t d, float *w, float *x, float *pos_out, float *neg_out, void *stream)
{
    URE_GCN_SIZES(n_user, n_item, d);
    URE_ARG(row && col && neg && tag && U && V && w && x);
    URE_ARG(nnz >= 1 && nnz <= INT32_MAX && step >= 0);
    URE_ARG(apart(w, nnz * 4, x, nnz * 4));
    hipStream_t st = (hipStream_t)stream;
    dispatch_group_width(d / 4, [&](auto lw) {
        constexpr int LPR = decltype(lw)::value;
        hipLaunchKernelGGL(bpr_coef_kernel<LPR>, dim3(pair_blocks(nnz, kWave / LPR, 4096)), dim3(kBlock), 0, st, row, col, neg, tag, nnz, (int)step, U, V,
                           n_user, n_item, w, x, pos_out, neg_out);
    });
    URE_HIP(hipGetLastError());
    return 0;
}

extern "C" int ure_bpr_grad_user(const int64_t *off, const int32_t *col, const int32_t *neg, const int32_t *tag, const float *w, const float *x,
                                 int64_t n_user, int64_t n_item, int64_t nnz, int32_t step, const float *V, int32_t d, float *G_out, double *row_loss,
                                 void *stream)
{
    URE_GCN_SIZES(n_user, n_item, d);
    URE_ARG(off && col && neg && tag && w && x && V && G_out);
    URE_ARG(nnz >= 1 && nnz <= INT32_MAX && step >= 0);
    URE_ARG(apart(G_out, n_user * d * 4, V, n_item * d * 4));
    hipStream_t st = (hipStream_t)stream;
    dispatch_group_width(d / 4, [&](auto gw) {
        constexpr int G = decltype(gw)::value;
        hipLaunchKernelGGL(bpr_grad_user_kernel<G>, dim3(group_blocks(n_user, G)), dim3(kBlock), 0, st, off, col, neg, tag, w, x, n_user, n_item,
                           (int)step, V, G_out, row_loss);
    });
    URE_HIP(hipGetLastError());
    return 0;
}

extern "C" int ure_bpr_grad_item(const int64_t *off_i, const int32_t *row, const int32_t *to_csr, const int64_t *off_n, const int32_t *map_n,
                                 const int32_t *usr_n, const int32_t *tag, const float *w, int64_t n_item, int64_t n_user, int64_t nnz, int32_t step,
                                 const float *U, int32_t d, float *G_out, void *stream)
{
    URE_GCN_SIZES(n_item, n_user, d);
    URE_ARG(off_i && row && to_csr && off_n && map_n && usr_n && tag && w && U && G_out);
    URE_ARG(nnz >= 1 && nnz <= INT32_MAX && step >= 0);
    URE_ARG(apart(G_out, n_item * d * 4, U, n_user * d * 4));
    hipStream_t st = (hipStream_t)stream;
    dispatch_group_width(d / 4, [&](auto gw) {
        constexpr int G = decltype(gw)::value;
        hipLaunchKernelGGL(bpr_grad_item_kernel<G>, dim3(group_blocks(n_item, G)), dim3(kBlock), 0, st, off_i, row, to_csr, off_n, map_n, usr_n, tag, w,
                           n_item, n_user, nnz, (int)step, U, G_out);
    });
    URE_HIP(hipGetLastError());
    return 0;
}

// pair_dist.hip -- reductions of an implicit n x n user-by-user distance matrix, for gfx950.
//
// The comparison clusterers of utils.py:422-611 (k-medoids, label propagation, the k-nearest-neighbour user graph) each
// need only a small reduction of D: the n_nb smallest entries of a row, the row sums, the columns of the medoids, or
// per-row sums of exp(-D) grouped by a label.  D is never written to memory.  A workgroup of 256 threads owns kTile
// rows and walks the columns kTile at a time; each step puts one kTile x kTile tile of D into LDS (pair_tile) and one
// wave folds it into its rows' state in column order.
//
// The source of D is a compile-time choice:
//   URE_DIST_GIVEN       D[u, v] = G[u * n + v], a row-major float32 array (the reference's own contract).
//   URE_DIST_EUCLIDEAN   sqrt(sum_j t_j^2), t_j = x_uj - y_vj: the direct difference form, never |x|^2 - 2 x.y + |y|^2.
//   URE_DIST_COSINE      1 - x.y / (|x| |y|), clamped to [0, 2]; 1 when either row is zero; 0 on the diagonal.
//   URE_DIST_MANHATTAN   sum_j |t_j|.
// Streamed sums run over j = 0, 1, ..., d - 1 in order, one fmaf / add per term into a single float32 accumulator
// (|x|^2 the same way), whatever the tile: D[u, v] is a pure function of rows u and v, D[u, v] == D[v, u] bit for bit
// (t^2 and |t| do not see the sign of t, x.y's products commute) and D[u, u] == 0.
//
// The three streamed sources also come from a sparse matrix (csr_pair_tile: the rows of a canonical CSR, the same D bit for
// bit, the n x d array never formed); the four reductions are written once, over the tile source (DenseSrc / CsrSrc).
//
// Nothing is accumulated with atomics, and every reduction takes its terms in an order fixed by n alone, so each
// result is bitwise reproducible and independent of the grid, the tile and how the query rows are batched.
#include "ure_internal.h"

#include <cmath>
#include <cstring>
#include <utility>

namespace ure {

constexpr int kTile = 64;                   // rows and columns of a tile of D
constexpr int kChunk = 16;                  // feature columns staged in LDS per step of a streamed tile
constexpr int kLdA = kTile + 1;             // LDS stride of the staged features (feature-major)
constexpr int kLdD = kTile + 1;             // LDS stride of the tile of D (row-major): a lane per row reads one column conflict-free
constexpr int kPairMaxNb = 128;
constexpr int kPairMaxGroups = 128;
constexpr int kPairMaxSplits = 64;
constexpr int kPairTargetBlocks = 1024;     // workgroups the kNN split aims for
constexpr int kStackDepth = 16;             // pairwise-sum partials pending per row (a buffer's tree has depth < 8)
constexpr int64_t kGivenMaxN = 1518500249;  // floor(sqrt(INT64_MAX / 4)): n * n * 4 bytes fits in int64

struct TileLds {
    float a[kChunk * kLdA];     // row features, feature-major
    float b[kChunk * kLdA];     // column features
    float d[kTile * kLdD];      // the tile of D
    int64_t row[kTile];         // source rows of the tile (-1: none)
    int64_t col[kTile];         // source columns (-1: none)
};

// One kTile x kTile tile of D into t.d: t.d[r * kLdD + c] = D[t.row[r], t.col[c]] (row or column -1: left undefined).
// TRANS (given source only): D[t.col[c], t.row[r]] instead.  Every thread of the workgroup calls it; it begins and ends
// with a barrier, so the caller may rewrite row / col before and read d after.
template <int MET, bool TRANS>
__device__ __forceinline__ void pair_tile(const float *__restrict__ src, int64_t n, int d, TileLds &t)
{
    const int tid = threadIdx.x;
    __syncthreads();
    if (MET == URE_DIST_GIVEN) {
        for (int e = tid; e < kTile * kTile; e += kBlock) {
            const int r = TRANS ? e % kTile : e / kTile, c = TRANS ? e / kTile : e % kTile;
            const int64_t u = t.row[r], v = t.col[c];
            if (u >= 0 && v >= 0) t.d[r * kLdD + c] = TRANS ? ldg(src + v * n + u) : ldg(src + u * n + v);
        }
        __syncthreads();
        return;
    }
    // thread (ty, tx) owns rows ty + 16 i and columns tx + 16 j, i, j < 4
    const int ty = tid >> 4, tx = tid & 15;
    float acc[4][4], na[4], nb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        na[i] = nb[i] = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    }
    for (int k0 = 0; k0 < d; k0 += kChunk) {
        const int kc = min(kChunk, d - k0);
        for (int e = tid; e < kTile * kChunk; e += kBlock) {
            const int r = e / kChunk, kk = e % kChunk;
            const int64_t u = t.row[r], v = t.col[r];
            const bool in = kk < kc;
            t.a[kk * kLdA + r] = (in && u >= 0) ? ldg(src + u * d + k0 + kk) : 0.f;
            t.b[kk * kLdA + r] = (in && v >= 0) ? ldg(src + v * d + k0 + kk) : 0.f;
        }
        __syncthreads();
        for (int kk = 0; kk < kc; ++kk) {
            float a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                a[i] = t.a[kk * kLdA + ty + 16 * i];
                b[i] = t.b[kk * kLdA + tx + 16 * i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (MET == URE_DIST_EUCLIDEAN) {
                        const float s = __fsub_rn(a[i], b[j]);
                        acc[i][j] = fmaf(s, s, acc[i][j]);
                    } else if (MET == URE_DIST_MANHATTAN) {
                        acc[i][j] = __fadd_rn(acc[i][j], fabsf(__fsub_rn(a[i], b[j])));
                    } else {
                        acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
                    }
                }
                if (MET == URE_DIST_COSINE) {
                    na[i] = fmaf(a[i], a[i], na[i]);
                    nb[i] = fmaf(b[i], b[i], nb[i]);
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = ty + 16 * i, c = tx + 16 * j;
            float v = acc[i][j];
            if (MET == URE_DIST_EUCLIDEAN) {
                v = __fsqrt_rn(v);
            } else if (MET == URE_DIST_COSINE) {
                const float den = __fmul_rn(__fsqrt_rn(na[i]), __fsqrt_rn(nb[j]));
                v = den == 0.f ? 1.f : __fsub_rn(1.f, __fdiv_rn(v, den));
                v = fminf(fmaxf(v, 0.f), 2.f);
                if (t.row[r] == t.col[c]) v = 0.f;
            }
            t.d[r * kLdD + c] = v;
        }
    }
    __syncthreads();
}

// ---- the CSR tile producer ------------------------------------------------------------------------------------------
// The same tile from a canonical CSR (ascending columns inside a row, no repeats, stored zeros kept), the n x n_item array
// never formed.  A dense term whose two operands are implicit zeros leaves its accumulator as it was (fmaf(0, 0, acc) ==
// acc, acc + |0 - 0| == acc, and the same for x.y and both |x|^2), so walking the UNION of the stored columns of rows u and
// v in ascending column, a column stored in one row only paired with 0.f, with the dense producer's own operation per term
// and its finishing step, gives the dense producer's bits.
//
// The tile's 2 kTile lists (kTile rows, then kTile columns) are staged in LDS one item-id window at a time: every list
// brings its next kCsrPairWindow entries, and the window ends below `hi`, the smallest column id that some list could not
// bring (INT32_MAX: every list is through).  Entries at or above `hi` wait for a later window; the list that set `hi`
// spends all it brought, so every window moves on, and the windows ascend, so each pair still sees its union in order.
// Thread (ty, tx) two-pointer-merges its 4 x 4 pairs inside the window; the accumulators live in registers across
// windows.  The squared norms of cosine are per list, summed by the thread that owns the list as its entries are spent.
constexpr int kCsrPairWindow = 32;              // entries a list stages per window (sparse_pair.WINDOW)
constexpr int kLdW = kCsrPairWindow + 1;        // LDS stride of a staged list
constexpr int kLists = 2 * kTile;

struct CsrTileLds {
    float d[kTile * kLdD];          // the tile of D
    int64_t row[kTile];             // source rows of the tile (-1: none)
    int64_t col[kTile];             // source columns (-1: none)
    int64_t cur[kLists];            // first entry of each list that no window has spent
    int64_t end[kLists];
    int32_t id[kLists * kLdW];      // the staged column ids
    float v[kLists * kLdW];         // ... and values
    float norm[kLists];             // cosine: |x|^2 over the spent entries
    int32_t cnt[kLists];            // staged entries below hi
    int32_t hi[2];                  // the window's end, of even and odd windows
};

template <int MET>
__device__ __forceinline__ void csr_pair_tile(const int64_t *__restrict__ row_off, const int32_t *__restrict__ col, const float *__restrict__ val,
                                              CsrTileLds &t)
{
    const int tid = threadIdx.x;
    const int ty = tid >> 4, tx = tid & 15;
    __syncthreads();
    if (tid < kLists) {
        const int64_t u = tid < kTile ? t.row[tid] : t.col[tid - kTile];
        t.cur[tid] = u >= 0 ? ldg(row_off + u) : 0;
        t.end[tid] = u >= 0 ? ldg(row_off + u + 1) : 0;
        t.norm[tid] = 0.f;
    }
    if (tid < 2) t.hi[tid] = INT32_MAX;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    __syncthreads();
    for (int w = 0;; w ^= 1) {
        // stage: entry p of list l; the owner of a list that has more than a window left bids its next id for hi
        for (int e = tid; e < kLists * kCsrPairWindow; e += kBlock) {
            const int l = e / kCsrPairWindow, p = e % kCsrPairWindow;
            const int64_t at = t.cur[l] + p;
            if (at < t.end[l]) {
                t.id[l * kLdW + p] = ldg(col + at);
                t.v[l * kLdW + p] = ldg(val + at);
            }
        }
        if (tid < kLists && t.cur[tid] + kCsrPairWindow < t.end[tid]) atomicMin(&t.hi[w], ldg(col + t.cur[tid] + kCsrPairWindow));
        __syncthreads();
        const int hi = t.hi[w];
        if (tid < kLists) {
            const int staged = (int)min<int64_t>(kCsrPairWindow, t.end[tid] - t.cur[tid]);
            int c = 0;
            float nn = t.norm[tid];
            while (c < staged && t.id[tid * kLdW + c] < hi) {
                if (MET == URE_DIST_COSINE) {
                    const float x = t.v[tid * kLdW + c];
                    nn = fmaf(x, x, nn);
                }
                ++c;
            }
            t.cnt[tid] = c;
            t.cur[tid] += c;
            t.norm[tid] = nn;
        }
        if (tid == 0) t.hi[w ^ 1] = INT32_MAX;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int la = (ty + 16 * i) * kLdW, ca = t.cnt[ty + 16 * i];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int lb = (kTile + tx + 16 * j) * kLdW, cb = t.cnt[kTile + tx + 16 * j];
                int pa = 0, pb = 0;
                int ia = pa < ca ? t.id[la] : INT32_MAX, ib = pb < cb ? t.id[lb] : INT32_MAX;
                float r = acc[i][j];
                while (pa < ca || pb < cb) {
                    const int m = min(ia, ib);
                    float a = 0.f, b = 0.f;
                    if (ia == m) {
                        a = t.v[la + pa];
                        ++pa;
                        ia = pa < ca ? t.id[la + pa] : INT32_MAX;
                    }
                    if (ib == m) {
                        b = t.v[lb + pb];
                        ++pb;
                        ib = pb < cb ? t.id[lb + pb] : INT32_MAX;
                    }
                    if (MET == URE_DIST_EUCLIDEAN) {
                        const float s = __fsub_rn(a, b);
                        r = fmaf(s, s, r);
                    } else if (MET == URE_DIST_MANHATTAN) {
                        r = __fadd_rn(r, fabsf(__fsub_rn(a, b)));
                    } else {
                        r = fmaf(a, b, r);
                    }
                }
                acc[i][j] = r;
            }
        }
        __syncthreads();
        if (hi == INT32_MAX) break;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = ty + 16 * i, c = tx + 16 * j;
            float v = acc[i][j];
            if (MET == URE_DIST_EUCLIDEAN) {
                // the correctly rounded root, which is what pair_tile's sixteen __fsqrt_rn compile to (np.sqrt's bits, as
                // tests/test_gpu_cluster.py holds them); spelled sqrtf here so that it does not hang on how this loop is
                // vectorized.  The norms of cosine take __fsqrt_rn as pair_tile's do: the hardware root in both.
                v = sqrtf(v);
            } else if (MET == URE_DIST_COSINE) {
                const float den = __fmul_rn(__fsqrt_rn(t.norm[r]), __fsqrt_rn(t.norm[kTile + c]));
                v = den == 0.f ? 1.f : __fsub_rn(1.f, __fdiv_rn(v, den));
                v = fminf(fmaxf(v, 0.f), 2.f);
                if (t.row[r] == t.col[c]) v = 0.f;
            }
            t.d[r * kLdD + c] = v;
        }
    }
    __syncthreads();
}

// The tile sources the reductions below are written over: Lds (d, row, col as TileLds names them) and tile<TRANS>(lds).
struct DenseArgs {
    const float *src;
    int64_t n;
    int d;
};
template <int MET>
struct DenseSrc {
    static constexpr int kMetric = MET;
    static constexpr bool kTakesGiven = true;
    using Lds = TileLds;
    DenseArgs a;
    template <bool TRANS>
    __device__ __forceinline__ void tile(Lds &t) const { pair_tile<MET, TRANS>(a.src, a.n, a.d, t); }
};
struct CsrArgs {
    const int64_t *row_off;
    const int32_t *col;
    const float *val;
};
template <int MET>
struct CsrSrc {
    static constexpr int kMetric = MET;
    static constexpr bool kTakesGiven = false;
    using Lds = CsrTileLds;
    CsrArgs a;
    template <bool TRANS>
    __device__ __forceinline__ void tile(Lds &t) const { csr_pair_tile<MET>(a.row_off, a.col, a.val, t); }
};

// Order-preserving 64-bit key of (distance, column): smaller distance first, then the smaller column; NaN above +inf.
__device__ __forceinline__ uint64_t pair_key(float v, int64_t col)
{
    uint32_t b = __float_as_uint(v);
    b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((uint64_t)b << 32) | (uint64_t)(uint32_t)col;
}
__device__ __forceinline__ float pair_key_dist(uint64_t key)
{
    const uint32_t b = (uint32_t)(key >> 32);
    return __uint_as_float((b & 0x80000000u) ? (b & 0x7fffffffu) : ~b);
}

// ---- kNN ------------------------------------------------------------------------------------------------------------
// Workgroup (blockIdx.x, blockIdx.y) = kTile query rows x the column span of split blockIdx.y.  Lane r of wave 0 keeps
// row r's n_nb smallest keys, ascending, in LDS (list[j * kTile + r]); a column enters only when its key is below the
// current n_nb-th, by insertion.  The list goes to keys[(split * n_query + q) * n_nb ...], unused places as ~0.
template <class SRC>
__global__ __launch_bounds__(kBlock) void pair_knn_kernel(const SRC s, int64_t n, const int32_t *__restrict__ query, int64_t n_query, int n_nb,
                                                          int64_t span, uint64_t *__restrict__ keys)
{
    using Lds = typename SRC::Lds;
    extern __shared__ uint64_t knn_lds[];
    Lds &t = *reinterpret_cast<Lds *>(knn_lds);
    uint64_t *list = knn_lds + (sizeof(Lds) + 7) / 8;
    const int tid = threadIdx.x;
    const int64_t q0 = (int64_t)blockIdx.x * kTile;
    const int64_t c_begin = (int64_t)blockIdx.y * span, c_end = min(n, c_begin + span);
    for (int e = tid; e < n_nb * kTile; e += kBlock) list[e] = ~(uint64_t)0;
    if (tid < kTile) t.row[tid] = q0 + tid < n_query ? (query ? (int64_t)query[q0 + tid] : q0 + tid) : -1;
    uint64_t thr = ~(uint64_t)0;
    for (int64_t v0 = c_begin; v0 < c_end; v0 += kTile) {
        if (tid < kTile) t.col[tid] = v0 + tid < c_end ? v0 + tid : -1;
        s.template tile<false>(t);
        if (tid < kTile && t.row[tid] >= 0) {
            const int cn = (int)min<int64_t>(kTile, c_end - v0);
            for (int c = 0; c < cn; ++c) {
                const uint64_t key = pair_key(t.d[tid * kLdD + c], v0 + c);
                if (key >= thr) continue;
                int j = n_nb - 1;
                while (j > 0 && list[(j - 1) * kTile + tid] > key) {
                    list[j * kTile + tid] = list[(j - 1) * kTile + tid];
                    --j;
                }
                list[j * kTile + tid] = key;
                thr = list[(n_nb - 1) * kTile + tid];
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < n_nb * kTile; e += kBlock) {
        const int r = e % kTile, j = e / kTile;
        if (q0 + r < n_query) keys[((int64_t)blockIdx.y * n_query + q0 + r) * n_nb + j] = list[j * kTile + r];
    }
}

// A thread per candidate (split s, query q, place p): its rank among all splits' candidates of q is p plus the
// number of smaller keys in every other split's (ascending) list.  Keys are unique, so the places < n_nb are each
// written once; the ~0 fillers rank at least n (>= n_nb) and are never written.
__global__ __launch_bounds__(kBlock) void pair_knn_merge_kernel(const uint64_t *__restrict__ keys, int64_t n_query, int n_nb, int splits,
                                                                float *__restrict__ dist, int32_t *__restrict__ idx)
{
    const int64_t total = n_query * n_nb * splits;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
        const int p = (int)(e % n_nb);
        const int64_t q = (e / n_nb) % n_query;
        const int s = (int)(e / ((int64_t)n_nb * n_query));
        const uint64_t key = keys[e];
        if (key == ~(uint64_t)0) continue;
        int64_t rank = p;
        for (int s2 = 0; s2 < splits && rank < n_nb; ++s2) {
            if (s2 == s) continue;
            const uint64_t *l = keys + ((int64_t)s2 * n_query + q) * n_nb;
            int lo = 0, hi = n_nb;                        // first place with l[place] >= key
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (l[mid] < key) lo = mid + 1;
                else hi = mid;
            }
            rank += lo;
        }
        if (rank < n_nb) {
            dist[q * n_nb + rank] = pair_key_dist(key);
            idx[q * n_nb + rank] = (int32_t)(uint32_t)key;
        }
    }
}

// ---- row sums in numpy's float32 order -----------------------------------------------------------------------------
// np.sum(A, axis=1) hands each row to pairwise_sum in buffers of 8192 elements (kNpBuf) and adds the buffer sums in
// order: R = p(a[0:8192]) + p(a[8192:16384]) + ...  pairwise_sum(a, m): m < 8 sequential from 0; m <= 128 one leaf of
// eight accumulators over stride-8 groups, ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the tail m % 8 in
// order; above, the halves h = m / 2 - (m / 2) % 8 and m - h summed the same way and added.  Every leaf but the last
// of a buffer starts at a multiple of 8 and has a multiple of 8 terms, so the walk takes the row eight columns at a
// time.  The leaves and the additions after each (how many finished right halves it closes) depend on m alone: thread
// 0 lists them for a full buffer and for the last one, table[i] = (length << 8) | closes, and every row folds its tile
// columns in through a stack of partial sums.
constexpr int64_t kNpBuf = 8192;
constexpr int kLeafCap = kNpBuf / 64 + 2;    // leaves of one buffer (every leaf but a lone one has >= 64 terms)

__device__ void rowsum_leaf_table(int64_t m, uint32_t *table, int64_t *stack)
{
    int sp = 0, n_leaf = 0;
    stack[sp++] = m << 8;                                   // length << 8 | closes; leaves come out in column order
    while (sp > 0) {
        const int64_t top = stack[--sp];
        const int64_t len = top >> 8;
        const int closes = (int)(top & 0xff);
        if (len <= 128) {
            table[n_leaf++] = ((uint32_t)len << 8) | (uint32_t)closes;
            continue;
        }
        int64_t h = len / 2;
        h -= h % 8;
        stack[sp++] = ((len - h) << 8) | (closes + 1);      // right half, after the left
        stack[sp++] = h << 8;
    }
}

template <class SRC>
__global__ __launch_bounds__(kBlock) void pair_rowsum_kernel(const SRC s, int64_t n, float *__restrict__ R)
{
    __shared__ typename SRC::Lds t;
    __shared__ float stk[kStackDepth * kTile];
    __shared__ int64_t build[kStackDepth];
    __shared__ uint32_t table[2][kLeafCap];                 // a full buffer, the last buffer
    const int tid = threadIdx.x;
    const int64_t u0 = (int64_t)blockIdx.x * kTile;
    const int64_t last = (n - 1) / kNpBuf * kNpBuf;          // first column of the last buffer
    if (tid == 0) {
        rowsum_leaf_table(min(n, kNpBuf), table[0], build);
        rowsum_leaf_table(n - last, table[1], build);
    }
    if (tid < kTile) t.row[tid] = u0 + tid < n ? u0 + tid : -1;
    // walk state (wave 0; uniform but for the values)
    int leaf = 0, sp = 0;
    int64_t pos = 0;              // column where the current leaf started
    float r[8], res = 0.f, total = 0.f;
    for (int64_t v0 = 0; v0 < n; v0 += kTile) {
        if (tid < kTile) t.col[tid] = v0 + tid < n ? v0 + tid : -1;
        s.template tile<false>(t);                    // (its first barrier also publishes the tables)
        if (tid < kTile) {
            const float *row = t.d + tid * kLdD;
            for (int g = 0; g < kTile && v0 + g < n; g += 8) {
                const uint32_t ent = table[v0 + g >= last ? 1 : 0][leaf];
                const int64_t L = ent >> 8;
                const int64_t at = v0 + g - pos;        // position of this group in the leaf
                const int64_t full = L - L % 8;
                if (L < 8) {
                    res = 0.f;
                    for (int j = 0; j < L; ++j) res = __fadd_rn(res, row[g + j]);
                } else if (at < full) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) r[j] = at == 0 ? row[g + j] : __fadd_rn(r[j], row[g + j]);
                    if (at + 8 == full)
                        res = __fadd_rn(__fadd_rn(__fadd_rn(r[0], r[1]), __fadd_rn(r[2], r[3])),
                                        __fadd_rn(__fadd_rn(r[4], r[5]), __fadd_rn(r[6], r[7])));
                    if (at + 8 < L) continue;           // the leaf goes on
                } else {
                    for (int j = 0; j < L - full; ++j) res = __fadd_rn(res, row[g + j]);
                }
                // the leaf is complete: push it and close the halves it ends
                float v = res;
                for (int c = 0; c < (int)(ent & 0xff); ++c) v = __fadd_rn(stk[--sp * kTile + tid], v);
                stk[sp++ * kTile + tid] = v;
                ++leaf;
                pos += L;
                if (pos == n || pos % kNpBuf == 0) {   // the buffer is complete (its stack holds one sum)
                    total = pos <= kNpBuf ? stk[tid] : __fadd_rn(total, stk[tid]);
                    sp = 0;
                    leaf = 0;
                }
            }
        }
    }
    if (tid < kTile && t.row[tid] >= 0) R[u0 + tid] = total;
}

// ---- columns --------------------------------------------------------------------------------------------------------
template <class SRC>
__global__ __launch_bounds__(kBlock) void pair_cols_kernel(const SRC s, int64_t n, const int32_t *__restrict__ cols, int m, float *__restrict__ out)
{
    __shared__ typename SRC::Lds t;
    const int tid = threadIdx.x;
    const int64_t u0 = (int64_t)blockIdx.x * kTile;
    const int c0 = blockIdx.y * kTile;
    if (tid < kTile) {
        t.row[tid] = u0 + tid < n ? u0 + tid : -1;
        t.col[tid] = c0 + tid < m ? (int64_t)cols[c0 + tid] : -1;
    }
    s.template tile<false>(t);
    for (int e = tid; e < kTile * kTile; e += kBlock) {
        const int r = e / kTile, c = e % kTile;
        if (u0 + r < n && c0 + c < m) out[(u0 + r) * m + c0 + c] = t.d[r * kLdD + c];
    }
}

// ---- label-grouped kernel sums (LPA, utils.py:471-475) ---------------------------------------------------------------
// W[u, g] = sum over i with label[i] = g of exp(-D[i, u]): float32 exp of each term, float64 sums over i = 0, 1, ...
// in order.  Lane r of wave 0 owns row u0 + r and its k sums (LDS acc[g * kTile + r]).
template <class SRC>
__global__ __launch_bounds__(kBlock) void pair_label_expsum_kernel(const SRC s, int64_t n, const int32_t *__restrict__ label, int k,
                                                                   double *__restrict__ W)
{
    using Lds = typename SRC::Lds;
    extern __shared__ uint64_t lp_lds[];
    Lds &t = *reinterpret_cast<Lds *>(lp_lds);
    double *acc = reinterpret_cast<double *>(lp_lds + (sizeof(Lds) + 7) / 8);       // [k][kTile]
    int32_t *lab = reinterpret_cast<int32_t *>(acc + (int64_t)k * kTile);           // [kTile]
    const int tid = threadIdx.x;
    const int64_t u0 = (int64_t)blockIdx.x * kTile;
    for (int e = tid; e < k * kTile; e += kBlock) acc[e] = 0.0;
    if (tid < kTile) t.row[tid] = u0 + tid < n ? u0 + tid : -1;
    for (int64_t v0 = 0; v0 < n; v0 += kTile) {
        if (tid < kTile) {
            t.col[tid] = v0 + tid < n ? v0 + tid : -1;
            lab[tid] = v0 + tid < n ? label[v0 + tid] : -1;
        }
        s.template tile<SRC::kMetric == URE_DIST_GIVEN>(t);
        if (tid < kTile) {
            const int cn = (int)min<int64_t>(kTile, n - v0);
            for (int c = 0; c < cn; ++c) {
                const int g = lab[c];
                if ((unsigned)g >= (unsigned)k) continue;
                acc[g * kTile + tid] += (double)expf(-t.d[tid * kLdD + c]);
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < k * kTile; e += kBlock) {
        const int r = e / k, g = e % k;
        if (u0 + r < n) W[(u0 + r) * k + g] = acc[g * kTile + r];
    }
}

// ---- launch helpers --------------------------------------------------------------------------------------------------
static bool metric_ok(int metric)
{
    return metric == URE_DIST_GIVEN || metric == URE_DIST_EUCLIDEAN || metric == URE_DIST_COSINE || metric == URE_DIST_MANHATTAN;
}

static int check_source(const float *src, int64_t n, int32_t d, int32_t metric)
{
    URE_ARG(metric_ok(metric));
    URE_ARG(src);
    URE_ARG(n >= 1 && n <= INT32_MAX);
    URE_ARG(metric == URE_DIST_GIVEN || d >= 1);
    URE_ARG(metric != URE_DIST_GIVEN || n <= kGivenMaxN);
    return 0;
}

// Splits of the columns of a kNN call: (splits, columns per split, a multiple of kTile); `want` 0 = automatic.
static std::pair<int, int64_t> knn_splits(int64_t n_query, int64_t n, int32_t want)
{
    const int64_t col_tiles = (n + kTile - 1) / kTile, row_tiles = (n_query + kTile - 1) / kTile;
    int64_t s = want > 0 ? want : (kPairTargetBlocks + row_tiles - 1) / row_tiles;
    s = std::max<int64_t>(1, std::min<int64_t>({s, col_tiles, (int64_t)kPairMaxSplits}));
    const int64_t per = (col_tiles + s - 1) / s;
    return {(int)((col_tiles + per - 1) / per), per * kTile};
}

static int check_csr(const int64_t *row_off, const int32_t *col, const float *val, int64_t n, int64_t n_item, int32_t metric)
{
    URE_ARG(metric == URE_DIST_EUCLIDEAN || metric == URE_DIST_COSINE || metric == URE_DIST_MANHATTAN);      // (no given matrix on a CSR)
    URE_ARG(row_off && col && val);
    URE_ARG(n >= 1 && n <= INT32_MAX);
    URE_ARG(n_item >= 1 && n_item <= INT32_MAX);
    return 0;
}

template <class LDS>
static size_t tile_lds() { return (sizeof(LDS) + 7) / 8 * 8; }

// KERNEL<SRC<metric>>(SRC<metric>{args}, ...) for the metric of the call (checked before: one SRC serves)
#define URE_PAIR_DISPATCH(SRC, args, metric, KERNEL, grid, lds, st, ...)                                                                \
    if (metric == URE_DIST_EUCLIDEAN) KERNEL<SRC<URE_DIST_EUCLIDEAN>><<<grid, kBlock, lds, st>>>(SRC<URE_DIST_EUCLIDEAN>{args}, __VA_ARGS__);   \
    else if (metric == URE_DIST_COSINE) KERNEL<SRC<URE_DIST_COSINE>><<<grid, kBlock, lds, st>>>(SRC<URE_DIST_COSINE>{args}, __VA_ARGS__);       \
    else if (metric == URE_DIST_MANHATTAN) KERNEL<SRC<URE_DIST_MANHATTAN>><<<grid, kBlock, lds, st>>>(SRC<URE_DIST_MANHATTAN>{args}, __VA_ARGS__); \
    else if constexpr (SRC<URE_DIST_GIVEN>::kTakesGiven) KERNEL<SRC<URE_DIST_GIVEN>><<<grid, kBlock, lds, st>>>(SRC<URE_DIST_GIVEN>{args}, __VA_ARGS__);

// The four launches, shared by the dense / given entries and the CSR ones (the arguments are checked by the entry).
template <template <int> class SRC, class ARGS>
static int launch_knn(const ARGS &a, int64_t n, int32_t metric, const int32_t *query, int64_t n_query, int32_t n_nb, int32_t splits, float *dist,
                      int32_t *idx, void *scratch, hipStream_t st)
{
    using Lds = typename SRC<URE_DIST_EUCLIDEAN>::Lds;
    const auto sp = knn_splits(n_query, n, splits);
    const size_t lds = tile_lds<Lds>() + (size_t)n_nb * kTile * sizeof(uint64_t);
    const dim3 grid((unsigned)((n_query + kTile - 1) / kTile), (unsigned)sp.first);
    uint64_t *keys = static_cast<uint64_t *>(scratch);
    URE_PAIR_DISPATCH(SRC, a, metric, pair_knn_kernel, grid, lds, st, n, query, n_query, n_nb, sp.second, keys);
    URE_HIP(hipGetLastError());
    const int64_t total = n_query * n_nb * sp.first;
    const unsigned blocks = (unsigned)std::min<int64_t>((total + kBlock - 1) / kBlock, 8192);
    pair_knn_merge_kernel<<<blocks, kBlock, 0, st>>>(keys, n_query, n_nb, sp.first, dist, idx);
    URE_HIP(hipGetLastError());
    return 0;
}

template <template <int> class SRC, class ARGS>
static int launch_rowsum(const ARGS &a, int64_t n, int32_t metric, float *R, hipStream_t st)
{
    const unsigned blocks = (unsigned)((n + kTile - 1) / kTile);
    URE_PAIR_DISPATCH(SRC, a, metric, pair_rowsum_kernel, blocks, 0, st, n, R);
    URE_HIP(hipGetLastError());
    return 0;
}

template <template <int> class SRC, class ARGS>
static int launch_cols(const ARGS &a, int64_t n, int32_t metric, const int32_t *cols, int32_t m, float *out, hipStream_t st)
{
    const dim3 grid((unsigned)((n + kTile - 1) / kTile), (unsigned)((m + kTile - 1) / kTile));
    URE_PAIR_DISPATCH(SRC, a, metric, pair_cols_kernel, grid, 0, st, n, cols, m, out);
    URE_HIP(hipGetLastError());
    return 0;
}

template <template <int> class SRC, class ARGS>
static int launch_label_expsum(const ARGS &a, int64_t n, int32_t metric, const int32_t *label, int32_t k, double *W, hipStream_t st)
{
    using Lds = typename SRC<URE_DIST_EUCLIDEAN>::Lds;
    const size_t lds = tile_lds<Lds>() + (size_t)k * kTile * sizeof(double) + kTile * sizeof(int32_t);
    const unsigned blocks = (unsigned)((n + kTile - 1) / kTile);
    URE_PAIR_DISPATCH(SRC, a, metric, pair_label_expsum_kernel, blocks, lds, st, n, label, k, W);
    URE_HIP(hipGetLastError());
    return 0;
}

// numpy pairwise_sum over float64
static double np_pairwise_f64(const double *a, int64_t m)
{
    if (m < 8) {
        double r = 0.;
        for (int64_t i = 0; i < m; ++i) r += a[i];
        return r;
    }
    if (m <= 128) {
        double r[8];
        for (int j = 0; j < 8; ++j) r[j] = a[j];
        int64_t i = 8;
        for (; i < m - (m % 8); i += 8)
            for (int j = 0; j < 8; ++j) r[j] += a[i + j];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < m; ++i) res += a[i];
        return res;
    }
    int64_t h = m / 2;
    h -= h % 8;
    return np_pairwise_f64(a, h) + np_pairwise_f64(a + h, m - h);
}

// np.sum of a float64 vector: pairwise sums of buffers of kNpBuf elements, added in order
static double np_sum_f64(const double *a, int64_t n)
{
    double s = np_pairwise_f64(a, std::min(n, kNpBuf));
    for (int64_t i = kNpBuf; i < n; i += kNpBuf) s += np_pairwise_f64(a + i, std::min(n - i, kNpBuf));
    return s;
}

}  // namespace ure

using namespace ure;

extern "C" {

int64_t ure_pair_knn_scratch(int64_t n_query, int64_t n, int32_t n_nb, int32_t splits)
{
    if (n_query < 1 || n < 1 || n > INT32_MAX || n_nb < 1 || n_nb > kPairMaxNb || n_nb > n || splits < 0) return -1;
    return n_query * n_nb * knn_splits(n_query, n, splits).first * (int64_t)sizeof(uint64_t);
}

int ure_pair_knn(const float *src, int64_t n, int32_t d, int32_t metric, const int32_t *query, int64_t n_query, int32_t n_nb,
                 int32_t splits, float *dist, int32_t *idx, void *scratch, int64_t scratch_bytes, void *stream)
{
    if (int rc = check_source(src, n, d, metric)) return rc;
    URE_ARG(n_query >= 1 && n_query <= INT32_MAX);
    URE_ARG(n_nb >= 1 && n_nb <= kPairMaxNb);
    URE_ARG(n_nb <= n);
    URE_ARG(splits >= 0);
    URE_ARG(dist && idx);
    URE_ARG(scratch && scratch_bytes >= ure_pair_knn_scratch(n_query, n, n_nb, splits));
    return launch_knn<DenseSrc>(DenseArgs{src, n, d}, n, metric, query, n_query, n_nb, splits, dist, idx, scratch, static_cast<hipStream_t>(stream));
}

int ure_pair_rowsum(const float *src, int64_t n, int32_t d, int32_t metric, float *R, void *stream)
{
    if (int rc = check_source(src, n, d, metric)) return rc;
    URE_ARG(R);
    return launch_rowsum<DenseSrc>(DenseArgs{src, n, d}, n, metric, R, static_cast<hipStream_t>(stream));
}

int ure_pair_cols(const float *src, int64_t n, int32_t d, int32_t metric, const int32_t *cols, int32_t m, float *out, void *stream)
{
    if (int rc = check_source(src, n, d, metric)) return rc;
    URE_ARG(cols && m >= 1);
    URE_ARG(out);
    return launch_cols<DenseSrc>(DenseArgs{src, n, d}, n, metric, cols, m, out, static_cast<hipStream_t>(stream));
}

int ure_pair_label_expsum(const float *src, int64_t n, int32_t d, int32_t metric, const int32_t *label, int32_t k, double *W, void *stream)
{
    if (int rc = check_source(src, n, d, metric)) return rc;
    URE_ARG(label);
    URE_ARG(k >= 1 && k <= kPairMaxGroups);
    URE_ARG(W);
    return launch_label_expsum<DenseSrc>(DenseArgs{src, n, d}, n, metric, label, k, W, static_cast<hipStream_t>(stream));
}

int32_t ure_csr_pair_window(void) { return kCsrPairWindow; }

int64_t ure_csr_pair_knn_scratch(int64_t n_query, int64_t n, int32_t n_nb, int32_t splits)
{
    return ure_pair_knn_scratch(n_query, n, n_nb, splits);
}

int ure_csr_pair_knn(const int64_t *row_off, const int32_t *col, const float *val, int64_t n, int64_t n_item, int32_t metric, const int32_t *query,
                     int64_t n_query, int32_t n_nb, int32_t splits, float *dist, int32_t *idx, void *scratch, int64_t scratch_bytes, void *stream)
{
    if (int rc = check_csr(row_off, col, val, n, n_item, metric)) return rc;
    URE_ARG(n_query >= 1 && n_query <= INT32_MAX);
    URE_ARG(n_nb >= 1 && n_nb <= kPairMaxNb);
    URE_ARG(n_nb <= n);
    URE_ARG(splits >= 0);
    URE_ARG(dist && idx);
    URE_ARG(scratch && scratch_bytes >= ure_csr_pair_knn_scratch(n_query, n, n_nb, splits));
    return launch_knn<CsrSrc>(CsrArgs{row_off, col, val}, n, metric, query, n_query, n_nb, splits, dist, idx, scratch, static_cast<hipStream_t>(stream));
}

int ure_csr_pair_rowsum(const int64_t *row_off, const int32_t *col, const float *val, int64_t n, int64_t n_item, int32_t metric, float *R, void *stream)
{
    if (int rc = check_csr(row_off, col, val, n, n_item, metric)) return rc;
    URE_ARG(R);
    return launch_rowsum<CsrSrc>(CsrArgs{row_off, col, val}, n, metric, R, static_cast<hipStream_t>(stream));
}

int ure_csr_pair_cols(const int64_t *row_off, const int32_t *col, const float *val, int64_t n, int64_t n_item, int32_t metric, const int32_t *cols,
                      int32_t m, float *out, void *stream)
{
    if (int rc = check_csr(row_off, col, val, n, n_item, metric)) return rc;
    URE_ARG(cols && m >= 1);
    URE_ARG(out);
    return launch_cols<CsrSrc>(CsrArgs{row_off, col, val}, n, metric, cols, m, out, static_cast<hipStream_t>(stream));
}

int ure_csr_pair_label_expsum(const int64_t *row_off, const int32_t *col, const float *val, int64_t n, int64_t n_item, int32_t metric,
                              const int32_t *label, int32_t k, double *W, void *stream)
{
    if (int rc = check_csr(row_off, col, val, n, n_item, metric)) return rc;
    URE_ARG(label);
    URE_ARG(k >= 1 && k <= kPairMaxGroups);
    URE_ARG(W);
    return launch_label_expsum<CsrSrc>(CsrArgs{row_off, col, val}, n, metric, label, k, W, static_cast<hipStream_t>(stream));
}

int ure_host_assign_desc_f64(const double *w, int64_t n, int32_t k, int64_t capacity, int32_t *label, double *inertia)
{
    URE_ARG(w && label);
    URE_ARG(n >= 1 && k >= 1);
    URE_ARG(n <= INT64_MAX / k);
    URE_ARG(capacity >= 1 && capacity <= INT64_MAX / k && capacity * k >= n);
    const int64_t total = n * k;
    std::vector<std::pair<uint64_t, int64_t>> key((size_t)total);
    for (int64_t t = 0; t < total; ++t) {
        const double v = w[t] == 0.0 ? 0.0 : w[t];                      // -0.0 ties with +0.0, as in np.argsort
        uint64_t b;
        std::memcpy(&b, &v, 8);
        b = (b >> 63) ? ~b : (b | ((uint64_t)1 << 63));                // order-preserving map of double bits (NaN last)
        key[(size_t)t] = {b, t};
    }
    std::sort(key.begin(), key.end());
    std::vector<int64_t> left((size_t)k, capacity);
    std::vector<char> done((size_t)n, 0);
    std::fill(label, label + n, 0);
    int64_t n_done = 0;
    for (int64_t q = total - 1; q >= 0 && n_done < n; --q) {           // descending weight, ties by descending flat index
        const int64_t t = key[(size_t)q].second;
        const int64_t u = t / k;
        const int c = (int)(t % k);
        if (done[(size_t)u] || left[(size_t)c] <= 0) continue;
        label[u] = c;
        done[(size_t)u] = 1;
        --left[(size_t)c];
        ++n_done;
    }
    if (inertia) {
        std::vector<double> v((size_t)n);
        for (int64_t i = 0; i < n; ++i) v[(size_t)i] = w[i * k + label[i]];
        *inertia = np_sum_f64(v.data(), n);
    }
    return 0;
}

}  // extern "C"

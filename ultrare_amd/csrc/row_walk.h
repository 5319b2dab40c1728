// row_walk.h -- the masked row walk of the kernels over a shard's graph (gcn.hip, bpr.hip, nmf.hip, influence.hip), written once:
// a group of G lanes owns an output row and goes through the row's entries a tile of G at a time.  Lane `sub` fetches entry
// p0 + sub -- on the CSC side through the map to its CSR position -- and decides whether the entry counts; the group then goes
// through the tile, entry u read from the lane that holds it, and adds one term per entry that counts.
//
// A kernel states what a fetch reads, what a term adds and what the row stores at the end.  The ORDER in which a chain receives
// its terms is the walk's, as csr_lanes.h says of its own walks: ascending entry position, never split across lanes, one lane
// per (row, column) chain.  (gcn_propagate_kernel's loop is another one: csr_row_walk's software-prefetched shape.)
#pragma once
#include "csr_lanes.h"

namespace ure {

// Where a thread stands in a kernel that gives every row a group of G lanes: lane `sub` of the group that owns row `r`.
template <int G>
struct RowLanes {
    const int sub = threadIdx.x % G;
    const int64_t r = (int64_t)blockIdx.x * (kBlock / G) + threadIdx.x / G;
    // (whole groups leave together: the lanes that stay always find their group complete)
    __device__ __forceinline__ bool past(int64_t n_rows) const { return r >= n_rows; }
};

// The CSR position of entry k of the side walked: k itself, or map[k] held inside the arrays whatever the map holds.
template <bool MAPPED>
__device__ __forceinline__ unsigned entry_pos(const int32_t *__restrict__ map, int64_t k, unsigned last_pos)
{
    return MAPPED ? min((unsigned)ldg(map + k), last_pos) : (unsigned)k;
}

// The entries [b, e) of a row.  fetch(k, inside) -> what this lane holds of entry k = p0 + sub (inside: k < e), a small plain
// struct that says whether the entry counts; use(mine, u) reads entry u's fields with group_read<G>(mine.field, u) -- they are
// uniform across the group -- and adds its term, or nothing when the entry does not count.
template <int G, typename Fetch, typename Use>
__device__ __forceinline__ void tile_walk(int64_t b, int64_t e, int sub, Fetch fetch, Use use)
{
    for (int64_t p0 = b; p0 < e; p0 += G) {
        const int64_t k = p0 + sub;
        const auto mine = fetch(k, k < e);
        const int m = (int)min<int64_t>(G, e - p0);
        for (int u = 0; u < m; ++u) use(mine, u);
    }
}

// Launches the kernel of a <G, MAPPED> pair that the side asks for -- `mapped` when it comes with a map -- a group of G lanes
// per row.
template <typename... P, typename... A>
inline void launch_by_map(const int32_t *map, void (*mapped)(P...), void (*plain)(P...), int64_t n_rows, int G, hipStream_t st, A... args)
{
    hipLaunchKernelGGL((map ? mapped : plain), dim3(group_blocks(n_rows, G)), dim3(kBlock), 0, st, args...);
}

}  // namespace ure

// block_cache.cpp -- library-owned device memory of touch mode (masks, tables, the slot index) comes from a small cache of blocks
// instead of hipMalloc / hipFree per job: a 32-shard job makes 32-128 allocations, each a driver call and a synchronous fill -- 24 ms of
// a 110 ms request at configs[3]'s shape (k = 16), 28 ms at k = 128 --, and every request of a process asks for the same sizes again.
// Blocks go back when their job is destroyed (after the device has been waited for); up to kBlockCacheBytes are kept per device, the
// rest is freed.  Host code only.
#include "ure_internal.h"

#include <map>
#include <mutex>

namespace ure {
namespace {
struct BlockCache {
    std::multimap<size_t, void *> idle;
    std::map<void *, size_t> size_of;
    size_t held = 0;
};
std::mutex g_block_lock;
std::map<int, BlockCache> g_block_cache;
constexpr size_t kBlockCacheBytes = (size_t)8 << 30;
}  // namespace

hipError_t block_malloc(void **out, size_t bytes)
{
    bytes = (std::max<size_t>(bytes, 1) + ((size_t)256 << 10) - 1) / ((size_t)256 << 10) * ((size_t)256 << 10);
    int dev = 0;
    (void)hipGetDevice(&dev);
    {
        std::lock_guard<std::mutex> hold(g_block_lock);
        BlockCache &C = g_block_cache[dev];
        auto it = C.idle.lower_bound(bytes);
        if (it != C.idle.end() && it->first <= bytes + bytes / 4 + ((size_t)1 << 20)) {
            *out = it->second;
            C.held -= it->first;
            C.idle.erase(it);
            return hipSuccess;
        }
    }
    hipError_t e = hipMalloc(out, bytes);
    if (e != hipSuccess) {                                   // (out of memory with idle blocks held: give them back and ask once more)
        std::vector<void *> drop;
        {
            std::lock_guard<std::mutex> hold(g_block_lock);
            BlockCache &C = g_block_cache[dev];
            for (auto &kv : C.idle) { drop.push_back(kv.second); C.size_of.erase(kv.second); }
            C.idle.clear();
            C.held = 0;
        }
        for (void *p : drop) (void)hipFree(p);
        (void)hipGetLastError();
        e = hipMalloc(out, bytes);
    }
    if (e == hipSuccess) {
        std::lock_guard<std::mutex> hold(g_block_lock);
        g_block_cache[dev].size_of[*out] = bytes;
    }
    return e;
}

void block_free(void *p)
{
    if (!p) return;
    // (the device the block lives on, not the calling thread's current one: a job is destroyed on a worker thread, whose current device is 0
    // whatever GPU its rank trains on)
    int dev = 0;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) == hipSuccess) dev = attr.device;
    else { (void)hipGetLastError(); (void)hipGetDevice(&dev); }
    {
        std::lock_guard<std::mutex> hold(g_block_lock);
        BlockCache &C = g_block_cache[dev];
        auto it = C.size_of.find(p);
        if (it != C.size_of.end() && C.held + it->second <= kBlockCacheBytes) {
            C.idle.emplace(it->second, p);
            C.held += it->second;
            return;
        }
        if (it != C.size_of.end()) C.size_of.erase(it);
    }
    (void)hipFree(p);
}

}  // namespace ure

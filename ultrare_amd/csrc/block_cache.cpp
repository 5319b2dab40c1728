// block_cache.cpp -- library-owned device memory of touch mode (masks, tables, the slot index) comes from a small cache of blocks
// instead of hipMalloc / hipFree per job: a 32-shard job makes 32-128 allocations, each a driver call and a synchronous fill -- 24 ms of
// a 110 ms request at configs[3]'s shape (k = 16), 28 ms at k = 128 --, and every request of a process asks for the same sizes again.
// Blocks go back when their job is destroyed (after the device has been waited for); up to kBlockCacheBytes are kept per device, the
// rest is freed.  Host code only.
//
// URE_BLOCK_FILL (read on every block_malloc, as plan_job reads URE_INDEX_STAGED): a byte 0 .. 255, decimal or 0x.., that every block
// handed out is filled with over its whole rounded size -- blocks of the idle list and blocks fresh from hipMalloc alike -- so that a test
// can start a job from memory of its choosing (the job's rule).  Unset or empty: nothing is filled, no device work is added.
// Anything else is an error: a typo must not turn such a test into a test of nothing.
#include "ure_internal.h"

#include <cerrno>
#include <cstdlib>
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

int block_fill_setting(int *byte)
{
    const char *e = std::getenv("URE_BLOCK_FILL");
    if (!e || !*e) return 0;
    char *end = nullptr;
    errno = 0;
    const long v = std::strtol(e, &end, 0);
    if (errno || end == e || *end || v < 0 || v > 255) return -1;
    if (byte) *byte = (int)v;
    return 1;
}

// the block as its job gets it: filled on the null stream, where job_block's own fill follows it in order
static hipError_t hand_out(void **out, size_t bytes, int filled, int byte)
{
    if (!filled) return hipSuccess;
    const hipError_t e = hipMemset(*out, byte, bytes);
    if (e != hipSuccess) { block_free(*out); *out = nullptr; }      // (nobody has recorded the block yet)
    return e;
}

hipError_t block_malloc(void **out, size_t bytes)
{
    int byte = 0;
    const int filled = block_fill_setting(&byte);
    if (filled < 0) return hipErrorInvalidValue;                // (ure_job_create names the variable)
    bytes = (std::max<size_t>(bytes, 1) + ((size_t)256 << 10) - 1) / ((size_t)256 << 10) * ((size_t)256 << 10);
    int dev = 0;
    (void)hipGetDevice(&dev);
    bool found = false;
    {
        std::lock_guard<std::mutex> hold(g_block_lock);
        BlockCache &C = g_block_cache[dev];
        auto it = C.idle.lower_bound(bytes);
        if (it != C.idle.end() && it->first <= bytes + bytes / 4 + ((size_t)1 << 20)) {
            *out = it->second;
            C.held -= it->first;
            bytes = it->first;
            C.idle.erase(it);
            found = true;
        }
    }
    if (found) return hand_out(out, bytes, filled, byte);
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
    return e == hipSuccess ? hand_out(out, bytes, filled, byte) : e;
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

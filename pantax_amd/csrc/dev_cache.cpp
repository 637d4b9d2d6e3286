// dev_cache.cpp -- the per-process cache of released device blocks behind DevBuf (common.hpp).
#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <vector>
#include "common.hpp"

namespace ptx {

namespace {
struct DevCache {
    struct Block { void *p; uint64_t epoch; };
    struct PerDevice {
        std::multimap<size_t, Block> free_blocks;   // by capacity
        size_t cached_bytes = 0;
        uint64_t free_epoch = 0, synced_epoch = 0;  // a block released at epoch e may be reused once synced_epoch >= e
        std::vector<hipStream_t> streams;           // the compute streams of the ctx's on this device: what "the device is idle" means for a cached block
    };
    std::mutex mu;
    std::map<int, PerDevice> dev;
};
DevCache &dev_cache() { static DevCache c; return c; }
inline size_t round_cap(size_t bytes) {
    if (bytes <= (1u << 20)) return (bytes + 4095) & ~size_t(4095);
    return (bytes + (1u << 20) - 1) & ~size_t((1u << 20) - 1);
}
}  // namespace

// The cap is PER DEVICE and sized from what is free when the device is first used: min(3/4 of the device, 9/10 of what was free) -- a process
// that shares its GPU (N ranks of a dry run on one device, parallel test workers) must not sit on memory its siblings need.  `dev_cache_gb`
// (option / pantax_hip_set_option) overrides it for every device of the process; 0 caches nothing.
static std::atomic<long long> g_dev_cache_cap_override{-1};
void dev_cache_set_max(long long bytes) { g_dev_cache_cap_override.store(bytes); }
size_t dev_cache_max(int dev) {
    const long long ov = g_dev_cache_cap_override.load();
    if (ov >= 0) return (size_t)ov;
    static std::mutex mu;
    static std::map<int, size_t> caps;
    std::lock_guard<std::mutex> g(mu);
    auto it = caps.find(dev);
    if (it != caps.end()) return it->second;
    int cur = 0;
    (void)hipGetDevice(&cur);
    size_t free_b = 0, total_b = 0, cap = (size_t)(48ull << 30);
    if (cur != dev) (void)hipSetDevice(dev);
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && total_b != 0) cap = std::min(total_b / 4 * 3, free_b / 10 * 9);
    if (cur != dev) (void)hipSetDevice(cur);
    caps[dev] = cap;
    return cap;
}
// a sibling process is short of memory when less than an eighth of the device is free: big blocks are then given back instead of kept
static bool dev_memory_is_tight() {
    size_t free_b = 0, total_b = 0;
    return hipMemGetInfo(&free_b, &total_b) == hipSuccess && total_b != 0 && free_b < total_b / 8;
}

hipError_t dev_cache_alloc(void **p, size_t bytes, size_t *cap_out, int *dev_out) {
    const size_t want = round_cap(bytes ? bytes : 1);
    int dev = 0;
    (void)hipGetDevice(&dev);
    *dev_out = dev;
    DevCache &c = dev_cache();
    {
        std::unique_lock<std::mutex> lk(c.mu);
        DevCache::PerDevice &d = c.dev[dev];
        auto it = d.free_blocks.lower_bound(want);
        if (it != d.free_blocks.end() && it->first <= std::max(2 * want, want + (size_t(1) << 20))) {
            const size_t cap = it->first;
            const DevCache::Block b = it->second;
            d.free_blocks.erase(it);
            d.cached_bytes -= cap;
            const bool need_sync = b.epoch > d.synced_epoch;
            const uint64_t now = d.free_epoch;
            const std::vector<hipStream_t> streams = d.streams;
            lk.unlock();
            if (need_sync) {   // kernels enqueued before the block was released may still be using it
                // every kernel of this library runs on a ctx's main or side stream (copy streams -- the GAF upload's, the graph loader's -- are waited
                // for by their owners before they release anything): those are waited for, not the whole device -- a device-wide wait also sits
                // out the graph loader's transfers of the NEXT group of species (round 6).  The owners keep that promise on every exit, failures
                // included: the chunk pipeline drains its stream before it returns (upload.cpp), and db_upload_arrays -- whose copy stream also carries
                // the widen and unpack kernels -- waits for it before its scratch buffers are released (api_core.cpp)
                if (streams.empty()) (void)hipDeviceSynchronize();
                else for (hipStream_t st : streams) (void)hipStreamSynchronize(st);
                std::lock_guard<std::mutex> g(c.mu);
                DevCache::PerDevice &d2 = c.dev[dev];
                if (now > d2.synced_epoch) d2.synced_epoch = now;
            }
            *p = b.p; *cap_out = cap;
            return hipSuccess;
        }
    }
    hipError_t e = hipMalloc(p, want);
    if (e != hipSuccess) {   // out of memory: give the cached blocks back and retry once
        (void)hipGetLastError();
        dev_cache_trim();
        e = hipMalloc(p, want);
    }
    *cap_out = e == hipSuccess ? want : 0;
    return e;
}

// blocks released inside such a scope are known to be idle (the caller has waited for every stream that could have used them): they may be handed out
// again without the device-wide wait -- which would also wait for whatever ELSE is in flight, e.g. the graph loader's copy stream (round 6: that wait
// cost every group of the file seam ~4 ms per stage that allocated)
static thread_local int g_frees_are_idle = 0;
DevCacheIdleFrees::DevCacheIdleFrees() { ++g_frees_are_idle; }
DevCacheIdleFrees::~DevCacheIdleFrees() { --g_frees_are_idle; }

void dev_cache_free(void *p, size_t cap, int dev) {
    if (!p) return;
    DevCache &c = dev_cache();
    {
        std::lock_guard<std::mutex> g(c.mu);
        DevCache::PerDevice &d = c.dev[dev];
        // (the memory query costs microseconds: only blocks of 64 MB and more pay it)
        if (cap && d.cached_bytes + cap <= dev_cache_max(dev) && !(cap >= (size_t(64) << 20) && dev_memory_is_tight())) {
            d.free_blocks.emplace(cap, DevCache::Block{p, g_frees_are_idle ? 0 : ++d.free_epoch});
            d.cached_bytes += cap;
            return;
        }
    }
    (void)hipFree(p);
}

void dev_cache_register_stream(int dev, hipStream_t st, bool add) {
    DevCache &c = dev_cache();
    std::lock_guard<std::mutex> g(c.mu);
    auto &v = c.dev[dev].streams;
    v.erase(std::remove(v.begin(), v.end(), st), v.end());
    if (add) v.push_back(st);
}

void dev_cache_trim() {
    int dev = 0;
    (void)hipGetDevice(&dev);
    DevCache &c = dev_cache();
    std::multimap<size_t, DevCache::Block> blocks;
    {
        std::lock_guard<std::mutex> g(c.mu);
        DevCache::PerDevice &d = c.dev[dev];
        blocks.swap(d.free_blocks);
        d.cached_bytes = 0;
    }
    for (auto &kv : blocks) (void)hipFree(kv.second.p);
}

}  // namespace ptx

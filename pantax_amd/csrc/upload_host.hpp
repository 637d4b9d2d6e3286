// upload_host.hpp -- the host side of the staged uploads (GAF text, graph arrays): what fills the pinned ring, the two policies that size it, and the
// lease that keeps two uploads out of one ring.  Plain C++ over plain values: nothing here names the HIP runtime, so tests/native/upload_host_check.cpp
// drives all of it under the host compiler's sanitizers.  The device side -- the ring itself, the copies, the one chunk pipeline -- is upload.cpp.
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include <sched.h>

namespace ptx {

// The host side of the big uploads (GAF text, graph arrays) is a crew of threads that pread into a pinned ring while the DMA engine empties
// it: both want the memory of the GPU's own NUMA node -- a filler on the far socket writes the ring across the inter-socket link, and the DMA
// reads it back the same way (round 4: 0.365 .. 0.49 s for the same 15-GB load from box to box).  pantax_hip_init looks the node up
// (/sys/bus/pci/devices/<gpu>/numa_node); the crew's threads are bound to its CPUs and the ring is allocated from it (option numa_bind=0: off).
struct NumaInfo {
    int node = -1;                   // -1: unknown / a single node: nothing is bound
    std::vector<int> cpus;           // the node's CPUs
};

// bind the calling thread to a NUMA node's CPUs and its new pages to that node (the pinned ring is allocated under it, the crew's threads are
// started under it); restores what was there when it goes out of scope
struct NumaBind {
    cpu_set_t saved;
    bool bound = false, policy = false;
    NumaBind(bool enabled, const NumaInfo &numa);
    ~NumaBind();
    NumaBind(const NumaBind &) = delete;
    NumaBind &operator=(const NumaBind &) = delete;
};

// ---- the ring's two policies ----
constexpr int STAGE_SLOTS = 3;   // chunk i+1 and i+2 are filled while chunk i is on its way
// Chunk size of a transfer of `total` bytes through a ring that holds `ring_bytes` already: a sixth of the transfer in whole MiB, 4 .. 64 MiB
// (pinning memory costs ~0.1 ms per MB, once per ctx), or the slot of a larger ring that is there already; stage_ch_mb > 0 (option): that size.
uint64_t stage_chunk_bytes(uint64_t total, uint64_t ring_bytes, int stage_ch_mb);
// Threads of the crew that fills a chunk: option stage_threads, at most half the hardware threads, at most one per MiB of the chunk, at least one.
// 32 threads: at 16 the crew, not the DMA, bounds a 15-GB load (filling 413 of 420 ms = 37 GB/s of pread; 32: 211 of 293 ms = 52 GB/s,
// 0.92 of the pinned copy rate); 48 and 64 fill no faster and slow the copies down (390 ms)
int stage_crew_threads(int stage_threads, unsigned hardware_threads, uint64_t chunk_bytes);

// A crew of host threads that fills pinned slots -- [src + pos, +n) or (fd, pos, n) -- for the lifetime of ONE upload (round 2
// created and joined 16 threads per 16-MB chunk: ~0.5 ms of thread start-up beside 0.6 ms of copy).  The box delivers 80 GB/s
// of pread from the page cache on 8-16 threads and 56 GB/s of pinned host->device copy (tools/h2d_probe.py): the crew only has
// to stay ahead of the DMA (it takes 32 threads for that inside the pipeline: see stage_crew_threads).
struct StageCrew {
    std::mutex mu;
    std::condition_variable cv_go, cv_done;
    uint64_t gen = 0;
    int done = 0, nth = 1;
    bool quit = false;
    uint8_t *slot = nullptr; const uint8_t *src = nullptr; int fd = -1; uint64_t pos = 0, n = 0;
    const std::function<void(int, int)> *job = nullptr;   // run(): any per-thread job instead of the copy
    std::vector<std::thread> th;
    explicit StageCrew(int n_threads);
    ~StageCrew();
    void run(const std::function<void(int, int)> &fn);   // fn(t, nth) on every thread of the crew; returns when all are done
    void fill(uint8_t *slot, const uint8_t *src, int fd, uint64_t pos, uint64_t n);   // thread t copies its share of [pos, pos + n) into the slot
};

// A stretch of a 32-bit device array as it lies on the host: in memory (`src`) or in a file (`file` = index into the paths the
// upload is given, bytes from `file_off`); `narrow`: the source holds 64-bit little-endian integers (bincode's i64 lengths / usize
// node ids, zip.rs:171-190) that become 32-bit ones on the way -- a value beyond 2^32 - 1 (or negative) fails the upload.
struct UploadSeg {
    const void *src = nullptr;
    int32_t file = -1;
    uint64_t file_off = 0;
    uint64_t out_bytes = 0;   // bytes this stretch occupies on the device (a multiple of 4); the source holds twice as many when narrow
    bool narrow = false;
    bool hole = false;        // nothing is filled (the bytes travel as they lie in the ring): a stretch another pass writes on the device
};

// ---- many stretches (files / memory, as they are or narrowed from 64 to 32 bits) -> ONE contiguous device range ----
// The db load of the pipeline seam (a6): 1 000 species' graphs are 2 000 stretches of a few megabytes in as many files.  One upload per
// stretch (round 4) created a crew of threads and drained the copy queue 2 000 times; here the stretches are one logical byte string
// that travels in 64-MB chunks like the GAF text: every thread of the crew fills its share of the chunk -- whatever stretches it spans --
// and the chunk leaves as one DMA.  Files are opened by the thread that needs them (one descriptor per thread at a time: no limit on
// the number of species), bincode's 64-bit integers are narrowed on the way into the pinned chunk (read in 1-MB blocks: L2-resident).
struct SegFiller {
    const UploadSeg *segs; size_t n_segs; const std::string *files;
    std::vector<uint64_t> prefix;            // [n_segs + 1] device byte offsets
    std::atomic<int64_t> bad{-1}, io_fail{-1};   // smallest stretch that held a value beyond 32 bits / that could not be read whole, or -1
    SegFiller(const UploadSeg *segs, size_t n_segs, const std::string *files);
    // device bytes [b, e) of the logical string -> out (which points at byte b); b and e are multiples of 4.  Any number of threads at once.
    void fill(uint8_t *out, uint64_t b, uint64_t e);
  private:
    static void note(std::atomic<int64_t> &a, int64_t k) { int64_t cur = a.load(); while ((cur < 0 || k < cur) && !a.compare_exchange_weak(cur, k)) {} }
};

// fn(begin, end) over [0, n) split across up to n_threads host threads (the calling thread takes the first slice)
void parallel_for(uint64_t n, int n_threads, const std::function<void(uint64_t, uint64_t)> &fn);

// ---- the lease of a staging ring ----
// A ring serves one upload at a time.  Whoever stages through it holds a RingLease on its gate for the duration of its pipeline; a second
// taker is refused at once (the lease tests false) -- it never waits: the GAF load's uploader holds the ring while it waits for the tokenizer.
struct RingGate { std::atomic<bool> in_use{false}; };
struct RingLease {
    explicit RingLease(RingGate &gate) : g(gate.in_use.exchange(true, std::memory_order_acquire) ? nullptr : &gate) {}
    ~RingLease() { if (g) g->in_use.store(false, std::memory_order_release); }
    RingLease(const RingLease &) = delete;
    RingLease &operator=(const RingLease &) = delete;
    explicit operator bool() const { return g != nullptr; }
  private:
    RingGate *g;
};

}  // namespace ptx

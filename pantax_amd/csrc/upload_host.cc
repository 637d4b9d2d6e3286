// upload_host.cc -- the host side of the staged uploads (upload_host.hpp): plain C++, no device pass.
#include <algorithm>
#include <cstring>
#include <exception>
#include <fcntl.h>
#include <sys/syscall.h>
#include <unistd.h>
#include "upload_host.hpp"

namespace ptx {

NumaBind::NumaBind(bool enabled, const NumaInfo &numa) {
    if (!enabled || numa.node < 0 || numa.cpus.empty()) return;
    if (sched_getaffinity(0, sizeof(saved), &saved) != 0) return;
    cpu_set_t want;
    CPU_ZERO(&want);
    int n = 0;
    for (int c : numa.cpus) if (CPU_ISSET(c, &saved)) { CPU_SET(c, &want); ++n; }   // only CPUs this process may use (cgroups / taskset)
    if (n == 0) return;
    bound = sched_setaffinity(0, sizeof(want), &want) == 0;
    if (bound && numa.node < 1024) {
#ifdef SYS_set_mempolicy
        unsigned long mask[16] = {0};
        mask[numa.node / 64] = 1ul << (numa.node % 64);
        policy = syscall(SYS_set_mempolicy, 1 /* MPOL_PREFERRED */, mask, 1024ul) == 0;
#endif
    }
}
NumaBind::~NumaBind() {
#ifdef SYS_set_mempolicy
    if (policy) (void)syscall(SYS_set_mempolicy, 0 /* MPOL_DEFAULT */, nullptr, 0ul);
#endif
    if (bound) (void)sched_setaffinity(0, sizeof(saved), &saved);
}

uint64_t stage_chunk_bytes(uint64_t total, uint64_t ring_bytes, int stage_ch_mb) {
    if (stage_ch_mb > 0) return (uint64_t)stage_ch_mb << 20;
    constexpr uint64_t MiB = 1ull << 20;
    const uint64_t ch = std::min<uint64_t>(64 * MiB, std::max<uint64_t>(4 * MiB, ((total / 6) + MiB - 1) & ~(MiB - 1)));
    if (ring_bytes >= STAGE_SLOTS * (4 * MiB) && ring_bytes / STAGE_SLOTS > ch) return std::min<uint64_t>(64 * MiB, (ring_bytes / STAGE_SLOTS) & ~(MiB - 1));   // a larger ring is there already
    return ch;
}

int stage_crew_threads(int stage_threads, unsigned hardware_threads, uint64_t chunk_bytes) {
    // min(stage_threads, hardware_concurrency() / 2), one at least, and no more than the chunk has MiB
    const int want = std::max(1, std::min(stage_threads, (int)hardware_threads / 2));
    return (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)want, chunk_bytes >> 20));
}

// thread t's share of a plain fill: [pos + b, pos + e) of the source -> [b, e) of the slot
static void crew_piece(uint8_t *slot, const uint8_t *src, int fd, uint64_t pos, uint64_t n, int t, int nth) {
    const uint64_t b = n * (uint64_t)t / (uint64_t)nth, e = n * (uint64_t)(t + 1) / (uint64_t)nth;
    if (src) { std::memcpy(slot + b, src + pos + b, e - b); return; }
    uint64_t at = b;
    while (at < e) {   // pread may return short
        const ssize_t r = ::pread(fd, slot + at, e - at, (off_t)(pos + at));
        if (r <= 0) { std::memset(slot + at, 0, e - at); break; }   // truncated file: the caller validated sizes, zeros keep the run defined
        at += (uint64_t)r;
    }
}

StageCrew::StageCrew(int n_threads) : nth(n_threads < 1 ? 1 : n_threads) {
    for (int t = 1; t < nth; ++t)
        th.emplace_back([this, t] {
            uint64_t seen = 0;
            for (;;) {
                std::unique_lock<std::mutex> lk(mu);
                cv_go.wait(lk, [&] { return quit || gen != seen; });
                if (quit) return;
                seen = gen;
                uint8_t *sl = slot; const uint8_t *sr = src; const int f = fd; const uint64_t p = pos, nn = n;
                const std::function<void(int, int)> *jb = job;
                lk.unlock();
                if (jb) (*jb)(t, nth); else crew_piece(sl, sr, f, p, nn, t, nth);
                lk.lock();
                if (++done == nth - 1) cv_done.notify_one();
            }
        });
}
StageCrew::~StageCrew() {
    { std::lock_guard<std::mutex> g(mu); quit = true; }
    cv_go.notify_all();
    for (auto &t : th) t.join();
}
void StageCrew::run(const std::function<void(int, int)> &fn) {
    { std::lock_guard<std::mutex> g(mu); job = &fn; done = 0; ++gen; }
    cv_go.notify_all();
    fn(0, nth);
    std::unique_lock<std::mutex> lk(mu);
    cv_done.wait(lk, [&] { return done == nth - 1; });
    job = nullptr;
}
void StageCrew::fill(uint8_t *slot_, const uint8_t *src_, int fd_, uint64_t pos_, uint64_t n_) {
    { std::lock_guard<std::mutex> g(mu); job = nullptr; slot = slot_; src = src_; fd = fd_; pos = pos_; n = n_; done = 0; ++gen; }
    cv_go.notify_all();
    crew_piece(slot_, src_, fd_, pos_, n_, 0, nth);
    std::unique_lock<std::mutex> lk(mu);
    cv_done.wait(lk, [&] { return done == nth - 1; });
}

SegFiller::SegFiller(const UploadSeg *segs_, size_t n_segs_, const std::string *files_) : segs(segs_), n_segs(n_segs_), files(files_), prefix(n_segs_ + 1, 0) {
    for (size_t k = 0; k < n_segs; ++k) prefix[k + 1] = prefix[k] + segs[k].out_bytes;
}

void SegFiller::fill(uint8_t *out, uint64_t b, uint64_t e) {
    size_t k = (size_t)(std::upper_bound(prefix.begin(), prefix.end(), b) - prefix.begin()) - 1;
    int fd = -1, fd_file = -1;
    std::vector<uint64_t> tmp;
    for (; b < e && k < n_segs; ++k) {
        const UploadSeg &s = segs[k];
        const uint64_t so = b - prefix[k], n = std::min(e, prefix[k + 1]) - b;
        if (n == 0) continue;
        if (s.hole) { out += n; b += n; continue; }
        const uint8_t *src = static_cast<const uint8_t *>(s.src);
        if (!src && s.file != fd_file) {
            if (fd >= 0) ::close(fd);
            fd = ::open(files[s.file].c_str(), O_RDONLY);
            fd_file = s.file;
            if (fd < 0) note(io_fail, (int64_t)k);
        }
        auto read_at = [&](uint8_t *dst, uint64_t off, uint64_t len) {
            if (src) { std::memcpy(dst, src + off, len); return; }
            uint64_t at = 0;
            while (fd >= 0 && at < len) {
                const ssize_t r = ::pread(fd, dst + at, len - at, (off_t)(s.file_off + off + at));
                if (r <= 0) break;
                at += (uint64_t)r;
            }
            if (at < len) { std::memset(dst + at, 0, len - at); note(io_fail, (int64_t)k); }   // zeros keep the run defined; the caller fails
        };
        if (!s.narrow) read_at(out, so, n);
        else {
            constexpr uint64_t BLK = 131072;                      // 64-bit values per block: a megabyte per pread
            uint32_t *o32 = reinterpret_cast<uint32_t *>(out);
            uint64_t hi = 0;
            for (uint64_t i0 = so / 4, i1 = (so + n) / 4; i0 < i1; i0 += BLK) {
                const uint64_t m = std::min(BLK, i1 - i0);
                const uint64_t *in;
                if (src) in = reinterpret_cast<const uint64_t *>(src) + i0;
                else { tmp.resize(BLK); read_at(reinterpret_cast<uint8_t *>(tmp.data()), 8 * i0, 8 * m); in = tmp.data(); }
                uint32_t *o = o32 + (i0 - so / 4);
                for (uint64_t i = 0; i < m; ++i) { const uint64_t x = in[i]; o[i] = (uint32_t)x; hi |= x; }
            }
            if (hi >> 32) note(bad, (int64_t)k);
        }
        out += n; b += n;
    }
    if (fd >= 0) ::close(fd);
}

void parallel_for(uint64_t n, int n_threads, const std::function<void(uint64_t, uint64_t)> &fn) {
    if (n_threads < 1) n_threads = 1;
    if ((uint64_t)n_threads > n) n_threads = n ? (int)n : 1;
    if (n_threads == 1) { fn(0, n); return; }
    // an exception on a worker thread would end the process (std::terminate): it is carried to the calling thread instead,
    // where the extern "C" entry points turn it into a status
    std::vector<std::thread> th;
    std::vector<std::exception_ptr> err(n_threads);
    for (int t = 1; t < n_threads; ++t)
        th.emplace_back([&, t] {
            try { fn(n * t / n_threads, n * (t + 1) / n_threads); } catch (...) { err[t] = std::current_exception(); }
        });
    try { fn(0, n / n_threads); } catch (...) { err[0] = std::current_exception(); }
    for (auto &t : th) t.join();
    for (auto &e : err) if (e) std::rethrow_exception(e);
}

}  // namespace ptx

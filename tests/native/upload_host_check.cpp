// upload_host_check.cpp -- the host side of the staged uploads (pantax_amd/csrc/upload_host.hpp: SegFiller, StageCrew, parallel_for, the two ring
// policies, the ring lease) on its own.  A program of its own: tests/test_upload_host.py compiles it with upload_host.cc by the host compiler, once under
// -fsanitize=address,undefined and once under -fsanitize=thread, and runs it; it returns non-zero at the first mismatch.  Inputs are temporary files
// it writes itself.
//
// `old_chunk_bytes*` and `old_crew_threads` are transcriptions of the expressions that stood twice in ctx.cpp before the two pipelines became one; the
// policy functions must answer the same over the whole grid.
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>
#include <fcntl.h>
#include <unistd.h>
#include "upload_host.hpp"

using namespace ptx;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "upload_host_check:%d: %s\n", __LINE__, #cond);     \
            std::exit(1);                                                            \
        }                                                                            \
    } while (0)

namespace {

std::string g_dir;
std::vector<std::string> g_made;
std::string write_file(const char *name, const void *data, size_t bytes) {
    const std::string path = g_dir + "/" + name;
    const int fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0600);
    CHECK(fd >= 0);
    const uint8_t *p = static_cast<const uint8_t *>(data);
    for (size_t at = 0; at < bytes;) { const ssize_t w = ::write(fd, p + at, bytes - at); CHECK(w > 0); at += (size_t)w; }
    CHECK(::close(fd) == 0);
    g_made.push_back(path);
    return path;
}
uint8_t pat(uint64_t i) { return (uint8_t)(i * 131 + 7); }
uint64_t val32(uint64_t i) { return (i * 2654435761ull + 12345) & 0xFFFFFFFFull; }   // a 64-bit source value that fits 32 bits
UploadSeg mem_seg(const void *src, uint64_t out_bytes, bool narrow) { UploadSeg s; s.src = src; s.out_bytes = out_bytes; s.narrow = narrow; return s; }
UploadSeg file_seg(int32_t file, uint64_t file_off, uint64_t out_bytes, bool narrow) { UploadSeg s; s.file = file; s.file_off = file_off; s.out_bytes = out_bytes; s.narrow = narrow; return s; }
UploadSeg hole_seg(uint64_t out_bytes) { UploadSeg s; s.hole = true; s.out_bytes = out_bytes; return s; }

// ---- SegFiller ----
void seg_every_window() {
    // 96 device bytes: memory plain 20 | file narrow 24 (6 values, 13 bytes into the file) | hole 16 | nothing | memory narrow 36 (9 values)
    std::vector<uint8_t> plain(20);
    for (size_t i = 0; i < plain.size(); ++i) plain[i] = pat(i);
    std::vector<uint8_t> fbytes(13 + 6 * 8);
    std::vector<uint64_t> fvals(6), mvals(9);
    for (size_t i = 0; i < 13; ++i) fbytes[i] = 0xEE;
    for (size_t i = 0; i < fvals.size(); ++i) fvals[i] = val32(100 + i);
    std::memcpy(fbytes.data() + 13, fvals.data(), 6 * 8);
    for (size_t i = 0; i < mvals.size(); ++i) mvals[i] = val32(200 + i);
    const std::string files[1] = {write_file("narrow6.bin", fbytes.data(), fbytes.size())};
    const UploadSeg segs[5] = {mem_seg(plain.data(), 20, false), file_seg(0, 13, 24, true), hole_seg(16), mem_seg(nullptr, 0, false), mem_seg(mvals.data(), 36, true)};
    uint8_t ref[96];
    std::memset(ref, 0xA5, sizeof(ref));
    std::memcpy(ref, plain.data(), 20);
    for (size_t i = 0; i < 6; ++i) { const uint32_t v = (uint32_t)fvals[i]; std::memcpy(ref + 20 + 4 * i, &v, 4); }
    for (size_t i = 0; i < 9; ++i) { const uint32_t v = (uint32_t)mvals[i]; std::memcpy(ref + 60 + 4 * i, &v, 4); }
    SegFiller f(segs, 5, files);
    CHECK(f.prefix.size() == 6 && f.prefix[1] == 20 && f.prefix[2] == 44 && f.prefix[3] == 60 && f.prefix[4] == 60 && f.prefix[5] == 96);
    for (uint64_t b = 0; b < 96; b += 4)
        for (uint64_t e = b + 4; e <= 96; e += 4) {
            alignas(8) uint8_t slot[96];
            std::memset(slot, 0xA5, sizeof(slot));
            f.fill(slot + b, b, e);
            for (uint64_t x = 0; x < 96; ++x) CHECK(slot[x] == (x >= b && x < e ? ref[x] : 0xA5));
        }
    CHECK(f.bad.load() == -1 && f.io_fail.load() == -1);
}

void seg_block_border() {
    constexpr uint64_t N = 131072 + 3;   // one block of the narrowing loop and three values
    std::vector<uint64_t> vals(N);
    for (uint64_t i = 0; i < N; ++i) vals[i] = val32(i);
    const std::string files[1] = {write_file("narrow_block.bin", vals.data(), 8 * N)};
    const UploadSeg seg = file_seg(0, 0, 4 * N, true);
    for (const uint64_t split : {(uint64_t)70000, (uint64_t)131073}) {   // the second call starts inside the first block / inside the block behind the border
        SegFiller f(&seg, 1, files);
        std::vector<uint32_t> out(N, 0xA5A5A5A5u);
        uint8_t *o = reinterpret_cast<uint8_t *>(out.data());
        f.fill(o, 0, 4 * split);
        f.fill(o + 4 * split, 4 * split, 4 * N);
        for (uint64_t i = 0; i < N; ++i) CHECK(out[i] == (uint32_t)vals[i]);
        CHECK(out[131071] == (uint32_t)vals[131071] && out[131072] == (uint32_t)vals[131072]);
        CHECK(f.bad.load() == -1 && f.io_fail.load() == -1);
    }
}

// a chunk [0, bytes) filled by a crew the way upload_segments hands it out: thread t takes its share of the words
void crew_fill_segments(StageCrew &crew, SegFiller &f, uint8_t *slot, uint64_t bytes) {
    const std::function<void(int, int)> job = [&](int t, int nt) {
        const uint64_t words = bytes / 4;
        const uint64_t b = 4 * (words * (uint64_t)t / (uint64_t)nt), e = 4 * (words * (uint64_t)(t + 1) / (uint64_t)nt);
        if (e > b) f.fill(slot + b, b, e);
    };
    crew.run(job);
}

void seg_first_bad() {
    constexpr size_t K = 5, N = 1024;
    std::vector<std::vector<uint64_t>> vals(K, std::vector<uint64_t>(N));
    for (size_t k = 0; k < K; ++k) for (size_t i = 0; i < N; ++i) vals[k][i] = val32(k * N + i);
    vals[3][17] = 1ull << 32;
    vals[1][N - 1] = ~0ull;   // a negative i64
    UploadSeg segs[K];
    for (size_t k = 0; k < K; ++k) segs[k] = mem_seg(vals[k].data(), 4 * N, true);
    SegFiller f(segs, K, nullptr);
    std::vector<uint32_t> out(K * N);
    StageCrew crew(4);
    crew_fill_segments(crew, f, reinterpret_cast<uint8_t *>(out.data()), 4 * K * N);
    CHECK(f.bad.load() == 1 && f.io_fail.load() == -1);
    for (size_t k = 0; k < K; ++k) for (size_t i = 0; i < N; ++i) CHECK(out[k * N + i] == (uint32_t)vals[k][i]);
}

void seg_io_failures() {
    std::vector<uint8_t> a(32), c(40), fbytes(54);
    for (size_t i = 0; i < a.size(); ++i) a[i] = pat(i);
    for (size_t i = 0; i < c.size(); ++i) c[i] = pat(1000 + i);
    for (size_t i = 0; i < fbytes.size(); ++i) fbytes[i] = pat(500 + i);
    {   // a file 10 bytes shorter than its stretch claims: zeros behind its end, and the stretch is named
        const std::string files[1] = {write_file("short.bin", fbytes.data(), fbytes.size())};
        const UploadSeg segs[3] = {mem_seg(a.data(), 32, false), file_seg(0, 0, 64, false), mem_seg(c.data(), 40, false)};
        SegFiller f(segs, 3, files);
        uint8_t out[136];
        std::memset(out, 0xA5, sizeof(out));
        f.fill(out, 0, 136);
        CHECK(std::memcmp(out, a.data(), 32) == 0 && std::memcmp(out + 32, fbytes.data(), 54) == 0 && std::memcmp(out + 96, c.data(), 40) == 0);
        for (size_t x = 32 + 54; x < 96; ++x) CHECK(out[x] == 0);
        CHECK(f.io_fail.load() == 1 && f.bad.load() == -1);
    }
    {   // a file that is not there: its stretch is named, every other stretch is as it should be
        const std::string files[2] = {g_dir + "/no_such_file.bin", write_file("there.bin", fbytes.data(), fbytes.size())};
        const UploadSeg segs[4] = {mem_seg(a.data(), 32, false), file_seg(0, 0, 16, false), file_seg(1, 2, 52, false), mem_seg(c.data(), 40, false)};
        SegFiller f(segs, 4, files);
        uint8_t out[140];
        std::memset(out, 0xA5, sizeof(out));
        StageCrew crew(4);
        crew_fill_segments(crew, f, out, 140);
        CHECK(std::memcmp(out, a.data(), 32) == 0 && std::memcmp(out + 48, fbytes.data() + 2, 52) == 0 && std::memcmp(out + 100, c.data(), 40) == 0);
        for (size_t x = 32; x < 48; ++x) CHECK(out[x] == 0);
        CHECK(f.io_fail.load() == 1 && f.bad.load() == -1);
    }
}

// ---- StageCrew ----
void crew_cases() {
    std::vector<uint8_t> src(9000);
    for (size_t i = 0; i < src.size(); ++i) src[i] = pat(i);
    const std::string path = write_file("crew.bin", src.data(), src.size());
    const int fd = ::open(path.c_str(), O_RDONLY);
    CHECK(fd >= 0);
    for (const int nth : {1, 2, 7}) {
        { StageCrew idle(nth); CHECK(idle.nth == nth); }   // made and ended without a job
        StageCrew crew(nth);
        std::vector<uint8_t> slot(8192);
        auto filled = [&](uint64_t pos, uint64_t n) {
            for (uint64_t i = 0; i < n; ++i) if (slot[i] != src[pos + i]) return false;
            for (uint64_t i = n; i < slot.size(); ++i) if (slot[i] != 0xA5) return false;
            return true;
        };
        std::fill(slot.begin(), slot.end(), 0xA5);
        crew.fill(slot.data(), src.data(), -1, 11, 5);   // fewer bytes than threads: empty shares
        CHECK(filled(11, 5));
        std::fill(slot.begin(), slot.end(), 0xA5);
        crew.fill(slot.data(), src.data(), -1, 3, 1001);
        CHECK(filled(3, 1001));
        std::fill(slot.begin(), slot.end(), 0xA5);
        crew.fill(slot.data(), nullptr, fd, 7, 4099);
        CHECK(filled(7, 4099));
        // 200 generations on one crew, a fill and a run in turn
        std::vector<int> hits((size_t)nth, 0);
        int runs = 0;
        for (int g = 0; g < 200; ++g) {
            if (g % 2 == 0) {
                const uint64_t pos = (uint64_t)g * 13 + 1, n = 1 + (uint64_t)g * 37 % 3000;
                std::fill(slot.begin(), slot.end(), 0xA5);
                crew.fill(slot.data(), g % 4 ? nullptr : src.data(), g % 4 ? fd : -1, pos, n);
                CHECK(filled(pos, n));
            } else {
                const std::function<void(int, int)> job = [&](int t, int nt) { CHECK(nt == nth && t >= 0 && t < nt); ++hits[(size_t)t]; };
                crew.run(job);
                ++runs;
                for (int t = 0; t < nth; ++t) CHECK(hits[(size_t)t] == runs);
            }
        }
    }
    CHECK(::close(fd) == 0);
}

// ---- parallel_for ----
void parallel_for_cases() {
    struct Case { uint64_t n; int threads; };
    for (const Case c : {Case{0, 4}, Case{3, 8}, Case{1000, 7}}) {
        std::vector<std::atomic<int>> seen(c.n);
        for (auto &s : seen) s.store(0);
        std::atomic<int> calls{0};
        parallel_for(c.n, c.threads, [&](uint64_t b, uint64_t e) {
            ++calls;
            CHECK(b <= e && e <= c.n);
            for (uint64_t i = b; i < e; ++i) ++seen[i];
        });
        for (auto &s : seen) CHECK(s.load() == 1);
        CHECK(calls.load() >= 1 && calls.load() <= c.threads);
    }
    for (const bool on_caller : {false, true}) {   // the slice that throws: one of a worker thread / the calling thread's own (it starts at 0)
        std::atomic<int> entered{0};
        bool caught = false;
        try {
            parallel_for(1000, 7, [&](uint64_t b, uint64_t) {
                ++entered;
                if (on_caller ? b == 0 : b == 1000 * 3 / 7) throw std::runtime_error("slice");
            });
        } catch (const std::runtime_error &e) {
            caught = std::strcmp(e.what(), "slice") == 0;
            CHECK(entered.load() == 7);   // every thread has been joined: no slice starts behind the catch
        }
        CHECK(caught);
    }
}

// ---- the ring's policies against the expressions they replace ----
constexpr int SLOTS = 3;
uint64_t old_chunk_bytes_staged(uint64_t total, uint64_t ring_n, int stage_ch_mb) {   // upload_staged_pieces
    uint64_t CH = stage_ch_mb > 0 ? (uint64_t)stage_ch_mb << 20
                                  : std::min<uint64_t>(64ull << 20, std::max<uint64_t>(4ull << 20, ((total / 6) + (1 << 20) - 1) & ~(uint64_t)((1 << 20) - 1)));
    if (ring_n >= SLOTS * (4ull << 20) && ring_n / SLOTS > CH && stage_ch_mb <= 0) CH = std::min<uint64_t>(64ull << 20, (ring_n / SLOTS) & ~(uint64_t)((1 << 20) - 1));
    return CH;
}
uint64_t old_chunk_bytes_segments(uint64_t total, uint64_t ring_n) {   // upload_segments: no option
    uint64_t CH = std::min<uint64_t>(64ull << 20, std::max<uint64_t>(4ull << 20, ((total / 6) + (1 << 20) - 1) & ~(uint64_t)((1 << 20) - 1)));
    if (ring_n >= SLOTS * (4ull << 20) && ring_n / SLOTS > CH) CH = std::min<uint64_t>(64ull << 20, (ring_n / SLOTS) & ~(uint64_t)((1 << 20) - 1));
    return CH;
}
int old_crew_threads(int stage_threads, unsigned hardware_concurrency, uint64_t CH) {
    return (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(1, std::min(stage_threads, (int)hardware_concurrency / 2)), CH >> 20));
}
void policy_grid() {
    static_assert(STAGE_SLOTS == SLOTS, "the ring has three slots");
    constexpr uint64_t MiB = 1ull << 20;
    for (const uint64_t total : {(uint64_t)1, 4 * MiB - 1, 4 * MiB, 24 * MiB + 1, 384 * MiB, 385 * MiB, (uint64_t)15000000000ull})
        for (const uint64_t ring : {(uint64_t)0, 12 * MiB - 1, 12 * MiB, 100 * MiB, 300 * MiB}) {
            CHECK(stage_chunk_bytes(total, ring, 0) == old_chunk_bytes_segments(total, ring));
            for (const int mb : {0, 1, 128}) {
                const uint64_t ch = stage_chunk_bytes(total, ring, mb);
                CHECK(ch == old_chunk_bytes_staged(total, ring, mb));
                for (const int st : {0, 1, 32, 64})
                    for (const unsigned hw : {1u, 2u, 16u, 256u}) CHECK(stage_crew_threads(st, hw, ch) == old_crew_threads(st, hw, ch));
            }
        }
}

// ---- the lease ----
void lease_cases() {
    RingGate gate;
    {
        RingLease first(gate);
        CHECK(first);
        RingLease second(gate);
        CHECK(!second);
    }   // (the refused lease ends first: it must not release what it never held)
    { RingLease again(gate); CHECK(again); }
    int inside = 0;   // written under the lease alone: a lease held twice at once is a data race on it, and a count other than 1
    std::atomic<int> got{0}, twice{0};
    auto racer = [&] {
        for (int i = 0; i < 10000; ++i) {
            RingLease l(gate);
            if (!l) continue;
            if (++inside != 1) ++twice;
            --inside;
            ++got;
        }
    };
    std::thread other(racer);
    racer();
    other.join();
    CHECK(twice.load() == 0 && inside == 0 && got.load() >= 1);
    { RingLease last(gate); CHECK(last); }
}

}  // namespace

int main() {
    const char *tmp = std::getenv("TMPDIR");
    std::string templ = std::string(tmp && *tmp ? tmp : "/tmp") + "/upload_host_check.XXXXXX";
    CHECK(::mkdtemp(&templ[0]) != nullptr);
    g_dir = templ;
    seg_every_window();
    seg_block_border();
    seg_first_bad();
    seg_io_failures();
    crew_cases();
    parallel_for_cases();
    policy_grid();
    lease_cases();
    for (const std::string &p : g_made) (void)::unlink(p.c_str());
    (void)::rmdir(g_dir.c_str());
    std::printf("upload_host_check: ok\n");
    return 0;
}

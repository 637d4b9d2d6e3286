// upload.cpp -- the staged uploads: host memory or files -> HBM through the ctx's ring of pinned chunks.  ONE chunk pipeline (run_chunk_pipeline)
// serves the plain transfers (upload_big, upload_file, upload_text_pieces) and the stretches of the graph arrays (upload_segments); what fills a chunk
// on the host, and the policies that size the ring and the crew, are upload_host.hpp.  Nobody else names ctx->pin_text.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <thread>
#include "common.hpp"

namespace ptx {
namespace {

struct ChunkPiece { void *d_dst; uint64_t size; };
// fills `slot` with bytes [off, off + n) of piece `piece`, on the crew's threads; returns when the slot is full
using ChunkFill = std::function<void(StageCrew &crew, uint8_t *slot, size_t piece, uint64_t off, uint64_t n)>;
struct ChunkStats {   // what the callers' trace lines print
    uint64_t total = 0, chunks = 0, chunk_bytes = 0;
    int threads = 0;
    bool bound = false, ran = false;
    double t_gate = 0, t_wait = 0, t_fill = 0, t_enq = 0, t_drain = 0, t_all = 0;   // ms
};
struct SlotEvents {   // one event per slot of the ring: recorded behind the slot's copy, awaited before the slot is filled again
    hipEvent_t ev[STAGE_SLOTS] = {};
    hipError_t create() {
        for (auto &e : ev) if (const hipError_t rc = hipEventCreateWithFlags(&e, hipEventDisableTiming)) return rc;
        return hipSuccess;
    }
    ~SlotEvents() { for (auto &e : ev) if (e) (void)hipEventDestroy(e); }
};
using Clock = std::chrono::steady_clock;
double ms_between(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

// Pieces with their own destinations -> HBM through the ring: chunk i+1 (and i+2) is filled while chunk i is on its way; `stream` carries the
// copies.  The pipeline runs across the piece borders without draining (the GAF load: a piece is tokenised while the next ones travel):
// before_piece(k) may block until piece k's destination is free (false aborts), after_piece(k) is called once the last chunk of piece k has been
// enqueued (the caller records an event there).  The calling thread fills with the crew, enqueues and waits; nothing else touches the ring: it is
// leased for the duration.  `stream` is drained before this returns, on success and on failure: no copy out of the ring, and nothing the caller
// enqueued on `stream` before, is in flight afterwards.
int run_chunk_pipeline(Ctx *ctx, hipStream_t stream, const ChunkPiece *pieces, size_t n_pieces, int stage_ch_mb, const ChunkFill &fill,
                       const std::function<bool(size_t)> &before_piece, const std::function<int(size_t)> &after_piece, ChunkStats &st) {
    RingLease lease(ctx->ring_gate);
    if (!lease) return fail(ctx, PANTAX_HIP_E_STATE, "staging ring in use by another upload on this ctx");
    PinBuf &ring = ctx->pin_text;
    for (size_t k = 0; k < n_pieces; ++k) st.total += pieces[k].size;
    const uint64_t CH = st.chunk_bytes = stage_chunk_bytes(st.total, ring.n, stage_ch_mb);
    NumaBind numa_bind(ctx->cfg.numa_bind, ctx->numa);   // the ring's pages, this thread and the crew it starts: on the GPU's NUMA node until the upload is over
    st.bound = numa_bind.bound;
    PTX_HIP(ctx, ring.reserve(STAGE_SLOTS * CH));
    st.threads = stage_crew_threads(ctx->cfg.stage_threads, std::thread::hardware_concurrency(), CH);
    StageCrew crew(st.threads);
    SlotEvents slots;
    PTX_HIP(ctx, slots.create());
    const auto t_begin = Clock::now();
    st.ran = true;
    int rc = 0;
    {
        struct Drain {   // on every way out of the loop; on the failure path a failed wait is ignored: the first error stays the reported one
            Ctx *ctx; hipStream_t stream; int &rc; ChunkStats &st; Clock::time_point t_begin;
            ~Drain() {
                const auto t0 = Clock::now();
                if (hipStreamSynchronize(stream) != hipSuccess && rc == 0) rc = fail(ctx, PANTAX_HIP_E_HIP, "upload failed");
                const auto t1 = Clock::now();
                st.t_drain = ms_between(t0, t1); st.t_all = ms_between(t_begin, t1);
            }
        } drain{ctx, stream, rc, st, t_begin};
        uint64_t &i = st.chunks;
        for (size_t pk = 0; pk < n_pieces && rc == 0; ++pk) {
            const auto tg = Clock::now();
            if (before_piece && !before_piece(pk)) { rc = PANTAX_HIP_E_STATE; break; }
            st.t_gate += ms_between(tg, Clock::now());
            uint8_t *dst = static_cast<uint8_t *>(pieces[pk].d_dst);
            for (uint64_t off = 0; off < pieces[pk].size && rc == 0; off += CH, ++i) {
                const uint64_t n = std::min<uint64_t>(CH, pieces[pk].size - off);
                const int k = (int)(i % STAGE_SLOTS);
                uint8_t *slot = ring.p + (uint64_t)k * CH;
                const auto t0 = Clock::now();
                if (i >= STAGE_SLOTS && hipEventSynchronize(slots.ev[k]) != hipSuccess) { rc = fail(ctx, PANTAX_HIP_E_HIP, "hipEventSynchronize failed"); break; }
                const auto t1 = Clock::now();
                fill(crew, slot, pk, off, n);
                const auto t2 = Clock::now();
                if (hipMemcpyAsync(dst + off, slot, n, hipMemcpyHostToDevice, stream) != hipSuccess ||
                    hipEventRecord(slots.ev[k], stream) != hipSuccess) rc = fail(ctx, PANTAX_HIP_E_HIP, "upload failed");
                st.t_wait += ms_between(t0, t1); st.t_fill += ms_between(t1, t2); st.t_enq += ms_between(t2, Clock::now());
            }
            if (rc == 0 && after_piece) rc = after_piece(pk);
        }
    }
    return rc;
}

struct UploadPiece { void *d_dst; const uint8_t *src; uint64_t file_off, size; };   // src, or bytes of `fd` from file_off
int upload_staged_pieces(Ctx *ctx, const UploadPiece *pieces, size_t n_pieces, int fd, hipStream_t stream,
                         const std::function<bool(size_t)> &before_piece, const std::function<int(size_t)> &after_piece) {
    std::vector<ChunkPiece> cps(n_pieces);
    for (size_t k = 0; k < n_pieces; ++k) cps[k] = ChunkPiece{pieces[k].d_dst, pieces[k].size};
    const ChunkFill fill = [&](StageCrew &crew, uint8_t *slot, size_t pk, uint64_t off, uint64_t n) {
        crew.fill(slot, pieces[pk].src, fd, (pieces[pk].src ? 0 : pieces[pk].file_off) + off, n);
    };
    ChunkStats st;
    const int rc = run_chunk_pipeline(ctx, stream, cps.data(), n_pieces, ctx->cfg.stage_ch_mb, fill, before_piece, after_piece, st);
    if (ctx->cfg.trace && st.ran)
        std::fprintf(stderr, "[upload_staged] %.1f MB in %.2f ms (%.1f GB/s): %zu piece(s), %llu chunks of %.0f MB, %d threads; waiting for a piece buffer %.2f, for a slot %.2f, "
                     "filling %.2f, enqueue %.2f, drain %.2f ms; NUMA node %d (%s)\n", st.total / 1e6, st.t_all, st.total / 1e6 / st.t_all, n_pieces,
                     (unsigned long long)st.chunks, st.chunk_bytes / 1048576.0, st.threads, st.t_gate, st.t_wait, st.t_fill, st.t_enq, st.t_drain, ctx->numa.node, st.bound ? "bound" : "not bound");
    return rc;
}

int upload_staged(Ctx *ctx, void *d_dst, const void *src, int fd, uint64_t file_off, uint64_t size, hipStream_t stream) {
    if (size == 0) return 0;
    if (src && size < (1ull << 20)) {   // small: not worth the staging
        PTX_HIP(ctx, hipMemcpyAsync(d_dst, src, size, hipMemcpyHostToDevice, stream));
        PTX_HIP(ctx, hipStreamSynchronize(stream));
        return 0;
    }
    const UploadPiece pc{d_dst, static_cast<const uint8_t *>(src), file_off, size};
    return upload_staged_pieces(ctx, &pc, 1, fd, stream, nullptr, nullptr);
}
}  // namespace

int upload_segments(Ctx *ctx, void *d_dst, const UploadSeg *segs, size_t n_segs, const std::string *files, int64_t *bad_seg, hipStream_t stream_arg) {
    const hipStream_t stream = stream_arg ? stream_arg : ctx->stream;
    if (bad_seg) *bad_seg = -1;
    for (size_t k = 0; k < n_segs; ++k)
        if (segs[k].out_bytes % 4) return fail(ctx, PANTAX_HIP_E_INVALID, "upload_segments: stretch %zu is not a whole number of 32-bit words", k);
    SegFiller f(segs, n_segs, files);
    const ChunkPiece all{d_dst, f.prefix[n_segs]};
    if (all.size == 0) return 0;
    const ChunkFill fill = [&](StageCrew &crew, uint8_t *slot, size_t, uint64_t c0, uint64_t n) {   // thread t: its share of the chunk's words, whatever stretches it spans
        const std::function<void(int, int)> job = [&](int t, int nt) {
            const uint64_t words = n / 4;
            const uint64_t b = c0 + 4 * (words * (uint64_t)t / (uint64_t)nt), e = c0 + 4 * (words * (uint64_t)(t + 1) / (uint64_t)nt);
            if (e > b) f.fill(slot + (b - c0), b, e);
        };
        crew.run(job);
    };
    ChunkStats st;
    const int rc = run_chunk_pipeline(ctx, stream, &all, 1, 0 /* option stage_ch_mb never applied to the stretches: their chunks follow the transfer */, fill, nullptr, nullptr, st);
    if (ctx->cfg.trace && st.ran)
        std::fprintf(stderr, "[upload_segments] %.1f MB in %.2f ms (%.1f GB/s): %zu stretches, %llu chunks of %.0f MB, %d threads; waiting for a slot %.2f, filling %.2f ms\n",
                     st.total / 1e6, st.t_all, st.total / 1e6 / st.t_all, n_segs, (unsigned long long)st.chunks, st.chunk_bytes / 1048576.0, st.threads, st.t_wait, st.t_fill);
    if (rc) return rc;
    if (f.io_fail.load() >= 0) {
        const UploadSeg &s = segs[f.io_fail.load()];
        return fail(ctx, PANTAX_HIP_E_IO, "cannot read %s (bytes from %llu)", s.file >= 0 ? files[s.file].c_str() : "<memory>", (unsigned long long)s.file_off);
    }
    if (bad_seg) *bad_seg = f.bad.load();
    return 0;
}

int upload_big(Ctx *ctx, void *d_dst, const void *src, uint64_t size) { return upload_staged(ctx, d_dst, src, -1, 0, size, ctx->stream); }
int upload_file(Ctx *ctx, void *d_dst, int fd, uint64_t file_off, uint64_t size) { return upload_staged(ctx, d_dst, nullptr, fd, file_off, size, ctx->stream); }
int upload_text_pieces(Ctx *ctx, size_t n_pieces, void *const *d_dst, const char *text, int fd, uint64_t file_base, const uint64_t *piece_off, const uint64_t *piece_end,
                       hipStream_t stream, const std::function<bool(size_t)> &before_piece, const std::function<int(size_t)> &after_piece) {
    std::vector<UploadPiece> pcs(n_pieces);
    for (size_t k = 0; k < n_pieces; ++k)
        pcs[k] = UploadPiece{d_dst[k], fd >= 0 ? nullptr : reinterpret_cast<const uint8_t *>(text) + piece_off[k], file_base + piece_off[k], piece_end[k] - piece_off[k]};
    return upload_staged_pieces(ctx, pcs.data(), n_pieces, fd, stream, before_piece, after_piece);
}

}  // namespace ptx

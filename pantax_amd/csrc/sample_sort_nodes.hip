// sample_sort_nodes.hip -- the LP rows of MANY species sorted straight from the NODE arrays: no compaction pass.  The entry point; the kernels of
// every stage are in the ssn_*.hip file named below, what they share in ssn_device.hpp, geometry and workspace layout in ssn_plan.hpp.
//
// A row of the LP is a node with a_v > 0 and a non-empty membership mask (profile.rs:1380-1385); the solver wants every species' rows ordered by
// (mask, a).  A species' SEGMENT is its node range [node_base[s], node_base[s+1]) -- known on the host -- and the sort's own passes skip the nodes
// that are no rows (earlier rounds sorted rows that a scan had compacted first: one more pass over everything):
//   1. ssn_sample.hip    : 4096 evenly spaced nodes of the segment, the rows among them sorted in LDS -> 1023 splitters at even ranks of the valid
//                          samples, stored as an implicit search tree in breadth-first order (a level's nodes are neighbours in LDS: the descent
//                          of 64 lanes meets no systematic bank conflict, where the upper levels of a binary search over the sorted array all fall
//                          on ONE bank).  A segment of <= 4096 nodes is sorted completely right there
//   2. ssn_node_pass.hip : bucket id of every row (ten tree levels; "equal to splitter j" is its own bucket 2j+1 whose rows need no sorting --
//                          coverage values tie massively).  A workgroup walks SEVERAL tiles of its segment with one LDS histogram and stores it as
//                          a row of the segment's count matrix: no global atomics.  The resident step's kernel (node_rows_kernel) forms the
//                          abundances, the node statistics, the masks and the column sums in the same pass; the stage calls and fallbacks run its
//                          two-kernel twin (ssn_hist_kernel)
//   3. ssn_partition.hip : column sums of the matrix -> bucket starts, the matrix rewritten as every workgroup's first slot in every bucket; rows
//                          per segment -> first output row of every segment, total row count
//   4. ssn_partition.hip : rows {mask, a} as 16-byte records into their bucket (slots from LDS counters seeded by the matrix row) -- the rows of
//                          the EVEN buckets only: a tie bucket holds copies of one key, so it is written as a fill of the output (coalesced) and
//                          its rows never travel -- and of its rows the step keeps `a` alone, so the fill stores no key words (ssn_keys_all).  One 16-byte store per row is what this pass costs (tools/native/scatter_probe.hip: 2e8 rows
//                          into 2048 buckets 4.2 ms, 1024: 3.5, 256: 2.9; the real rows, which tie massively, take 3.15 ms either way)
//   5. ssn_local.hip     : a wave per even bucket, up to 512 rows sorted in registers; 513 .. 1024 rows in a second kernel; the rare larger buckets
//                          through an LDS network, above 4096 rows (every bucket of a species of millions of nodes) in place through memory
//   6. ssn_patterns.hip  : (with `pat`) the runs of equal mask, found from the splitters without a pass over the rows
// The number of rows of a segment is only known on the device; launch geometry comes from the node counts (ssn_plan).
#include <algorithm>
#include <cstdio>
#include <vector>
#include "ssn_device.hpp"

namespace ptx {

size_t sample_sort_nodes_ws_elems(uint32_t S, uint64_t seg_bound, uint64_t V) { return ssn_plan(S, seg_bound, V).total_words; }

// Nodes of segment s: [node_base[s], node_base[s + 1]) (device array, the host knows that no segment exceeds seg_bound <= SSN_MAX_SEG
// nodes); a node is a row when ab > 0 and mask != 0.  Output: the rows of all segments back to back, every segment sorted by
// (mask, a), in the words k -- pack_shift < 0: {species, mask, a}; otherwise {species << pack_shift | mask, a} and k[2] is not used;
// *d_n = the number of rows.  rows16: 4 V words of scratch.
int sample_sort_nodes(Ctx *ctx, const double *ab, const uint64_t *mask, const uint32_t *d_node_base, uint32_t S, uint64_t seg_bound, uint64_t V,
                      uint64_t *rows16, uint64_t *const k[3], int pack_shift, uint32_t *d_ws, uint32_t *d_n, const RowPatterns *pat,
                      const RowMaskSource *haps, const NodeCovSource *fused) {
    if (S == 0 || V == 0) {
        PTX_HIP(ctx, hipMemsetAsync(d_n, 0, sizeof(uint32_t), ctx->stream));
        if (pat) { PTX_HIP(ctx, hipMemsetAsync(pat->d_K, 0, sizeof(uint32_t), ctx->stream)); PTX_HIP(ctx, hipMemsetAsync(pat->sp_pat_off, 0, (S + 1) * sizeof(uint32_t), ctx->stream));
                   PTX_HIP(ctx, hipMemsetAsync(pat->pat_start, 0, sizeof(uint32_t), ctx->stream)); }
        return 0;
    }
    if (seg_bound > SSN_MAX_SEG) return fail(ctx, PANTAX_HIP_E_LIMIT, "sample_sort_nodes: a segment of %llu nodes exceeds %llu", (unsigned long long)seg_bound, (unsigned long long)SSN_MAX_SEG);
    if (S > 65535) return fail(ctx, PANTAX_HIP_E_LIMIT, "sample_sort_nodes: %u segments exceed the launch grid", S);
    if (haps) { if (haps->max_haps > 64) return fail(ctx, PANTAX_HIP_E_INVALID, "sample_sort_nodes: masks from haplotype words take species of at most 64 haplotypes"); }
    else if (!mask) return fail(ctx, PANTAX_HIP_E_INVALID, "sample_sort_nodes: neither a mask array nor haplotype words");
    if (fused && (!haps || !fused->bases || !fused->bit_off || !fused->full || !fused->bitmap || !fused->amax || !fused->nvalid || !fused->nzsum || !fused->nzcnt))
        return fail(ctx, PANTAX_HIP_E_INVALID, "sample_sort_nodes: the fused node pass takes haplotype words and the coverage arena");
    if (!fused && !ab) return fail(ctx, PANTAX_HIP_E_INVALID, "sample_sort_nodes: no abundance array");

    const int keys_all = ssn_keys_all(ctx->cfg.ssn_keys.c_str(), pat != nullptr);
    if (keys_all < 0) return fail(ctx, PANTAX_HIP_E_INVALID, "sample_sort_nodes: option ssn_keys=%s%s", ctx->cfg.ssn_keys.c_str(), pat ? "" : " (a sort whose caller reads the keys stores all of them)");
    const int node_bits = ssn_node_bits(ctx->cfg.node_bits.c_str(), ctx->cfg.node_bits_words);
    if (node_bits < 0) return fail(ctx, PANTAX_HIP_E_INVALID, "sample_sort_nodes: option node_bits is \"range\" or \"gather\" and node_bits_words 0, 1 or 2, not \"%s\" and %d", ctx->cfg.node_bits.c_str(), ctx->cfg.node_bits_words);

    const SsnPlan pl = ssn_plan(S, seg_bound, V);
    Sn sn;
    sn.node_base = d_node_base; sn.ab = ab; sn.mask = haps ? nullptr : mask;
    if (haps) sn.hp = *haps;
    if (fused) { sn.fz = *fused; sn.ab = nullptr; sn.hp.cov = nullptr; }
    sn.G = pl.G; sn.per = pl.per;
    sn.ablate = ctx->cfg.ssn_ablate;
    sn.skip_empty = ctx->cfg.no_absent_skip ? 0u : 1u;
    sn.ws = d_ws + pl.ws;                                         // (d_ws: a DevBuf allocation, 16-byte aligned and more; the plan keeps c0p and npart at even words)
    sn.cntm = d_ws + pl.cntm;
    sn.stage_cnt = d_ws + pl.stage_cnt;
    sn.c0p = reinterpret_cast<double *>(d_ws + pl.c0p);
    sn.c0 = pat ? pat->c0 : nullptr;
    sn.seg_n = d_ws + pl.seg_n; sn.seg_out = d_ws + pl.seg_out;
    uint32_t *sub_k = d_ws + pl.sub_k;
    sn.ids = reinterpret_cast<uint16_t *>(d_ws + pl.ids);
    sn.npart = reinterpret_cast<NodePartial *>(d_ws + pl.npart);
    sn.rows = reinterpret_cast<ulonglong2 *>(rows16);
    sn.stage = reinterpret_cast<ulonglong2 *>(rows16) + V;
    sn.ksp = pack_shift >= 0 ? nullptr : k[0];
    sn.km = pack_shift >= 0 ? k[0] : k[1];
    sn.ka = pack_shift >= 0 ? k[1] : k[2];
    sn.pack_shift = pack_shift;
    sn.keys_all = (uint32_t)keys_all;
    if (!keys_all && ctx->cfg.ssn_poison_keys) {   // tests: the buffers outlive the step, and an earlier sort's key words would pass for this one's
        PTX_TRY(byte_fill(ctx, sn.km, 0xA5, V * sizeof(uint64_t)));
        if (sn.ksp) PTX_TRY(byte_fill(ctx, sn.ksp, 0xA5, V * sizeof(uint64_t)));
    }

    { KTimer t(ctx, "ssn_sample_kernel");
      ssn_sample_launch(ctx, sn, S, fused != nullptr); }
    if (fused) {
        // The one pass over the nodes of the resident step.  With ssn_gather_kernel above it is the LAST reader of `bases`, the bit vector and the full-node
        // flags: the side-stream zero fill of the coverage arena (coverage_arena_clean_async) is enqueued by strain_enqueue after lad_prepare has returned,
        // i.e. behind this launch; the event the next step's index rebuild waits for (ev_trio_free) was recorded before the sort and concerns the trio
        // tables only, which nothing here reads.
        KTimer t(ctx, "node_rows_kernel");
        ssn_node_rows_launch(ctx, sn, S, haps->max_haps, node_bits);
    } else {
        KTimer t(ctx, "ssn_hist_kernel");
        ssn_hist_launch(ctx, sn, S, haps != nullptr, haps ? haps->max_haps : 0u);
    }
    { KTimer t(ctx, "ssn_offsets_kernel");
      ssn_offsets_launch(ctx, sn, S, d_n); }
    // The tie fill writes the odd bucket ranges of the output and reads the bucket starts, the splitter tree and seg_out, all complete behind the offsets
    // kernels; the scatter and the local sorts touch the even buckets and the scratch.  ssn_ties_async: the fill goes onto the side stream from here and is
    // joined in front of the first reader of the whole output (the heads kernel; without `pat`, the caller).  The guard joins on the host if anything
    // between fork and join fails: nothing may return with the fill still running unordered on the side stream.
    const bool clocked = ctx->timing && ctx->timing_filter.empty();
    const bool ties_async = ssn_ties_async(ctx->cfg.ssn_ties_async, clocked, ctx->stream_main != nullptr, ctx->stream2 != nullptr);
    struct TieJoin {
        Ctx *c; bool armed;
        ~TieJoin() { if (armed) (void)hipStreamSynchronize(c->stream2); }
    } tie_join{ctx, false};
    if (ties_async) {
        if (!ctx->ev_ssn_fork) PTX_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_ssn_fork, hipEventDisableTiming));
        if (!ctx->ev_ssn_join) PTX_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_ssn_join, hipEventDisableTiming));
        PTX_HIP(ctx, hipEventRecord(ctx->ev_ssn_fork, ctx->stream));
        PTX_HIP(ctx, hipStreamWaitEvent(ctx->stream2, ctx->ev_ssn_fork, 0));
        hipError_t e;
        {
            SideStream side(ctx);   // (never refused: the plan above keeps the fill in line on a ctx that is on its side stream already)
            tie_join.armed = true;
            { KTimer t(ctx, "ssn_ties_kernel");
              ssn_ties_launch(ctx, sn, S, pl.tie_grid); }
            e = hipEventRecord(ctx->ev_ssn_join, ctx->stream2);
        }
        PTX_HIP(ctx, e);
    }
    { KTimer t(ctx, "ssn_scatter_kernel");
      ssn_scatter_launch(ctx, sn, S); }
    if (!ties_async) {
        KTimer t(ctx, "ssn_ties_kernel");
        ssn_ties_launch(ctx, sn, S, pl.tie_grid);
    }
    { KTimer t(ctx, "ssn_local_wave_kernel");
      ssn_local_launch(ctx, sn, S); }
    if (ties_async) {
        PTX_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_ssn_join, 0));
        tie_join.armed = false;   // joined: everything later on the main stream is ordered behind the fill
    }
    if (pat) {
        KTimer t(ctx, "ssn_heads_kernel");
        ssn_patterns_launch(ctx, sn, S, sub_k, *pat, d_n);
    }
    PTX_HIP(ctx, hipGetLastError());
    if (ctx->cfg.ssn_debug) {   // measurements: bucket statistics of this sort on stderr (synchronises)
        PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
        std::vector<uint32_t> h((size_t)S * SN_WS_WORDS);
        PTX_HIP(ctx, hipMemcpy(h.data(), sn.ws, h.size() * 4, hipMemcpyDeviceToHost));
        uint64_t n_small = 0, rows = 0, n_med = 0, n_big = 0, n_over = 0, max_b = 0, max_rows = 0, n512 = 0, n256 = 0, nb = 0;
        for (uint32_t sg = 0; sg < S; ++sg) {
            const uint32_t *w = h.data() + (size_t)sg * SN_WS_WORDS;
            rows += w[SN_OFF_FLAGS + 3]; max_rows = std::max<uint64_t>(max_rows, w[SN_OFF_FLAGS + 3]);
            if (w[SN_OFF_FLAGS]) { ++n_small; continue; }
            n_med += w[SN_OFF_FLAGS + 2]; n_big += w[SN_OFF_FLAGS + 1];
            for (int b = 0; b < SN_NBUCKET; b += 2) {
                const uint32_t m = w[SN_OFF_START + b + 1] - w[SN_OFF_START + b];
                if (!m) continue;
                ++nb; max_b = std::max<uint64_t>(max_b, m);
                if (m > 256) ++n256;
                if (m > 512) ++n512;
                if (m > (uint32_t)SN_CAP) ++n_over;
            }
        }
        std::fprintf(stderr, "[ssn] S=%u small=%llu rows=%llu max rows/segment=%llu | even buckets in use %llu, >256: %llu, >512: %llu (list %llu), >1024: %llu, >4096: %llu, largest %llu | G=%u per=%u\n", S,
                     (unsigned long long)n_small, (unsigned long long)rows, (unsigned long long)max_rows, (unsigned long long)nb, (unsigned long long)n256, (unsigned long long)n512,
                     (unsigned long long)n_med, (unsigned long long)n_big, (unsigned long long)n_over, (unsigned long long)max_b, sn.G, sn.per);
    }
    return 0;
}

}  // namespace ptx

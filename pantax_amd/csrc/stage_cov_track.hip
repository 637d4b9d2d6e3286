// stage_cov_track.hip -- per-strain windowed coverage track (pantax_hip_strain_cov_track, the --strain-coverage report): coverage along the genome of
// selected haplotypes, from what the coverage pass leaves in HBM.  Not a stage of the reference.
//
// Contract (include/pantax_hip.h, DESIGN.md "Per-strain coverage track"): along the walk v_0 .. v_{n-1} of a haplotype, step i starts at the path offset
// o_i = sum_{j<i} node_len[v_j] (u64) and belongs to window w_i = o_i / W -- the window of the node's FIRST base; a node is never cut.  Per window:
// the number of steps, and the sums of node_len, node_base_cov and bases_per_node over them.  Integers only: the result does not depend on any order.
//
// A selected walk is cut into tiles at the multiples of CT_TILE path positions (so a lane's quads of node ids are 16-byte aligned); a wave per tile,
// 16 consecutive positions per lane.
//   cov_track_len_kernel    the summed node length of every tile.  The host scans the sums per haplotype: base offset of every tile, G_h, n_win.
//   cov_track_accum_kernel  o_i from the lane's own 16 lengths on top of the DPP scan of the lane sums on top of the tile base.  Window ids do not
//                           decrease along a walk: a lane folds its positions into runs of equal id, adds the runs that END inside it to the output
//                           itself, and hands its last run to a segmented DPP scan over the lanes (a lane opens a segment when its first window is
//                           not its predecessor's last, or when it closed a run itself).  The last lane of a segment adds the segment's sums: one
//                           64-bit atomic per (wave, window) and quantity wherever windows are longer than a lane's 16 nodes.
//
// Algorithmic bytes (P_sel selected path positions, n_win windows):
//   4 P_sel (node ids) + 4 P_sel (lengths)                  cov_track_len_kernel
//   4 P_sel (node ids) + (4 + 4 + 8) P_sel (len, cov, bases)  cov_track_accum_kernel
//   28 n_win                                                 the four output arrays (zero fill, atomics, download)
#include <algorithm>
#include "common.hpp"
#include "cov_track_plan.hpp"
#include "cov_track_tile.hpp"
#include "primitives.hpp"
#include "wave.hpp"

namespace ptx {

namespace {

// (CT_TILE, CtTile, CtTileOut, ct_load_ids and ct_incl_scan64: cov_track_tile.hpp, shared with stage_segments.hip and stage_growth.hip)

__global__ void __launch_bounds__(256) cov_track_len_kernel(uint32_t n_tiles, const CtTile *__restrict__ tiles, const uint32_t *__restrict__ path_nodes,
                                                            const uint32_t *__restrict__ node_len, unsigned long long *__restrict__ tile_sum) {
    const int lane = threadIdx.x & 63;
    for (uint32_t t = blockIdx.x * 4 + (threadIdx.x >> 6); t < n_tiles; t += gridDim.x * 4) {
        const CtTile tl = tiles[t];
        uint32_t v[16];
        const uint32_t live = ct_load_ids(path_nodes, (tl.p0 & ~(CT_TILE - 1)) + 16u * (uint32_t)lane, tl.p0, tl.p0 + tl.n, tl.node_base, v);
        unsigned long long s = 0ull;
#pragma unroll
        for (int j = 0; j < 16; ++j) { const uint32_t l = node_len[v[j]]; s += ((live >> j) & 1u) ? l : 0u; }
        s = wave_reduce(s, [](unsigned long long a, unsigned long long b) { return a + b; });
        if (lane == 0) tile_sum[t] = s;
    }
}

// (CtAcc, ct_seg_scan, CtOut and ct_add: cov_track_tile.hpp, shared with stage_growth.hip)
__global__ void __launch_bounds__(256) cov_track_accum_kernel(uint32_t n_tiles, const CtTile *__restrict__ tiles, const CtTileOut *__restrict__ touts,
                                                              const uint32_t *__restrict__ path_nodes, const uint32_t *__restrict__ node_len,
                                                              const uint32_t *__restrict__ cov, const unsigned long long *__restrict__ bases, uint64_t W, CtOut out) {
    const int lane = threadIdx.x & 63;
    for (uint32_t t = blockIdx.x * 4 + (threadIdx.x >> 6); t < n_tiles; t += gridDim.x * 4) {
        const CtTile tl = tiles[t];
        const CtTileOut to = touts[t];
        uint32_t v[16], len[16], cv[16];
        unsigned long long bs[16];
        const uint32_t live = ct_load_ids(path_nodes, (tl.p0 & ~(CT_TILE - 1)) + 16u * (uint32_t)lane, tl.p0, tl.p0 + tl.n, tl.node_base, v);
        unsigned long long lane_sum = 0ull;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const bool on = (live >> j) & 1u;
            const uint32_t l = node_len[v[j]], c = cov[v[j]];
            const unsigned long long b = bases[v[j]];
            len[j] = on ? l : 0u; cv[j] = on ? c : 0u; bs[j] = on ? b : 0ull;
            lane_sum += len[j];
        }
        const uint64_t o0 = to.base + (ct_incl_scan64(lane_sum) - lane_sum);   // path offset of the lane's first position
        // the window of the running position: one division per lane, another only where a step leaves its window
        uint64_t w = o0 / W, rem = o0 - w * W;
        uint64_t w_first = 0, w_cur = 0;
        bool have = false, closed = false;
        CtAcc acc{0u, 0ull, 0ull, 0ull};
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const bool on = (live >> j) & 1u;
            if (on & have & (w != w_cur)) {   // the run before this step ends inside the lane
                ct_add(out, to.out0, to.n_win, true, w_cur, acc);
                acc = CtAcc{0u, 0ull, 0ull, 0ull};
                closed = true;
            }
            w_first = (on & !have) ? w : w_first;
            w_cur = on ? w : w_cur;
            have = have | on;
            acc.n += on ? 1u : 0u; acc.len += len[j]; acc.cov += cv[j]; acc.bases += bs[j];
            rem += len[j];
            if (rem >= W) { const uint64_t k = rem / W; w += k; rem -= k * W; }
        }
        // the lane's last run goes on over the lanes that follow: a lane opens a segment unless it is the plain continuation of its predecessor's run
        const uint32_t p_lo = wave_shr1((uint32_t)w_cur), p_hi = wave_shr1((uint32_t)(w_cur >> 32)), p_have = wave_shr1(have ? 1u : 0u);
        const uint64_t w_prev = ((uint64_t)p_hi << 32) | p_lo;
        const bool head = (lane == 0) | !have | (p_have == 0u) | closed | (w_first != w_prev);
        const unsigned long long heads = __builtin_amdgcn_ballot_w64(head);
        const int seg = 63 - __builtin_clzll(heads & (~0ull >> (63 - lane)));   // (bit 0 is always set)
        ct_seg_scan(acc, lane, seg);
        const bool last = have & ((lane == 63) | (((heads >> 1) >> lane) & 1ull));   // the segment ends here: among live lanes only
        ct_add(out, to.out0, to.n_win, last, w_cur, acc);
    }
}

}  // namespace

// The tiles of the selected walks, the length pass over them and the host scan of its sums per haplotype (base offset of every tile, G_h, n_win):
// win_off_out [C+1] is written, the tiles and their output records are left on the device.  `who` names the caller in messages (cov_track_launch here,
// growth_launch in stage_growth.hip).
int cov_track_plan(Ctx *ctx, Db *db, const char *who, const uint64_t *sel_off, const uint32_t *sel_hap, uint64_t W, uint64_t *win_off_out, uint64_t cap, CtPlan &pl) {
    const uint32_t S = db->S;
    const uint64_t C = sel_off[S];
    std::vector<CtTile> tiles;
    std::vector<uint64_t> tile_first(C + 1, 0);   // first tile of every selected haplotype
    for (uint32_t s = 0; s < S; ++s)
        for (uint64_t c = sel_off[s]; c < sel_off[s + 1]; ++c) {
            const uint64_t h = db->h_hap_off[s] + sel_hap[c], p1 = db->h_path_off[h + 1];
            for (uint64_t p = db->h_path_off[h]; p < p1;) {
                const uint64_t e = std::min(p1, (p & ~(CT_TILE - 1)) + CT_TILE);
                tiles.push_back(CtTile{p, (uint32_t)(e - p), (uint32_t)db->h_node_off[s]});
                p = e;
            }
            tile_first[c + 1] = tiles.size();
        }
    if (tiles.size() >= 0xFFFFFFFFull) return fail(ctx, PANTAX_HIP_E_LIMIT, "%s: %llu tiles of selected walks exceed 32-bit positions", who, (unsigned long long)tiles.size());
    const uint32_t n_tiles = (uint32_t)tiles.size();
    DevBuf<unsigned long long> d_sum;
    std::vector<unsigned long long> sums(n_tiles);
    if (n_tiles) {
        PTX_TRY(upload(ctx, pl.d_tiles, tiles.data(), tiles.size()));
        PTX_HIP(ctx, d_sum.alloc(n_tiles));
        {
            KTimer tm(ctx, "cov_track_len_kernel");
            hipLaunchKernelGGL(cov_track_len_kernel, dim3(grid_for(n_tiles, 4, ctx->n_cu * 16)), dim3(256), 0, ctx->stream, n_tiles, pl.d_tiles.p, db->d_path_nodes.p,
                               db->d_node_len.p, d_sum.p);
        }
        PTX_HIP(ctx, hipGetLastError());
        PTX_TRY(download(ctx, sums.data(), d_sum.p, n_tiles));
        PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    // per haplotype: the exclusive scan of its tiles' sums, its length, its windows
    std::vector<CtTileOut> touts(n_tiles);
    win_off_out[0] = 0;
    for (uint64_t c = 0; c < C; ++c) {
        uint64_t g = 0;
        for (uint64_t t = tile_first[c]; t < tile_first[c + 1]; ++t) { touts[t].base = g; g += sums[t]; }
        const uint64_t n_win = g / W + (g % W ? 1 : 0);
        for (uint64_t t = tile_first[c]; t < tile_first[c + 1]; ++t) { touts[t].out0 = win_off_out[c]; touts[t].n_win = n_win; }
        win_off_out[c + 1] = win_off_out[c] + n_win;
    }
    pl.n_tiles = n_tiles;
    pl.tile_first = std::move(tile_first);
    const uint64_t N = win_off_out[C];
    if (N > cap) return fail(ctx, PANTAX_HIP_E_LIMIT, "%s: the selection has %llu windows, the output arrays hold %llu (win_off_out is filled: size the arrays by it)", who,
                             (unsigned long long)N, (unsigned long long)cap);
    if (N) PTX_TRY(upload(ctx, pl.d_touts, touts.data(), touts.size()));
    return 0;
}

// sel_off [S+1], sel_hap validated by the caller (in range, no repeats).  win_off_out [C+1] is always written; more than `cap` windows: PANTAX_HIP_E_LIMIT
// and nothing else is touched.
int cov_track_launch(Ctx *ctx, Db *db, const uint64_t *sel_off, const uint32_t *sel_hap, uint64_t W, uint64_t *win_off_out, uint64_t cap, uint32_t *n_nodes_out,
                     uint64_t *len_out, uint64_t *covered_out, uint64_t *bases_out) {
    CtPlan pl;
    PTX_TRY(cov_track_plan(ctx, db, "strain_cov_track", sel_off, sel_hap, W, win_off_out, cap, pl));
    const uint64_t N = win_off_out[sel_off[db->S]];
    const uint32_t n_tiles = pl.n_tiles;
    if (N == 0) return 0;
    if (!n_nodes_out || !len_out || !covered_out || !bases_out) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_cov_track: null output array");
    if (N > (~(size_t)0) / 32) return fail(ctx, PANTAX_HIP_E_LIMIT, "strain_cov_track: %llu windows", (unsigned long long)N);
    // one device block, zero-filled once: [len N u64][covered N u64][bases N u64][n_nodes N u32]
    DevBuf<uint8_t> d_out;
    PTX_HIP(ctx, d_out.alloc((size_t)N * 28));
    PTX_TRY(zero_fill(ctx, d_out.p, (size_t)N * 28));
    unsigned long long *o64 = reinterpret_cast<unsigned long long *>(d_out.p);
    const CtOut out{reinterpret_cast<uint32_t *>(o64 + 3 * N), o64, o64 + N, o64 + 2 * N};
    {
        KTimer tm(ctx, "cov_track_accum_kernel");
        hipLaunchKernelGGL(cov_track_accum_kernel, dim3(grid_for(n_tiles, 4, ctx->n_cu * 16)), dim3(256), 0, ctx->stream, n_tiles, pl.d_tiles.p, pl.d_touts.p,
                           db->d_path_nodes.p, db->d_node_len.p, db->d_cov.p, db->d_bases.p, W, out);
    }
    PTX_HIP(ctx, hipGetLastError());
    PTX_TRY(download(ctx, (unsigned long long *)len_out, out.len, N));
    PTX_TRY(download(ctx, (unsigned long long *)covered_out, out.cov, N));
    PTX_TRY(download(ctx, (unsigned long long *)bases_out, out.bases, N));
    PTX_TRY(download(ctx, n_nodes_out, out.n, N));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));   // host arrays are filled, the temporaries are released on return
    return 0;
}

}  // namespace ptx

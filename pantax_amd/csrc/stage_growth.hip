// stage_growth.hip -- own-node windows along selected haplotypes (pantax_hip_strain_growth, the --strain-growth report): per window of a strain's walk
// the steps, length and aligned bases of the nodes that, among the selected haplotypes of its species, only this strain walks.  What the coverage track
// cannot give: its windows hold the depth of every strain that shares a node.  The fit over the windows (sort by depth, trim, line through log2 depth
// against rank: the replication index) is the host helper pantax_hip_growth_fit (growth_plan.hpp).  Not a stage of the reference.
//
// Contract (include/pantax_hip.h, DESIGN.md "Replication index per strain"): walk, o_i, G_h, w_i = o_i / W and n_win(h) of pantax_hip_strain_cov_track.
// Step i of entry c is OWN when the node's membership over the selected haplotypes of the species is exactly {c's haplotype}.  Per window: n_own (own steps),
// len (node_len over all steps, as the track has it), len_own and bases_own (node_len and bases_per_node over own steps).  Integers only: no order matters.
//
// Membership: the two routes of member_plan.hpp over the selected haplotypes (option growth_route), nw = ceil(K_s / 64) words per node on route 2.  Own <=>
// the popcount over the node's words is 1 and the entry's bit is set; the entry's word and bit travel in the tile record (route 1: word 0, bit = haplotype
// index; route 2: word k / 64, bit k % 64 for the k-th selected haplotype of the species).
//
// Tiling, length pass and host scan are the track's (cov_track_plan, stage_cov_track.hip).  growth_accum_kernel is the track's accumulation kernel with
// another gather: per position node id -> {node_len, bases_per_node, membership word(s)}; node_base_cov is not read.  bases_per_node is loaded beside
// the words and dropped by a select where the step is not own, so the dependent chain stays two loads deep (ids, then everything else) and does not
// become three (ids, words, bases); the price is 8 B per non-own position.  A lane folds its 16 steps into runs of equal window id, the last run goes
// through the segmented DPP scan: one 64-bit atomicAdd per (wave, window) and quantity wherever windows are longer than a lane's 16 nodes.  Registers: the
// lane holds v[16], len[16], bases[16] (64-bit) and a 16-bit own mask; without a bound the compiler takes 132 VGPRs (three waves a SIMD), under
// __launch_bounds__(256, 4) it takes 128 without a spill: four waves a SIMD, what the track's kernel has.  On route 2 the words of a position are taken
// in a loop of nw rounds inside the unrolled positions, so a position's loads wait for the one before.  Three loop-free forms were compiled (word by word
// over all 16 positions, over two halves of eight, both words of a position for nw <= 2, as one kernel and as an instance per route): at the 128-register
// cap each spilled 1 to 15 VGPRs in one of the two routes.  Neither form has been timed; tools/growth_probe.py with route "walk" is the measurement to
// take before the pass is relied on for wide species.
//
// Algorithmic bytes (P_sel selected path positions, n_win windows):
//   4 P_sel (node ids) + 4 P_sel (lengths)                                     cov_track_len_kernel
//   4 P_sel (node ids) + (4 + 8 + 8 nw) P_sel (len, bases, membership words)   growth_accum_kernel (nw = 1 on route 1)
//   28 n_win                                                                   the four output arrays (zero fill, atomics, download)
//   route 2: the mask pass of WalkMasks ahead of it
#include "common.hpp"
#include "cov_track_plan.hpp"
#include "cov_track_tile.hpp"
#include "member_device.hpp"
#include "primitives.hpp"
#include "wave.hpp"

namespace ptx {

namespace {

// what a tile knows of its entry beside CtTile / CtTileOut: the species' membership row, the entry's word among the node's words and its bit in it
struct GrTile { MemberRow m; uint32_t ew, eb; };

__global__ void __launch_bounds__(256, 4) growth_accum_kernel(uint32_t n_tiles, const CtTile *__restrict__ tiles, const CtTileOut *__restrict__ touts,
                                                              const GrTile *__restrict__ gtiles, const uint32_t *__restrict__ path_nodes,
                                                              const uint32_t *__restrict__ node_len, const unsigned long long *__restrict__ bases,
                                                              const unsigned long long *__restrict__ node_haps, const unsigned long long *__restrict__ mask,
                                                              uint64_t W, CtOut out) {
    const int lane = threadIdx.x & 63;
    for (uint32_t t = blockIdx.x * 4 + (threadIdx.x >> 6); t < n_tiles; t += gridDim.x * 4) {
        const CtTile tl = tiles[t];
        const CtTileOut to = touts[t];
        const GrTile gt = gtiles[t];
        uint32_t v[16], len[16];
        unsigned long long bs[16];
        const uint32_t live = ct_load_ids(path_nodes, (tl.p0 & ~(CT_TILE - 1)) + 16u * (uint32_t)lane, tl.p0, tl.p0 + tl.n, tl.node_base, v);
        unsigned long long lane_sum = 0ull;
        uint32_t own = 0u;   // bit j: step j is live and own
        if (gt.m.route == 1u) {   // (uniform over the wave)
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const bool on = (live >> j) & 1u;
                const uint32_t l = node_len[v[j]];
                const unsigned long long b = bases[v[j]], word = node_haps[v[j]] & gt.m.bits;
                const bool mine = on & (__popcll(word) == 1) & (((word >> gt.eb) & 1ull) != 0ull);
                len[j] = on ? l : 0u; bs[j] = mine ? b : 0ull; own |= (mine ? 1u : 0u) << j;
                lane_sum += len[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const bool on = (live >> j) & 1u;
                const uint32_t l = node_len[v[j]];
                const unsigned long long b = bases[v[j]];
                const uint64_t row = member_mask_row(gt.m, v[j]);
                uint32_t m = 0u;
                unsigned long long mw = 0ull;
                for (uint32_t w = 0; w < gt.m.nw; ++w) {
                    const unsigned long long x = mask[row + w];
                    m += (uint32_t)__popcll(x);
                    mw = w == gt.ew ? x : mw;
                }
                const bool mine = on & (m == 1u) & (((mw >> gt.eb) & 1ull) != 0ull);
                len[j] = on ? l : 0u; bs[j] = mine ? b : 0ull; own |= (mine ? 1u : 0u) << j;
                lane_sum += len[j];
            }
        }
        const uint64_t o0 = to.base + (ct_incl_scan64(lane_sum) - lane_sum);   // path offset of the lane's first position
        // the window of the running position: one division per lane, another only where a step leaves its window
        uint64_t w = o0 / W, rem = o0 - w * W;
        uint64_t w_first = 0, w_cur = 0;
        bool have = false, closed = false;
        CtAcc acc{0u, 0ull, 0ull, 0ull};   // {n_own, len, len_own, bases_own}
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const bool on = (live >> j) & 1u, mine = (own >> j) & 1u;
            if (on & have & (w != w_cur)) {   // the run before this step ends inside the lane
                ct_add(out, to.out0, to.n_win, true, w_cur, acc);
                acc = CtAcc{0u, 0ull, 0ull, 0ull};
                closed = true;
            }
            w_first = (on & !have) ? w : w_first;
            w_cur = on ? w : w_cur;
            have = have | on;
            acc.n += mine ? 1u : 0u; acc.len += len[j]; acc.cov += mine ? len[j] : 0u; acc.bases += bs[j];
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

// sel_off [S+1], sel_hap validated by the caller (in range, no repeats).  win_off_out [C+1] is always written; more than `cap` windows: PANTAX_HIP_E_LIMIT
// and nothing else is touched.
int growth_launch(Ctx *ctx, Db *db, const uint64_t *sel_off, const uint32_t *sel_hap, uint64_t W, uint64_t *win_off_out, uint64_t cap, uint32_t *n_own_out,
                  uint64_t *len_out, uint64_t *len_own_out, uint64_t *bases_own_out) {
    const uint32_t S = db->S;
    CtPlan pl;
    PTX_TRY(cov_track_plan(ctx, db, "strain_growth", sel_off, sel_hap, W, win_off_out, cap, pl));
    const uint64_t N = win_off_out[sel_off[S]];
    const uint32_t n_tiles = pl.n_tiles;
    if (N == 0) return 0;
    if (!n_own_out || !len_out || !len_own_out || !bases_own_out) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_growth: null output array");
    if (N > (~(size_t)0) / 32) return fail(ctx, PANTAX_HIP_E_LIMIT, "strain_growth: %llu windows", (unsigned long long)N);
    // membership of every species with a selection, and per tile its entry's word and bit
    const bool by_node = member_by_node(db->nh_built, ctx->cfg.growth_route);
    WalkMasks wm;
    std::vector<GrTile> gtiles(n_tiles);
    for (uint32_t s = 0; s < S; ++s) {
        const uint64_t K = sel_off[s + 1] - sel_off[s];
        if (K == 0) continue;
        const MemberRow m = wm.row(db, s, by_node, sel_hap + sel_off[s], K);
        for (uint64_t k = 0; k < K; ++k) {
            const uint64_t c = sel_off[s] + k;
            const GrTile g = m.route == 1u ? GrTile{m, 0u, sel_hap[c]} : GrTile{m, (uint32_t)(k >> 6), (uint32_t)(k & 63u)};
            for (uint64_t t = pl.tile_first[c]; t < pl.tile_first[c + 1]; ++t) gtiles[t] = g;
        }
    }
    PTX_TRY(wm.build(ctx, db));
    // one device block, zero-filled once: [len N u64][len_own N u64][bases_own N u64][n_own N u32]
    DevBuf<uint8_t> d_out;
    DevBuf<GrTile> d_gtiles;
    PTX_HIP(ctx, d_out.alloc((size_t)N * 28));
    PTX_TRY(zero_fill(ctx, d_out.p, (size_t)N * 28));
    PTX_TRY(upload(ctx, d_gtiles, gtiles.data(), gtiles.size()));
    unsigned long long *o64 = reinterpret_cast<unsigned long long *>(d_out.p);
    const CtOut out{reinterpret_cast<uint32_t *>(o64 + 3 * N), o64, o64 + N, o64 + 2 * N};
    {
        KTimer tm(ctx, "growth_accum_kernel");
        hipLaunchKernelGGL(growth_accum_kernel, dim3(grid_for(n_tiles, 4, ctx->n_cu * 16)), dim3(256), 0, ctx->stream, n_tiles, pl.d_tiles.p, pl.d_touts.p, d_gtiles.p,
                           db->d_path_nodes.p, db->d_node_len.p, db->d_bases.p, by_node ? (const unsigned long long *)db->d_node_haps.p : (const unsigned long long *)nullptr,
                           wm.d_mask.p, W, out);
    }
    PTX_HIP(ctx, hipGetLastError());
    PTX_TRY(download(ctx, (unsigned long long *)len_out, out.len, N));
    PTX_TRY(download(ctx, (unsigned long long *)len_own_out, out.cov, N));
    PTX_TRY(download(ctx, (unsigned long long *)bases_own_out, out.bases, N));
    PTX_TRY(download(ctx, n_own_out, out.n, N));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));   // host arrays are filled, the temporaries are released on return
    return 0;
}

}  // namespace ptx

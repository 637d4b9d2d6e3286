// stage_segments.hip -- absent and amplified segments along selected haplotypes (pantax_hip_strain_segments, the --strain-segments report): the maximal runs
// of consecutive steps of a walk that the sample does not cover (gap) or covers at peak_depth and more (peak), in path coordinates, from what the coverage
// pass leaves in HBM.  Not a stage of the reference.
//
// Contract: include/pantax_hip.h, DESIGN.md "Segments along a strain".  Integers only: the result does not depend on any order.
//
// The walks are cut into the tiles of the coverage track (cov_track_tile.hpp): a wave per tile, 16 consecutive positions per lane, no communication between
// workgroups.  A position outside the walk (before the first step of a walk that begins mid-tile, behind its last) is a position of class SG_DEAD with
// length 0: dead runs stand at a tile's ends only and are dropped like the runs of class 0, so nothing below treats a short tile specially.
//   segments_tile_kernel  (pass A) gathers {node_len, cov, bases}, forms the class of every step and writes one SegTileSum per tile: the tile's summed
//                         length; the run at its first step (lead) and the run at its last (trail) as pieces, since they may go on in the neighbouring
//                         tiles; over the runs that touch neither (interior): per class their number, summed and longest length, and how many have
//                         len >= min_len.
//   host                  segments_plan (segments_plan.hpp) scans the tile sums, stitches trail -> lead pieces over the tile borders and gives every kept
//                         run its output slot: per tile the slot of its first kept interior run.
//   segments_emit_kernel  (pass B) the same gathers and runs; the lane in which a kept interior run ends writes it at the tile's first slot plus the
//                         wave prefix of the lanes' counts.  The host writes the stitched border runs into their slots behind the download.
// Runs in a lane: the lane's LAST run (found backwards) goes into a segmented DPP scan over the lanes -- a lane opens a segment unless all its 16 positions
// have the class of its predecessor's last position -- so every lane knows what its FIRST run inherits from the lanes before it.  A forward pass then folds
// the 16 positions into runs on top of that and hands every run that ENDS in the lane (at a change of class inside it, or because the next lane begins with
// another class) to the kernel's sink with its full sums: one writer per run, no atomics, plain vector stores.
//
// Algorithmic bytes (P_sel selected path positions, N kept segments): 4 P_sel (node ids) + (4 + 4 + 8) P_sel (len, cov, bases) per pass, twice;
// 104 bytes per tile of summaries; 37 N out.
#include <algorithm>
#include "common.hpp"
#include "cov_track_tile.hpp"
#include "primitives.hpp"
#include "segments_plan.hpp"
#include "wave.hpp"

namespace ptx {

namespace {

constexpr uint32_t SG_DEAD = 3;   // class of a position outside the walk

struct SgTileB { uint64_t base, out0, step0, peak; };   // SegTilePlace of the tile and the peak_depth of its haplotype

// the sums of a run of positions
struct SgAcc { uint32_t n; unsigned long long len, bases; };

// inclusive sum over the lanes [seg, lane] (seg <= lane: the first lane of my segment); all 64 lanes active.  The steps of ct_seg_scan (stage_cov_track.hip):
// a lane takes a value only from a source lane of its own segment; lanes a row operation does not reach read zero.
__device__ __forceinline__ void sg_seg_scan(SgAcc &a, int lane, int seg) {
#define SG_MOVE(x, CTRL, RM, BC) ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)(x), CTRL, RM, 0xF, BC))
#define SG_STEP(CTRL, RM, BC, SRC)                                                                                                             \
    {                                                                                                                                          \
        const uint32_t tn = SG_MOVE(a.n, CTRL, RM, BC);                                                                                        \
        const unsigned long long tlen = ((unsigned long long)SG_MOVE((uint32_t)(a.len >> 32), CTRL, RM, BC) << 32) | SG_MOVE((uint32_t)a.len, CTRL, RM, BC);       \
        const unsigned long long tbas = ((unsigned long long)SG_MOVE((uint32_t)(a.bases >> 32), CTRL, RM, BC) << 32) | SG_MOVE((uint32_t)a.bases, CTRL, RM, BC);   \
        const bool take = (SRC) >= seg;                                                                                                        \
        a.n += take ? tn : 0u; a.len += take ? tlen : 0ull; a.bases += take ? tbas : 0ull;                                                     \
    }
    SG_STEP(0x111, 0xF, true, lane - 1)
    SG_STEP(0x112, 0xF, true, lane - 2)
    SG_STEP(0x114, 0xF, true, lane - 4)
    SG_STEP(0x118, 0xF, true, lane - 8)
    SG_STEP(0x142, 0xA, false, (lane & ~15) - 1)   // rows 1 and 3 <- lanes 15 and 47
    SG_STEP(0x143, 0xC, false, 31)                 // rows 2 and 3 <- lane 31
#undef SG_STEP
#undef SG_MOVE
}

// a lane's 16 positions, ready to be folded into runs
struct SgLane {
    uint32_t len[16];
    unsigned long long bs[16];
    uint32_t cls;                 // two bits per position
    uint32_t next_first;          // class of the next lane's first position (lane 63: none)
    SgAcc carry;                  // what the lane's first run inherits from the lanes before it
    unsigned long long o0;        // summed length of the tile's positions before the lane
    unsigned long long tile_sum;
};

__device__ __forceinline__ void sg_load(SgLane &s, const CtTile &tl, uint64_t peak, int lane, const uint32_t *__restrict__ path_nodes,
                                        const uint32_t *__restrict__ node_len, const uint32_t *__restrict__ cov, const unsigned long long *__restrict__ bases) {
    uint32_t v[16];
    const uint32_t live = ct_load_ids(path_nodes, (tl.p0 & ~(CT_TILE - 1)) + 16u * (uint32_t)lane, tl.p0, tl.p0 + tl.n, tl.node_base, v);
    const uint32_t peak32 = (uint32_t)peak;   // at most 2^31 (validated by the caller)
    unsigned long long lane_sum = 0ull;
    s.cls = 0u;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const bool on = (live >> j) & 1u;
        const uint32_t l = node_len[v[j]], c = cov[v[j]];
        const unsigned long long b = bases[v[j]];
        const uint32_t k = !on ? SG_DEAD : c == 0u ? SEG_GAP : ((peak32 != 0u) & (b >= (unsigned long long)peak32 * l)) ? SEG_PEAK : 0u;   // (one 32 x 32 -> 64 multiply)
        s.cls |= k << (2 * j);
        s.len[j] = on ? l : 0u; s.bs[j] = on ? b : 0ull;
        lane_sum += s.len[j];
    }
    const unsigned long long incl = ct_incl_scan64(lane_sum);
    s.o0 = incl - lane_sum;
    s.tile_sum = lane_get(incl, 63);
    // the lane's last run, backwards
    const uint32_t c_last = s.cls >> 30, c_first = s.cls & 3u;
    SgAcc tail{0u, 0ull, 0ull};
    bool same = true;
#pragma unroll
    for (int j = 15; j >= 0; --j) {
        same = same & (((s.cls >> (2 * j)) & 3u) == c_last);
        tail.n += same ? 1u : 0u; tail.len += same ? s.len[j] : 0u; tail.bases += same ? s.bs[j] : 0ull;
    }
    const bool joins = c_first == wave_shr1(c_last, 0xFFu);   // my first run is the continuation of my predecessor's last (never in lane 0)
    const bool head = !(same & joins);                        // ... and unless it is my only one, my last run begins a segment
    const unsigned long long heads = __builtin_amdgcn_ballot_w64(head);
    const int seg = 63 - __builtin_clzll(heads & (~0ull >> (63 - lane)));   // (bit 0 is always set)
    sg_seg_scan(tail, lane, seg);
    s.carry.n = wave_shr1(tail.n);
    s.carry.len = ((unsigned long long)wave_shr1((uint32_t)(tail.len >> 32)) << 32) | wave_shr1((uint32_t)tail.len);
    s.carry.bases = ((unsigned long long)wave_shr1((uint32_t)(tail.bases >> 32)) << 32) | wave_shr1((uint32_t)tail.bases);
    if (!joins) s.carry = SgAcc{0u, 0ull, 0ull};
    s.next_first = wave_shl1(c_first, 0xFFu);
}

// every run that ends in the lane, in ascending position: sink(class, sums, tile position of its last step, summed length of the tile up to its end).
// Dead positions count in n, so a run's first tile position is end + 1 - n whatever its class.  No cross-lane operation in here.
template <class Sink>
__device__ __forceinline__ void sg_fold(const SgLane &s, int lane, Sink &&sink) {
    SgAcc acc = s.carry;
    unsigned long long o = s.o0;
    uint32_t cur = s.cls & 3u;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const uint32_t c = (s.cls >> (2 * j)) & 3u;
        if (j > 0 && c != cur) {
            sink(cur, acc, 16u * (uint32_t)lane + (uint32_t)j - 1u, o);
            acc = SgAcc{0u, 0ull, 0ull};
            cur = c;
        }
        acc.n += 1u; acc.len += s.len[j]; acc.bases += s.bs[j];
        o += s.len[j];
    }
    if (cur != s.next_first) sink(cur, acc, 16u * (uint32_t)lane + 15u, o);
}

__global__ void __launch_bounds__(256) segments_tile_kernel(uint32_t n_tiles, const CtTile *__restrict__ tiles, const unsigned long long *__restrict__ tile_peak,
                                                            const uint32_t *__restrict__ path_nodes, const uint32_t *__restrict__ node_len,
                                                            const uint32_t *__restrict__ cov, const unsigned long long *__restrict__ bases, uint64_t min_len,
                                                            SegTileSum *__restrict__ sums) {
    const int lane = threadIdx.x & 63;
    for (uint32_t t = blockIdx.x * 4 + (threadIdx.x >> 6); t < n_tiles; t += gridDim.x * 4) {
        const CtTile tl = tiles[t];
        SgLane s;
        sg_load(s, tl, tile_peak[t], lane, path_nodes, node_len, cov, bases);
        const uint32_t first_pos = (uint32_t)(tl.p0 & (CT_TILE - 1)), last_pos = first_pos + tl.n - 1u;
        SegTileSum *out = sums + t;
        // interior runs of the lane: n_gap | n_peak << 16 | n_keep << 32 (at most 512 runs a tile), summed and longest length per class
        unsigned long long cnt = 0ull, len_gap = 0ull, len_peak = 0ull, max_gap = 0ull, max_peak = 0ull;
        sg_fold(s, lane, [&](uint32_t c, const SgAcc &r, uint32_t end, unsigned long long) {
            if (c == SG_DEAD) return;
            const bool lead = end + 1u - r.n == first_pos, trail = end == last_pos;
            const SegPiece piece{r.len, r.bases, r.n, c};
            if (lead) { out->lead = piece; out->whole = trail ? 1u : 0u; }
            if (trail) out->trail = piece;
            if (!lead & !trail & (c != 0u)) {
                const bool gap = c == SEG_GAP;
                cnt += (gap ? 1ull : 1ull << 16) + (r.len >= min_len ? 1ull << 32 : 0ull);
                len_gap += gap ? r.len : 0ull; len_peak += gap ? 0ull : r.len;
                max_gap = gap && r.len > max_gap ? r.len : max_gap; max_peak = !gap && r.len > max_peak ? r.len : max_peak;
            }
        });
        const auto add = [](unsigned long long a, unsigned long long b) { return a + b; };
        const auto mx = [](unsigned long long a, unsigned long long b) { return a > b ? a : b; };
        cnt = wave_reduce(cnt, add); len_gap = wave_reduce(len_gap, add); len_peak = wave_reduce(len_peak, add);
        max_gap = wave_reduce(max_gap, mx); max_peak = wave_reduce(max_peak, mx);
        if (lane == 0) {
            out->sum_len = s.tile_sum;
            out->n_keep = (uint32_t)(cnt >> 32);
            out->n[0] = (uint32_t)(cnt & 0xFFFFu); out->n[1] = (uint32_t)((cnt >> 16) & 0xFFFFu);
            out->len[0] = len_gap; out->len[1] = len_peak; out->max[0] = max_gap; out->max[1] = max_peak;
        }
    }
}

struct SgOut { uint8_t *cls; uint32_t *n_steps; unsigned long long *step, *start, *len, *bases; uint64_t n; };

__global__ void __launch_bounds__(256) segments_emit_kernel(uint32_t n_tiles, const CtTile *__restrict__ tiles, const SgTileB *__restrict__ place,
                                                            const uint32_t *__restrict__ path_nodes, const uint32_t *__restrict__ node_len,
                                                            const uint32_t *__restrict__ cov, const unsigned long long *__restrict__ bases, uint64_t min_len, SgOut out) {
    const int lane = threadIdx.x & 63;
    for (uint32_t t = blockIdx.x * 4 + (threadIdx.x >> 6); t < n_tiles; t += gridDim.x * 4) {
        const CtTile tl = tiles[t];
        const SgTileB tb = place[t];
        SgLane s;
        sg_load(s, tl, tb.peak, lane, path_nodes, node_len, cov, bases);
        const uint32_t first_pos = (uint32_t)(tl.p0 & (CT_TILE - 1)), last_pos = first_pos + tl.n - 1u;
        const auto kept = [&](uint32_t c, const SgAcc &r, uint32_t end) {
            return ((c == SEG_GAP) | (c == SEG_PEAK)) & (end + 1u - r.n != first_pos) & (end != last_pos) & (r.len >= min_len);
        };
        uint32_t mine = 0u;
        sg_fold(s, lane, [&](uint32_t c, const SgAcc &r, uint32_t end, unsigned long long) { mine += kept(c, r, end) ? 1u : 0u; });
        uint64_t slot = tb.out0 + (wave_incl_scan_dpp(mine) - mine);
        sg_fold(s, lane, [&](uint32_t c, const SgAcc &r, uint32_t end, unsigned long long o_end) {
            if (!kept(c, r, end)) return;
            if (slot < out.n) {   // (always: the plan counted the same runs)
                out.cls[slot] = (uint8_t)c;
                out.n_steps[slot] = r.n;
                out.step[slot] = tb.step0 + (end + 1u - r.n - first_pos);
                out.start[slot] = tb.base + o_end - r.len;
                out.len[slot] = r.len;
                out.bases[slot] = r.bases;
            }
            ++slot;
        });
    }
}

}  // namespace

// sel_off [S+1], sel_hap, peak_depth and min_len validated by the caller.  seg_off_out [C+1] and the four summaries are always written; more than `cap`
// segments: PANTAX_HIP_E_LIMIT and the six segment arrays are not touched.
int segments_launch(Ctx *ctx, Db *db, const uint64_t *sel_off, const uint32_t *sel_hap, const uint64_t *peak_depth, uint64_t min_len, uint64_t *seg_off_out,
                    uint64_t cap, uint64_t *hap_len_out, uint64_t *n_runs_out, uint64_t *run_len_out, uint64_t *run_max_out, uint8_t *seg_class_out,
                    uint64_t *seg_step_out, uint32_t *seg_n_steps_out, uint64_t *seg_start_out, uint64_t *seg_len_out, uint64_t *seg_bases_out) {
    const uint32_t S = db->S;
    const uint64_t C = sel_off[S];
    std::vector<CtTile> tiles;
    std::vector<unsigned long long> peak;
    std::vector<uint32_t> steps;
    std::vector<uint64_t> tile_first(C + 1, 0);   // first tile of every selected haplotype
    for (uint32_t s = 0; s < S; ++s)
        for (uint64_t c = sel_off[s]; c < sel_off[s + 1]; ++c) {
            const uint64_t h = db->h_hap_off[s] + sel_hap[c], p1 = db->h_path_off[h + 1];
            for (uint64_t p = db->h_path_off[h]; p < p1;) {
                const uint64_t e = std::min(p1, (p & ~(CT_TILE - 1)) + CT_TILE);
                tiles.push_back(CtTile{p, (uint32_t)(e - p), (uint32_t)db->h_node_off[s]});
                peak.push_back(peak_depth[c]);
                steps.push_back((uint32_t)(e - p));
                p = e;
            }
            tile_first[c + 1] = tiles.size();
        }
    if (tiles.size() >= 0xFFFFFFFFull) return fail(ctx, PANTAX_HIP_E_LIMIT, "strain_segments: %llu tiles of selected walks exceed 32-bit positions", (unsigned long long)tiles.size());
    const uint32_t n_tiles = (uint32_t)tiles.size();
    DevBuf<CtTile> d_tiles;
    DevBuf<unsigned long long> d_peak;
    DevBuf<SegTileSum> d_sums;
    std::vector<SegTileSum> sums(n_tiles);
    if (n_tiles) {
        PTX_TRY(upload(ctx, d_tiles, tiles.data(), tiles.size()));
        PTX_TRY(upload(ctx, d_peak, peak.data(), peak.size()));
        PTX_HIP(ctx, d_sums.alloc(n_tiles));
        {
            KTimer tm(ctx, "segments_tile_kernel");
            hipLaunchKernelGGL(segments_tile_kernel, dim3(grid_for(n_tiles, 4, ctx->n_cu * 16)), dim3(256), 0, ctx->stream, n_tiles, d_tiles.p, d_peak.p,
                               db->d_path_nodes.p, db->d_node_len.p, db->d_cov.p, db->d_bases.p, min_len, d_sums.p);
        }
        PTX_HIP(ctx, hipGetLastError());
        PTX_TRY(download(ctx, sums.data(), d_sums.p, n_tiles));
        PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    SegPlan plan;
    segments_plan(C, tile_first.data(), steps.data(), sums.data(), min_len, seg_off_out, hap_len_out, n_runs_out, run_len_out, run_max_out, plan);
    const uint64_t N = seg_off_out[C];
    if (N > cap) return fail(ctx, PANTAX_HIP_E_LIMIT, "strain_segments: the selection has %llu segments, the output arrays hold %llu (seg_off_out is filled: size the arrays by it)",
                             (unsigned long long)N, (unsigned long long)cap);
    if (N == 0) return 0;
    if (!seg_class_out || !seg_step_out || !seg_n_steps_out || !seg_start_out || !seg_len_out || !seg_bases_out) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_segments: null output array");
    if (N > (~(size_t)0) / 64) return fail(ctx, PANTAX_HIP_E_LIMIT, "strain_segments: %llu segments", (unsigned long long)N);
    if (N > plan.border.size()) {   // some tile has a kept interior run.  One device block: [step N u64][start N u64][len N u64][bases N u64][n_steps N u32][class N u8]
        std::vector<SgTileB> place(n_tiles);
        for (uint32_t t = 0; t < n_tiles; ++t) place[t] = SgTileB{plan.place[t].base, plan.place[t].out0, plan.place[t].step0, peak[t]};
        DevBuf<uint8_t> d_out;
        DevBuf<SgTileB> d_place;
        PTX_HIP(ctx, d_out.alloc((size_t)N * 37));
        PTX_TRY(upload(ctx, d_place, place.data(), place.size()));
        unsigned long long *o64 = reinterpret_cast<unsigned long long *>(d_out.p);
        uint32_t *o32 = reinterpret_cast<uint32_t *>(o64 + 4 * N);
        const SgOut out{reinterpret_cast<uint8_t *>(o32 + N), o32, o64, o64 + N, o64 + 2 * N, o64 + 3 * N, N};
        {
            KTimer tm(ctx, "segments_emit_kernel");
            hipLaunchKernelGGL(segments_emit_kernel, dim3(grid_for(n_tiles, 4, ctx->n_cu * 16)), dim3(256), 0, ctx->stream, n_tiles, d_tiles.p, d_place.p,
                               db->d_path_nodes.p, db->d_node_len.p, db->d_cov.p, db->d_bases.p, min_len, out);
        }
        PTX_HIP(ctx, hipGetLastError());
        PTX_TRY(download(ctx, (unsigned long long *)seg_step_out, out.step, N));
        PTX_TRY(download(ctx, (unsigned long long *)seg_start_out, out.start, N));
        PTX_TRY(download(ctx, (unsigned long long *)seg_len_out, out.len, N));
        PTX_TRY(download(ctx, (unsigned long long *)seg_bases_out, out.bases, N));
        PTX_TRY(download(ctx, seg_n_steps_out, out.n_steps, N));
        PTX_TRY(download(ctx, seg_class_out, out.cls, N));
        PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));   // host arrays are filled, the temporaries are released on return
    }
    for (const SegBorder &b : plan.border) {   // the runs that touch a tile border, into the slots the plan kept for them
        seg_class_out[b.slot] = b.cls; seg_step_out[b.slot] = b.step; seg_n_steps_out[b.slot] = b.n_steps;
        seg_start_out[b.slot] = b.start; seg_len_out[b.slot] = b.len; seg_bases_out[b.slot] = b.bases;
    }
    return 0;
}

}  // namespace ptx

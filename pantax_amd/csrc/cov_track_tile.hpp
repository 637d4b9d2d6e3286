// cov_track_tile.hpp -- what the passes along selected walks share (stage_cov_track.hip, stage_segments.hip, stage_growth.hip; device code only): a selected walk is cut
// into tiles at the multiples of CT_TILE global path positions (so a lane's quads of node ids are 16-byte aligned); a wave per tile, 16 consecutive
// positions per lane.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace ptx {

constexpr uint64_t CT_TILE = 1024;   // path positions per tile: 64 lanes x 16

struct CtTile { uint64_t p0; uint32_t n, node_base; };        // global path positions [p0, p0 + n), inside one aligned block of CT_TILE; first global node of the species

// the global node indices of the lane's 16 positions q0 .. q0 + 15 (q0 a multiple of 16); bit j of the result: position j lies in [lo, hi).
// A dead position names the node of position `lo`: every gather below stays inside its array, its value is dropped by a select.
__device__ __forceinline__ uint32_t ct_load_ids(const uint32_t *__restrict__ path_nodes, uint64_t q0, uint64_t lo, uint64_t hi, uint32_t node_base, uint32_t (&v)[16]) {
    uint32_t live = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint64_t q = q0 + 4u * k;
        if ((q >= lo) & (q + 4 <= hi)) {   // a quad inside the tile: one 16-byte load (false only in the first and last lane of a walk)
            const uint4 x = *reinterpret_cast<const uint4 *>(path_nodes + q);
            v[4 * k] = x.x; v[4 * k + 1] = x.y; v[4 * k + 2] = x.z; v[4 * k + 3] = x.w;
            live |= 0xFu << (4 * k);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint64_t pos = q + e;
                const bool in = (pos >= lo) & (pos < hi);
                v[4 * k + e] = path_nodes[in ? pos : lo];
                live |= (in ? 1u : 0u) << (4 * k + e);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] += node_base;
    return live;
}

// inclusive prefix sum of a 64-bit value over the 64 lanes (the steps of wave_incl_scan_dpp, wave.hpp, on both halves)
__device__ __forceinline__ unsigned long long ct_incl_scan64(unsigned long long v) {
#define CT_STEP(CTRL, RM, BC)                                                                                        \
    {                                                                                                                \
        const uint32_t tl = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, RM, 0xF, BC);           \
        const uint32_t th = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, RM, 0xF, BC);   \
        v += ((unsigned long long)th << 32) | tl;                                                                    \
    }
    CT_STEP(0x111, 0xF, true) CT_STEP(0x112, 0xF, true) CT_STEP(0x114, 0xF, true) CT_STEP(0x118, 0xF, true)
    CT_STEP(0x142, 0xA, false) CT_STEP(0x143, 0xC, false)
#undef CT_STEP
    return v;
}

// ---- the windowed sums of stage_cov_track.hip and stage_growth.hip: four sums per window, a run of steps of one window at a time ----
struct CtTileOut { uint64_t base, out0, n_win; };             // o of position p0; first output window of the haplotype; its number of windows

// the four sums of a run of steps of one window
struct CtAcc { uint32_t n; unsigned long long len, cov, bases; };

// inclusive sum over the lanes [seg, lane] (seg <= lane: the first lane of my segment); all 64 lanes active.  The steps of seg_and (stage_read_strain.hip):
// a lane takes a value only from a source lane of its own segment; lanes a row operation does not reach read zero.
__device__ __forceinline__ void ct_seg_scan(CtAcc &a, int lane, int seg) {
#define CT_MOVE(x, CTRL, RM, BC) ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)(x), CTRL, RM, 0xF, BC))
#define CT_STEP(CTRL, RM, BC, SRC)                                                                                                             \
    {                                                                                                                                          \
        const uint32_t tn = CT_MOVE(a.n, CTRL, RM, BC);                                                                                        \
        const unsigned long long tlen = ((unsigned long long)CT_MOVE((uint32_t)(a.len >> 32), CTRL, RM, BC) << 32) | CT_MOVE((uint32_t)a.len, CTRL, RM, BC);       \
        const unsigned long long tcov = ((unsigned long long)CT_MOVE((uint32_t)(a.cov >> 32), CTRL, RM, BC) << 32) | CT_MOVE((uint32_t)a.cov, CTRL, RM, BC);       \
        const unsigned long long tbas = ((unsigned long long)CT_MOVE((uint32_t)(a.bases >> 32), CTRL, RM, BC) << 32) | CT_MOVE((uint32_t)a.bases, CTRL, RM, BC);   \
        const bool take = (SRC) >= seg;                                                                                                        \
        a.n += take ? tn : 0u; a.len += take ? tlen : 0ull; a.cov += take ? tcov : 0ull; a.bases += take ? tbas : 0ull;                        \
    }
    CT_STEP(0x111, 0xF, true, lane - 1)
    CT_STEP(0x112, 0xF, true, lane - 2)
    CT_STEP(0x114, 0xF, true, lane - 4)
    CT_STEP(0x118, 0xF, true, lane - 8)
    CT_STEP(0x142, 0xA, false, (lane & ~15) - 1)   // rows 1 and 3 <- lanes 15 and 47
    CT_STEP(0x143, 0xC, false, 31)                 // rows 2 and 3 <- lane 31
#undef CT_STEP
#undef CT_MOVE
}

struct CtOut { uint32_t *n; unsigned long long *len, *cov, *bases; };

// window w of the haplotype whose windows start at out0; guarded by the haplotype's window count (a live step always lies below it: node lengths are > 0)
__device__ __forceinline__ void ct_add(const CtOut &o, uint64_t out0, uint64_t n_win, bool on, uint64_t w, const CtAcc &a) {
    if (on & (w < n_win)) {
        const uint64_t i = out0 + w;
        atomicAdd(o.n + i, a.n); atomicAdd(o.len + i, a.len); atomicAdd(o.cov + i, a.cov); atomicAdd(o.bases + i, a.bases);
    }
}

}  // namespace ptx

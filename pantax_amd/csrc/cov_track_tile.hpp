// cov_track_tile.hpp -- what the passes along selected walks share (stage_cov_track.hip, stage_segments.hip; device code only): a selected walk is cut
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

}  // namespace ptx

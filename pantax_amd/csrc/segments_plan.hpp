// segments_plan.hpp -- the host side of pantax_hip_strain_segments (stage_segments.hip) as pure functions of plain values: what a wave reports about its
// tile of a walk (SegTileSum), how the tiles of a haplotype are stitched into runs that cross tile borders, where every kept run goes in the output, and the
// host helper that chains kept segments (pantax_hip_segment_chain).  Standard headers only: tests/native/segments_check.cpp compiles this with the host
// compiler alone.
//
// A run is a maximal stretch of consecutive steps of one walk with one class (0 = neither, SEG_GAP, SEG_PEAK).  Inside a tile the device knows every run
// that touches neither the tile's first nor its last step (the interior runs) in full; the run at the first step (lead) and the run at the last (trail) may
// go on in the neighbouring tiles and come to the host as pieces.
#pragma once
#include <cstdint>
#include <vector>

namespace ptx {

constexpr uint32_t SEG_GAP = 1, SEG_PEAK = 2;
constexpr uint64_t SEG_PEAK_DEPTH_MAX = 1ull << 31;   // peak_depth * node_len stays below 2^63

struct SegPiece { uint64_t len, bases; uint32_t n_steps, cls; };
// one tile of a walk, written by the wave that owns it (every field has one writer)
struct SegTileSum {
    uint64_t sum_len;        // the summed node length of the tile's steps
    SegPiece lead, trail;    // the run at the tile's first step, the run at its last; whole != 0: the tile is one run, lead == trail
    uint32_t whole;
    uint32_t n_keep;         // interior runs of class gap or peak with len >= min_len
    uint32_t n[2];           // interior runs per class (gap, peak), ...
    uint64_t len[2], max[2]; // ... their summed length, the longest
};

struct SegTilePlace { uint64_t base, out0, step0; };   // o of the tile's first step; output slot of its first kept interior run; walk-local index of its first step
// a kept run that touches a tile border: the host writes it into its slot behind the download
struct SegBorder { uint64_t slot, step, start, len, bases; uint32_t n_steps; uint8_t cls; };
struct SegPlan {
    std::vector<SegTilePlace> place;   // [n_tiles]
    std::vector<SegBorder> border;     // in ascending slot
};

// The tiles [tile_first[c], tile_first[c + 1]) of selected haplotype c in walk order, tile_steps[t] their steps (>= 1), sums[t] what the device reported.
// Writes hap_len [C], n_runs / run_len / run_max [2C] (gap, peak: over ALL runs), seg_off [C + 1] (the prefix of the runs with len >= min_len) and the plan.
// Within a haplotype the slots ascend with the runs' start: a run that began before a tile, the run that begins at the tile's first step, the tile's interior
// runs, the run that begins inside the tile and reaches its last step.
void segments_plan(uint64_t C, const uint64_t *tile_first, const uint32_t *tile_steps, const SegTileSum *sums, uint64_t min_len, uint64_t *seg_off,
                   uint64_t *hap_len, uint64_t *n_runs, uint64_t *run_len, uint64_t *run_max, SegPlan &plan);

}  // namespace ptx

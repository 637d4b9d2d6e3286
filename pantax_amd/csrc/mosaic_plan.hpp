// mosaic_plan.hpp -- the host side of pantax_hip_strain_mosaic (stage_mosaic.hip) as pure functions of plain values: the greedy cut of one walk
// (pantax_hip_mosaic_walk, the C statement of the contract), the junctions a report prints (pantax_hip_mosaic_top), and the sort and run-length that turn
// the break records of the device into distinct junctions with their counts.  Standard headers only: tests/native/mosaic_check.cpp compiles this with the
// host compiler alone.
#pragma once
#include <cstdint>
#include <vector>

namespace ptx {

constexpr uint32_t MOSAIC_MAX_K = 64;   // candidates of a species the cut serves: a candidate word is one u64
// the species classes of pantax_hip_strain_mosaic, in the order of species_out
enum MosaicClass { MOS_COUNTED, MOS_COMPATIBLE, MOS_MOSAIC1, MOS_MOSAIC2, MOS_MOSAIC3PLUS, MOS_FOREIGN, MOS_N_CLASSES };
// the class of a cut read of k >= 1 segments
constexpr uint32_t mosaic_class_of(uint64_t k) { return k <= 1 ? MOS_COMPATIBLE : k == 2 ? MOS_MOSAIC1 : k == 3 ? MOS_MOSAIC2 : MOS_MOSAIC3PLUS; }

// one break as the device records it: the species, the last step of the left segment, the first step of the right one (species-local node indices)
struct MosaicBreak { uint32_t species, node_a, node_b; };
inline bool operator<(const MosaicBreak &x, const MosaicBreak &y) {
    return x.species != y.species ? x.species < y.species : x.node_a != y.node_a ? x.node_a < y.node_a : x.node_b < y.node_b;
}
inline bool operator==(const MosaicBreak &x, const MosaicBreak &y) { return x.species == y.species && x.node_a == y.node_a && x.node_b == y.node_b; }
// sorts the records in place (ascending species, node_a, node_b) and run-lengths them: distinct[i] occurs count[i] times
void mosaic_junctions(std::vector<MosaicBreak> &recs, std::vector<MosaicBreak> &distinct, std::vector<uint64_t> &count);

}  // namespace ptx

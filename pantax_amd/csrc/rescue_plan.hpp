// rescue_plan.hpp -- the host side of pantax_hip_strain_read_rescue (stage_rescue.hip) as pure functions of plain values: the classes of one walk
// (pantax_hip_rescue_walk, the C statement of the contract), the order in which a species' candidates are printed (pantax_hip_rescue_rank), and the
// candidate list the file seam hands the stage call.  pantax_hip.h and standard headers only: tests/native/rescue_check.cpp compiles this with the host
// compiler alone.
#pragma once
#include <cstdint>
#include <vector>

namespace ptx {

constexpr uint32_t RESCUE_MAX_LIST = 64;   // K_s + J_s of an open species: the word over Sel ++ Cand is one u64
// the species classes of pantax_hip_strain_read_rescue, in the order of species_out
enum RescueClass {
    RES_COUNTED, RES_COMPATIBLE, RES_FOREIGN, RES_FOREIGN_RESCUED, RES_FOREIGN_PATCHWORK, RES_FOREIGN_NOVEL, RES_MOSAIC, RES_MOSAIC_RESCUED, RES_CONTESTED,
    RES_N_CLASSES
};
// the sums of a candidate entry, in the order of cand_out
enum RescueCand { RES_RESCUED, RES_ALONE, RES_FROM_FOREIGN, RES_N_CAND };

// The seam's candidates of one species with K reported rows: `ranked` (positions into the species' n_cand near-miss candidates, the order of
// pantax_hip_near_miss_rank with top = 0) first, then the remaining positions in ascending haplotype index (cand_hap [n_cand], no repeats), cut to
// 64 - K; K >= 64 gives none.  -> positions into the species' candidates
std::vector<uint32_t> rescue_candidates(uint64_t K, uint32_t n_cand, const uint32_t *cand_hap, const uint32_t *ranked, uint32_t n_ranked);

}  // namespace ptx

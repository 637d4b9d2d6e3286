// links_plan.hpp -- the host side of pantax_hip_strain_links (stage_links.hip) as pure functions of plain values: the classes of one walk's crossings
// (pantax_hip_link_crossings, the C statement of the contract) and the order in which a strain's breaks are printed (pantax_hip_link_top).  pantax_hip.h
// and standard headers only: tests/native/links_check.cpp compiles this with the host compiler alone.
#pragma once
#include <cstdint>

namespace ptx {

constexpr uint32_t LINKS_MAX_LIST = 64;   // K_s of an open species: a link mask is one u64
// the species counters of pantax_hip_strain_links, in the order of species_out
enum LinkSpecies { LNK_COUNTED, LNK_CROSSINGS, LNK_KNOWN, LNK_SKIP, LNK_SWITCH, LNK_FOREIGN, LNK_N_SPECIES };
// the link counters of a species, in the order of link_out
enum LinkTable { LNK_DISTINCT, LNK_DISTINCT_CROSSED, LNK_CORE, LNK_CORE_CROSSED, LNK_N_TABLE };
// the counters of a selection entry, in the order of hap_out
enum LinkHap { LNK_LINKS, LNK_CROSSED, LNK_OPEN, LNK_BROKEN, LNK_PRIVATE, LNK_PRIVATE_CROSSED, LNK_PRIVATE_BROKEN, LNK_SUPPORT, LNK_N_HAP };

// the class of a crossing that is no link of a member, from the membership words of its two steps: LNK_SKIP, LNK_SWITCH or LNK_FOREIGN
constexpr int link_unknown_class(unsigned long long ma, unsigned long long mb) {
    return (ma == 0ull || mb == 0ull) ? LNK_FOREIGN : (ma & mb) ? LNK_SKIP : LNK_SWITCH;
}

}  // namespace ptx

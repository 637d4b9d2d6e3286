// rarefy_plan.cpp -- the host helpers of the contract of pantax_hip_strain_rarefy (rarefy_plan.hpp, rarefy_depth.hpp).  Nothing here touches the device.
#include "rarefy_plan.hpp"
#include <algorithm>
#include "../../include/pantax_hip.h"
#include "rarefy_depth.hpp"

namespace ptx {

bool rarefy_plan(uint32_t n_levels, uint64_t arrays_fit, uint64_t levels_max, RarefyPlan &plan, std::string &why) {
    plan = RarefyPlan{};
    if (n_levels == 0 || n_levels > RAREFY_MAX_LEVELS) {
        why = "strain_rarefy: " + std::to_string(n_levels) + " levels (1 .. " + std::to_string(RAREFY_MAX_LEVELS) + ")";
        return false;
    }
    uint64_t per = std::min<uint64_t>(n_levels, arrays_fit);
    if (levels_max) per = std::min(per, levels_max);
    if (per == 0) {
        why = "strain_rarefy: the free device memory does not hold one level array (a u64 per node)";
        return false;
    }
    plan.per_pass = (uint32_t)per;
    plan.n_passes = (n_levels + plan.per_pass - 1u) / plan.per_pass;
    return true;
}

}  // namespace ptx

extern "C" uint32_t pantax_hip_rarefy_depth(uint64_t seed, uint32_t replicate, uint64_t read) {
    return ptx::rarefy_depth_hashed(ptx::rarefy_replicate_hash(seed, replicate), read);
}

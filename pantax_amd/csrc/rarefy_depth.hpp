// rarefy_depth.hpp -- the thinning rule of the rarefaction of the strain fit (pantax_hip_strain_rarefy; include/pantax_hip.h "Rarefaction of the strain
// fit"), the ONE definition rarefy_depth_kernel (stage_rarefy.hip) and the host helper pantax_hip_rarefy_depth (rarefy_plan.cpp) both compile, as
// bootstrap_weight.hpp is.  Plain integer arithmetic: the same bits on either side.  Standard headers only.
#pragma once
#include <cstdint>
#include "bootstrap_weight.hpp"

namespace ptx {

constexpr uint32_t RAREFY_DEPTH_MAX = 63;   // the deepest level a read can belong to
// the part of the hash that is the same for every read of a replicate: sm(seed ^ sm(b))
PTX_BOOT_HD inline uint64_t rarefy_replicate_hash(uint64_t seed, uint64_t b) { return boot_sm(seed ^ boot_sm(b)); }
// depth of read r (its index in the uploaded columns) from the replicate's hash: the leading zero bits of sm(hash + r), 63 at the most.  The read belongs
// to level l iff depth >= l: level 0 is every read, level l keeps a read with probability 2^-l, the levels of a replicate are nested
PTX_BOOT_HD inline uint32_t rarefy_depth_hashed(uint64_t replicate_hash, uint64_t r) {
    const uint64_t h = boot_sm(replicate_hash + r);
    if (h == 0) return RAREFY_DEPTH_MAX;
    const uint32_t z = (uint32_t)__builtin_clzll((unsigned long long)h);
    return z < RAREFY_DEPTH_MAX ? z : RAREFY_DEPTH_MAX;
}

}  // namespace ptx

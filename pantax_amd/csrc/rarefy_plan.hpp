// rarefy_plan.hpp -- the host side of pantax_hip_strain_rarefy (stage_rarefy.hip) as pure functions of plain values: how many of a replicate's levels
// one pass over the reads serves (each level is an array of V u64 on the device), and the entry of a (replicate, level).  pantax_hip.h and standard headers
// only: tests/native/rarefy_check.cpp compiles this with the host compiler alone.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

namespace ptx {

constexpr uint32_t RAREFY_MAX_LEVELS = 16;   // n_levels of a call: the thinned levels 1 .. n_levels

// The level arrays the device holds when the option rarefy_levels_max is 0: a quarter of what is free when the call begins (the refit's rows, sort buffers
// and solver scratch are allocated beside them), in arrays of V u64
inline uint64_t rarefy_default_arrays(size_t free_bytes, uint64_t V) { return V ? (uint64_t)(free_bytes / 4) / (V * 8ull) : RAREFY_MAX_LEVELS; }

struct RarefyPlan {
    uint32_t per_pass = 0;   // levels a pass serves (the last pass of a replicate: the rest)
    uint32_t n_passes = 0;   // passes per replicate
};
// n_levels in 1 .. RAREFY_MAX_LEVELS; arrays_fit = level arrays the memory holds; levels_max = the option (0: from memory).  false: not one array fits
bool rarefy_plan(uint32_t n_levels, uint64_t arrays_fit, uint64_t levels_max, RarefyPlan &plan, std::string &why);
// the levels [l0, l1) of pass i of a replicate (levels count from 1)
inline void rarefy_pass_levels(const RarefyPlan &plan, uint32_t n_levels, uint32_t i, uint32_t &l0, uint32_t &l1) {
    l0 = 1u + i * plan.per_pass;
    l1 = l0 + plan.per_pass < n_levels + 1u ? l0 + plan.per_pass : n_levels + 1u;
}
// entry of level l >= 1 of replicate b >= 1; entry 0 is the full sample
inline uint64_t rarefy_entry(uint32_t n_levels, uint32_t b, uint32_t l) { return 1ull + (uint64_t)(b - 1u) * n_levels + (l - 1u); }

}  // namespace ptx

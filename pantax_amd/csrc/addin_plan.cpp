// addin_plan.cpp -- the host decisions of pantax_hip_strain_addin and the host helper of its contract (addin_plan.hpp).  Nothing here touches the device.
#include "addin_plan.hpp"
#include <algorithm>
#include <cmath>
#include "../../include/pantax_hip.h"

#if defined(__clang__)
#pragma clang fp contract(off)   // the helper's differences and sums are plain IEEE operations
#endif

namespace ptx {

bool addin_x_offsets(uint64_t S, const uint64_t *sel_off, const uint64_t *cand_off, uint64_t *x_off) {
    typedef unsigned __int128 u128;
    u128 t = 0;
    x_off[0] = 0;
    for (uint64_t s = 0; s < S; ++s) {
        const u128 K = sel_off[s + 1] - sel_off[s], J = cand_off[s + 1] - cand_off[s];
        if (K + J > (u128)~0ull || J + 1 > (u128)~0ull) return false;
        t += (J + 1) * (K + J);   // both factors below 2^64, t below 2^64: no u128 overflow
        if (t > (u128)~0ull) return false;
        x_off[s + 1] = (uint64_t)t;
    }
    return true;
}

uint64_t addin_default_cap(uint64_t free_bytes) { return std::min<uint64_t>(free_bytes / 4 / ADDIN_BYTES_PER_PATTERN, ADDIN_PATTERNS_HARD_MAX); }

bool addin_plan(uint64_t P, uint64_t S, uint64_t rounds, uint64_t cap, AddinPlan &plan, std::string &err) {
    plan = AddinPlan();
    if (rounds == 0 || rounds > 65) { err = "strain_addin: " + std::to_string((unsigned long long)rounds) + " rounds (1 .. 65: the refit and one per candidate)"; return false; }
    cap = std::min(cap, ADDIN_PATTERNS_HARD_MAX);
    if (P == 0) { plan.per_chunk = (uint32_t)rounds; plan.n_chunks = 1; return true; }
    if (P >= ADDIN_PATTERNS_HARD_MAX || P + 1 > cap || S >= ADDIN_PATTERNS_HARD_MAX) {
        err = "strain_addin: one round of " + std::to_string((unsigned long long)P) + " patterns and " + std::to_string((unsigned long long)S) +
              " species needs " + (P == ~0ull ? std::string("2^64") : std::to_string((unsigned long long)(P + 1))) + " replicated patterns, more than the " +
              std::to_string((unsigned long long)cap) + " in flight that addin_patterns_max (or the free device memory, or 32-bit pattern positions) allows";
        return false;
    }
    uint64_t per = std::min(rounds, cap / (P + 1));                                // >= 1: P + 1 <= cap
    per = std::min(per, std::max<uint64_t>(1, ADDIN_PATTERNS_HARD_MAX / (S + 1)));   // S + 1 <= the hard bound: the quotient is >= 1
    plan.per_chunk = (uint32_t)per;
    plan.n_chunks = (uint32_t)((rounds + per - 1) / per);
    plan.chunk_patterns = per * (P + 1);
    plan.chunk_entries = per * (S + 1);
    return true;
}

}  // namespace ptx

extern "C" {

int pantax_hip_addin_donor(uint32_t W, uint32_t K, const double *x_base, const double *x_add, double *out) {
    if (!out || K > W || !x_base || !x_add) return PANTAX_HIP_E_INVALID;
    double best = 0.0, shift = 0.0;
    int64_t arg = -1;
    for (uint32_t j = 0; j < K; ++j) {
        const double d = x_base[j] - x_add[j];
        if (d > best) { best = d; arg = (int64_t)j; }   // strictly larger: ties go to the lowest j, and a loss must be positive
        shift += std::fabs(x_add[j] - x_base[j]);
    }
    out[0] = (double)arg; out[1] = arg < 0 ? 0.0 : best; out[2] = shift;
    return 0;
}

}  // extern "C"

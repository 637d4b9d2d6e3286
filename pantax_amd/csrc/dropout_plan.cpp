// dropout_plan.cpp -- the host decisions of pantax_hip_strain_dropout and the host helper of its contract (dropout_plan.hpp).  Nothing here touches
// the device.
#include "dropout_plan.hpp"
#include <algorithm>
#include <cmath>
#include "../../include/pantax_hip.h"

#if defined(__clang__)
#pragma clang fp contract(off)   // the helper's differences and sums are plain IEEE operations
#endif

namespace ptx {

bool dropout_x_offsets(uint64_t S, const uint64_t *sel_off, uint64_t *x_off) {
    typedef unsigned __int128 u128;
    u128 t = 0;
    x_off[0] = 0;
    for (uint64_t s = 0; s < S; ++s) {
        const uint64_t K = sel_off[s + 1] - sel_off[s];
        t += ((u128)K + 1) * K;
        if (t > (u128)~0ull) return false;
        x_off[s + 1] = (uint64_t)t;
    }
    return true;
}

uint64_t dropout_default_cap(uint64_t free_bytes) { return std::min<uint64_t>(free_bytes / 4 / DROP_BYTES_PER_PATTERN, DROP_PATTERNS_HARD_MAX); }

bool dropout_plan(uint64_t P, uint64_t S, uint64_t rounds, uint64_t cap, DropoutPlan &plan, std::string &err) {
    plan = DropoutPlan();
    if (rounds == 0 || rounds > 65) { err = "strain_dropout: " + std::to_string((unsigned long long)rounds) + " rounds (1 .. 65: the refit and one per column)"; return false; }
    cap = std::min(cap, DROP_PATTERNS_HARD_MAX);
    if (P == 0) { plan.per_chunk = (uint32_t)rounds; plan.n_chunks = 1; return true; }
    if (P >= DROP_PATTERNS_HARD_MAX || P + 1 > cap || S >= DROP_PATTERNS_HARD_MAX) {
        err = "strain_dropout: one round of " + std::to_string((unsigned long long)P) + " patterns and " + std::to_string((unsigned long long)S) +
              " species needs " + (P == ~0ull ? std::string("2^64") : std::to_string((unsigned long long)(P + 1))) + " replicated patterns, more than the " +
              std::to_string((unsigned long long)cap) + " in flight that dropout_patterns_max (or the free device memory, or 32-bit pattern positions) allows";
        return false;
    }
    uint64_t per = std::min(rounds, cap / (P + 1));                               // >= 1: P + 1 <= cap
    per = std::min(per, std::max<uint64_t>(1, DROP_PATTERNS_HARD_MAX / (S + 1)));   // S + 1 <= the hard bound: the quotient is >= 1
    plan.per_chunk = (uint32_t)per;
    plan.n_chunks = (uint32_t)((rounds + per - 1) / per);
    plan.chunk_patterns = per * (P + 1);
    plan.chunk_entries = per * (S + 1);
    return true;
}

}  // namespace ptx

extern "C" {

int pantax_hip_dropout_substitute(uint32_t K, uint32_t k, const double *x_full, const double *x_drop, double *out) {
    if (!out || k >= K || !x_full || !x_drop) return PANTAX_HIP_E_INVALID;
    double best = 0.0, shift = 0.0;
    int64_t arg = -1;
    for (uint32_t j = 0; j < K; ++j) {
        if (j == k) continue;
        const double d = x_drop[j] - x_full[j];
        if (d > best) { best = d; arg = (int64_t)j; }   // strictly larger: ties go to the lowest j, and a gain must be positive
        shift += std::fabs(d);
    }
    out[0] = (double)arg; out[1] = arg < 0 ? 0.0 : best; out[2] = shift;
    return 0;
}

}  // extern "C"

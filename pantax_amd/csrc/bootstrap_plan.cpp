// bootstrap_plan.cpp -- the host decisions of pantax_hip_strain_bootstrap and the two host helpers of its contract (bootstrap_plan.hpp).  Nothing here
// touches the device.
#include "bootstrap_plan.hpp"
#include <algorithm>
#include <cmath>
#include <vector>
#include "../../include/pantax_hip.h"
#include "bootstrap_weight.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)   // the summary's sums are plain IEEE additions and multiplications, as the reference's
#endif

namespace ptx {

uint64_t bootstrap_rows_bound(uint64_t n_rows) {
    if (n_rows == 0) return 0;
    typedef unsigned __int128 u128;   // (r + 1)^2 passes 2^64 for n_rows near it
    uint64_t r = (uint64_t)std::sqrt((double)n_rows);   // integer ceil(sqrt(n_rows)) from the floating-point estimate
    while ((u128)r * r > n_rows) --r;
    while ((u128)(r + 1) * (r + 1) <= n_rows) ++r;
    if ((u128)r * r < n_rows) ++r;
    const u128 soft = (u128)n_rows + 8 * (u128)r + 64, hard = (u128)BOOT_W_MAX * n_rows, b = std::min(soft, hard);
    return b > (u128)~0ull ? ~0ull : (uint64_t)b;   // saturates: such a replicate fits no cap
}

uint64_t bootstrap_default_cap(uint64_t free_bytes) { return std::min<uint64_t>(free_bytes / 4 / BOOT_BYTES_PER_ROW, BOOT_ROWS_HARD_MAX); }

bool bootstrap_plan(uint64_t n_rows, uint64_t R, uint64_t cap, BootstrapPlan &plan, std::string &err) {
    plan = BootstrapPlan();
    if (R == 0 || R > 0xFFFFFFFFull) { err = "strain_bootstrap: " + std::to_string((unsigned long long)R) + " replicates (1 .. 2^32 - 1 with the refit)"; return false; }
    cap = std::min(cap, BOOT_ROWS_HARD_MAX);
    plan.bound = bootstrap_rows_bound(n_rows);
    if (n_rows == 0) { plan.per_chunk = (uint32_t)R; plan.n_chunks = 1; return true; }
    if (plan.bound > cap) {
        err = "strain_bootstrap: one replicate of " + std::to_string((unsigned long long)n_rows) + " rows is sized for " + std::to_string((unsigned long long)plan.bound) +
              " expanded rows, more than the " + std::to_string((unsigned long long)cap) + " in flight that bootstrap_rows_max (or the free device memory, or 32-bit row positions) allows";
        return false;
    }
    uint64_t per = std::min(R, cap / plan.bound);                    // >= 1: bound <= cap
    per = std::min(per, std::max<uint64_t>(1, BOOT_ROWS_HARD_MAX / n_rows));   // n_rows <= bound <= cap <= BOOT_ROWS_HARD_MAX: the quotient is >= 1
    plan.per_chunk = (uint32_t)per;
    plan.n_chunks = (uint32_t)((R + per - 1) / per);
    plan.chunk_rows = per * plan.bound;
    return true;
}

}  // namespace ptx

extern "C" {

uint32_t pantax_hip_bootstrap_weight(uint64_t seed, uint64_t sp_key, uint32_t replicate, uint64_t v_local) {
    return ptx::boot_weight_hashed(ptx::boot_species_hash(seed, sp_key), replicate, v_local);
}

int pantax_hip_bootstrap_summary(uint64_t n, const double *x, const int32_t *status, double *out) {
    if (!out || (n && !x)) return PANTAX_HIP_E_INVALID;
    for (int i = 0; i < 10; ++i) out[i] = 0.0;
    std::vector<double> v;
    v.reserve(n);
    for (uint64_t b = 0; b < n; ++b)
        if (!status || status[b] == 0) v.push_back(x[b]);
    const uint64_t m = v.size();
    out[0] = (double)m;
    if (m == 0) return 0;
    double sum = 0.0;
    uint64_t zeros = 0;
    for (uint64_t i = 0; i < m; ++i) { sum += v[i]; zeros += v[i] == 0.0 ? 1 : 0; }
    const double mean = sum / (double)m;
    double ss = 0.0;
    for (uint64_t i = 0; i < m; ++i) { const double d = v[i] - mean; ss += d * d; }
    out[1] = mean;
    out[2] = m < 2 ? 0.0 : std::sqrt(ss / (double)(m - 1));
    std::sort(v.begin(), v.end());
    static const uint64_t P[5] = {25, 250, 500, 750, 975};   // per mille
    // p * (m - 1) stays below 2^64 for every m a caller can hold in memory (m < 2^54)
    for (int q = 0; q < 5; ++q) out[3 + q] = v[(size_t)(P[q] * (m - 1) / 1000)];
    out[8] = (double)zeros / (double)m;
    out[9] = v[0];
    return 0;
}

}  // extern "C"

// growth_plan.hpp -- the host side of the replication index report (pantax_hip_strain_growth, stage_growth.hip) as a pure function of plain values: the fit
// over the own-node windows of ONE selection entry (pantax_hip_growth_fit, include/pantax_hip.h "own-node windows and the replication index").  Standard
// headers only: tests/native/growth_plan_check.cpp compiles this with the host compiler alone.
#pragma once
#include <cstdint>

namespace ptx {

enum GrowthStatus : int32_t { GROWTH_OK = 0, GROWTH_EMPTY = 1, GROWTH_FEW_WINDOWS = 2, GROWTH_LOW_DEPTH = 3, GROWTH_FLAT = 4 };
struct GrowthFit {
    uint64_t n_kept = 0, n_zero = 0, n_f = 0, n_fit = 0, own_len = 0;
    double median_depth = 0.0, slope = 0.0, intercept = 0.0, r2 = 0.0, index = 1.0;
    int32_t status = GROWTH_EMPTY;
};
// len_own, bases_own [n]; min_own >= 1, trim_permille < 500 (the caller's checks).  The steps, in this order: keep (len_own >= min_own), set the windows
// without bases aside (n_zero), sort by depth as an exact rational (128-bit products, ties by window index), drop what lies outside [median / 8, median x 8]
// around the lower median, trim floor(n_f x trim_permille / 1000) from each end, least squares of log2 depth against (rank + 0.5) / n_f in centred two-pass
// sums, the status.  No floating point enters the order.
GrowthFit growth_fit(uint64_t n, const uint64_t *len_own, const uint64_t *bases_own, uint64_t min_own, uint64_t trim_permille, uint64_t min_windows, double min_depth);
const char *growth_status_name(int32_t status);

}  // namespace ptx

// growth_plan.cpp -- the host helper of the replication index report (growth_plan.hpp).  Nothing here touches the device.
#include "growth_plan.hpp"
#include <algorithm>
#include <cmath>
#include <vector>
#include "../../include/pantax_hip.h"

static_assert(ptx::GROWTH_OK == PANTAX_HIP_GROWTH_OK && ptx::GROWTH_EMPTY == PANTAX_HIP_GROWTH_EMPTY && ptx::GROWTH_FEW_WINDOWS == PANTAX_HIP_GROWTH_FEW_WINDOWS &&
                  ptx::GROWTH_LOW_DEPTH == PANTAX_HIP_GROWTH_LOW_DEPTH && ptx::GROWTH_FLAT == PANTAX_HIP_GROWTH_FLAT,
              "the status values of pantax_hip_growth_fit_result");

namespace ptx {

GrowthFit growth_fit(uint64_t n, const uint64_t *len_own, const uint64_t *bases_own, uint64_t min_own, uint64_t trim_permille, uint64_t min_windows, double min_depth) {
    GrowthFit r;
    // 1. the kept windows; those without bases are counted and set aside
    std::vector<uint64_t> idx;
    for (uint64_t i = 0; i < n; ++i) {
        if (len_own[i] < min_own) continue;
        ++r.n_kept; r.own_len += len_own[i];
        if (bases_own[i] == 0) ++r.n_zero;
        else idx.push_back(i);
    }
    // 2. ascending depth as an exact rational, ties by window index
    std::sort(idx.begin(), idx.end(), [&](uint64_t a, uint64_t b) {
        const unsigned __int128 l = (unsigned __int128)bases_own[a] * len_own[b], h = (unsigned __int128)bases_own[b] * len_own[a];
        return l != h ? l < h : a < b;
    });
    const auto depth = [&](uint64_t i) { return (double)bases_own[i] / (double)len_own[i]; };
    // 3. the lower median, and the windows within a factor of 8 of it (a stretch of the sorted order)
    std::vector<double> y;
    if (!idx.empty()) {
        r.median_depth = depth(idx[(idx.size() - 1) / 2]);
        const double lo = r.median_depth / 8.0, hi = r.median_depth * 8.0;
        for (const uint64_t i : idx) {
            const double d = depth(i);
            if (d >= lo && d <= hi) y.push_back(d);
        }
    }
    r.n_f = y.size();
    // 4. the trim from each end
    const uint64_t t_lo = (uint64_t)((unsigned __int128)r.n_f * trim_permille / 1000);
    const uint64_t m = r.n_f - 2 * t_lo;   // (trim_permille < 500: at least one window is left of n_f >= 1)
    r.n_fit = m;
    // 5. the line through log2 depth against rank: centred two-pass sums in ascending j
    bool flat = true;
    if (m) {
        for (uint64_t j = 0; j < m; ++j) y[j] = std::log2(y[t_lo + j]);
        const auto x = [&](uint64_t j) { return ((double)(t_lo + j) + 0.5) / (double)r.n_f; };
        for (uint64_t j = 1; j < m; ++j) flat = flat && y[j] == y[0];
        if (flat) r.intercept = y[0];
        else {
            double sx = 0.0, sy = 0.0;
            for (uint64_t j = 0; j < m; ++j) { sx += x(j); sy += y[j]; }
            const double mx = sx / (double)m, my = sy / (double)m;
            double sxx = 0.0, sxy = 0.0, syy = 0.0;
            for (uint64_t j = 0; j < m; ++j) {
                const double dx = x(j) - mx, dy = y[j] - my;
                sxx += dx * dx; sxy += dx * dy; syy += dy * dy;
            }
            r.slope = sxy / sxx;
            r.intercept = my - r.slope * mx;
            r.r2 = (sxy * sxy) / (sxx * syy);
            r.index = std::exp2(r.slope);
        }
    }
    // 6. the first status that applies
    r.status = m == 0 ? GROWTH_EMPTY : m < min_windows ? GROWTH_FEW_WINDOWS : r.median_depth < min_depth ? GROWTH_LOW_DEPTH : flat ? GROWTH_FLAT : GROWTH_OK;
    return r;
}

const char *growth_status_name(int32_t status) {
    switch (status) {
    case GROWTH_OK: return "ok";
    case GROWTH_EMPTY: return "empty";
    case GROWTH_FEW_WINDOWS: return "few_windows";
    case GROWTH_LOW_DEPTH: return "low_depth";
    case GROWTH_FLAT: return "flat";
    }
    return "?";
}

}  // namespace ptx

extern "C" int pantax_hip_growth_fit(uint64_t n, const uint64_t *len_own, const uint64_t *bases_own, uint64_t min_own, uint64_t trim_permille, uint64_t min_windows,
                                     double min_depth, pantax_hip_growth_fit_result *out) {
    if (!out || (n && (!len_own || !bases_own)) || trim_permille >= 500 || min_own == 0) return PANTAX_HIP_E_INVALID;
    const ptx::GrowthFit r = ptx::growth_fit(n, len_own, bases_own, min_own, trim_permille, min_windows, min_depth);
    *out = pantax_hip_growth_fit_result{r.n_kept, r.n_zero, r.n_f, r.n_fit, r.own_len, r.median_depth, r.slope, r.intercept, r.r2, r.index, r.status, 0};
    return 0;
}
extern "C" const char *pantax_hip_growth_status_name(int32_t status) { return ptx::growth_status_name(status); }

// read_em_plan.cpp -- the host decisions of pantax_hip_strain_read_em and the host helper of its contract (read_em_plan.hpp).  Nothing here touches the device.
#include "read_em_plan.hpp"
#include <algorithm>
#include <cmath>
#include <numeric>
#include "../../include/pantax_hip.h"

#if defined(__clang__)
#pragma clang fp contract(off)   // the helper's sums, products and quotients are plain IEEE operations, one rounding each
#endif

namespace ptx {

std::vector<uint64_t> read_class_rank(uint64_t J, const uint64_t *mask, const uint64_t *span, uint64_t N) {
    std::vector<uint64_t> idx(J);
    std::iota(idx.begin(), idx.end(), 0ull);
    const uint64_t n = std::min(J, N);
    std::partial_sort(idx.begin(), idx.begin() + n, idx.end(),
                      [&](uint64_t a, uint64_t b) { return span[a] != span[b] ? span[a] > span[b] : mask[a] < mask[b]; });
    idx.resize(n);
    return idx;
}

}  // namespace ptx

extern "C" {

int pantax_hip_read_em(uint32_t K, uint64_t J, const uint64_t *mask, const uint64_t *b, const uint64_t *len, uint32_t max_iter, double tol, double *x_out,
                       uint32_t *n_iter_out, int32_t *converged_out, double *delta_out) {
    if (K > ptx::READ_EM_MAX_K || max_iter == 0 || !(tol >= 0.0) || !std::isfinite(tol)) return PANTAX_HIP_E_INVALID;
    if ((K && (!len || !x_out)) || (J && (!mask || !b)) || !n_iter_out || !converged_out || !delta_out) return PANTAX_HIP_E_INVALID;
    if (K < 64)
        for (uint64_t j = 0; j < J; ++j)
            if (mask[j] >> K) return PANTAX_HIP_E_INVALID;   // a bit that names no candidate
    double x[64], y[64];
    for (uint32_t k = 0; k < K; ++k) x[k] = len[k] > 0 ? 1.0 : 0.0;
    std::vector<double> r(J);
    uint32_t n_iter = 0;
    int32_t converged = 0;
    double delta = 0.0;
    for (uint32_t t = 1; t <= max_iter; ++t) {
        for (uint64_t j = 0; j < J; ++j) {
            double D = 0.0;
            for (uint64_t m = mask[j]; m; m &= m - 1ull) D = D + x[__builtin_ctzll(m)];
            r[j] = D > 0.0 ? (double)b[j] / D : 0.0;
        }
        delta = 0.0;
        double top = 0.0;
        for (uint32_t k = 0; k < K; ++k) {
            double R = 0.0;
            for (uint64_t j = 0; j < J; ++j)
                if ((mask[j] >> k) & 1ull) R = R + r[j];
            double v = len[k] > 0 ? (x[k] * R) / (double)len[k] : 0.0;
            if (v < 1e-200) v = 0.0;
            y[k] = v;
            delta = std::max(delta, std::fabs(v - x[k]));
            top = std::max(top, v);
        }
        for (uint32_t k = 0; k < K; ++k) x[k] = y[k];
        n_iter = t;
        if (delta <= tol * top) { converged = 1; break; }
    }
    for (uint32_t k = 0; k < K; ++k) x_out[k] = x[k];
    *n_iter_out = n_iter; *converged_out = converged; *delta_out = delta;
    return 0;
}

}  // extern "C"
